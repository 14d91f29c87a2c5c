"""Writes tests/golden/tail_plan.json: the words of the plan door (Engine.tail_plan -> svc_debug_tail_plan) of the default engine
for every (shape, hdbscan_min) the host tests of the tail's paths use (tests/tail_paths.fixture_requests).  Needs a GPU (the door
takes a handle); tests/test_gpu_tail_paths.py::test_the_plan_fixture_is_the_doors holds the file equal to the door.

    python tools/make_tail_plan_fixture.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    import tail_paths
    from retargetvid_amd import ops
    eng = ops.tail_engine(reference=False)
    try:
        plans = {key: eng.tail_plan(h, w, CP) for key, (h, w, CP) in sorted(tail_paths.fixture_requests().items())}
    finally:
        eng.close()
    out = sys.argv[1] if len(sys.argv) > 1 else tail_paths.PLAN_FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(dict(engine='default', words=list(ops.TAIL_PLAN_WORDS), plans=plans), f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d plans -> %s' % (len(plans), out))


if __name__ == '__main__':
    main()
