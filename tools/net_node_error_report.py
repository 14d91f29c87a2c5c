"""Measures the per-element error of every node of the saliency network on the device against the float64 node oracle
(oracle/unisal_nodes_ref.py) and writes profiles/net_node_error.md: per node and pipe the largest |device - value| / (u bound)
over the eleven geometries (the oracle's activations of tl and ri on the goldens' frames) and the adversarial inputs at
three geometries, and the gate constants C that tests/net_node_cases.py cites (twice the fp32 pipe's maximum).

    python tools/net_node_error_report.py [--out profiles/net_node_error.md]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np          # noqa: E402
import torch                # noqa: E402

import net_node_cases as C  # noqa: E402
from oracle import unisal_nodes_ref as N  # noqa: E402
from retargetvid_amd import ops  # noqa: E402
from test_oracle_unisal import ELEVEN, NET_SIZES  # noqa: E402

PIPES = ('f32', 'bf16x6')


def engine(ck, pipe):
    old = os.environ.get('SVC_MX')
    os.environ['SVC_MX'] = pipe
    try:
        eng = ops.Engine(C.checkpoint(ck)[0])
    finally:
        if old is None:
            os.environ.pop('SVC_MX', None)
        else:
            os.environ['SVC_MX'] = old
    assert eng.matrix_pipe() == pipe
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'net_node_error.md'))
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    nodes = C.MAIN_NODES + ['smooth']
    worst = {(p, n): (0.0, '') for p in PIPES for n in nodes + ['front']}
    t0 = time.time()

    def note(pipe, node, ratio, where):
        if ratio > worst[(pipe, node)][0]:
            worst[(pipe, node)] = (ratio, where)

    for ck in ('tl', 'ri'):
        engs = {p: engine(ck, p) for p in PIPES}
        ref = C.checkpoint(ck)[2]
        for gname, (h, w) in ELEVEN.items():
            NH, NW = NET_SIZES[gname]
            frames = C.golden_frames(ck, gname)
            nf = len(frames)
            for node, in0, in1, value, bound in C.oracle_activation_cases(ck, frames, h, w, NH, NW, nodes):
                for p in PIPES:
                    dev, _ = C.run_device(engs[p], node, nf, h, w, NH, NW, in0, in1)
                    note(p, node, C.error_ratio(dev, value, bound), '%s %s oracle' % (ck, gname))
            value, bound = ref.run('front', C.network_input(frames, torch.float32))
            for p in PIPES:
                dev, _ = C.run_device(engs[p], 'front', nf, h, w, NH, NW, frames)
                note(p, 'front', C.error_ratio(dev, value, bound), '%s %s oracle' % (ck, gname))
            if ck == 'tl' and gname in C.ADVERSARIAL_GEOMS:
                kinds = [('outliers', node) + C.adversarial_inputs(node, 3, NH, NW, C.adversarial_seed(node, NH)) for node in C.MAIN_NODES]
                kinds += [('straddling', node) + C.straddling_inputs(ref, node, 3, NH, NW, C.adversarial_seed(node, NH)) for node in N.PW_NODES]
                for kind, node, in0, in1 in kinds:
                    value, bound = ref.run(node, in0, in1)
                    for p in PIPES:
                        dev, _ = C.run_device(engs[p], node, 3, h, w, NH, NW, in0, in1)
                        note(p, node, C.error_ratio(dev, value, bound), '%s %s %s' % (ck, gname, kind))
            print('%s %s done at %.0f s' % (ck, gname, time.time() - t0), flush=True)
        for e in engs.values():
            e.close()
    main_max = {p: max(worst[(p, n)][0] for n in C.MAIN_NODES + ['front']) for p in PIPES}
    lines = ['# Per-element error of the saliency network\'s nodes on the device',
             '',
             'Written by `tools/net_node_error_report.py` on %s.' % torch.cuda.get_device_name(0),
             '',
             'Each figure is the largest `|device - value| / (u * bound)` over the elements of a node\'s output, `u = 2^-24`, `value`',
             'and `bound` from `oracle/unisal_nodes_ref.py` (float64 value; first-order running bound `sum|x||w| + |b|` per stage).',
             'Inputs: the float64 oracle\'s own activations of `tl` and `ri`, rounded to fp32, on the golden frames (one batch) of each of the',
             'eleven geometries; for the nodes other than `front` and `smooth` also N(0, 1) with 1 % of the entries x100 and 10 % exact',
             'zeros, and inputs solved to sit at the clamps 0 and 6 of the first ReLU6 (`tl`, n = 3) at %s.' % ', '.join(C.ADVERSARIAL_GEOMS),
             '',
             '| node | f32 | where | bf16x6 | where |',
             '|---|---|---|---|---|']
    for n in ['front'] + nodes:
        a, b = worst[('f32', n)], worst[('bf16x6', n)]
        lines.append('| %s | %.3f | %s | %.3f | %s |' % (n, a[0], a[1], b[0], b[1]))
    lines += ['',
              'Largest ratio over all nodes but `smooth`: f32 %.3f, bf16x6 %.3f.' % (main_max['f32'], main_max['bf16x6']),
              '',
              '`C_GATE` (twice the fp32 pipe\'s maximum, the gate of BOTH pipes) = %.3f' % (2 * main_max['f32']),
              '',
              '`C_NODE` (twice each node\'s own fp32 maximum; the gate of a node is the smaller of this and `C_GATE`):',
              '',
              '    C_NODE = {%s}' % ', '.join("'%s': %.3f" % (n, 2 * worst[('f32', n)][0]) for n in ['front'] + C.MAIN_NODES),
              '',
              '`C_SMOOTH` (twice the fp32 pipe\'s maximum of `smooth`) = %.3f (bf16x6 handle: %.3f; the smoothing kernel is the same code on both)'
              % (2 * worst[('f32', 'smooth')][0], worst[('bf16x6', 'smooth')][0]),
              '']
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
