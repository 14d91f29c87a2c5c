"""Measures the per-element error of every node of the saliency network on the device against the float64 node oracle
(oracle/unisal_nodes_ref.py) and writes profiles/net_node_error.md: per node and pipe the largest |device - value| / (u bound)
over the eleven geometries (the oracle's activations of tl and ri on the goldens' frames) and the adversarial inputs at
three geometries, and the gate constants C that tests/net_node_cases.py cites (twice the fp32 pipe's maximum).

A second section holds the two nodes whose work depends on the map shape itself, `front` and `smooth`, at the map shapes of
tests/test_net_plan_census.py (SHAPES) on the carrier checkpoint, with the inputs of tests/test_gpu_map_shapes.py, and the share
of u8 pixels one grey level off the fp32 oracle.  Its rows enter C_NODE['front'] and C_SMOOTH by the same rule.

    python tools/net_node_error_report.py [--out profiles/net_node_error.md] [--sections nodes,shapes]

--sections shapes measures the second section alone: the first section and the constants it sets are kept as the file has them,
and `front` / `smooth` are raised where the new rows exceed them (the kernels of the other nodes do not see the map shape)."""
import argparse
import ast
import os
import re
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


SHAPES_HEADING = '## `front` and `smooth` at the map shapes of the census'


def measure_nodes():
    """-> {(pipe, node): (largest ratio, where)} over the eleven geometries and the adversarial inputs."""
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
    return worst


def nodes_section(worst):
    """-> (lines of the first section, {constant: value})"""
    nodes = C.MAIN_NODES + ['smooth']
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
    lines += ['', 'Largest ratio over all nodes but `smooth`: f32 %.3f, bf16x6 %.3f.' % (main_max['f32'], main_max['bf16x6']), '']
    consts = dict(C_GATE=round(2 * main_max['f32'], 3), C_SMOOTH=round(2 * worst[('f32', 'smooth')][0], 3),
                  C_NODE={n: round(2 * worst[('f32', n)][0], 3) for n in ['front'] + C.MAIN_NODES})
    return lines, consts


def kept_nodes_section(path):
    """The first section and its constants as the file at `path` has them."""
    text = open(path).read()
    head = text.split(SHAPES_HEADING)[0].split('`C_GATE`')[0].rstrip('\n').split('\n')
    consts = dict(C_GATE=float(re.search(r'`C_GATE` \(.*?\) = ([0-9.]+)', text).group(1)),
                  C_SMOOTH=float(re.search(r'`C_SMOOTH` \(.*?\) = ([0-9.]+)', text).group(1)),
                  C_NODE=ast.literal_eval(re.search(r'C_NODE = (\{.*?\})', text).group(1)))
    return head + [''], consts


def shapes_section():
    """`front` and `smooth` at SHAPES on the carrier checkpoint (the inputs of tests/test_gpu_map_shapes.py), u8 maps against
    the fp32 oracle.  -> (lines, largest f32 ratio of front, of smooth, and the shapes they lie at)"""
    import test_gpu_map_shapes as M
    from retargetvid_amd import ops as O
    sd, ref = M._node_ref()
    engs = {p: M._engine(p, sd=sd) for p in PIPES}
    lines = [SHAPES_HEADING, '',
             'The two nodes whose kernels depend on the map shape `(h, w)` itself, at the shapes of `tests/test_net_plan_census.py` (`SHAPES`:',
             'the extremes of the plan\'s geometry over every shape the ingest can produce), carrier checkpoint, three frames per shape (blobs,',
             'random bytes, a rim frame).  `front`: from the uint8 frames, against the float64 stem + features.1 on the fp32 oracle\'s network',
             'input; `ch`: the output channel of the largest ratio.  `smooth`: the largest over three logit fields (the oracle\'s own adapt',
             'output, N(0, 1), a checkerboard of cells plus a ramp), `rows`: the map rows per workgroup the plan chose.  `u8`: the largest share',
             'over the frames of pixels one grey level off the fp32 oracle (no pixel is further off), maps of at least %d pixels.' % M.U8_MIN_PX,
             'On this checkpoint the largest `front` ratio lies in output channel 0 at every shape: the luminance carrier, a pass-through with',
             'weight 1 whose bound has few terms (about 10, against about 130 in the other channels) and so does not overestimate the rounding of',
             "the stem's 27-term sum as the bounds of `tl` and `ri` do; the other fifteen channels stay at 0.11 - 0.36.  The excess is spread",
             'evenly over the rows and columns of a tile and over the border and the interior of the image, is equal on both pipes and is the',
             "same at 140x250, one of the eleven (1.42): rounding on a tight bound, not a window or an edge defect -- so it enters `C_NODE['front']`.",
             '',
             '| shape | front f32 | ch | front bf16x6 | ch | rows | smooth f32 | field | smooth bf16x6 | u8 f32 | u8 bf16x6 |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    top = {'front': (0.0, None), 'smooth': (0.0, None)}
    for shape in M.SHAPES:
        h, w = shape
        NH, NW = M.U.get_optimal_out_size(shape)
        o = M._oracle(shape)
        row = {}
        if shape in M.NODE_SHAPES:
            value, bound = ref.run('front', o['input'])
            for p in PIPES:
                dev, _ = C.run_device(engs[p], 'front', 3, h, w, NH, NW, o['frames'])
                with np.errstate(divide='ignore', invalid='ignore'):
                    r = np.where(bound > 0, np.abs(dev.astype(np.float64) - value) / (C.U32 * bound), 0.0)
                row['front', p] = (C.error_ratio(dev, value, bound), int(np.unravel_index(r.argmax(), r.shape)[-1]))
            for name, logit in M._logit_fields(o['adapt'], NH // 8, NW // 8).items():
                value, bound = ref.run('smooth', logit, out_hw=shape)
                for p in PIPES:
                    dev, _ = C.run_device(engs[p], 'smooth', 3, h, w, NH, NW, logit)
                    row['smooth', p] = max(row.get(('smooth', p), (0.0, '')), (C.error_ratio(dev, value, bound), name))
            for node in top:
                top[node] = max(top[node], (row[node, 'f32'][0], shape))
        if h * w >= M.U8_MIN_PX:
            for p in PIPES:
                m = engs[p].saliency(torch.from_numpy(o['frames'].copy()).cuda()).cpu().numpy().astype(int)
                d = np.abs(m - o['maps'].astype(int))
                assert d.max() <= 1, (shape, p, int(d.max()))
                row['u8', p] = max(float((d[i] > 0).mean()) for i in range(3))
        cells = ['%dx%d' % shape]
        for p in PIPES:
            cells += ['%.3f' % row['front', p][0], '%d' % row['front', p][1]] if ('front', p) in row else ['-', '-']
        cells.append('%d' % O.net_plan(h, w)['sd_rows'])
        cells += ['%.3f' % row['smooth', 'f32'][0], row['smooth', 'f32'][1], '%.3f' % row['smooth', 'bf16x6'][0]] if ('smooth', 'f32') in row else ['-'] * 3
        cells += ['%.2e' % row['u8', p] if ('u8', p) in row else '-' for p in PIPES]
        lines.append('| ' + ' | '.join(cells) + ' |')
        print(lines[-1], flush=True)
    for e in engs.values():
        e.close()
    return lines, top


def constants_lines(consts, top):
    """The end of the report: which constants the second section sets (top: its largest fp32 ratios and their shapes), and the
    constants over both sections.  A constant is raised where twice the section's maximum exceeds it; consts is updated."""
    moved = []
    for name, node in (("C_NODE['front']", 'front'), ('C_SMOOTH', 'smooth')):
        old = consts['C_NODE']['front'] if node == 'front' else consts['C_SMOOTH']
        new = round(2 * top[node][0], 3)
        if new >= old:
            moved.append('`%s` = %.3f (%dx%d)' % ((name, new) + top[node][1]))
            if node == 'front':
                consts['C_NODE']['front'] = new
            else:
                consts['C_SMOOTH'] = new
    return ['',
            'Largest fp32-pipe ratio of this section: `front` %.3f at %dx%d, `smooth` %.3f at %dx%d.'
            % ((top['front'][0],) + top['front'][1] + (top['smooth'][0],) + top['smooth'][1]),
            'Constants these rows set (the others come from the first section): %s.' % ('; '.join(moved) if moved else 'none'),
            '',
            '## Constants',
            '',
            'Over both sections:',
            '',
            '`C_GATE` (twice the fp32 pipe\'s maximum over all nodes but `smooth`, the gate of BOTH pipes) = %.3f' % consts['C_GATE'],
            '',
            '`C_NODE` (twice each node\'s own fp32 maximum; the gate of a node is the smaller of this and `C_GATE`):',
            '',
            '    C_NODE = {%s}' % ', '.join("'%s': %.3f" % (n, consts['C_NODE'][n]) for n in ['front'] + C.MAIN_NODES),
            '',
            '`C_SMOOTH` (twice the fp32 pipe\'s maximum of `smooth`; the smoothing kernel is the same code on both pipes) = %.3f' % consts['C_SMOOTH'],
            '']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'net_node_error.md'))
    ap.add_argument('--sections', default='nodes,shapes', help='nodes,shapes (all) or shapes (keep the first section of --out)')
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lines, consts = nodes_section(measure_nodes()) if 'nodes' in args.sections.split(',') else kept_nodes_section(args.out)
    shape_lines, top = shapes_section()
    lines += shape_lines + constants_lines(consts, top)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
