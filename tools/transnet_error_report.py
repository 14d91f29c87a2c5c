"""GPU box helper: error of every TransNet V1 layer (svc_debug_transnet_tap) against the FLOAT64 oracle, per weight variant and cell
form -- the numbers behind the gates of tests/test_gpu_transnet_layers.py.

Per (variant, pipe, layer): max and mean |device - float64| / max|float64| over the cases of the test (window lengths 1 .. 100 and 3
windows of 17 frames, the five input kinds); a cell's and a pool's max|float64| is that of the cell's pre-ReLU values, as in the
test.  Per (variant, pipe): the largest |log(P / (1 - P)) - (logit1 - logit0)| where the float64 P is in [1e-3, 1 - 1e-3].

  python tools/transnet_error_report.py [--variants seed0,...] [--pipes default,...] [--out profiles/transnet_layer_error.md]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_transnet_layers as G                                            # noqa: E402

SHOW = ['input', 'cell1', 'cell2', 'pool1', 'cell3', 'cell4', 'pool2', 'cell5', 'cell6', 'pool3', 'dense']


def measure(net, variant):
    sd, refs = G.oracle(variant)
    err = {k: [0.0, [], 0] for k in SHOW}
    logit = own = 0.0
    for fr, label, ref in refs:
        for li, layer in enumerate(G.LAYERS):
            got = net.debug_tap(fr, li).astype(np.float64)
            m = G.tap_scale(ref, layer, slice(None))
            d = np.abs(got - ref[layer]) / (m if m > 0 else 1.0)
            e = err[layer]
            e[0] = max(e[0], float(d.max()))
            e[1].append(float(d.sum()))
            e[2] += d.size
        p3 = net.debug_tap(fr, G.LAYERS.index('pool3')).astype(np.float64)
        d64 = np.maximum(p3.reshape(p3.shape[:2] + (-1,)) @ sd['TransNet/dense/kernel'].astype(np.float64)
                         + sd['TransNet/dense/bias'].astype(np.float64), 0)
        dd = np.abs(net.debug_tap(fr, G.LAYERS.index('dense')) - d64)
        own = max(own, float(dd.max() / max(np.abs(d64).max(), 1e-30)))
        P = net.predict_raw(fr).astype(np.float64)
        band = (ref['P'] >= 1e-3) & (ref['P'] <= 1 - 1e-3)
        if band.any():
            want = (ref['logits'][..., 1] - ref['logits'][..., 0])[band]
            logit = max(logit, float(np.abs(np.log(P[band] / (1 - P[band])) - want).max()))
    return {k: (v[0], sum(v[1]) / v[2]) for k, v in err.items()}, logit, own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variants', default=','.join(G.R.VARIANTS))
    ap.add_argument('--pipes', default=','.join(G.PIPES))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transnet_layer_error.md'))
    args = ap.parse_args()
    lines = ['# TransNet V1 layers against the float64 oracle (MI355X)', '',
             '`python tools/transnet_error_report.py --out <file>`: max and mean |device - float64 oracle| / max|float64| per layer over '
             'the cases of `tests/test_gpu_transnet_layers.py` (window lengths 1, 2, 8, 9, 16, 17, 37, 100 and 3 windows of 17 frames; '
             'video, noise, all-0, all-255 and gradient frames), per weight variant and cell form; for a cell and a pool, max|float64| '
             'is that of the cell\'s pre-ReLU values.  `logit`: the largest |log(P / (1 - P)) - (logit1 - logit0)| where the float64 P '
             'is in [1e-3, 1 - 1e-3] (`-` where no frame is: the loud network saturates P).  `dense (own pool 3)`: Dense(256) of the '
             'device against a float64 Dense(256) on the device\'s own pool-3 tap, / its max.', '',
             '| variant | pipe | ' + ' | '.join('%s max / mean' % k for k in SHOW) + ' | logit | dense (own pool 3) |',
             '|---|---|' + '---|' * (len(SHOW) + 2)]
    for pipe in args.pipes.split(','):
        net = None
        for variant in args.variants.split(','):
            if net is None:
                net = G.make_net(pipe, G.oracle(variant)[0])
            else:
                G.load(net, G.oracle(variant)[0])
            err, logit, own = measure(net, variant)
            row = '| %s | %s | ' % (variant, pipe) + ' | '.join('%.1e / %.1e' % err[k] for k in SHOW) + ' | %s |' % (
                '%.1e' % logit if variant != 'loud' or logit > 0 else '-') + ' %.1e |' % own
            print(row, flush=True)
            lines.append(row)
        net.close()
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
