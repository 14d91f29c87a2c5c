"""CPU restatement of TransNet V1 (shot-boundary network) as the reference builds it -- TEST INFRASTRUCTURE ONLY
(imported by tests/ and tools/ only; the product path is retargetvid_amd/transnetv1_handler.py -> libsvc_hip.so).

PARITY UNPINNED: the reference runs this network in TensorFlow 1.x (3rd_party_libs/transnetv1/transnetv1_handler.py:17-130)
and neither TensorFlow nor the pre-trained checkpoint (note.txt:1) is available in the build container, so no output of the
reference itself could be recorded.  What is restated here is the graph the reference constructs, layer by layer:

  _build (:25-84)      uint8 [B, T, 27, 48, 3] / 255 -> L = 3 SDDCNN blocks of S = 2 DDCNN cells; a cell = four
                       Conv3D(filters, kernel 3x3x3, dilation (d, 1, 1), d = 1, 2, 4, 8, padding SAME, bias, ReLU) on the SAME
                       input, concatenated on the channel axis (:33-36, :55-59); filters = 16 * 2**block (:47);
                       MaxPool3D (1, 2, 2) after each block (:64); flatten (h, w, c) per frame (:68-69); Dense 256 ReLU
                       (:72); Dense 2 (:76); softmax, class 1 (:79)
  predict_video (:100-130)  windows of 100 frames, stride 50, the middle 50 kept; 25 copies of the first frame in front,
                       25 + 50 - (n % 50 or 50) copies of the last frame behind
Weights are TensorFlow-layout arrays: conv kernels [kt, kh, kw, cin, cout], dense kernels [in, out]
(retargetvid_amd/weights.make_transnet_state_dict names them after the reference's variable scopes)."""
import numpy as np
import torch
import torch.nn.functional as F

F0, L, S, D = 16, 3, 2, 256
H, W = 27, 48
DILATIONS = (1, 2, 4, 8)


def conv_name(block, cell, d):
    return 'TransNet/SDDCNN_%d/DDCNN_%d/Conv3D_%d' % (block + 1, cell + 1, d)


def forward(sd, frames_u8, dtype=torch.float32, taps=False):
    """frames_u8 [B, T, 27, 48, 3] uint8 -> P(transition) [B, T]  (ShotTransNet.predict_raw, :93-97), in `dtype` (the weights are
    converted to it: torch.float64 = the float64 restatement the device's layers are gated against).  taps=True: (P, taps) with
    every layer in the device's layout NDHWC: 'input' (v / 255), 'pre1'..'pre6' (a cell's four convolutions concatenated, before
    the ReLU), 'cell1'..'cell6' (after it), 'pool1'..'pool3', 'dense' [B, T, 256] (after bias and ReLU), 'logits' [B, T, 2], 'P'."""
    tp = {}
    ndhwc = lambda t: t.permute(0, 2, 3, 4, 1).numpy()
    x = torch.from_numpy(np.ascontiguousarray(frames_u8)).to(dtype) / 255.0              # :41
    x = x.permute(0, 4, 1, 2, 3).contiguous()                         # NDHWC -> NCDHW
    if taps:
        tp['input'] = ndhwc(x)
    with torch.no_grad():
        for b in range(L):
            for c in range(S):
                pre = []
                for d in DILATIONS:
                    k = torch.from_numpy(sd[conv_name(b, c, d) + '/kernel']).to(dtype).permute(4, 3, 0, 1, 2).contiguous()
                    bias = torch.from_numpy(sd[conv_name(b, c, d) + '/bias']).to(dtype)
                    # kernel 3, dilation (d, 1, 1), SAME: symmetric zero padding of (d, 1, 1)  (:33-36)
                    pre.append(F.conv3d(x, k, bias, padding=(d, 1, 1), dilation=(d, 1, 1)))
                x = torch.cat([F.relu(p) for p in pre], 1)                   # ReLU (:35), concat (:59)
                if taps:
                    tp['pre%d' % (b * S + c + 1)] = ndhwc(torch.cat(pre, 1))
                    tp['cell%d' % (b * S + c + 1)] = ndhwc(x)
            x = F.max_pool3d(x, (1, 2, 2))                            # VALID: floor  (:64)
            if taps:
                tp['pool%d' % (b + 1)] = ndhwc(x)
        Bn, C, T, h, w = x.shape
        x = x.permute(0, 2, 3, 4, 1).reshape(Bn, T, h * w * C)        # flatten (h, w, c) per frame  (:68-69)
        x = F.relu(x @ torch.from_numpy(sd['TransNet/dense/kernel']).to(dtype) + torch.from_numpy(sd['TransNet/dense/bias']).to(dtype))  # :72
        logits = x @ torch.from_numpy(sd['TransNet/dense_1/kernel']).to(dtype) + torch.from_numpy(sd['TransNet/dense_1/bias']).to(dtype)  # :76
        P = torch.softmax(logits, -1)[:, :, 1].numpy()                # :79
        if not taps:
            return P
        tp.update(dense=x.numpy(), logits=logits.numpy(), P=P)
        return P, tp


def window_indices(n):
    """Frame index of every slot of every 100-frame window of predict_video (:104-121) for a video of n frames."""
    pad_end = 25 + 50 - (n % 50 if n % 50 != 0 else 50)
    idx = np.concatenate([np.zeros(25, np.int64), np.arange(n), np.full(pad_end, n - 1, np.int64)])
    wins, ptr = [], 0
    while ptr + 100 <= len(idx):
        wins.append(idx[ptr:ptr + 100])
        ptr += 50
    return np.stack(wins)


def predict_video(sd, frames_u8, batch=4):
    """[n, 27, 48, 3] uint8 -> [n] float32 (:100-130)."""
    n = len(frames_u8)
    wi = window_indices(n)
    res = []
    for i in range(0, len(wi), batch):
        p = forward(sd, frames_u8[wi[i:i + batch]])
        res.append(p[:, 25:75].reshape(-1))
    return np.concatenate(res)[:n]


def predictions_to_scenes(predictions, threshold=0.5):
    """smartVidCrop.py:214-230 (same walk as transnet_utils.scenes_from_predictions + the all-ones fix)."""
    pred = (np.asarray(predictions) > threshold).astype(np.uint8)
    scenes, t, t_prev, start, i = [], -1, 0, 0, 0
    for i, t in enumerate(pred):
        if t_prev == 1 and t == 0:
            start = i
        if t_prev == 0 and t == 1 and i != 0:
            scenes.append([start, i])
        t_prev = t
    if t == 0:
        scenes.append([start, i])
    if len(scenes) == 0:
        return np.array([[0, len(pred) - 1]], dtype=np.int32)
    return np.array(scenes, dtype=np.int32)


# ---- weights and inputs that do not hide errors (tests/test_gpu_transnet_layers.py, tools/transnet_error_report.py) --------------
VARIANTS = ('seed0', 'calibrated', 'sparse', 'loud')
INPUTS = ('video', 'noise', 'zeros', 'full', 'gradient')


def variant_state_dict(name):
    """'seed0': weights.make_transnet_state_dict(0) as it is.  'calibrated': seed 1 with the Dense(2) bias moved so that most P of the
    test inputs lie in [0.05, 0.95] (the logit error is visible in P).  'sparse': seed 2 with every conv bias shifted negative, so that
    at least 70 % of every cell's outputs are exact zeros (the ReLU edge, everywhere).  'loud': seed 3 with every conv kernel and bias
    scaled so that the last cell reaches ~1e3 (relative precision at large exponents; the network is homogeneous, so only the scale
    changes)."""
    from retargetvid_amd import weights
    seed = VARIANTS.index(name)
    sd = weights.make_transnet_state_dict(seed)
    if name == 'calibrated':
        sd['TransNet/dense_1/kernel'] = (sd['TransNet/dense_1/kernel'] * np.float32(0.5)).astype(np.float32)
        sd['TransNet/dense_1/bias'] = np.array(CALIBRATED_BIAS, np.float32)
    elif name == 'sparse':
        for b in range(L):
            for c in range(S):
                for d in DILATIONS:
                    sd[conv_name(b, c, d) + '/bias'] = (sd[conv_name(b, c, d) + '/bias'] - np.float32(SPARSE_SHIFT[b * S + c])).astype(np.float32)
    elif name == 'loud':
        for b in range(L):
            for c in range(S):
                i = b * S + c
                for d in DILATIONS:
                    sd[conv_name(b, c, d) + '/kernel'] = (sd[conv_name(b, c, d) + '/kernel'] * np.float32(LOUD_GAIN)).astype(np.float32)
                    sd[conv_name(b, c, d) + '/bias'] = (sd[conv_name(b, c, d) + '/bias'] * np.float32(LOUD_GAIN ** (i + 1))).astype(np.float32)
    return sd


CALIBRATED_BIAS = (0.0, 0.0)                                  # with Dense(2)'s kernel halved: logit1 - logit0 within about +-2
SPARSE_SHIFT = (0.7, 0.3, 0.14, 0.09, 0.07, 0.06)              # the 82nd percentile of each cell's pre-ReLU values (seed 2, test inputs)
LOUD_GAIN = 2.6                                                # 2.6 ** 6 ~ 300: the last cell at ~1e3


def frames(kind, n, seed=0):
    """[n, 27, 48, 3] uint8.  'video': slowly varying frames with two hard cuts (tests/test_gpu_transnet.py's generator); 'noise':
    uniform bytes; 'zeros' / 'full': every byte 0 / 255 (the output is set by the biases and the zero padding at the borders alone);
    'gradient': a spatial ramp whose direction and offset change from frame to frame."""
    rng = np.random.RandomState(seed)
    if kind == 'video':
        fr = rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
        base = rng.randint(0, 256, (3, H, W, 3)).astype(np.float32)
        for i in range(n):
            s = 0 if i < n // 3 else (1 if i < 2 * n // 3 else 2)
            fr[i] = np.clip(base[s] + 8 * np.sin(i / 5.0) + rng.randn(H, W, 3) * 3, 0, 255).astype(np.uint8)
        return fr
    if kind == 'noise':
        return rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    if kind == 'zeros':
        return np.zeros((n, H, W, 3), np.uint8)
    if kind == 'full':
        return np.full((n, H, W, 3), 255, np.uint8)
    if kind == 'gradient':
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        out = np.empty((n, H, W, 3), np.uint8)
        for i in range(n):
            a = rng.uniform(0, 2 * np.pi)
            g = (np.cos(a) * x / W + np.sin(a) * y / H) * 255 + rng.uniform(-128, 128)
            out[i] = np.clip(np.stack([g, 255 - g, g * 0.5 + 64], -1), 0, 255).astype(np.uint8)
        return out
    raise ValueError(kind)
