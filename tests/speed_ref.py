'''
numpy restatement of the speed perturbation of the wavdir dataset, written from the rule in
include/danet_speed_hip.h (not from datasets.py / ops.py / speed.hip): the filter table, the output length,
the draw, the resampler in float64 (with the per-sample magnitude sum S_n its float32 error bound is
stated in), and the helpers the speed tests share (a WAV tree of mixed lengths, scales and sample rates).
'''
import math
import os

import numpy as np

Q = 512          # DANET_SPEED_PHASES
Z = 16           # half of DANET_SPEED_TAPS
P_MIN, P_MAX = Q - Q // 4, Q + Q // 4


def table(P):
    '''tab[phi][j] = h(j - (Z - 1) - phi / Q): float64, rounded once to float32 [Q][2Z]'''
    fc = 1.0 / (1.0 + P)
    j, phi = np.meshgrid(np.arange(2 * Z), np.arange(Q))
    t = (j - (Z - 1)).astype(np.float64) - phi.astype(np.float64) / Q
    a = fc * t
    k = np.rint(a)
    sin_pi_a = np.sin(np.pi * (a - k)) * (1.0 - 2.0 * (np.abs(k) % 2))      # (-1)^k sin(pi (a - k))
    with np.errstate(invalid='ignore', divide='ignore'):
        sinc = np.where(a == 0.0, 1.0, sin_pi_a / (np.pi * a))
    h = fc * sinc * 0.5 * (1.0 + np.cos(np.pi * t / Z))
    h[np.abs(t) >= Z] = 0.0
    return (h + 0.0).astype(np.float32)                                     # a zero tap is +0


def out_len(L, p):
    '''L' = floor((L - 1) * Q / p) + 1 in python integers'''
    return (int(L) - 1) * Q // int(p) + 1


def draw(lengths, rng, P, fft_size):
    '''(p, L') per utterance: one uniform draw each, in order; an utterance whose L' would fall below fft_size
    keeps p = Q'''
    k = int(math.floor(Q * P))
    ps, Ls = [], []
    for L in lengths:
        u = rng.uniform(-P, P)
        p = Q + int(np.rint(Q * u))
        p = min(max(p, Q - k), Q + k)
        if out_len(L, p) < fft_size:
            p = Q
        ps.append(p)
        Ls.append(out_len(L, p))
    return np.asarray(ps, dtype=np.int64), np.asarray(Ls, dtype=np.int64)


def stream(rank, subset):
    '''the RandomState of a subset's speeds: seeded by (1337 + rank, index of the subset, 1)'''
    return np.random.RandomState([1337 + rank, ('train', 'valid', 'test').index(subset), 1])


def _windows(x, p, n_out):
    '''(tab rows index phi [n], input windows [n][2Z] float32 with zeros outside the utterance)'''
    x = np.asarray(x, dtype=np.float32)
    n = np.arange(n_out, dtype=np.int64)
    m, phi = (n * p) // Q, (n * p) % Q
    idx = m[:, None] + np.arange(2 * Z, dtype=np.int64)[None, :] - (Z - 1)
    inside = (idx >= 0) & (idx < len(x))
    xw = np.where(inside, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0).astype(np.float32)
    return phi, xw


def resample(x, p, tab, n_out=None):
    '''(y64 [n], S [n]): y[n] = sum_j tab[phi][j] * x[m + j - (Z - 1)] in float64 over the float32 table and the
    float32 input, and S_n = sum_j |tab * x|'''
    n_out = out_len(len(x), p) if n_out is None else n_out
    phi, xw = _windows(x, p, n_out)
    prod = tab[phi].astype(np.float64) * xw.astype(np.float64)
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def resample_f32(x, p, tab, n_out=None):
    '''the same sum as sequential float32 products and additions, j ascending (no fused multiply-add)'''
    n_out = out_len(len(x), p) if n_out is None else n_out
    phi, xw = _windows(x, p, n_out)
    w = tab[phi]
    acc = np.zeros(n_out, np.float32)
    for j in range(2 * Z):
        acc = (acc + (w[:, j] * xw[:, j]).astype(np.float32)).astype(np.float32)
    return acc


def bound(S):
    '''the bar of a 32-term float32 dot product in any order, with or without fused multiply-adds'''
    return 33.0 * 2.0 ** -24 * np.asarray(S, np.float64) + 2.0 ** -126


def write_tree(root, seed=0, n_per_subset=12, subsets=('train', 'test'), seconds=(0.3, 0.8)):
    '''a wavdir tree of int16 files of speech-shaped noise: stored RMS over 40 dB (30 ... 6000), lengths mixed,
    every third file at 16 kHz (the dataset resamples it to 8 kHz) -> {subset: [paths]}'''
    import scipy.io.wavfile
    from danet_amd import datasets
    rng = np.random.RandomState(seed)
    made = {}
    for subset in subsets:
        made[subset] = []
        os.makedirs(os.path.join(str(root), subset), exist_ok=True)
        for i in range(n_per_subset):
            rate = 16000 if i % 3 == 2 else 8000
            n = int(rng.uniform(*seconds) * rate)
            rms = 30.0 * (200.0 ** (i / float(max(n_per_subset - 1, 1))))
            w = datasets.speech_shaped_wave(rng, n, rate, rms=rms, phase=rng.uniform(0, 2 * np.pi))
            fn = os.path.join(str(root), subset, 'utt%03d.wav' % i)
            scipy.io.wavfile.write(fn, rate, np.clip(w, -32768, 32767).astype(np.int16))
            made[subset].append(fn)
    return made
