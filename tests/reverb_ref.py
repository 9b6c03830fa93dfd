'''
numpy restatement of the reverberation of the wavdir dataset, written from the rule in
include/danet_reverb_hip.h (not from datasets.py / ops.py / reverb.hip): the tap count, the bank, the draw,
the span of samples a crop reads, the convolution in float64 (np.convolve, with the per-sample magnitude sum
its float32 error bound is stated in) and the clamping of a descriptor row.
'''
import math

import numpy as np

NB = 32              # DANET_REVERB_ROWS
MAX_TAPS = 8192      # DANET_REVERB_MAX_TAPS
MAX_LEN = 1 << 40


def taps(R, smprate):
    '''K = 4 * ceil(R * smprate / 4), at least 4'''
    return max(4, 4 * int(math.ceil(R * smprate / 4.0)))


def bank(R, smprate):
    '''float32 [NB][K]: row 0 the unit impulse, row k >= 1 a direct path plus an exponentially decaying
    Gaussian tail at DRR_k, unit energy; float64, rounded once'''
    K = taps(R, smprate)
    assert K <= MAX_TAPS
    out = np.zeros((NB, K), np.float64)
    out[0, 0] = 1.0
    for k in range(1, NB):
        rt60 = R * k / (NB - 1.0)
        h = np.zeros(K, np.float64)
        h[0] = 1.0
        if rt60 > 0:
            g = np.random.RandomState([1337, 2, k]).standard_normal(K)
            t = np.zeros(K, np.float64)
            for n in range(1, K):
                t[n] = g[n] * math.exp(-3.0 * math.log(10.0) * n / (rt60 * smprate))
            energy = float((t * t).sum())
            if energy > 0:
                drr = 10.0 - 10.0 * k / (NB - 1.0)
                t *= math.sqrt(10.0 ** (-drr / 10.0) / energy)
            h = (h + t) / math.sqrt(1.0 + float((t * t).sum()))
        out[k] = h
    return out.astype(np.float32)


def stream(rank, subset):
    '''the RandomState of a subset's rows: seeded by (1337 + rank, index of the subset, 2)'''
    return np.random.RandomState([1337 + rank, ('train', 'valid', 'test').index(subset), 2])


def draw(n, rng):
    '''the rows of one batch: ONE randint call'''
    return rng.randint(0, NB, size=n).astype(np.int64)


def num_frames(L, N, S):
    return (L + (-L % S) % N) // S + 1


def span(L, pad, beg, cnt, N, S):
    '''(first sample, count) that frames [beg, beg + cnt) of the padded axis read of an L-sample utterance whose
    own frame t sits at pad + t and covers samples [t S - N / 2, t S + N / 2)'''
    a, b = max(beg - pad, 0), min(beg + cnt - pad, num_frames(L, N, S))
    if b <= a:
        return 0, 0
    lo, hi = max(a * S - N // 2, 0), min((b - 1) * S + N // 2, L)
    return (lo, hi - lo) if hi > lo else (0, 0)


def apply(x, h):
    '''(y64 [L], S [L]): y[n] = sum_j h[j] x[n - j] in float64 over the float32 inputs, the tail beyond L cut,
    and S_n = sum_j |h[j] x[n - j]|'''
    x, h = np.asarray(x, np.float32).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0)
    return np.convolve(x, h)[:len(x)], np.convolve(np.abs(x), np.abs(h))[:len(x)]


def apply_f32(x, h):
    '''the same sum as sequential float32 products and additions, j ascending (no fused multiply-add)'''
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    acc = np.zeros(len(x), np.float32)
    for j in range(min(len(h), len(x))):
        acc[j:] = (acc[j:] + (h[j] * x[:len(x) - j]).astype(np.float32)).astype(np.float32)
    return acc


def bound(S, K):
    '''the bar of a K-term float32 dot product in any order, with or without fused multiply-adds:
    gamma_K <= 1.01 K 2^-24 for K <= 8192'''
    return 1.01 * K * 2.0 ** -24 * np.asarray(S, np.float64) + 2.0 ** -126


def clamp_row(src, dst_len, so, sl, do, ob, oc, row):
    '''a descriptor row as the header clamps it -> (x the kernel may see, float32 [L] with zeros where the source
    span leaves `src`; first and last + 1 output sample written; the row used)'''
    L = min(max(sl, 0), MAX_LEN)
    x = np.zeros(min(L, 1 << 22), np.float32)
    assert L == len(x)
    for i in range(L):
        if 0 <= so + i < len(src):
            x[i] = src[so + i]
    lo, hi = max(ob, 0), min(ob + min(max(oc, 0), MAX_LEN), L)
    lo, hi = max(lo, -do), min(hi, dst_len - do)
    if hi <= lo:
        lo = hi = 0
    return x, lo, hi, min(max(row, 0), NB - 1)
