'''
Restatement of the waveform metric (include/danet_metric_hip.h, THE RULE) in numpy float64, written from the
rule and independently of csrc/metric/metric.hip: overlap-add synthesis with an exact window-sum division,
Gram matrices, the permutation search and the mixture baseline.  The synthesis has a float32 variant (a
single-precision inverse FFT and single-precision sums in the order the rule gives) that measures the noise
floor of float32 arithmetic -- the tests compare the kernel's error with it.
'''
import itertools
import math

import numpy as np
import scipy.fft
import scipy.signal

MAX_C = 4


def stft(x, window, N, S, dtype=np.complex64):
    '''the reference's STFT call (app/utils.py:117-122) -> [T, F], cast to `dtype`'''
    Z = scipy.signal.stft(np.asarray(x, dtype=np.float64), window=np.asarray(window), nperseg=N, noverlap=N - S)[2]
    return Z.T.astype(dtype)


def synth(X, window, S, dtype=np.float64):
    '''X complex [..., T, F] -> dtype [..., (T - 1) * S]: y[n] = sum_t w[k] f_t[k] / sum_t w[k]^2'''
    X = np.asarray(X)
    T, F = X.shape[-2:]
    N = 2 * (F - 1)
    if T < 2:
        raise ValueError('synth: T must be >= 2')
    if dtype == np.float32:
        f = scipy.fft.irfft(X.astype(np.complex64), n=N, axis=-1)
        assert f.dtype == np.float32
    else:
        f = np.fft.irfft(X.astype(np.complex128), n=N, axis=-1)
    w = np.asarray(window).astype(dtype)
    assert w.shape == (N,)
    Ls = (T - 1) * S
    acc = np.zeros(X.shape[:-2] + (Ls,), dtype)
    wsum = np.zeros(Ls, dtype)
    for t in range(T):                                  # ascending t: the order of the rule's sums
        lo = t * S - N // 2
        a, b = max(lo, 0), min(lo + N, Ls)
        if a >= b:
            continue
        acc[..., a:b] += w[a - lo:b - lo] * f[..., t, a - lo:b - lo]
        wsum[a:b] += w[a - lo:b - lo] * w[a - lo:b - lo]
    out = np.zeros_like(acc)
    ok = wsum > 0
    out[..., ok] = acc[..., ok] / wsum[ok]
    return out


def window_sum_min(window, S, T=64):
    '''the smallest overlap-added w^2 over the samples of a T-frame signal'''
    w = np.asarray(window, dtype=np.float64)
    N = len(w)
    Ls = (T - 1) * S
    wsum = np.zeros(Ls)
    for t in range(T):
        lo = t * S - N // 2
        a, b = max(lo, 0), min(lo + N, Ls)
        if a < b:
            wsum[a:b] += w[a - lo:b - lo] ** 2
    return wsum.min()


def gram(wav):
    '''wav [B, M, Ls] -> float64 [B, M, M]'''
    w = np.asarray(wav, dtype=np.float64)
    return np.einsum('bin,bjn->bij', w, w)


def gram_fsum(wav):
    '''the same by math.fsum of the float64 products: exactly rounded'''
    w = np.asarray(wav, dtype=np.float64)
    B, M, _ = w.shape
    G = np.zeros((B, M, M))
    for b in range(B):
        for i in range(M):
            for j in range(i, M):
                G[b, i, j] = G[b, j, i] = math.fsum(w[b, i] * w[b, j])
    return G


def sdr(a, b, c):
    t = c * c / a
    r = b - t
    if not t > 0:
        return -100.0
    if not r > 0:
        return 100.0
    return min(100.0, max(-100.0, 10.0 * math.log10(t / r)))


def finalize(G, C):
    '''G [B, 2C, 2C] -> (per_utt [B, 2], perm_idx [B], mean2 [2])'''
    G = np.asarray(G, dtype=np.float64)
    B = G.shape[0]
    assert G.shape == (B, 2 * C, 2 * C) and 1 <= C <= MAX_C
    perms = list(itertools.permutations(range(C)))
    per_utt, perm_idx = np.zeros((B, 2)), np.zeros(B, np.int32)
    for u in range(B):
        g = [[float(v) for v in row] for row in G[u]]
        live = [i for i in range(C) if g[i][i] != 0.0]
        if not live:
            continue
        mm = 0.0
        for k in range(C):
            for l in range(C):
                mm += g[k][l]
        base = {}
        for i in live:
            ms = 0.0
            for k in range(C):
                ms += g[k][i]
            base[i] = sdr(g[i][i], mm, ms)
        s = {(i, j): sdr(g[i][i], g[C + j][C + j], g[i][C + j]) for i in live for j in range(C)}
        best, best_v = 0, None
        for p, perm in enumerate(perms):
            v = 0.0
            for i in live:
                v += s[i, perm[i]]
            if best_v is None or v > best_v:            # ties: the first permutation
                best, best_v = p, v
        imp = 0.0
        for i in live:
            imp += s[i, perms[best][i]] - base[i]
        per_utt[u] = best_v / len(live), imp / len(live)
        perm_idx[u] = best
    has = np.asarray([any(G[u, i, i] != 0.0 for i in range(C)) for u in range(B)])
    mean2 = per_utt[has].mean(axis=0) if has.any() else np.zeros(2)
    return per_utt, perm_idx, mean2


def si_sdr(S_ref, E, window, stride, dtype=np.float64):
    '''references and (unpermuted) estimates complex [B, C, T, F] -> (per_utt, perm_idx, mean2).  dtype
    float32: the synthesis in single precision (the Gram matrix and the finalize step stay float64, as in
    the library)'''
    X = np.concatenate([np.asarray(S_ref), np.asarray(E)], axis=1)
    wav = synth(X, window, stride, dtype)
    return finalize(gram(wav), np.asarray(S_ref).shape[1])
