'''
Restatement of the noisy-evaluation metric (include/danet_neval_hip.h, THE RULE) in numpy float64, written from the
rule and independently of csrc/neval/neval.hip, on top of tests/metric_ref.py (synth, gram_fsum, sdr): the noise row
with its float32 pre-rounding, the finalize step with the baseline of the mixture the model was given, the metric end
to end, and a DIRECT form of the baseline -- synthesise the float64 mixture `sum of the references + noise` and take
its SI-SDR against every reference -- that the linear form is checked against.
'''
import itertools
import math

import numpy as np

import metric_ref as MR

MAX_C = 4


def scaled_noise(noise, gain=None):
    '''complex64 [B, T, F]: (fl(g re), fl(g im)), each product rounded on its own to float32; gain None: g = 1'''
    Z = np.asarray(noise).astype(np.complex64)
    if gain is None:
        return Z
    g = np.asarray(gain, dtype=np.float32).reshape(-1, 1, 1)
    out = np.empty_like(Z)
    out.real = (g * Z.real).astype(np.float32)
    out.imag = (g * Z.imag).astype(np.float32)
    return out


def synth(S_ref, E, noise, gain, window, stride, dtype=np.float64):
    '''-> wav [B, 2C + 1, Ls]: references, estimates, the scaled noise'''
    X = np.concatenate([np.asarray(S_ref), np.asarray(E), scaled_noise(noise, gain)[:, None]], axis=1)
    return MR.synth(X, window, stride, dtype)


def nsnr(cc, nn):
    if not cc > 0:
        return -100.0
    if not nn > 0:
        return 100.0
    return min(100.0, max(-100.0, 10.0 * math.log10(cc / nn)))


def perm_sums(g, C):
    '''the sums the permutation search compares, in itertools.permutations order (None: no live reference)'''
    live = [i for i in range(C) if g[i][i] != 0.0]
    if not live:
        return None, live, {}
    s = {(i, j): MR.sdr(g[i][i], g[C + j][C + j], g[i][C + j]) for i in live for j in range(C)}
    sums = []
    for perm in itertools.permutations(range(C)):
        v = 0.0
        for i in live:
            v += s[i, perm[i]]
        sums.append(v)
    return sums, live, s


def finalize(G, C):
    '''G [B, 2C + 1, 2C + 1] -> (per_utt [B, 3], perm_idx [B], mean3 [3])'''
    G = np.asarray(G, dtype=np.float64)
    B, M, n = G.shape[0], 2 * C + 1, 2 * C
    assert G.shape == (B, M, M) and 1 <= C <= MAX_C
    perms = list(itertools.permutations(range(C)))
    per_utt, perm_idx = np.zeros((B, 3)), np.zeros(B, np.int32)
    has = np.zeros(B, bool)
    for u in range(B):
        g = [[float(v) for v in row] for row in G[u]]
        sums, live, s = perm_sums(g, C)
        if not live:
            continue
        has[u] = True
        cc = 0.0
        for k in range(C):
            for l in range(C):
                cc += g[k][l]
        cn = 0.0
        for k in range(C):
            cn += g[k][n]
        nn = g[n][n]
        mm = (cc + 2.0 * cn) + nn
        best, best_v = 0, None
        for p, v in enumerate(sums):
            if best_v is None or v > best_v:            # ties: the first permutation
                best, best_v = p, v
        imp = 0.0
        for i in live:
            ms = 0.0
            for k in range(C):
                ms += g[k][i]
            imp += s[i, perms[best][i]] - MR.sdr(g[i][i], mm, ms + g[n][i])
        per_utt[u] = best_v / len(live), imp / len(live), nsnr(cc, nn)
        perm_idx[u] = best
    mean3 = per_utt[has].mean(axis=0) if has.any() else np.zeros(3)
    return per_utt, perm_idx, mean3


def perm_margin(G, C):
    '''per utterance: best minus second-best permutation sum, dB (inf with one permutation or no live reference)'''
    out = []
    for g in np.asarray(G, dtype=np.float64):
        sums = perm_sums([[float(v) for v in row] for row in g], C)[0]
        if sums is None or len(sums) < 2:
            out.append(float('inf'))
            continue
        top = sorted(sums, reverse=True)
        out.append(top[0] - top[1])
    return np.asarray(out)


def si_sdr_noisy(S_ref, E, noise, gain, window, stride, dtype=np.float64, fsum=False):
    '''-> (per_utt [B, 3], perm_idx [B], mean3 [3]).  dtype float32: the synthesis in single precision'''
    wav = synth(S_ref, E, noise, gain, window, stride, dtype)
    G = MR.gram_fsum(wav) if fsum else MR.gram(wav)
    return finalize(G, np.asarray(S_ref).shape[1])


def baseline_direct(S_ref, noise, gain, window, stride):
    '''base [B, C] the DIRECT way: the float64 mixture spectra sum_c S_c + fl(g Z) synthesised as ONE signal, and
    its SI-SDR against every reference's waveform (nan for a silent reference)'''
    S_ref = np.asarray(S_ref).astype(np.complex128)
    B, C = S_ref.shape[:2]
    mix = S_ref.sum(axis=1) + scaled_noise(noise, gain).astype(np.complex128)
    wm = MR.synth(mix, window, stride)
    ws = MR.synth(S_ref, window, stride)
    out = np.full((B, C), np.nan)
    for b in range(B):
        for i in range(C):
            a = math.fsum(ws[b, i] * ws[b, i])
            if a != 0.0:
                out[b, i] = MR.sdr(a, math.fsum(wm[b] * wm[b]), math.fsum(wm[b] * ws[b, i]))
    return out


def baseline_linear(G, C):
    '''base [B, C] by the rule's linear form from Gram matrices [B, 2C + 1, 2C + 1] (nan for a silent reference)'''
    G = np.asarray(G, dtype=np.float64)
    n = 2 * C
    out = np.full((G.shape[0], C), np.nan)
    for u, g in enumerate(G):
        cc = 0.0
        for k in range(C):
            for l in range(C):
                cc += float(g[k][l])
        cn = 0.0
        for k in range(C):
            cn += float(g[k][n])
        mm = (cc + 2.0 * cn) + float(g[n][n])
        for i in range(C):
            if g[i][i] != 0.0:
                ms = 0.0
                for k in range(C):
                    ms += float(g[k][i])
                out[u, i] = MR.sdr(float(g[i][i]), mm, ms + float(g[n][i]))
    return out
