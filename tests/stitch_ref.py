'''
The rule of include/danet_stitch_hip.h restated in numpy float64 (plan, affinity, assignment, merge), for the tests of
chunked inference (tests/test_stitch_cpu.py, tests/test_gpu_stitch.py).  Pure numpy: needs neither the library nor a
GPU.
'''
import itertools
import math

import numpy as np

MAX_C = 4
MAX_CHUNKS = 65536
TILE = 8192


def chunks(T, L, V):
    '''n of the plan (1 when T <= L)'''
    assert T >= 1 and L >= 2 and 1 <= V <= L // 2, (T, L, V)
    if T <= L:
        return 1
    H = L - V
    return 1 + -((L - T) // H)               # 1 + ceil((T - L) / H)


def plan(T, L, V):
    '''the chunk starts: s_i = i * H for i < n - 1, the last chunk slid back to end at T'''
    n = chunks(T, L, V)
    if n == 1:
        return [0]
    return [i * (L - V) for i in range(n - 1)] + [T - L]


def workspace_bytes(T, L, V, C, F):
    return (chunks(T, L, V) - 1) * (-(-(L * F) // TILE)) * C * C * 8


def owner(t, starts, L):
    '''the smallest i with t < e_i'''
    for i, s in enumerate(starts):
        if t < s + L:
            return i
    raise AssertionError(t)


def fade(V):
    '''w_k = (k + 1) / (V + 1) in float64, rounded once to float32'''
    return ((np.arange(V, dtype=np.float64) + 1.0) / (V + 1.0)).astype(np.float32)


def overlap_runs(mags, i, starts):
    '''(a [C, |O_i| * F], b [C, |O_i| * F]): the two factors of pair i's overlap, float32 as stored'''
    n, C, L, F = mags.shape
    hop = starts[i + 1] - starts[i]
    return mags[i, :, hop:, :].reshape(C, -1), mags[i + 1, :, :L - hop, :].reshape(C, -1)


def affinity(mags, T, V):
    '''S float64 [n - 1, C, C] by numpy float64 dot products (affinity_exact: the same by math.fsum, with the sum of
    the terms' magnitudes)'''
    n, C, L, F = mags.shape
    starts = plan(T, L, V)
    assert len(starts) == n
    S = np.zeros((n - 1, C, C))
    for i in range(n - 1):
        a, b = overlap_runs(mags, i, starts)
        S[i] = a.astype(np.float64) @ b.astype(np.float64).T
    return S


def affinity_exact(mags, T, V):
    '''(S, A): S[i][c][d] = math.fsum of the float64 products (each exact), A the same over their magnitudes'''
    n, C, L, F = mags.shape
    starts = plan(T, L, V)
    S, A = np.zeros((n - 1, C, C)), np.zeros((n - 1, C, C))
    for i in range(n - 1):
        a, b = overlap_runs(mags, i, starts)
        a, b = a.astype(np.float64), b.astype(np.float64)
        for c in range(C):
            for d in range(C):
                p = a[c] * b[d]
                S[i, c, d] = math.fsum(p)
                A[i, c, d] = math.fsum(np.abs(p))
    return S, A


def totals(Si):
    '''[sum_c S_i[c][p[c]] (ascending c) for p in itertools.permutations order]'''
    C = Si.shape[0]
    out = []
    for p in itertools.permutations(range(C)):
        t = 0.0
        for c in range(C):
            t += float(Si[c, p[c]])
        out.append(t)
    return out


def local_perm(Si):
    '''pi_i: the first permutation with the largest total'''
    t = totals(Si)
    best = 0
    for k in range(1, len(t)):
        if t[k] > t[best]:
            best = k
    return list(list(itertools.permutations(range(Si.shape[0])))[best])


def margin(Si):
    '''(best - runner-up) / max(|best|, tiny) of pair i's totals; inf with one channel'''
    t = sorted(totals(Si), reverse=True)
    if len(t) == 1:
        return float('inf')
    return (t[0] - t[1]) / max(abs(t[0]), 1e-300)


def chain(S):
    '''perm int32 [n, C]: P_0 = identity, P_{i+1}[c] = pi_i[P_i[c]]'''
    n1, C = S.shape[0], S.shape[1]
    P = [list(range(C))]
    for i in range(n1):
        pi = local_perm(S[i])
        P.append([pi[P[-1][c]] for c in range(C)])
    return np.asarray(P, np.int32)


def merge_mag(mags, perm, T, V, w=None):
    '''(mag float64 [C, T, F], a float32, b float32, faded bool [T]): the merged magnitudes with w_k the float32 table,
    the arithmetic in float64; a, b the two sources (b = a outside the fades)'''
    n, C, L, F = mags.shape
    starts = plan(T, L, V)
    w = fade(V) if w is None else w
    a = np.empty((C, T, F), np.float32)
    b = np.empty((C, T, F), np.float32)
    wt = np.zeros(T)
    faded = np.zeros(T, bool)
    for t in range(T):
        i = owner(t, starts, L)
        e = starts[i] + L
        for c in range(C):
            a[c, t] = mags[i, perm[i][c], t - starts[i]]
        if i < n - 1 and t >= e - V:
            faded[t] = True
            wt[t] = float(w[t - (e - V)])
            for c in range(C):
                b[c, t] = mags[i + 1, perm[i + 1][c], t - starts[i + 1]]
        else:
            b[:, t] = a[:, t]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return a64 + wt[None, :, None] * (b64 - a64), a, b, faded


def owner_phasor(phasor, T, V):
    '''phasor float32 [n, L, F, 2] -> the owner chunk's row for every frame, float32 [T, F, 2]'''
    n, L = phasor.shape[0], phasor.shape[1]
    starts = plan(T, L, V)
    out = np.empty((T,) + phasor.shape[2:], np.float32)
    for t in range(T):
        i = owner(t, starts, L)
        out[t] = phasor[i, t - starts[i]]
    return out


def stitch(mags, phasor, T, V):
    '''the whole rule -> dict(S, perm, mag [C, T, F] float64, a, b, faded, ph [T, F, 2], out complex128 [C, T, F])'''
    S = affinity(mags, T, V)
    perm = chain(S)
    mag, a, b, faded = merge_mag(mags, perm, T, V)
    ph = owner_phasor(phasor, T, V)
    out = mag * ph[None, :, :, 0].astype(np.float64) + 1j * (mag * ph[None, :, :, 1].astype(np.float64))
    return dict(S=S, perm=perm, mag=mag, a=a, b=b, faded=faded, ph=ph, out=out)


def cut(x, T, L, V):
    '''[..., T, F] -> the chunks of the plan, [n, ..., L, F]'''
    return np.stack([x[..., s:s + L, :] for s in plan(T, L, V)])
