'''
Float64 numpy restatements of THE RULE of include/danet_bss_hip.h (BSS-eval v3 bss_eval_sources with an L-tap
distortion filter), two independent ones:

  (a) `evaluate_literal`: the literal one -- explicit matrices of delayed references, np.linalg.lstsq, the
      projections s_target, e_interf, e_artif in the time domain (Ls + L - 1 samples) and their energies;
  (b) `evaluate`: the quadratic-form one -- lagged correlations, the block-Toeplitz G and its diagonal blocks,
      scipy.linalg.cho_factor / cho_solve, pall = D^T G^-1 D and st = D_i^T G_ii^-1 D_i;

and what both share: the clamp q, the silent-reference rule, the permutation (the largest sum of SIR over the live
references, ties to the first in itertools.permutations order), the flags and the batch means.  The pieces of (b) are
exported one by one (correlations, systems, solve, finalize) so that a GPU test can restate one stage from the
kernel's own output of the stage before.
'''
import itertools
import math

import numpy as np
import scipy.linalg

MAX_C, MAX_L, MAX_N, MAX_RHS, MAX_BATCH, BLOCK = 4, 512, 2048, 16, 65535, 64
FLAG_PIVOT, FLAG_SILENT = 1, 2


def round256(n):
    return (n + 255) & ~255


def workspace_bytes(B, C, L):
    n = C * L
    parts = [B * C * C * (2 * L - 1) * 8, B * C * C * L * 8, B * C * 8, B * n * n * 8, B * C * L * L * 8, B * C * n * 8,
             B * C * (C + 1) * L * 8, B * 4, B * C * 4, B * 4 * 8, B * 4, B * 4, 4 * 8]
    return sum(round256(p) for p in parts)


def q(a, b):
    '''-100 when a <= 0; +100 when b <= 0 (and a > 0); else 10 log10(a / b) clamped to [-100, 100]'''
    if not a > 0.0:
        return -100.0
    if not b > 0.0:
        return 100.0
    return float(min(100.0, max(-100.0, 10.0 * math.log10(a / b))))


def lagged(x, y, L):
    '''r[tau + L - 1] = sum_n x[n] y[n + tau], |tau| < L, both zero outside their Ls samples (float64)'''
    Ls = len(x)
    full = np.correlate(np.asarray(y, np.float64), np.asarray(x, np.float64), 'full')     # lag tau at index tau + Ls - 1
    out = np.zeros(2 * L - 1)
    for tau in range(-(L - 1), L):
        if abs(tau) < Ls:
            out[tau + L - 1] = full[tau + Ls - 1]
    return out


def correlations(wav, L):
    '''wav [2C, Ls] (references first) -> R [C, C, 2L - 1], D [C, C, L] (D[j, i] = D_ji), ee [C]; R_ki mirrored from
    R_ik, i <= k, as the kernel does'''
    wav = np.asarray(wav, np.float64)
    C = wav.shape[0] // 2
    R = np.zeros((C, C, 2 * L - 1))
    D = np.zeros((C, C, L))
    for i in range(C):
        for k in range(i, C):
            r = lagged(wav[i], wav[k], L)
            if i == k:
                r[:L - 1] = r[L:][::-1]
            R[i, k] = r
            R[k, i] = r[::-1]
        for j in range(C):
            D[j, i] = lagged(wav[i], wav[C + j], L)[L - 1:]
    ee = np.array([np.dot(wav[C + j], wav[C + j]) for j in range(C)])
    return R, D, ee


def live_refs(R):
    L = (R.shape[2] + 1) // 2
    return [bool(R[i, i, L - 1] != 0.0) for i in range(R.shape[0])]


def systems(R, D):
    '''-> G [CL, CL], Gs [C, L, L], Xg [C, CL], Xs [C, C + 1, L]: copies of R and D (and the ascending-k baseline sum,
    started from 0.0), identity rows / columns and zero right-hand sides for a silent reference'''
    C, L = D.shape[0], D.shape[2]
    live = live_refs(R)
    t = np.arange(L)
    lag = t[:, None] - t[None, :] + L - 1
    G = np.zeros((C * L, C * L))
    Gs = np.zeros((C, L, L))
    Xg = np.zeros((C, C * L))
    Xs = np.zeros((C, C + 1, L))
    for i in range(C):
        Gs[i] = R[i, i][lag] if live[i] else np.eye(L)
        for k in range(C):
            if live[i] and live[k]:
                G[i * L:(i + 1) * L, k * L:(k + 1) * L] = R[i, k][lag]
            elif i == k:
                G[i * L:(i + 1) * L, k * L:(k + 1) * L] = np.eye(L)
        if live[i]:
            for j in range(C):
                Xg[j, i * L:(i + 1) * L] = D[j, i]
                Xs[i, j] = D[j, i]
            m = np.zeros(L)
            for k in range(C):
                m = m + R[i, k, L - 1:]
            Xs[i, C] = m
    return G, Gs, Xg, Xs


def chol_solve(A, X):
    '''A [n, n], X [nrhs, n] -> (solutions [nrhs, n], flag): flag 1 when the factorisation meets a pivot that is not
    a positive finite number (LinAlgError / non-finite), the solutions then meaningless'''
    try:
        c = scipy.linalg.cho_factor(A, lower=True, check_finite=False)
        if not np.all(np.isfinite(np.diag(c[0]))) or not np.all(np.diag(c[0]) > 0):
            return np.zeros_like(X), 1
        return scipy.linalg.cho_solve(c, X.T, check_finite=False).T, 0
    except np.linalg.LinAlgError:
        return np.zeros_like(X), 1


def backward_error(A, x, b):
    '''the normwise backward error  ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf)  of one right-hand side'''
    r = np.abs(b - A @ x).max()
    return float(r / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def search(sir, live):
    '''(index, permutation) of the first permutation in itertools.permutations order with the largest sum of
    sir[i][p[i]] over the live i, added in ascending i; (0, identity) when nothing is live'''
    C = len(live)
    best, best_v, best_p = 0, 0.0, tuple(range(C))
    if not any(live):
        return best, best_p
    for n, p in enumerate(itertools.permutations(range(C))):
        v = 0.0
        for i in range(C):
            if live[i]:
                v += sir[i][p[i]]
        if n == 0 or v > best_v:
            best, best_v, best_p = n, v, p
    return best, best_p


def scores(st, stm, pall, ee, mm, live, flag=0):
    '''st [C, C] (st[i][j]), stm [C], pall [C], ee [C], mm -> (per_utt [4], perm_idx, flags): the table, the search and
    the means over the live references'''
    C = len(live)
    flags = (FLAG_PIVOT if flag else 0) | (0 if any(live) else FLAG_SILENT)
    if flags:
        return np.zeros(4), 0, flags
    sdr = [[q(st[i][j], ee[j] - st[i][j]) for j in range(C)] for i in range(C)]
    sir = [[q(st[i][j], pall[j] - st[i][j]) for j in range(C)] for i in range(C)]
    sar = [q(pall[j], ee[j] - pall[j]) for j in range(C)]
    base = [q(stm[i], mm - stm[i]) for i in range(C)]
    idx, p = search(sir, live)
    out = np.zeros(4)
    for i in range(C):
        if live[i]:
            out += [sdr[i][p[i]], sir[i][p[i]], sar[p[i]], sdr[i][p[i]] - base[i]]
    return out / sum(live), idx, flags


def finalize(R, D, ee, Xg, Xs, fg=0, fs=0):
    '''the decibels from the correlations, the right-hand sides and the SOLUTIONS Xg, Xs (restatement (b)'s last
    stage, and the restatement of danet_bss_finalize from the kernel's own solutions)'''
    C, L = D.shape[0], D.shape[2]
    live = live_refs(R)
    mm = 0.0
    for i in range(C):
        for k in range(C):
            mm += R[i, k, L - 1]
    pall = [float(np.dot(D[j].reshape(-1), Xg[j])) for j in range(C)]
    st = [[float(np.dot(D[j, i], Xs[i, j])) for j in range(C)] for i in range(C)]
    stm = []
    for i in range(C):
        m = np.zeros(L)
        for k in range(C):
            m = m + R[i, k, L - 1:]
        stm.append(float(np.dot(m, Xs[i, C])))
    return scores(st, stm, pall, ee, mm, live, flag=int(bool(fg) or bool(np.any(fs))))


def evaluate(wav, L, with_cond=False):
    '''restatement (b) of one utterance: wav [2C, Ls] -> (per_utt [4], perm_idx, flags[, cond(G)])'''
    R, D, ee = correlations(wav, L)
    G, Gs, Xg, Xs = systems(R, D)
    C = D.shape[0]
    Xg, fg = chol_solve(G, Xg)
    fs = 0
    Xs = Xs.copy()
    for i in range(C):
        Xs[i], f = chol_solve(Gs[i], Xs[i])
        fs |= f
    out = finalize(R, D, ee, Xg, Xs, fg, fs)
    return out + (float(np.linalg.cond(G)),) if with_cond else out


def _delays(x, L):
    '''[Ls + L - 1, L]: column t is x delayed by t samples'''
    Ls = len(x)
    M = np.zeros((Ls + L - 1, L))
    for t in range(L):
        M[t:t + Ls, t] = x
    return M


def _project(A, y):
    return A @ np.linalg.lstsq(A, y, rcond=None)[0]


def evaluate_literal(wav, L, with_table=False):
    '''restatement (a) of one utterance: time-domain least squares.  -> (per_utt [4], perm_idx, flags); with_table:
    also (sdr, sir, sar) as nested lists over (i, j) / j'''
    wav = np.asarray(wav, np.float64)
    C, Ls = wav.shape[0] // 2, wav.shape[1]
    live = [bool(np.dot(wav[i], wav[i]) != 0.0) for i in range(C)]
    if not any(live):
        return (np.zeros(4), 0, FLAG_SILENT) + (((), (), ()),) * with_table
    blocks = [_delays(wav[i], L) for i in range(C)]
    A = np.concatenate(blocks, axis=1)
    pad = np.zeros(L - 1)
    sdr = [[0.0] * C for _ in range(C)]
    sir = [[0.0] * C for _ in range(C)]
    sar = [0.0] * C
    for j in range(C):
        y = np.concatenate([wav[C + j], pad])
        p_all = _project(A, y)
        e_artif = y - p_all
        sar[j] = q(float(p_all @ p_all), float(e_artif @ e_artif))
        for i in range(C):
            if not live[i]:
                continue
            s_target = _project(blocks[i], y)
            e_interf = p_all - s_target
            rest = e_interf + e_artif
            sdr[i][j] = q(float(s_target @ s_target), float(rest @ rest))
            sir[i][j] = q(float(s_target @ s_target), float(e_interf @ e_interf))
    m = np.concatenate([wav[:C].sum(axis=0), pad])
    base = [0.0] * C
    for i in range(C):
        if live[i]:
            s_target = _project(blocks[i], m)
            rest = m - s_target
            base[i] = q(float(s_target @ s_target), float(rest @ rest))
    idx, p = search(sir, live)
    out = np.zeros(4)
    for i in range(C):
        if live[i]:
            out += [sdr[i][p[i]], sir[i][p[i]], sar[p[i]], sdr[i][p[i]] - base[i]]
    res = (out / sum(live), idx, 0)
    return res + ((sdr, sir, sar),) if with_table else res


def batch_mean(per_utt, flags):
    '''mean4 over the utterances with flags = 0, or zeros'''
    per_utt, flags = np.asarray(per_utt, np.float64), np.asarray(flags)
    keep = flags == 0
    return per_utt[keep].mean(axis=0) if keep.any() else np.zeros(4)


def evaluate_batch(wav, L, literal=False):
    '''wav [B, 2C, Ls] -> (mean4, per_utt [B, 4], perm_idx [B], flags [B])'''
    rows = [(evaluate_literal if literal else evaluate)(w, L) for w in wav]
    per_utt = np.stack([r[0] for r in rows])
    flags = np.array([r[2] for r in rows], np.int32)
    return batch_mean(per_utt, flags), per_utt, np.array([r[1] for r in rows], np.int32), flags


def make_case(C, Ls, L, seed, B=1, noise=0.3, leak=0.3):
    '''float32 wav [B, 2C, Ls]: white references; estimate j = reference j through a 3-tap filter + the other
    references through drawn 5-tap filters * leak + white noise * noise'''
    rng = np.random.RandomState(seed)
    out = np.zeros((B, 2 * C, Ls), np.float32)
    for b in range(B):
        refs = rng.standard_normal((C, Ls)).astype(np.float32).astype(np.float64)
        h = rng.standard_normal((C, C, 5)) * 0.3
        for j in range(C):
            e = np.convolve(refs[j], [1.0, 0.5, 0.2])[:Ls] + noise * rng.standard_normal(Ls)
            for k in range(C):
                if k != j:
                    e = e + leak * np.convolve(refs[k], h[j, k])[:Ls]
            out[b, C + j] = e
        out[b, :C] = refs
    return out
