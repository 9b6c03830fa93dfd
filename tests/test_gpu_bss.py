'''
GPU tests (run with -m gpu) of the BSS-eval figures (EVAL_BSS_SDR): the kernels of libdanet_bss_hip.so through ops,
stage by stage, against the float64 restatements of tests/bss_ref.py; every output between poisoned guard bands and
every kernel run twice for bit-identical repeats; then ops.bss_eval from spectra, Model.valid_step and the command line
at the shape of smoke().

Bars.
  xcorr:      every entry within 1e-9 * sqrt(R_ii[0] R_kk[0]) (for D: sqrt(R_ii[0] ee_j); for ee: ee_j) of math.fsum of
              the float64 products -- the Gram kernel's bar, the same kind of sum.
  chol_solve: the normwise backward error eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf) of every right-hand side
              is at most 4 x the eta scipy.linalg.cho_solve reaches on the same system (computed here), floor n 2^-53:
              the factor 4 allows for the different summation order of a blocked update.
  systems:    bit for bit the restatement built from the kernel's own R and D.
  decibels:   max(1e-9, 100 x the largest |(a) - (b)| of the same case) dB, (a) and (b) the two float64 restatements;
              where (a) is too large to run ((1, 2, 8128, 512)) the largest over the smaller cases.  Two float64
              computations of one quantity set the noise floor, the 100 covers the different tree.
The estimates of those cases are filtered references + leakage + noise, so that the restatement alone shows SDR, SIR,
SAR within [-30, 60] dB and cond(G) <= 1e6, asserted before the kernel is looked at.  With ONE reference SIR is +100
by definition (nothing interferes: pall = st exactly in both restatements and in the kernel), so at (1, 1, 40, 1) SIR
is asserted to be exactly 100 on all sides instead.

Measured on an MI355X (this file's prints; also in README, "BSS-eval SDR / SIR / SAR in `valid` / `test`"): xcorr worst
1.9e-15 of sqrt(R_ii[0] R_kk[0]); chol_solve eta 4.7e-17 .. 8.5e-17 where scipy reaches 3.0e-17 .. 9.0e-17; decibels
worst 2.1e-13 dB against (b) (at (1, 2, 8128, 512)) where (a) and (b) differ by up to 5.0e-14 dB.
'''
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg
import torch

import bss_ref as BR
import prep_ref as P
from gpu_helpers import ROOT

pytestmark = pytest.mark.gpu

POISON = -7.25e33
IPOISON = -1234567
GUARD = 1024
E2E = [(1, 1, 40, 1), (3, 2, 300, 8), (2, 3, 200, 16), (2, 4, 120, 4), (2, 2, 2000, 64), (1, 2, 8128, 512)]
LITERAL_MAX = 2000 * 2 * 64          # Ls * C * L up to which restatement (a) is run


def _guarded(shape, dtype=torch.float64, poison=POISON):
    '''(whole buffer, the view of `shape` in its middle): everything poisoned'''
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, poison=POISON):
    return bool((buf[:GUARD] == poison).all()) and bool((buf[-GUARD:] == poison).all())


def _bits(t):
    a = t.detach().cpu().contiguous()
    return a.numpy().view({4: np.uint32, 8: np.uint64}[a.element_size()]).copy()


def _wav(B, C, Ls, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((B, 2 * C, Ls)) * rng.uniform(0.5, 2.0, (B, 2 * C, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------- xcorr
def _fsum_lagged(x, y, L, taus):
    '''{tau: math.fsum of x[n] * y[n + tau]} in float64, both zero outside their samples'''
    Ls = len(x)
    out = {}
    for tau in taus:
        if abs(tau) >= Ls:
            out[tau] = 0.0
        elif tau >= 0:
            out[tau] = math.fsum(x[:Ls - tau] * y[tau:])
        else:
            out[tau] = math.fsum(x[-tau:] * y[:Ls + tau])
    return out


def _xcorr(wav, L):
    from danet_amd import ops
    B, M, Ls = wav.shape
    C = M // 2
    bufs = [_guarded((B, C, C, 2 * L - 1)), _guarded((B, C, C, L)), _guarded((B, C))]
    outs = tuple(v for _, v in bufs)
    ops.bss_xcorr(wav, L, out=outs)
    torch.cuda.synchronize()
    first = [_bits(v) for v in outs]
    for _, v in bufs:
        v.fill_(POISON)
    ops.bss_xcorr(wav, L, out=outs)
    torch.cuda.synchronize()
    for f, v in zip(first, outs):
        assert np.array_equal(f, _bits(v))                   # bit-identical repeats
    assert all(_guards_intact(b) for b, _ in bufs)
    return outs


@pytest.mark.parametrize('B,C', [(1, 1), (3, 2), (2, 4)])
@pytest.mark.parametrize('L', [1, 2, 31, 32, 33, 512])
@pytest.mark.parametrize('Ls', [1, 2, 63, 64, 65, 257, 4097])
def test_xcorr_against_fsum(Ls, L, B, C):
    wav_h = _wav(B, C, Ls, seed=Ls * 1000 + L * 10 + C)
    R, D, ee = (t.cpu().numpy() for t in _xcorr(torch.from_numpy(wav_h).cuda(), L))
    w = wav_h.astype(np.float64)
    worst = 0.0
    for b in range(B):
        e0 = [math.fsum(w[b, m] * w[b, m]) for m in range(2 * C)]
        for j in range(C):
            assert abs(ee[b, j] - e0[C + j]) <= 1e-9 * e0[C + j]
        for i in range(C):
            # R_ii and the mirrored halves: symmetric bit for bit
            assert np.array_equal(R[b, i, i].view(np.uint64), R[b, i, i][::-1].copy().view(np.uint64))
            for k in range(C):
                assert np.array_equal(R[b, k, i].view(np.uint64), R[b, i, k][::-1].copy().view(np.uint64))
            for k in range(i, C):
                ref = _fsum_lagged(w[b, i], w[b, k], L, range(-(L - 1), L))
                ref = np.array([ref[t] for t in range(-(L - 1), L)])
                err = np.abs(R[b, i, k] - ref).max() / math.sqrt(e0[i] * e0[k])
                worst = max(worst, err)
                assert err <= 1e-9, (b, i, k, err)
            for j in range(C):
                ref = _fsum_lagged(w[b, i], w[b, C + j], L, range(L))
                ref = np.array([ref[t] for t in range(L)])
                err = np.abs(D[b, j, i] - ref).max() / math.sqrt(e0[i] * e0[C + j])
                worst = max(worst, err)
                assert err <= 1e-9, (b, j, i, err)
    print('xcorr Ls %d L %d B %d C %d: worst error %.3g of sqrt(R_ii[0] R_kk[0])' % (Ls, L, B, C, worst))


# ----------------------------------------------------------------------------------- chol_solve
@functools.lru_cache(maxsize=4)
def _spd(n, nmat):
    '''A = M M^T + I from float64 normal M, [nmat, n, n]; right-hand sides [nmat, 5, n]'''
    rng = np.random.RandomState(7 * n + nmat)
    M = rng.standard_normal((nmat, n, n))
    A = M @ M.transpose(0, 2, 1) + np.eye(n)
    A = 0.5 * (A + A.transpose(0, 2, 1))
    b = rng.standard_normal((nmat, 5, n))
    host = np.stack([scipy.linalg.cho_solve(scipy.linalg.cho_factor(A[m], lower=True), b[m].T).T for m in range(nmat)])
    A.setflags(write=False)
    b.setflags(write=False)
    host.setflags(write=False)
    return A, b, host


def _chol(A_h, b_h):
    from danet_amd import ops
    nmat, n = A_h.shape[:2]
    bufs = [_guarded(A_h.shape), _guarded(b_h.shape), _guarded((nmat,), torch.int32, IPOISON)]
    res = []
    for _ in range(2):
        bufs[0][1].copy_(torch.from_numpy(np.array(A_h)))
        bufs[1][1].copy_(torch.from_numpy(np.array(b_h)))
        bufs[2][1].fill_(IPOISON)
        ops.bss_chol_solve(bufs[0][1], bufs[1][1], bufs[2][1])
        torch.cuda.synchronize()
        res.append([_bits(v) for _, v in bufs])
    assert all(np.array_equal(a, b) for a, b in zip(*res))               # bit-identical repeats
    assert _guards_intact(bufs[0][0]) and _guards_intact(bufs[1][0]) and _guards_intact(bufs[2][0], IPOISON)
    return bufs[0][1].cpu().numpy(), bufs[1][1].cpu().numpy(), bufs[2][1].cpu().numpy()


@pytest.mark.parametrize('nmat', [1, 7])
@pytest.mark.parametrize('nrhs', [1, 3, 5])
@pytest.mark.parametrize('n', [1, 2, 15, 16, 17, 63, 64, 65, 127, 130, 1024])
def test_chol_solve_backward_error(n, nrhs, nmat):
    A, b, host = _spd(n, nmat)
    b, host = b[:, :nrhs], host[:, :nrhs]
    fac, x, flags = _chol(A, b)
    assert not flags.any()
    worst, worst_host = 0.0, 0.0
    for m in range(nmat):
        for r in range(nrhs):
            eta = BR.backward_error(A[m], x[m, r], b[m, r])
            eta_host = BR.backward_error(A[m], host[m, r], b[m, r])
            worst, worst_host = max(worst, eta), max(worst_host, eta_host)
            assert eta <= max(4.0 * eta_host, n * 2.0 ** -53), (m, r, eta, eta_host)
        # the factor: L in the lower triangle
        Lm = np.tril(fac[m])
        assert np.abs(Lm @ Lm.T - A[m]).max() <= 64 * n * 2.0 ** -53 * np.abs(A[m]).max()
    print('chol_solve n %d nrhs %d nmat %d: eta %.3g (scipy %.3g)' % (n, nrhs, nmat, worst, worst_host))


def test_chol_solve_at_the_largest_system():
    '''n = DANET_BSS_MAX_N (C = 4, L = 512): 32 panels, 496 tiles behind the first, the whole LDS vector of the solve'''
    n = BR.MAX_N
    A, b, host = _spd(n, 1)
    b, host = b[:, :4], host[:, :4]
    fac, x, flags = _chol(A, b)
    assert not flags.any()
    for r in range(4):
        eta, eta_host = BR.backward_error(A[0], x[0, r], b[0, r]), BR.backward_error(A[0], host[0, r], b[0, r])
        print('chol_solve n %d rhs %d: eta %.3g (scipy %.3g)' % (n, r, eta, eta_host))
        assert eta <= max(4.0 * eta_host, n * 2.0 ** -53), (r, eta, eta_host)


@pytest.mark.parametrize('n', [17, 130])
def test_a_negative_eigenvalue_sets_its_flag_and_leaves_the_others_exact(n):
    A, b, _ = _spd(n, 7)
    A, b = A[:3].copy(), b[:3, :3].copy()
    good = _chol(A, b)
    rng = np.random.RandomState(n)
    u = rng.standard_normal(n)
    u /= np.linalg.norm(u)
    bad = A.copy()
    bad[1] = A[1] - (u @ A[1] @ u + 1.0) * np.outer(u, u)               # u^T A u = -1: indefinite by construction
    bad[1] = 0.5 * (bad[1] + bad[1].T)
    assert np.linalg.eigvalsh(bad[1]).min() < -0.5
    fac, x, flags = _chol(bad, b)
    assert flags.tolist() == [0, 1, 0]
    for m in (0, 2):
        assert np.array_equal(x[m].view(np.uint64), good[1][m].view(np.uint64))
        assert np.array_equal(fac[m].view(np.uint64), good[0][m].view(np.uint64))
    assert good[2].tolist() == [0, 0, 0]


# -------------------------------------------------------------------------------------- systems
@pytest.mark.parametrize('B,C,Ls,L', [(1, 1, 40, 1), (3, 2, 300, 8), (2, 3, 200, 16), (2, 4, 120, 4), (1, 2, 90, 33)])
def test_systems_bit_for_bit(B, C, Ls, L):
    from danet_amd import ops
    wav_h = _wav(B, C, Ls, seed=B + C + L)
    if C > 1:
        wav_h[B - 1, 1] = 0.0                                # a silent reference
    wav = torch.from_numpy(wav_h).cuda()
    R, D, ee = ops.bss_xcorr(wav, L)
    n = C * L
    bufs = [_guarded((B, n, n)), _guarded((B, C, L, L)), _guarded((B, C, n)), _guarded((B, C, C + 1, L))]
    outs = tuple(v for _, v in bufs)
    ops.bss_systems(R, D, out=outs)
    torch.cuda.synchronize()
    first = [_bits(v) for v in outs]
    for v in outs:
        v.fill_(POISON)
    ops.bss_systems(R, D, out=outs)
    torch.cuda.synchronize()
    assert all(np.array_equal(f, _bits(v)) for f, v in zip(first, outs)) and all(_guards_intact(b) for b, _ in bufs)
    R_h, D_h = R.cpu().numpy(), D.cpu().numpy()
    for b in range(B):
        want = BR.systems(R_h[b], D_h[b])
        for name, got, ref in zip(('G', 'Gs', 'Xg', 'Xs'), outs, want):
            assert np.array_equal(got[b].cpu().numpy(), ref), (b, name)
        assert np.array_equal(want[0], want[0].T)            # G is symmetric bit for bit
    if C > 1:
        assert BR.live_refs(R_h[B - 1])[1] is False
        assert np.array_equal(outs[0][B - 1].cpu().numpy()[L:2 * L, L:2 * L], np.eye(L))
        assert not outs[3][B - 1, 1].any()


# ------------------------------------------------------------------ finalize and end to end from waveforms
@functools.lru_cache(maxsize=None)
def _case(B, C, Ls, L):
    '''the waveforms of a case and what the restatements alone say: (wav, (b), gap between (a) and (b) or None)'''
    wav = BR.make_case(C, Ls, L, seed=B * 1000 + C * 100 + L, B=B)
    mean_b, per_b, perm_b, flags_b = BR.evaluate_batch(wav, L)
    gap = None
    if Ls * C * L <= LITERAL_MAX:
        mean_a, per_a, perm_a, flags_a = BR.evaluate_batch(wav, L, literal=True)
        assert np.array_equal(perm_a, perm_b) and np.array_equal(flags_a, flags_b)
        gap = float(np.abs(per_a - per_b).max())
    # the recipe keeps the restatement itself honest: moderate figures, a well-conditioned system
    for b in range(B):
        R, D, ee = BR.correlations(wav[b], L)
        assert np.linalg.cond(BR.systems(R, D)[0]) <= 1e6
        sdr, sir, sar = _table_b(wav[b], L)
        figures = sdr + sar + (sir if C > 1 else [])
        assert all(-30.0 <= v <= 60.0 for v in figures), (B, C, Ls, L, figures)
        if C == 1:
            assert sir == [100.0]
    wav.setflags(write=False)
    return wav, (mean_b, per_b, perm_b, flags_b), gap


def _table_b(wav, L):
    '''(sdr, sir, sar) of restatement (b) over all (i, j) as flat lists'''
    R, D, ee = BR.correlations(wav, L)
    G, Gs, Xg, Xs = BR.systems(R, D)
    C = D.shape[0]
    xg = BR.chol_solve(G, Xg)[0]
    pall = [float(D[j].reshape(-1) @ xg[j]) for j in range(C)]
    sdr, sir = [], []
    for i in range(C):
        xs = BR.chol_solve(Gs[i], Xs[i])[0]
        for j in range(C):
            st = float(D[j, i] @ xs[j])
            sdr.append(BR.q(st, ee[j] - st))
            sir.append(BR.q(st, pall[j] - st))
    return sdr, sir, [BR.q(pall[j], ee[j] - pall[j]) for j in range(C)]


def _bar(gap):
    if gap is None:
        gap = max(_case(*c)[2] for c in E2E if c[2] * c[1] * c[3] <= LITERAL_MAX)
    return max(1e-9, 100.0 * gap)


def _pipeline(wav, L, group=None):
    '''the five stages through ops on `wav` [B, 2C, Ls] -> (mean4, per_utt, perm_idx, flags, stage outputs)'''
    from danet_amd import ops
    B, C = wav.shape[0], wav.shape[1] // 2
    R, D, ee = ops.bss_xcorr(wav, L)
    G, Gs, Xg, Xs = ops.bss_systems(R, D)
    fg = ops.bss_chol_solve(G, Xg)
    fs = ops.bss_chol_solve(Gs.view(B * C, L, L), Xs.view(B * C, C + 1, L)).view(B, C)
    bufs = [_guarded((B, 4)), _guarded((B,), torch.int32, IPOISON), _guarded((B,), torch.int32, IPOISON), _guarded((4,))]
    outs = tuple(v for _, v in bufs)
    ops.bss_finalize(R, D, ee, Xg, Xs, fg, fs, out=outs)
    torch.cuda.synchronize()
    first = [_bits(v) for v in outs]
    ops.bss_finalize(R, D, ee, Xg, Xs, fg, fs, out=outs)
    torch.cuda.synchronize()
    assert all(np.array_equal(f, _bits(v)) for f, v in zip(first, outs))
    assert _guards_intact(bufs[0][0]) and _guards_intact(bufs[3][0])
    assert _guards_intact(bufs[1][0], IPOISON) and _guards_intact(bufs[2][0], IPOISON)
    per_utt, perm_idx, flags, mean4 = (v.cpu().numpy() for v in outs)
    return mean4, per_utt, perm_idx, flags, (R, D, ee, Xg, Xs, fg, fs)


@pytest.mark.parametrize('B,C,Ls,L', E2E)
def test_end_to_end_from_waveforms(B, C, Ls, L):
    wav_h, (mean_b, per_b, perm_b, flags_b), gap = _case(B, C, Ls, L)
    bar = _bar(gap)
    mean4, per_utt, perm_idx, flags, stages = _pipeline(torch.from_numpy(np.array(wav_h)).cuda(), L)
    worst = float(np.abs(per_utt - per_b).max())
    print('end to end B %d C %d Ls %d L %d: worst |kernel - (b)| %.3g dB, |(a) - (b)| %s dB, bar %.3g dB'
          % (B, C, Ls, L, worst, 'not run' if gap is None else '%.3g' % gap, bar))
    assert np.array_equal(perm_idx, perm_b) and np.array_equal(flags, flags_b) and not flags.any()
    assert worst <= bar
    assert np.abs(mean4 - mean_b).max() <= bar
    # finalize alone: the restatement of the last stage from the kernel's own correlations and solutions
    R, D, ee, Xg, Xs, fg, fs = (t.cpu().numpy() for t in stages)
    for b in range(B):
        per, idx, fl = BR.finalize(R[b], D[b], ee[b], Xg[b], Xs[b], fg[b], fs[b])
        assert idx == perm_idx[b] and fl == flags[b] and np.abs(per - per_utt[b]).max() <= 1e-9
    assert np.abs(BR.batch_mean(per_utt, flags) - mean4).max() <= 1e-12 * max(1.0, np.abs(per_utt).max())


def test_finalize_ties_clamps_silence_and_a_flagged_utterance():
    from danet_amd import ops
    B, C, L = 6, 2, 3
    rng = np.random.RandomState(11)
    R = np.zeros((B, C, C, 2 * L - 1))
    D = rng.uniform(0.5, 1.5, (B, C, C, L))
    Xg = rng.uniform(0.5, 1.5, (B, C, C * L))
    Xs = rng.uniform(0.1, 0.3, (B, C, C + 1, L))
    ee = np.full((B, C), 50.0)
    R[:, 0, 0, L - 1] = 30.0
    R[:, 1, 1, L - 1] = 20.0
    R[:, 0, 1] = R[:, 1, 0] = 0.5
    fg = np.zeros(B, np.int32)
    fs = np.zeros((B, C), np.int32)
    R[1] = 0.0                                               # 1: all silent
    fg[2] = 1                                                # 2: the big system failed
    fs[3, 1] = 1                                             # 3: a small system failed
    D[4], Xg[4], Xs[4] = 1.0, 0.25, 0.125                    # 4: every entry of the table equal: a tie -> perm 0
    D[5, 0] = 0.0                                            # 5: estimate 0 has no target part: -100s
    ee[5, 1] = float(D[5, 1, 1] @ Xs[5, 1, 1])               #    and SDR(1, 1) = +100: ee - st = 0
    R[0, 1, 1] = 0.0                                         # 0: ONE silent reference
    dev = [torch.from_numpy(a).cuda() for a in (R, D, ee, Xg, Xs, fg, fs)]
    mean4, per_utt, perm_idx, flags = (t.cpu().numpy() for t in ops.bss_finalize(*dev))
    want = [BR.finalize(R[b], D[b], ee[b], Xg[b], Xs[b], fg[b], fs[b]) for b in range(B)]
    for b in range(B):
        assert np.abs(per_utt[b] - want[b][0]).max() <= 1e-9 and perm_idx[b] == want[b][1] and flags[b] == want[b][2], b
    assert flags.tolist() == [0, BR.FLAG_SILENT, BR.FLAG_PIVOT, BR.FLAG_PIVOT, 0, 0]
    assert not per_utt[1:4].any() and perm_idx[4] == 0
    assert want[5][0][0] <= 0.0 and abs(per_utt[5]).max() <= 100.0
    keep = np.array([0, 4, 5])
    assert np.abs(mean4 - per_utt[keep].mean(axis=0)).max() <= 1e-12           # the flagged and the silent left out
    # nothing to average: zeros
    mean4 = ops.bss_finalize(*[t[1:4].contiguous() for t in dev])[0].cpu().numpy()
    assert not mean4.any()
    # the batch in two calls: the means are formed by the last one, over all rows
    out = (torch.full((B, 4), POISON, dtype=torch.float64, device='cuda'),
           torch.full((B,), IPOISON, dtype=torch.int32, device='cuda'),
           torch.full((B,), IPOISON, dtype=torch.int32, device='cuda'),
           torch.full((4,), POISON, dtype=torch.float64, device='cuda'))
    ops.bss_finalize(*[t[:4].contiguous() for t in dev], b0=0, out=out)
    torch.cuda.synchronize()
    assert bool((out[3] == POISON).all()) and bool((out[0][4:] == POISON).all())
    got = ops.bss_finalize(*[t[4:].contiguous() for t in dev], b0=4, out=out)
    assert np.array_equal(_bits(got[1]), per_utt.view(np.uint64)) and np.array_equal(got[0].cpu().numpy().view(np.uint64),
                                                                                     ops.bss_finalize(*dev)[0].cpu().numpy().view(np.uint64))


# ------------------------------------------------------------------------------ from spectra
def _smoke_spectra():
    rng = np.random.RandomState(0)
    src = ((rng.randn(2, 2, 6, 33) + 1j * rng.randn(2, 2, 6, 33)) * 3).astype(np.complex64)
    est = (0.8 * src + 0.3 * src[:, ::-1] + 0.5 * (rng.randn(2, 2, 6, 33) + 1j * rng.randn(2, 2, 6, 33))).astype(np.complex64)
    return src, est


def test_bss_eval_from_spectra_and_its_groups(hp):
    from danet_amd import ops
    hp.load(dict(FFT_SIZE=64, FFT_STRIDE=16, MAX_N_SIGNAL=2, BATCH_SIZE=2))
    hp.digest()
    src_h, est_h = _smoke_spectra()
    src, est = torch.from_numpy(src_h).cuda(), torch.from_numpy(est_h).cuda()
    L = 8
    wav = ops.metric_synth(src, est, 16)
    whole = ops.bss_eval(src, est, filter_len=L, fft_stride=16)
    ones = ops.bss_eval(src, est, filter_len=L, fft_stride=16, group=1)
    given = ops.bss_eval(src, est, filter_len=L, wav=wav, group=2)
    torch.cuda.synchronize()
    for a, b, c in zip(whole, ones, given):
        assert np.array_equal(_bits(a.reshape(-1)), _bits(b.reshape(-1)))      # groups of 1 and of all: bit for bit
        assert np.array_equal(_bits(a.reshape(-1)), _bits(c.reshape(-1)))
    mean_b, per_b, perm_b, flags_b = BR.evaluate_batch(wav.cpu().numpy(), L)
    sdr, sir, sar, sdri, per_utt, perm_idx, flags = whole
    assert sdr.dtype == torch.float64 and sdr.dim() == 0 and per_utt.shape == (2, 4)
    got = np.array([float(sdr), float(sir), float(sar), float(sdri)])
    print('bss_eval from spectra: %s dB, restatement %s dB' % (got.round(6), mean_b.round(6)))
    assert np.isfinite(got).all() and np.abs(got - mean_b).max() <= _bar(None)
    assert np.abs(per_utt.cpu().numpy() - per_b).max() <= _bar(None)
    assert np.array_equal(perm_idx.cpu().numpy(), perm_b) and np.array_equal(flags.cpu().numpy(), flags_b)


# ---------------------------------------------------------------------------------------- model
_MODEL_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import __graft_entry__ as g
g.load_package()
import bss_ref as BR
from danet_amd import _lib, ops
from danet_amd.hparams import hparams
from danet_amd.model import Model
base = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
            NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
            INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig')
rng = np.random.RandomState(0)
src_h = ((rng.randn(2, 2, 6, 33) + 1j * rng.randn(2, 2, 6, 33)) * 3).astype(np.complex64)
src = torch.as_tensor(src_h).cuda()
res = {}
def run(tag, **keys):
    hparams.reset(); hparams.load(dict(base, **keys)); hparams.digest()
    model = Model('bss', device='cuda:0', seed=3).build()
    out = model.valid_step(src)
    torch.cuda.synchronize()
    res[tag] = {k: float(v) for k, v in out.items()}
    res[tag + '_hex'] = {k: float(v).hex() for k, v in out.items()}
    res[tag + '_keys'] = list(out)
    res[tag + '_mapped'] = 'libdanet_bss' in open('/proc/self/maps').read()
    return model
run('never')
run('null', EVAL_BSS_SDR=None, EVAL_BSS_FILTER_LEN=None)
run('false', EVAL_BSS_SDR=False)
run('si', EVAL_SI_SDR=True)
model = run('on', EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=8)
run('both', EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=8, EVAL_SI_SDR=True)
with torch.no_grad():
    o = model.forward(src, with_valid=True, with_train=False)
    est = ops.reattach_phase(o['sep_pwr_valid'], o['phasor'])
    wav = ops.metric_synth(src, est, 16).cpu().numpy()
torch.cuda.synchronize()
res['ok'] = bool(ops.lstm_status_ok())
res['ref'] = [float(v) for v in BR.evaluate_batch(wav, 8)[0]]
print('RESULT ' + json.dumps(res))
'''


def test_valid_step_with_the_keys_off_and_on():
    code = _MODEL_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split('RESULT ')[1])
    assert r['ok']
    for tag in ('never', 'null', 'false'):
        assert r[tag + '_keys'] == ['loss', 'SNR'] and not r[tag + '_mapped'], tag
        assert r[tag + '_hex'] == r['never_hex'], tag                 # bit for bit
    assert r['si_keys'] == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi'] and not r['si_mapped']
    assert r['on_keys'] == ['loss', 'SNR', 'SDR', 'SIR', 'SAR', 'SDRi'] and r['on_mapped']
    assert r['both_keys'] == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi', 'SDR', 'SIR', 'SAR', 'SDRi']
    assert all(np.isfinite(v) for v in r['on'].values()) and all(np.isfinite(v) for v in r['both'].values())
    for k in ('loss', 'SNR'):
        assert r['on_hex'][k] == r['never_hex'][k] == r['both_hex'][k] == r['si_hex'][k], k
    for k in ('SI-SDR', 'SI-SDRi'):
        assert r['both_hex'][k] == r['si_hex'][k], k                  # the shared synthesis changes nothing
    for k, ref in zip(('SDR', 'SIR', 'SAR', 'SDRi'), r['ref']):
        print('%s %.9f (float64 restatement %.9f)' % (k, r['on'][k], ref))
        assert abs(r['on'][k] - ref) <= _bar(None), (k, r['on'][k], ref)
        assert r['both_hex'][k] == r['on_hex'][k], k


# ------------------------------------------------------------------------------------------ CLI
def test_command_line_valid_prints_the_four_figures(tmp_path):
    P.write_tree(tmp_path / 'tree', seed=7, n_per_subset=8, subsets=('train', 'test'), seconds=(0.2, 0.4))
    cfg = dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2,
               LSTM_HDIM=8, NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
               INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64,
               DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'), EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=16)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'bss', '-m', 'valid', '-ds', 'wavdir',
                          '-c', str(path)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = out.stdout.split('Valid: ')[1].splitlines()[0]
    assert line.index('loss=') < line.index('SNR=') < line.index('SDR=') < line.index('SIR=') < line.index('SAR=') \
        < line.index('SDRi=')
    for k in (' SDR=', ' SIR=', ' SAR=', ' SDRi='):
        assert np.isfinite(float(line.split(k)[1].split()[0])), line
