'''
GPU tests (run with -m gpu) of the intelligibility figures (EVAL_STOI): the kernels of libdanet_stoi_hip.so through
ops, stage by stage, against the float64 restatement of tests/stoi_ref.py on the kernel's own inputs; outputs between
poisoned guard bands, every kernel run twice for bit-identical repeats; then ops.stoi_eval from spectra,
Model.valid_step and the command line.

Bars.
  resample: every output sample within (taps + 1) * 2^-24 * sum |h x| + 2^-126 of the float64 sum, taps the number of
            table entries that sample uses (the derived bound of test_gpu_speed.py); at 10 kHz a bit-identical copy.
  frames:   masks, k(.) and M EXACTLY, after the restatement alone has shown every frame energy at least 1e-6 dB
            from the threshold; the energies within 1e-12 of the loudest frame.
  bands, segments, end to end: the restatement is run in float32 numpy on the same cases and its worst deviation
            from float64 is measured (relative to each row's maximum: a row of T is one band of one signal, a row of
            d or of the final figures is one figure of one utterance); the bar is 4 times that deviation.
The test signals are AR(1) processes gated by a slow sine with a 60 dB floor, plus white noise for the estimates.

Measured on an MI355X (this file's prints; also in README, "STOI and ESTOI in `valid` / `test`"): resample worst 0.48 of
its bar; frames exact with the nearest energy 0.23 dB from the threshold; bands: float32 numpy 1.2e-7 .. 1.7e-7, kernel
at most 4.7e-16; segments: float32 numpy 7.8e-8 .. 1.2e-7, kernel at most 4.1e-16; end to end: float32 numpy
1.8e-7 .. 1.9e-6, figures equal to the restatement's to the printed six decimals.
'''
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prep_ref as P
import stoi_ref as SR
from gpu_helpers import ROOT

pytestmark = pytest.mark.gpu

POISON = -7.25e33
IPOISON = -1234567
GUARD = 1024
W = SR.window()


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


def _rowrel(got, want):
    '''the largest |got - want| of a row (the last axis) over that row's largest |want| (rows of zeros: absolute)'''
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not want.size:
        return 0.0
    top = np.abs(want).max(axis=-1, keepdims=True)
    return float((np.abs(got - want) / np.where(top > 0, top, 1.0)).max())


# ---------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize('smprate', [8000, 16000, 44100, 10000, 81900])
def test_resample_against_float64(smprate):
    '''81900 Hz is the rate with the longest table that fits (16381 entries): the launch with more than 64 KiB of LDS'''
    from danet_amd import ops
    U, D, H = SR.rate(smprate)
    t = ops.stoi_tables(smprate, torch.device('cuda', torch.cuda.current_device()))
    h32 = t['h'].cpu().numpy()
    assert (t['U'], t['D'], t['H']) == (U, D, H) and h32.dtype == np.float32 and len(h32) == 2 * H + 1
    assert np.array_equal(h32, SR.table(smprate).astype(np.float32)) and t['bins'] == SR.BAND_BINS
    assert np.array_equal(t['w'].cpu().numpy(), W)
    ang = -2 * np.pi * np.arange(256) / 512
    assert np.abs(t['tw'].cpu().numpy() - np.stack([np.cos(ang), np.sin(ang)], 1)).max() <= 1e-15
    worst, case = 0.0, 0
    shapes = [(B, C) for B in (1, 7) for C in (1, 2, 4)] if smprate != 81900 else [(2, 2)]
    for B, C in shapes:
        for Ls in (1, 2, 255, 256, 257, 4097, 8128):
            rng = np.random.RandomState(1000 * C + Ls + B)
            wav_h = (rng.standard_normal((B, 2 * C, Ls)) * rng.uniform(0.5, 2.0, (B, 2 * C, 1))).astype(np.float32)
            L10 = SR.out_len(Ls, U, D)
            rows = np.concatenate([wav_h, np.stack([SR.mixture(u[:C]) for u in wav_h])[:, None]], axis=1)
            want, taps, a = SR.resample(rows, U, D, H, h32, with_bound=True)
            bar = (taps + 1) * 2.0 ** -24 * a + 2.0 ** -126
            # every residue mod 4 of the input's address over the cases of a rate, all four at one shape
            for r in ((0, 1, 2, 3) if (B, C, Ls) in ((7, 2, 4097), (2, 2, 4097)) else (case % 4,)):
                holder = torch.zeros(wav_h.size + 4, dtype=torch.float32, device='cuda')
                wav = holder[r:r + wav_h.size].view(B, 2 * C, Ls)
                wav.copy_(torch.from_numpy(wav_h))
                assert (wav.data_ptr() // 4) % 4 == r
                buf, out = _guarded((B, 2 * C + 1, L10), torch.float32, POISON)
                got = ops.stoi_resample(wav, smprate, out=out)
                first = _bits(got)
                ops.stoi_resample(wav, smprate, out=out)
                torch.cuda.synchronize()
                assert _guards_intact(buf) and np.array_equal(first, _bits(out)), (B, C, Ls, r)
                g = out.cpu().numpy()
                if H == 0:
                    assert np.array_equal(g.view(np.uint32), rows.view(np.uint32)), (B, C, Ls)   # a bit-identical copy
                err = np.abs(g.astype(np.float64) - want)
                assert (err <= bar).all(), (smprate, B, C, Ls, r, float((err / bar).max()))
                worst = max(worst, float((err / bar).max()))
            case += 1
    # (the last row of `rows` is the float32 sum of the references: the mixture row is held to the same bar)
    print('resample %d Hz (U / D = %d / %d, %d entries): worst error %.3g of the bar' % (smprate, U, D, 2 * H + 1, worst))


# ------------------------------------------------------------------------------------------ frames
def _gated(rng, n, period, edges=False):
    x = SR.make_signal(rng, n, period).astype(np.float64)
    if edges:                                            # the first and the last frames far under the threshold
        x[:300] *= 1e-4
        x[-300:] *= 1e-4
    return x.astype(np.float32)


def _frames_case(L10, C, seed):
    rng = np.random.RandomState(seed)
    sig = np.zeros((3, 2 * C + 1, L10), np.float32)
    for b in range(3):
        for i in range(C):
            if (b + i) % 3 == 0:
                sig[b, i] = _gated(rng, L10, 1500 + 211 * i)
            elif (b + i) % 3 == 1:
                sig[b, i] = rng.standard_normal(L10)                 # no frame removed
            else:
                sig[b, i] = _gated(rng, L10, 2100, edges=True)
    if C > 1:
        sig[2, 1] = 0.0                                              # a silent reference
    sig[:, C:] = rng.standard_normal((3, C + 1, L10))                # the other rows are not looked at
    return sig


@pytest.mark.parametrize('L10,C', [(10160, 2), (10160, 4), (40000, 1), (255, 2), (256, 2), (383, 1), (384, 2), (385, 3)])
def test_frames_exactly(L10, C):
    from danet_amd import ops
    sig_h = _frames_case(L10, C, seed=L10 + C)
    nf = SR.num_frames(L10)
    assert nf == {255: 0, 256: 1, 383: 1, 384: 2, 385: 2}.get(L10, nf)
    n = max(nf, 1)
    ref = [[SR.kept(sig_h[b, i], W) for i in range(C)] for b in range(3)]
    # from the restatement alone: no frame energy within 1e-6 dB of its threshold
    margin = min(SR.margin_db(ref[b][i][2]) for b in range(3) for i in range(C))
    assert margin >= 1e-6, margin
    sig = torch.from_numpy(sig_h).cuda()
    bufs = [_guarded((3, C, n)), _guarded((3, C, n), torch.int32, IPOISON), _guarded((3, C, n), torch.int32, IPOISON),
            _guarded((3, C), torch.int32, IPOISON), _guarded((3, C))]
    got = ops.stoi_frames(sig, out=tuple(v for _, v in bufs))
    first = [_bits(g) for g in got]
    ops.stoi_frames(sig, out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    assert all(np.array_equal(a, _bits(g)) for a, g in zip(first, got))
    assert all(_guards_intact(buf, IPOISON if v.dtype == torch.int32 else POISON) for buf, v in bufs)
    E, mask, kidx, M, Emax = [g.cpu().numpy() for g in got]
    removed = []
    for b in range(3):
        for i in range(C):
            m, k, e = ref[b][i]
            assert M[b, i] == len(k) and np.array_equal(mask[b, i, :nf], m.astype(np.int32)), (b, i)
            assert np.array_equal(kidx[b, i, :len(k)], k) and not kidx[b, i, len(k):].any(), (b, i)
            top = e.max() if nf else 0.0
            assert np.abs(E[b, i, :nf] - e).max(initial=0.0) <= 1e-12 * top and abs(Emax[b, i] - top) <= 1e-12 * top
            removed.append((nf - len(k), bool(nf and not m[0]), bool(nf and not m[-1])))
    if nf == 0:
        assert not M.any() and not mask.any() and not E.any() and not Emax.any()
    if L10 >= 10160:
        assert any(r[0] == 0 for r in removed) and any(r[1] and r[2] for r in removed) and any(r[0] > 5 for r in removed)
        if C > 1:
            assert M[2, 1] == 0 and Emax[2, 1] == 0.0 and M[2, 0] > 0
    print('frames L10 %d C %d: nf %d, removed %s, margin %.3g dB' % (L10, C, nf, sorted(set(r[0] for r in removed)), margin))


# --------------------------------------------------------------------------------- bands and segments
# (name, nf, M): the kept frames are a seeded choice of M out of nf; 'all': every frame kept
BAND_CASES = [('M30', 78, 30), ('M31', 78, 31), ('M56', 78, 56), ('all', 40, 40), ('one', 1, 1)]


@functools.lru_cache(maxsize=None)
def _band_case(name):
    nf, M = {c[0]: c[1:] for c in BAND_CASES}[name]
    B, C, L10 = 2, 2, 128 * (nf - 1) + 256 + 77
    rng = np.random.RandomState(len(name) + nf + M)
    wav = np.stack([SR.make_case(C, L10, seed=10 * b + M) for b in range(B)])
    sig = np.concatenate([wav, np.stack([SR.mixture(u[:C]) for u in wav])[:, None]], axis=1)
    kidx = np.zeros((B, C, nf), np.int32)
    Ms = np.zeros((B, C), np.int32)
    for b in range(B):
        for i in range(C):
            m = M if (b, i) != (1, 1) or name == 'one' else max(M - 3, 0)      # the references differ in M
            k = np.sort(rng.choice(nf, m, replace=False))
            if name == 'M56' and (b, i) == (0, 0):
                k = np.arange(nf - m, nf)                                      # the last frame kept, the first not
            kidx[b, i, :m], Ms[b, i] = k, m
    T64 = np.zeros((B, C, C + 2, 15, nf))
    T32 = np.zeros((B, C, C + 2, 15, nf))
    for b in range(B):
        for i in range(C):
            k = kidx[b, i, :Ms[b, i]]
            for s, r in enumerate([i] + [C + j for j in range(C)] + [2 * C]):
                c = SR.compact(sig[b, r], W, k)
                T64[b, i, s, :, :len(k)] = SR.band_mags(c, W)
                T32[b, i, s, :, :len(k)] = SR.band_mags(c, W, dtype=np.float32)
    return sig.astype(np.float32), kidx, Ms, T64, T32


@pytest.mark.parametrize('name', [c[0] for c in BAND_CASES])
def test_bands_against_float64(name):
    from danet_amd import ops
    sig_h, kidx_h, M_h, T64, T32 = _band_case(name)
    B, C, nf = M_h.shape[0], M_h.shape[1], kidx_h.shape[2]
    dev32 = _rowrel(T32, T64)                                # the float32 restatement's own deviation
    bar = 4 * dev32
    sig, kidx, M = (torch.from_numpy(a).cuda() for a in (sig_h, kidx_h, M_h))
    buf, out = _guarded((B, C, C + 2, 15, nf))
    got = ops.stoi_bands(sig, kidx, M, out=out)
    first = _bits(got)
    ops.stoi_bands(sig, kidx, M, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(buf) and np.array_equal(first, _bits(out))
    T = out.cpu().numpy()
    err = _rowrel(T, T64)
    print('bands %s: kernel %.3g, float32 numpy %.3g of the row maximum (bar %.3g)' % (name, err, dev32, bar))
    assert dev32 > 0 and err <= bar
    for b in range(B):
        for i in range(C):
            assert not T[b, i, :, :, M_h[b, i]:].any()       # behind M: zeros, written
            assert T[b, i, :, :, :M_h[b, i]].min(initial=1.0) > 0
    # what only the device can see is clamped: wild M and k leave the guards alone
    wild_k = torch.from_numpy(np.where(kidx_h % 2 == 0, 1 << 30, -5).astype(np.int32)).cuda()
    ops.stoi_bands(sig, wild_k, torch.full_like(M, 1 << 30), out=out)
    ops.stoi_segments(out, torch.full_like(M, -7), nf)
    torch.cuda.synchronize()
    assert _guards_intact(buf) and bool(torch.isfinite(out).all())


def _segments_ref(T, Ms, dtype):
    B, C = Ms.shape
    d = np.zeros((B, C, C + 1, 2))
    for b in range(B):
        for i in range(C):
            for j in range(C + 1):
                d[b, i, j] = SR.segments(T[b, i, 0, :, :Ms[b, i]], T[b, i, 1 + j, :, :Ms[b, i]], dtype)
    return d


@pytest.mark.parametrize('name', ['M30', 'M31', 'M56', 'all', 'one', 'zeros'])
def test_segments_against_float64(name):
    '''on the bands kernel's own output; 'zeros': a band row of zeros in one signal and a constant row in another'''
    from danet_amd import ops
    sig_h, kidx_h, M_h, T64, _ = _band_case('M56' if name == 'zeros' else name)
    B, C, nf = M_h.shape[0], M_h.shape[1], kidx_h.shape[2]
    T = ops.stoi_bands(*(torch.from_numpy(a).cuda() for a in (sig_h, kidx_h, M_h)))
    if name == 'zeros':
        T[:, :, 1, 3] = 0.0                                  # |Y_b| = 0
        T[:, :, 2, 5] = 0.25                                 # a constant row: zero norm once the mean is off
        T[:, 0, 0, 7] = 0.0                                  # |X_b| = 0
    T_h = T.cpu().numpy()
    M = torch.from_numpy(M_h).cuda()
    want = _segments_ref(T_h, M_h, np.float64)
    dev32 = _rowrel(np.moveaxis(_segments_ref(T_h, M_h, np.float32), 2, -1), np.moveaxis(want, 2, -1))
    buf, out = _guarded((B, C, C + 1, 2))
    got = ops.stoi_segments(T, M, nf, out=out)
    first = _bits(got)
    ops.stoi_segments(T, M, nf, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(buf) and np.array_equal(first, _bits(out))
    d = out.cpu().numpy()
    err = _rowrel(np.moveaxis(d, 2, -1), np.moveaxis(want, 2, -1))
    print('segments %s: kernel %.3g, float32 numpy %.3g of the row maximum (bar %.3g)' % (name, err, dev32, 4 * dev32))
    assert np.isfinite(d).all() and err <= 4 * dev32
    if M_h.max() >= 30:
        assert dev32 > 0 and np.abs(want).max() > 0.1
    for b in range(B):
        for i in range(C):
            if M_h[b, i] < 30:
                assert not d[b, i].any()


# -------------------------------------------------------------------------------------- end to end
def _spectra(B, C, T, seed, short=(), swap=()):
    '''complex64 (src, est) [B, C, T, 129] at FFT_SIZE 256, FFT_STRIDE 64: the STFT of gated AR(1) references and noisy
    estimates; the utterances of `short` have references with energy in 20 frames only, those of `swap` their
    estimates in reverse order'''
    Ls = (T - 1) * 64 + 256
    win = torch.hann_window(256, periodic=True, dtype=torch.float64)
    src, est = [], []
    for b in range(B):
        wav = SR.make_case(C, Ls, seed=seed + b).astype(np.float64)
        if b in short:
            wav[:, :Ls // 3] = 0.0
            wav[:, Ls // 3 + 20 * 64:] = 0.0
        if b in swap:
            wav[C:] = wav[C:][::-1].copy()
        X = torch.stft(torch.from_numpy(wav), 256, 64, window=win, center=False, return_complex=True)   # [2C, F, T]
        X = X.permute(0, 2, 1).to(torch.complex64)
        src.append(X[:C])
        est.append(X[C:])
    return torch.stack(src).cuda().contiguous(), torch.stack(est).cuda().contiguous()


def _restate(wav_h, h32, dtype=np.float64):
    '''[(st, es, M, live)] per utterance and evaluate_batch's tuple, from the kernel's own waveforms'''
    U, D, H = SR.rate(8000)
    tabs = [SR.pair_tables(SR.signals10(u, U, D, H, h32), W, dtype) for u in wav_h]
    res = [SR.scores(*t) for t in tabs]
    per = np.stack([r[0] for r in res])
    flags = np.array([r[2] for r in res], np.int32)
    mean4, count = SR.batch_mean(per, flags)
    return tabs, (mean4, per, np.array([r[1] for r in res], np.int32), flags, count)


@pytest.mark.parametrize('C,T,short', [(1, 128, ()), (2, 128, (1, 4)), (3, 128, ()), (4, 128, (0,)),
                                       (2, 40, ())])
def test_stoi_eval_from_spectra(hp, C, T, short):
    '''B = 7; (2, 128, (1, 4)) and (4, 128, (0,)): some utterances flagged; (2, 40): every utterance flagged'''
    from danet_amd import ops
    hp.load(dict(FFT_SIZE=256, FFT_STRIDE=64, MAX_N_SIGNAL=C, BATCH_SIZE=7, SMPRATE=8000))
    hp.digest()
    B = 7
    src, est = _spectra(B, C, T, seed=50 * C + T, short=short, swap=(2, 5))
    wav = ops.metric_synth(src, est, 64)
    whole = ops.stoi_eval(src, est, with_count=True)
    ones = ops.stoi_eval(src, est, group=1, with_count=True)
    given = ops.stoi_eval(src, est, wav=wav, group=3, with_count=True)
    again = ops.stoi_eval(src, est, with_count=True)
    torch.cuda.synchronize()
    for a, b, c, e in zip(whole, ones, given, again):
        assert np.array_equal(_bits(a.reshape(-1)), _bits(b.reshape(-1)))      # groups of 1 and of all: bit for bit
        assert np.array_equal(_bits(a.reshape(-1)), _bits(c.reshape(-1)))
        assert np.array_equal(_bits(a.reshape(-1)), _bits(e.reshape(-1)))      # and a repeat
    h32 = ops.stoi_tables(8000, src.device)['h'].cpu().numpy()
    wav_h = wav.cpu().numpy()
    tabs, (mean_r, per_r, perm_r, flags_r, count_r) = _restate(wav_h, h32)
    U, D, H = SR.rate(8000)
    margin = min(SR.margin_db(SR.frame_energies(SR.resample(u[i], U, D, H, h32).astype(np.float32), W))
                 for u in wav_h for i in range(C))
    assert margin >= 1e-6, margin                            # the masks are the restatement's, exactly
    _, (mean_32, per_32, _, flags_32, _) = _restate(wav_h, h32, np.float32)
    assert np.array_equal(flags_32, flags_r)
    dev32 = max(_rowrel(per_32.T, per_r.T), _rowrel(mean_32[:, None], mean_r[:, None]))
    bar = 4 * dev32
    stoi, estoi, stoii, estoii, per_utt, perm_idx, flags, count = whole
    assert stoi.dtype == torch.float64 and stoi.dim() == 0 and per_utt.shape == (B, 4) and count.dtype == torch.int32
    got = np.array([float(stoi), float(estoi), float(stoii), float(estoii)])
    print('stoi_eval C %d T %d: %s, restatement %s, flags %s, float32 numpy deviates %.3g'
          % (C, T, got.round(6), mean_r.round(6), flags_r.tolist(), dev32))
    assert np.array_equal(flags.cpu().numpy(), flags_r) and int(count) == count_r == int((flags_r == 0).sum())
    want_flagged = len(short) if T >= 128 else B
    assert int((flags_r != 0).sum()) == want_flagged, flags_r
    if count_r:
        assert dev32 > 0
        assert _rowrel(per_utt.cpu().numpy().T, per_r.T) <= bar and _rowrel(got[:, None], mean_r[:, None]) <= bar
        # the search is safe: best and second-best sums differ by more than 100 bars
        top = np.abs(per_r).max()
        for (st, es, Ms, live), f in zip(tabs, flags_r):
            if f == 0 and C > 1:
                assert SR.search_gap(st, live) > 100 * bar * top
        assert set(perm_r[flags_r == 0].tolist()) >= {0, (0, 0, 1, 5, 23)[C]}             # the swapped ones are found
    else:
        assert not got.any() and not per_utt.cpu().numpy().any()
    assert np.array_equal(perm_idx.cpu().numpy(), perm_r)
    assert not per_utt.cpu().numpy()[flags_r != 0].any()


# ---------------------------------------------------------------------------------------- model
_MODEL_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import __graft_entry__ as g
g.load_package()
from danet_amd import _lib, ops
from danet_amd.hparams import hparams
H = sys.modules['danet_amd.hparams']
from danet_amd.model import Model
base = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
            NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
            INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig')
rng = np.random.RandomState(0)
src_h = ((rng.randn(2, 2, 260, 33) + 1j * rng.randn(2, 2, 260, 33)) * 3).astype(np.complex64)
src = torch.as_tensor(src_h).cuda()
res = {'has_key': 'EVAL_STOI' in H.DEFAULTS}
def run(tag, **keys):
    hparams.reset(); hparams.load(dict(base, **keys)); hparams.digest()
    model = Model('stoi', device='cuda:0', seed=3).build()
    out = model.valid_step(src)
    torch.cuda.synchronize()
    res[tag + '_hex'] = {k: float(v).hex() for k, v in out.items()}
    res[tag + '_keys'] = list(out)
    res[tag + '_mapped'] = 'libdanet_stoi' in open('/proc/self/maps').read()
    return model
combos = {'': {}, 'si': dict(EVAL_SI_SDR=True), 'bss': dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=8),
          'both': dict(EVAL_SI_SDR=True, EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=8)}
for name, keys in combos.items():
    run(name + '/never', **keys)
    if res['has_key']:
        run(name + '/null', EVAL_STOI=None, **keys)
        run(name + '/false', EVAL_STOI=False, **keys)
if res['has_key']:
    for name, keys in combos.items():
        model = run(name + '/on', EVAL_STOI=True, **keys)
    with torch.no_grad():
        o = model.forward(src, with_valid=True, with_train=False)
        est = ops.reattach_phase(o['sep_pwr_valid'], o['phasor'])
        ref = ops.stoi_eval(src, est)
    torch.cuda.synchronize()
    res['ref_hex'] = [float(v).hex() for v in ref[:4]]
    res['ref_flags'] = ref[6].cpu().tolist()
res['ok'] = bool(ops.lstm_status_ok())
print('RESULT ' + json.dumps(res))
'''
OLD_KEYS = {'': ['loss', 'SNR'], 'si': ['loss', 'SNR', 'SI-SDR', 'SI-SDRi'],
            'bss': ['loss', 'SNR', 'SDR', 'SIR', 'SAR', 'SDRi'],
            'both': ['loss', 'SNR', 'SI-SDR', 'SI-SDRi', 'SDR', 'SIR', 'SAR', 'SDRi']}
NEW_KEYS = ['STOI', 'ESTOI', 'STOIi', 'ESTOIi']


@functools.lru_cache(maxsize=None)
def _run_model():
    '''one process for both tests: every combination with the key never set, null, false and (where it exists) true'''
    code = _MODEL_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split('RESULT ')[1])
    assert r['ok']
    return r


def test_valid_step_with_the_key_off():
    '''what valid_step returned before the key existed, in all four combinations of EVAL_SI_SDR / EVAL_BSS_SDR: the
    same keys, the same bits with the key null or false, the library never mapped'''
    r = _run_model()
    for name, keys in OLD_KEYS.items():
        assert r[name + '/never_keys'] == keys and not r[name + '/never_mapped'], name
        for tag in (('/null', '/false') if r['has_key'] else ()):
            assert r[name + tag + '_keys'] == keys and not r[name + tag + '_mapped'], (name, tag)
            assert r[name + tag + '_hex'] == r[name + '/never_hex'], (name, tag)             # bit for bit
    for k in ('loss', 'SNR'):
        assert len(set(r[name + '/never_hex'][k] for name in OLD_KEYS)) == 1, k


def test_valid_step_with_the_key_on():
    r = _run_model()
    assert r['has_key'] and r['ref_flags'] == [0, 0]
    for name, keys in OLD_KEYS.items():
        assert r[name + '/on_keys'] == keys + NEW_KEYS and r[name + '/on_mapped'], name
        for k in keys:
            assert r[name + '/on_hex'][k] == r[name + '/never_hex'][k], (name, k)            # the older figures: bit for bit
        for k, ref in zip(NEW_KEYS, r['ref_hex']):
            assert r[name + '/on_hex'][k] == ref, (name, k)                                  # ops.stoi_eval on the same tensors
    vals = [float.fromhex(v) for v in r['ref_hex']]
    print('valid_step STOI %.6f ESTOI %.6f STOIi %.6f ESTOIi %.6f' % tuple(vals))
    assert all(np.isfinite(v) for v in vals) and -1 <= vals[0] <= 1 and vals[0] != 0.0


# ------------------------------------------------------------------------------------------ CLI
def test_command_line_valid_prints_the_four_figures(tmp_path):
    P.write_tree(tmp_path / 'tree', seed=7, n_per_subset=8, subsets=('train', 'test'), seconds=(0.7, 0.9))
    cfg = dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2,
               LSTM_HDIM=8, NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
               INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=320,
               DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'), EVAL_STOI=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)
    path = tmp_path / 'cfg.json'
    path.write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'stoi', '-m', 'valid', '-ds', 'wavdir',
                          '-c', str(path)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = out.stdout.split('Valid: ')[1].splitlines()[0]
    assert line.index('loss=') < line.index('SNR=') < line.index(' STOI=') < line.index(' ESTOI=') \
        < line.index(' STOIi=') < line.index(' ESTOIi=')
    for k in (' STOI=', ' ESTOI=', ' STOIi=', ' ESTOIi='):
        assert np.isfinite(float(line.split(k)[1].split()[0])), line
