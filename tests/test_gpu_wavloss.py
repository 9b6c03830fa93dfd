'''
GPU tests of the waveform training loss (TRAIN_LOSS = "si-sdr", run with -m gpu): the two kernels of
libdanet_wavloss_hip.so, each against the float64 restatement tests/wavloss_ref.py on the kernel's OWN inputs -- the
finalize step on random Gram matrices, the backward step on random waveforms with a hand-made pairing -- then the
adjoint identity against the device synthesis, ops.si_sdr_loss end to end from the spectra, Model.train_step with
the key off and on, and the command line.

Bars.  Finalize: 1e-12 dB and 1e-12 relative.  Backward: 1e-5 of each signal's max|grad| (the project's bar for the
synthesis, whose float32 floor is 2.7e-7); the float32 restatement's error is printed beside the kernel's.  End to
end: 1e-3 dB for the loss (the bar of ops.si_sdr); max(1e-5, twice the float32 restatement's error on the same case)
of max|dsep| for the gradient, the project's noise-floor rule: the loss of float32 waveforms grows as 10^(SDR/20).
'''
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metric_ref as MR
import wavloss_ref as WR
from gpu_helpers import ROOT

pytestmark = pytest.mark.gpu
POISON = -7.25e33
GUARD = 1024


def _window(N):
    import scipy.signal
    return np.sqrt(scipy.signal.windows.hann(N)).astype(np.float32)


def _spectra(rng, B, C, T, N, scale=3.0):
    F = N // 2 + 1
    return ((rng.standard_normal((B, C, T, F)) + 1j * rng.standard_normal((B, C, T, F))) * scale).astype(np.complex64)


def _guarded(shape, dtype):
    '''(whole buffer, the view of `shape` in its middle): everything poisoned'''
    n = int(np.prod(shape))
    real = torch.float32 if dtype == torch.complex64 else dtype
    m = 2 * n if dtype == torch.complex64 else n
    buf = torch.full((m + 2 * GUARD,), POISON if real.is_floating_point else -77, dtype=real, device='cuda')
    view = buf[GUARD:GUARD + m]
    if dtype == torch.complex64:
        view = torch.view_as_complex(view.view(n, 2))
    return buf, view.view(shape)


def _guards_intact(buf):
    bad = POISON if buf.dtype.is_floating_point else -77
    return bool((buf[:GUARD] == bad).all()) and bool((buf[-GUARD:] == bad).all())


def _bits(t):
    a = t.detach().cpu().contiguous()
    if a.dtype == torch.complex64:
        a = torch.view_as_real(a)
    return a.numpy().view({4: np.uint32, 8: np.uint64}[a.element_size()]).copy()


# ------------------------------------------------------------------------------------- finalize
def _fwd_both(G, C):
    '''the kernel and the restatement on the same Gram matrices; every output guarded, the launch repeated'''
    from danet_amd import ops
    B = G.shape[0]
    Gd = torch.from_numpy(np.ascontiguousarray(G, dtype=np.float64)).cuda()
    shapes = (((1,), torch.float64), ((1,), torch.float32), ((B,), torch.float64), ((B,), torch.int32),
              ((B, C), torch.int32), ((B, C, 2), torch.float64))
    bufs = [_guarded(s, d) for s, d in shapes]
    got = ops.wavloss_fwd(Gd, out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    first = [_bits(v) for v in got]
    vals = [v.cpu().numpy().copy() for v in got]
    assert all(_guards_intact(buf) for buf, _ in bufs)
    for _, v in bufs:
        v.fill_(POISON if v.dtype.is_floating_point else -77)
    again = ops.wavloss_fwd(Gd, out=tuple(v for _, v in bufs))
    assert all(np.array_equal(a, _bits(v)) for a, v in zip(first, again))
    ref = WR.fwd(G, C)
    loss64, loss32, per_utt, perm_idx, pair, coef = vals
    assert abs(loss64[0] - ref['loss']) <= 1e-12, (loss64[0], ref['loss'])
    assert loss32[0] == np.float32(loss64[0])
    assert np.abs(per_utt - ref['per_utt']).max() <= 1e-12
    assert np.array_equal(perm_idx, ref['perm_idx']), (perm_idx, ref['perm_idx'])
    assert np.array_equal(pair, ref['pair']), (pair, ref['pair'])
    assert (np.abs(coef - ref['coef']) <= 1e-12 * np.abs(ref['coef'])).all(), np.abs(coef - ref['coef']).max()
    assert np.array_equal(coef == 0, ref['coef'] == 0)
    return ref, loss64[0]


@pytest.mark.parametrize('B', [1, 5, 257])
@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_fwd_against_the_restatement_on_random_gram_matrices(C, B):
    rng = np.random.RandomState(100 * C + B)
    L = 48
    perms = list(itertools.permutations(range(C)))
    s = rng.standard_normal((B, C, L))
    e = np.zeros((B, C, L))
    for b in range(B):
        p = perms[rng.randint(len(perms))]
        for i in range(C):
            e[b, p[i]] = s[b, i]
    e += 10.0 ** (-rng.uniform(-5, 50, (B, 1, 1)) / 20) * rng.standard_normal((B, C, L))
    if B > 4:
        s[1] = 0                                                      # no live reference
        s[2, 0] = 0                                                   # one silent reference (C = 1: none live)
        e[3] = s[3]                                                   # the +100 clamp
        e[4] = 0                                                      # the -100 clamp
    G = MR.gram(np.concatenate([s, e], axis=1))
    ref, loss = _fwd_both(G, C)
    per_utt, perm_idx, mean2 = MR.finalize(G, C)
    assert abs(loss + mean2[0]) <= 1e-12 and np.array_equal(ref['perm_idx'], perm_idx)
    if B > 4:
        assert not ref['coef'][[1, 3, 4]].any() and (ref['pair'][1] == -1).all() and (ref['pair'][2] == -1).sum() == 1
        assert ref['per_utt'][3] == 100.0 and ref['per_utt'][4] == -100.0
        assert ref['coef'][0].all() and ref['coef'][5:].all()


def test_fwd_clamps_ties_silence_and_an_utterance_free_batch():
    rng = np.random.RandomState(9)
    L = 64
    a, b = np.zeros(L), np.zeros(L)
    a[:32], b[32:] = rng.standard_normal(32), rng.standard_normal(32)        # disjoint support: exactly orthogonal
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    z = np.zeros(L)
    wav = np.stack([np.stack([a, b, a, b]),          # identical: +100, identity, no gradient
                    np.stack([a, b, b, a]),          # identical, swapped
                    np.stack([a, z, b, b]),          # orthogonal to the one live reference: -100
                    np.stack([a, b, a + b, a + b]),  # a tie: the first permutation
                    np.stack([z, z, a, b]),          # no live reference
                    np.stack([z, b, a, b + 0.1 * a])])   # one silent reference: 20 dB from the live one
    ref, loss = _fwd_both(MR.gram(wav), 2)
    assert np.array_equal(ref['perm_idx'], [0, 1, 0, 0, 0, 0])
    assert np.array_equal(ref['pair'], [[0, 1], [1, 0], [0, -1], [0, 1], [-1, -1], [-1, 1]])
    assert not ref['coef'][[0, 1, 2, 4]].any() and ref['coef'][3].all() and ref['coef'][5, 1].all()
    assert abs(loss + ref['per_utt'][[0, 1, 2, 3, 5]].mean()) <= 1e-12
    ref, loss = _fwd_both(MR.gram(wav[4:5].repeat(3, axis=0)), 2)
    assert loss == 0.0 and not ref['coef'].any() and (ref['pair'] == -1).all()


_METRIC_BATCH = {}


def _metric_batch(C):
    '''float64 Gram matrices [257, 2C, 2C] built on the host, once per C and never written again: W W^T of random
    rows (positive definite), with the cases of the rule in utterances 1..5 made of small integers, so that their
    entries are exact.  Utterance 0 is a plain one: a batch of it alone has a live reference.'''
    if C not in _METRIC_BATCH:
        rng = np.random.RandomState(40 + C)
        B, L = 257, 6 * C
        wav = rng.standard_normal((B, 2 * C, L)) * 10.0 ** rng.uniform(-2, 2, (B, 2 * C, 1))
        wav[1:6] = rng.randint(-4, 5, (5, 2 * C, L))
        wav[1:6, :, 0] = 1                                            # (no row of these is zero by chance)
        wav[1, 0] = 0                                                 # a dead reference: zero diagonal
        wav[2, :C] = 0                                                # every reference dead
        wav[3, C:] = wav[3, C]                                        # equal estimates: all permutations tie
        wav[4, C] = wav[4, 0]                                         # estimate 0 is reference 0: the +100 clamp
        wav[5, C] = 0                                                 # a silent estimate: the -100 clamp
        G = np.einsum('bin,bjn->bij', wav, wav)
        assert G[1, 0, 0] == 0 and not G[2, :C, :C].any() and (np.diagonal(G[0], axis1=-2, axis2=-1) > 0).all()
        assert MR.sdr(G[4, 0, 0], G[4, C, C], G[4, 0, C]) == 100.0 and MR.sdr(G[5, 0, 0], G[5, C, C], G[5, 0, C]) == -100.0
        if C > 1:
            sums = [sum(MR.sdr(G[3, i, i], G[3, C + p[i], C + p[i]], G[3, i, C + p[i]]) for i in range(C))
                    for p in itertools.permutations(range(C))]
            assert sums.count(max(sums)) >= 2                         # an exact tie between permutations
        G.setflags(write=False)
        _METRIC_BATCH[C] = G
    return _METRIC_BATCH[C]


@pytest.mark.parametrize('B', [1, 257])                              # 257: the per-thread utterance loop wraps once
@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_fwd_is_the_metric_finalize_bit_for_bit(C, B):
    '''the loss is defined as the metric's: on one Gram batch danet_wavloss_fwd and danet_metric_si_sdr agree as
    bits in the permutation, the SI-SDR of every utterance and (negated) the batch mean'''
    from danet_amd import ops
    G = torch.from_numpy(_metric_batch(C)[:B].copy()).cuda()
    loss64, _, per_utt, perm_idx, _, _ = ops.wavloss_fwd(G)
    mean2, m_per_utt, m_perm_idx = ops.metric_finalize(G)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(perm_idx), _bits(m_perm_idx)), (perm_idx, m_perm_idx)
    assert np.array_equal(_bits(per_utt), _bits(m_per_utt[:, 0]))
    assert np.array_equal(_bits(loss64), _bits(-mean2[:1])), (loss64, mean2)
    if B > 5:
        got = per_utt.cpu().numpy()
        assert got[2] == 0.0 and int(perm_idx[2]) == 0 and int(perm_idx[3]) == 0 and np.isfinite(got).all()
        assert float(mean2[0]) != 0.0


# ------------------------------------------------------------------------------------- backward
def _frame_counts(N, S):
    tile = WR.tile_frames(N)
    return sorted({2, 3, N // S, N // S + 1, 9, 130, tile - 1, tile, tile + 1})


@pytest.mark.parametrize('N,S', [(64, 16), (64, 24), (64, 32), (256, 64), (1024, 256)])
def test_bwd_against_float64_evaluation_of_the_rule_on_its_own_inputs(N, S):
    from danet_amd import ops
    rng = np.random.RandomState(N + S)
    w = _window(N)
    wd = torch.from_numpy(w).cuda()
    F = N // 2 + 1
    worst = worst32 = 0.0
    case = 0
    for T in _frame_counts(N, S):
        for B, C in ((1, 1), (3, 2), (2, 4)):
            case += 1
            Ls = (T - 1) * S
            wav = (rng.standard_normal((B, 2 * C, Ls)) * 10.0 ** rng.uniform(-1, 1, (B, 2 * C, 1))).astype(np.float32)
            pair = rng.randint(0, C, (B, C)).astype(np.int32)
            coef = rng.standard_normal((B, C, 2)) * 10.0 ** rng.uniform(-2, 1, (B, C, 1))
            coef[0, 0, 1] = 0.0                                       # an alpha-only row: the pure adjoint
            if B > 1:
                pair[1, 0] = -1                                       # a row without a pair: exact zeros
                coef[1, 0] = 0.0
                coef[1, 1] = coef[1, 1, 0], -coef[1, 1, 0] * (1 + 1e-4)    # near-cancelling terms (the 40 dB regime)
                pair[1, 1] = 1
                wav[1, C + 1] = wav[1, 1] + np.float32(1e-3) * wav[1, C + 1]
            ph_ang = rng.uniform(-np.pi, np.pi, (B, T, F))
            phasor = np.stack([np.cos(ph_ang), np.sin(ph_ang)], axis=-1).astype(np.float32)
            dl = (None, 0.37)[case % 2], (0.37, None)[case % 2]       # (complex form, real form)
            args = [torch.from_numpy(x).cuda() for x in (wav, pair, coef)]
            for form, dloss in zip(('complex', 'real'), dl):
                ph = torch.from_numpy(phasor).cuda() if form == 'real' else None
                dld = None if dloss is None else torch.tensor(dloss, dtype=torch.float32, device='cuda')
                buf, out = _guarded((B, C, T, F), torch.complex64 if ph is None else torch.float32)
                got = ops.wavloss_bwd(*args, N, S, window=wd, dloss=dld, phasor=ph, out=out)
                torch.cuda.synchronize()
                first, val = _bits(got), got.cpu().numpy().copy()
                assert _guards_intact(buf), (T, B, C, form)
                out.fill_(POISON)
                again = ops.wavloss_bwd(*args, N, S, window=wd, dloss=dld, phasor=ph, out=out)
                assert np.array_equal(_bits(again), first), (T, B, C, form)
                kw = dict(dloss=np.float32(1.0 if dloss is None else dloss), phasor=None if ph is None else phasor)
                ref = WR.bwd(wav, pair, coef, w, S, **kw)
                ref32 = WR.bwd(wav, pair, coef, w, S, dtype=np.float32, **kw)
                peak = np.abs(ref).max(axis=(-2, -1), keepdims=True)
                live = peak[..., 0, 0] > 0
                assert np.isfinite(val).all()
                assert not val[~live].any() and (B == 1 or not live[1, 0])      # exact zeros without a pair
                err = (np.abs(val - ref)[live] / peak[live]).max()
                err32 = (np.abs(ref32 - ref)[live] / peak[live]).max()
                worst, worst32 = max(worst, err), max(worst32, err32)
                assert err <= 1e-5, (T, B, C, form, err, err32)
                if form == 'complex':
                    assert not val[..., 0].imag.any() and not val[..., -1].imag.any()
                    if dloss is None:                                 # the alpha-only row IS the adjoint of the synthesis
                        wsum = WR.window_sum(w, S, T)
                        adj = WR.adjoint(coef[0, 0, 0] * wav[0, pair[0, 0]].astype(np.float64) / wsum, w, S, T)
                        assert np.abs(val[0, 0] - adj).max() <= 1e-5 * np.abs(adj).max()
    print('N %d S %d: worst error %.3g of a signal\'s max|grad| (float32 restatement %.3g)' % (N, S, worst, worst32))


def test_bwd_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    wd = torch.from_numpy(_window(64)).cuda()
    wav = torch.zeros(1, 2, 0, device='cuda')                           # T = 1
    pair = torch.zeros(1, 1, dtype=torch.int32, device='cuda')
    coef = torch.ones(1, 1, 2, dtype=torch.float64, device='cuda')
    buf, out = _guarded((1, 1, 1, 33), torch.complex64)
    with pytest.raises(_lib.DanetHipError, match='T must be >= 2'):
        ops.wavloss_bwd(wav, pair, coef, 64, 16, window=wd, out=out)
    buf2, out2 = _guarded((1, 1, 5, 49), torch.complex64)                 # N = 96: not a power of two
    with pytest.raises(_lib.DanetHipError, match='power of two'):
        ops.wavloss_bwd(torch.zeros(1, 2, 96, device='cuda'), pair, coef, 96, 24, window=torch.ones(96, device='cuda'),
                        out=out2)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all()) and bool((buf2 == POISON).all())


# ------------------------------------------------------------------------------------- adjoint
@pytest.mark.parametrize('N,S,T', [(64, 24, 35), (256, 64, 33), (1024, 256, 11)])
def test_bwd_is_the_adjoint_of_the_device_synthesis(N, S, T):
    '''<metric_synth(X)[estimate rows], g> = Re<X, bwd(g)>: g goes in as the paired "reference" with (alpha, beta)
    = (1, 0), so bwd(g) is the adjoint applied to g'''
    from danet_amd import ops
    rng = np.random.RandomState(N + T)
    B, C = 2, 2
    wd = torch.from_numpy(_window(N)).cuda()
    X = _spectra(rng, B, C, T, N)
    X[..., 0] = X[..., 0].real                                        # (the synthesis ignores these two)
    X[..., -1] = X[..., -1].real
    Xd = torch.from_numpy(X).cuda()
    y = ops.metric_synth(Xd, Xd, S, wd)[:, C:].double().cpu().numpy()
    g = rng.standard_normal((B, C, (T - 1) * S)).astype(np.float32)
    wav = torch.from_numpy(np.concatenate([g, np.zeros_like(g)], axis=1)).cuda()
    pair = torch.arange(C, dtype=torch.int32, device='cuda').repeat(B, 1).contiguous()
    coef = torch.tensor([1.0, 0.0], dtype=torch.float64, device='cuda').repeat(B, C, 1).contiguous()
    A = ops.wavloss_bwd(wav, pair, coef, N, S, window=wd).cpu().numpy().astype(np.complex128)
    lhs = float((y * g.astype(np.float64)).sum())
    rhs = float((X.real.astype(np.float64) * A.real + X.imag.astype(np.float64) * A.imag).sum())
    scale = np.linalg.norm(y) * np.linalg.norm(g.astype(np.float64))
    print('N %d S %d T %d: |<synth X, g> - Re<X, bwd g>| = %.3g of |synth X| |g|' % (N, S, T, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-5 * scale


# ----------------------------------------------------------------------------------- end to end
def test_si_sdr_loss_end_to_end_against_the_restatement(hp):
    from danet_amd import ops
    hp.load(dict(FFT_SIZE=256, FFT_STRIDE=64))
    hp.digest()
    rng = np.random.RandomState(11)
    B, C, T, N, S = 8, 2, 40, 256, 64
    w = np.asarray(hp.FFT_WND)
    # the estimates of the model are real magnitudes times ONE phase per bin, the mixture's: references that share a
    # phase per bin are the ones such estimates can come within 30 dB of
    F = N // 2 + 1
    ang = rng.uniform(-np.pi, np.pi, (B, T, F))
    phasor = np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)
    mag = np.abs(rng.standard_normal((B, C, T, F))) * 3.0
    src = (mag * (phasor[:, None, ..., 0] + 1j * phasor[:, None, ..., 1])).astype(np.complex64)
    db = np.linspace(-5, 30, B)
    # estimates = references (swapped) + noise at about `db` dB below them
    sep = (mag[:, ::-1] + 10.0 ** (-db[:, None, None, None] / 20) * 3.0 * rng.standard_normal((B, C, T, F))).astype(np.float32)
    sep_d = torch.from_numpy(sep).cuda().requires_grad_(True)
    loss, perm = ops.si_sdr_loss(torch.from_numpy(src).cuda(), sep_d, torch.from_numpy(phasor).cuda())
    assert loss.dtype == torch.float32 and loss.dim() == 0 and perm.dtype == torch.int32 and not perm.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    dsep = sep_d.grad.cpu().numpy()
    ref, dref = WR.loss_from_sep(src, sep, phasor, w, S)
    ref32, dref32 = WR.loss_from_sep(src, sep, phasor, w, S, np.float32)
    print('per-utterance SI-SDR of the estimates (restatement): %s' % np.round(ref['per_utt'], 2))
    assert ref['per_utt'].min() < -2 and ref['per_utt'].max() > 27, ref['per_utt']      # the spread asked for
    assert np.array_equal(ref['perm_idx'], [1] * B)
    assert np.array_equal(perm.cpu().numpy(), ref['perm_idx'])
    print('loss %.6f dB (float64 restatement %.6f, float32 %.6f)' % (float(loss.detach()), ref['loss'], ref32['loss']))
    assert abs(float(loss.detach()) - ref['loss']) <= 1e-3
    worst = (0.0, 0.0)
    for b in range(B):
        peak = np.abs(dref[b]).max()
        err, err32 = np.abs(dsep[b] - dref[b]).max() / peak, np.abs(dref32[b] - dref[b]).max() / peak
        bar = max(1e-5, 2 * err32)
        print('utterance %d (%.1f dB): dsep error %.3g of max|dsep| (float32 restatement %.3g)' % (b, ref['per_utt'][b],
                                                                                                 err, err32))
        worst = max(worst, (err, err32))
        assert err <= bar, (b, err, err32)
        dot = float((dsep[b].astype(np.float64) * sep[b]).sum())
        assert abs(dot) <= bar * peak * np.abs(sep[b]).max() * sep[b].size, (b, dot)
    print('worst pair: kernel %.3g, float32 restatement %.3g' % worst)


# ---------------------------------------------------------------------------------------- model
_MODEL_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import __graft_entry__ as g
g.load_package()
import wavloss_ref as WR
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
def build(**keys):
    hparams.reset(); hparams.load(dict(base, **keys)); hparams.digest()
    return Model('wavloss', device='cuda:0', seed=3).build()
def hexes(t):
    return [float(v).hex() for v in t.detach().cpu().reshape(-1).tolist()]
def run(tag, **keys):
    model = build(**keys)
    with torch.no_grad():
        res[tag + '_fwd_snr'] = float(model.forward(src)['SNR']).hex()
    out = model.train_step(src)
    torch.cuda.synchronize()
    res[tag + '_train_loss'] = model.train_loss
    res[tag] = {k: float(v).hex() for k, v in out.items()}
    res[tag + '_keys'] = list(out)
    res[tag + '_flat'] = hexes(model._flat)
    res[tag + '_mapped'] = 'libdanet_wavloss' in open('/proc/self/maps').read()
    res[tag + '_metric_mapped'] = 'libdanet_metric' in open('/proc/self/maps').read()
run('never')
run('null', TRAIN_LOSS=None)
run('mse', TRAIN_LOSS='pit-mse')
# the waveform loss: what the step reports against the restatement on a forward pass of the same parameters
model = build(TRAIN_LOSS='si-sdr')
with torch.no_grad():
    o = model.forward(src)
    sep, ph = o['sep_pwr'].cpu().numpy(), o['phasor'].cpu().numpy()
    res['on_fwd_loss'] = float(o['loss'])
    res['on_has_loss_perm'] = 'loss_perm_idx' in o and 'perm_idx' in o
f64 = WR.loss_from_sep(src_h, sep, ph, np.asarray(hparams.FFT_WND), 16)[0]
res['ref_loss'] = f64['loss']
res['ref_perm'] = [int(v) for v in f64['perm_idx']]
res['on_loss_perm'] = [int(v) for v in o['loss_perm_idx'].cpu()]
model.keep_grads = True
out = model.train_step(src)
torch.cuda.synchronize()
res['on'] = {k: float(v) for k, v in out.items()}
res['on_snr_hex'] = float(out['SNR']).hex()
res['on_keys'] = list(out)
res['on_train_loss'] = model.train_loss
res['on_mapped'] = 'libdanet_wavloss' in open('/proc/self/maps').read()
res['on_metric_mapped'] = 'libdanet_metric' in open('/proc/self/maps').read()
g1 = model._flat_grad.detach().cpu().numpy().astype(np.float64)
# a second identical step of this tree: the run-to-run difference of the flat gradient
twin = build(TRAIN_LOSS='si-sdr')
twin.keep_grads = True
twin.train_step(src)
torch.cuda.synchronize()
g2 = twin._flat_grad.detach().cpu().numpy().astype(np.float64)
# the reference: the unfused forward, then dsep from ops.wavloss_bwd on the same step pushed through sep_pwr
ref = build(TRAIN_LOSS='si-sdr')
ref.zero_grad()
chain = ops.heads_chain()                # the streams and the backward mode of train_step itself
chain.__enter__()
o = ref.forward(src, fuse_heads=False)
with torch.no_grad():
    est = ops.reattach_phase(o['sep_pwr'].detach(), o['phasor'])
    wav = ops.metric_synth(src, est, 16)
    _l64, _l32, _pu, _pi, pair, coef = ops.wavloss_fwd(ops.metric_gram(wav))
    dsep = ops.wavloss_bwd(wav, pair, coef, 64, 16, phasor=o['phasor'].contiguous())
with ops.fast_backward():
    o['sep_pwr'].backward(dsep)
    ops.join_deferred()
chain.__exit__(None, None, None)
ops.join_deferred()
torch.cuda.synchronize()
g3 = ref._flat_grad.detach().cpu().numpy().astype(np.float64)
res['grad_max'] = float(np.abs(g1).max())
res['grad_run_to_run'] = float(np.abs(g1 - g2).max())
res['grad_vs_reference'] = float(np.abs(g1 - g3).max())
# 40 steps on one fixed batch
m = build(TRAIN_LOSS='si-sdr')
losses = [float(m.train_step(src)['loss']) for _ in range(40)]
res['loss_first'], res['loss_last'] = losses[0], losses[-1]
torch.cuda.synchronize()
res['ok'] = bool(ops.lstm_status_ok())
print('RESULT ' + json.dumps(res))
'''


def test_train_step_with_the_key_off_and_on():
    code = _MODEL_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split('RESULT ')[1])
    assert r['ok']
    for tag in ('never', 'null', 'mse'):
        assert r[tag + '_keys'] == ['loss', 'SNR', 'LR'] and r[tag + '_train_loss'] == 'pit-mse', tag
        assert not r[tag + '_mapped'] and not r[tag + '_metric_mapped'], tag
        assert r[tag] == r['never'] and r[tag + '_flat'] == r['never_flat'], tag          # bit for bit
    assert r['on_keys'] == ['loss', 'SNR', 'LR'] and r['on_train_loss'] == 'si-sdr'
    assert r['on_mapped'] and r['on_metric_mapped'] and r['on_has_loss_perm']
    print('train_step loss %.6f dB, forward %.6f, float64 restatement %.6f' % (r['on']['loss'], r['on_fwd_loss'],
                                                                            r['ref_loss']))
    assert abs(r['on']['loss'] - r['ref_loss']) <= 1e-3 and abs(r['on_fwd_loss'] - r['ref_loss']) <= 1e-3
    assert r['on_loss_perm'] == r['ref_perm']
    # SNR keeps its meaning: the null model's, on the same parameters, bit for bit
    print('SNR: si-sdr step %s, null step %s, null forward %s' % (r['on_snr_hex'], r['never']['SNR'], r['never_fwd_snr']))
    assert r['on_snr_hex'] == r['never']['SNR'] and r['on_snr_hex'] == r['never_fwd_snr']
    bar = max(2 * r['grad_run_to_run'], 1e-6 * r['grad_max'])
    print('flat gradient: max %.3g, run to run %.3g, against forward + wavloss_bwd + backward %.3g'
          % (r['grad_max'], r['grad_run_to_run'], r['grad_vs_reference']))
    assert r['grad_max'] > 0 and r['grad_vs_reference'] <= bar
    print('loss at step 0: %.4f dB, at step 39: %.4f dB' % (r['loss_first'], r['loss_last']))
    assert r['loss_last'] < r['loss_first']


# ------------------------------------------------------------------------------------------ CLI
def test_command_line_trains_on_the_waveform_loss(tmp_path):
    base = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2,
                LSTM_HDIM=8, NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
                INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig',
                MAX_TRAIN_LEN=128)       # the toy dataset's own length: no crop, so no draw from the unseeded `random`
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)

    def main(tag, keys):
        cfg = tmp_path / ('%s.json' % tag)
        cfg.write_text(json.dumps(dict(base, **keys)))
        return subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', tag, '-m', 'train', '-ds', 'toy',
                               '-c', str(cfg), '-ne', '1', '-bs', '2'], cwd=str(tmp_path), capture_output=True,
                              text=True, timeout=600, env=env)

    out = main('wl', dict(TRAIN_LOSS='si-sdr'))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    loss = float(out.stdout.split('Epoch 1/1 loss=')[1].split()[0])
    assert np.isfinite(loss) and -100.0 <= loss <= 100.0 and 'Valid  1/1 loss=' in out.stdout
    plain, mse = main('plain', {}), main('mse', dict(TRAIN_LOSS='pit-mse'))
    assert plain.returncode == 0 and mse.returncode == 0, plain.stderr[-2000:] + mse.stderr[-2000:]
    lines = [[l for l in o.stdout.splitlines() if l.startswith(('Epoch 1/1', 'Valid  1/1'))] for o in (plain, mse, out)]
    assert len(lines[0]) == 2 and lines[0] == lines[1] and lines[0][0] != lines[2][0]
    bad = main('bad', dict(TRAIN_LOSS='SI-SDR'))
    assert bad.returncode != 0 and 'TRAIN_LOSS' in bad.stderr, bad.stdout[-2000:] + bad.stderr[-2000:]
