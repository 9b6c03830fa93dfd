'''
GPU tests of noisy evaluation (run with -m gpu): the three kernels of libdanet_neval_hip.so, each against the output
it can be pinned on -- waveforms against the float64 restatement and, bit for bit, against libdanet_metric_hip.so;
Gram matrices against math.fsum of the kernel's own waveforms; decibels against tests/neval_ref.py on the kernel's own
Gram matrices -- then ops.si_sdr_noisy end to end, Model.valid_step with and without noise, the wavdir dataset's
`valid` / `test` route and the command line.

Bars.  Synthesis: the project's 1e-5 STFT bar, relative to each signal's max|y| (float32 arithmetic sits near 3e-7).
Gram: 1e-9 of sqrt(G_ii G_jj).  Finalize: 1e-9 dB.  End to end: the project's 1e-3 dB per utterance.
'''
import itertools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import metric_ref as MR
import mix_ref as M
import neval_ref as NV
import noise_ref as NR
import prep_ref as P
import speed_ref as SR
from gpu_helpers import ROOT, cu

pytestmark = pytest.mark.gpu
POISON = -7.25e33
GUARD = 1024


def _window(N):
    import scipy.signal
    return np.sqrt(scipy.signal.windows.hann(N)).astype(np.float32)


def _spectra(rng, *shape, scale=3.0):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)


def _guarded(shape, dtype):
    '''(whole buffer, the view of `shape` in its middle): everything poisoned'''
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON if dtype.is_floating_point else -77, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, n):
    bad = POISON if buf.dtype.is_floating_point else -77
    return bool((buf[:GUARD] == bad).all()) and bool((buf[GUARD + n:] == bad).all())


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------ synthesis
@pytest.mark.parametrize('N,S', [(64, 16), (64, 32), (256, 64), (1024, 256)])
def test_synthesis_against_the_float64_restatement_and_the_metric_library(N, S):
    from danet_amd import ops
    rng = np.random.RandomState(N + S)
    w = _window(N)
    wd = torch.from_numpy(w).cuda()
    F = N // 2 + 1
    worst, where = 0.0, None
    for T in sorted({2, 3, N // S, N // S + 1, 9, 130}):
        for B, C in ((1, 1), (3, 2), (2, 4)):
            src, est = _spectra(rng, B, C, T, F), _spectra(rng, B, C, T, F, scale=0.5)
            noise = _spectra(rng, B, T, F, scale=1.5)                 # random spectra: no consistent STFT
            assert np.abs(noise[..., 0].imag).min() > 0 and np.abs(noise[..., N // 2].imag).min() > 0
            sd, ed, nd = (torch.from_numpy(a).cuda() for a in (src, est, noise))
            Ls, Mr = (T - 1) * S, 2 * C + 1
            clean = ops.metric_synth(sd, ed, S, wd).cpu().numpy()     # rows 0..2C-1 as the metric library writes them
            as_ref = ops.metric_synth(nd[:, None].contiguous(), nd[:, None].contiguous(), S, wd).cpu().numpy()[:, 0]
            ref_rows = MR.synth(np.concatenate([src, est], axis=1), w, S)
            gains = [None, np.zeros(B, np.float32), np.ones(B, np.float32),
                     rng.uniform(0.05, 7.0, size=B).astype(np.float32)]    # non-dyadic, one per utterance
            for gi, gain in enumerate(gains):
                gd = None if gain is None else torch.from_numpy(gain).cuda()
                buf, out = _guarded((B, Mr, Ls), torch.float32)
                got = ops.neval_synth(sd, ed, nd, gd, S, wd, out=out).cpu().numpy().copy()
                assert _guards_intact(buf, B * Mr * Ls), (T, B, C, gi)
                assert np.isfinite(got).all()
                ref = np.concatenate([ref_rows, MR.synth(NV.scaled_noise(noise, gain), w, S)[:, None]], axis=1)
                peak = np.abs(ref).max(axis=-1, keepdims=True)
                peak[peak == 0] = 1.0                                  # (a zero row: absolute)
                err = float((np.abs(got - ref) / peak).max())
                if err > worst:
                    worst, where = err, (T, B, C, gi)
                assert err <= 1e-5, (T, B, C, gi, err)
                assert np.array_equal(_u32(got[:, :2 * C]), _u32(clean)), (T, B, C, gi)
                if gi in (0, 2):                                       # NULL, and 1 (an exact product)
                    assert np.array_equal(_u32(got[:, 2 * C]), _u32(as_ref)), (T, B, C, gi)
                if gi == 1:
                    assert not got[:, 2 * C].any()
                out.fill_(POISON)
                again = ops.neval_synth(sd, ed, nd, gd, S, wd, out=out).cpu().numpy()
                assert np.array_equal(_u32(again), _u32(got)), (T, B, C, gi)
    print('N %d S %d: worst error %.3g of max|y| at (T, B, C, gain) = %s' % (N, S, worst, where))


def test_synthesis_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    wd = torch.from_numpy(_window(64)).cuda()
    x = torch.from_numpy(_spectra(np.random.RandomState(0), 1, 1, 1, 33)).cuda()
    buf, out = _guarded((1, 3, 0), torch.float32)
    with pytest.raises(_lib.DanetHipError, match='T must be >= 2'):
        ops.neval_synth(x, x, x[:, 0], None, 16, wd, out=out)
    x = torch.zeros(1, 1, 5, 49, dtype=torch.complex64, device='cuda')           # N = 96: not a power of two
    buf2, out2 = _guarded((1, 3, 4 * 24), torch.float32)
    with pytest.raises(_lib.DanetHipError, match='power of two'):
        ops.neval_synth(x, x, x[:, 0], None, 24, torch.ones(96, device='cuda'), out=out2)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all()) and bool((buf2 == POISON).all())


# ----------------------------------------------------------------------------------------- Gram
@pytest.mark.parametrize('Ls', [1, 63, 64, 65, 4097, 33024])
def test_gram_against_fsum_and_the_metric_library(Ls):
    from danet_amd import _lib, ops
    rng = np.random.RandomState(Ls)
    for Mr in (3, 5, 9):
        for B in (1, 5):
            wav = (rng.standard_normal((B, Mr, Ls)) * 10.0 ** rng.uniform(-2, 2, (B, Mr, 1))).astype(np.float32)
            wd = torch.from_numpy(wav).cuda()
            buf, out = _guarded((B, Mr, Mr), torch.float64)
            G = ops.neval_gram(wd, out=out).cpu().numpy().copy()
            assert _guards_intact(buf, B * Mr * Mr)
            ref = MR.gram_fsum(wav)
            d = np.sqrt(np.einsum('bii->bi', ref))
            err = (np.abs(G - ref) / (d[:, :, None] * d[:, None, :])).max()
            assert err <= 1e-9, (Mr, B, err)
            assert np.array_equal(G.view(np.uint64), np.swapaxes(G, 1, 2).copy().view(np.uint64))
            out.fill_(POISON)
            again = ops.neval_gram(wd, out=out).cpu().numpy()
            assert np.array_equal(again.view(np.uint64), G.view(np.uint64))
            if Mr <= 8:
                assert np.array_equal(ops.metric_gram(wd).cpu().numpy().view(np.uint64), G.view(np.uint64)), (Mr, B)
    wd = torch.zeros(1, 10, 8, device='cuda')
    buf, out = _guarded((1, 10, 10), torch.float64)
    with pytest.raises(_lib.DanetHipError, match='M must'):
        ops.neval_gram(wd, out=out)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())


# ------------------------------------------------------------------------------------- finalize
def _finalize_both(wav, C, margin=True):
    '''the kernel and the restatement on the kernel's own Gram matrices of `wav` [B, 2C + 1, L]'''
    from danet_amd import ops
    G = ops.neval_gram(torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).cuda())
    B = G.shape[0]
    bufs = [_guarded((B, 3), torch.float64), _guarded((B,), torch.int32), _guarded((3,), torch.float64)]
    mean3, per_utt, perm = ops.neval_finalize(G, out=tuple(v for _, v in bufs))
    got = per_utt.cpu().numpy().copy(), perm.cpu().numpy().copy(), mean3.cpu().numpy().copy()
    for (buf, _), n in zip(bufs, (3 * B, B, 3)):
        assert _guards_intact(buf, n)
    Gh = G.cpu().numpy()
    ref = NV.finalize(Gh, C)
    assert np.abs(got[0] - ref[0]).max() <= 1e-9, (got[0], ref[0])
    if margin:      # the restatement alone: best and second-best sums differ by more than 1e-6 dB on every utterance
        m = NV.perm_margin(Gh, C)
        assert (m > 1e-6).all(), m.min()
        assert np.array_equal(got[1], ref[1]), (got[1], ref[1])
    assert np.abs(got[2] - ref[2]).max() <= 1e-9
    return got, G


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_finalize_against_the_restatement_on_the_kernels_own_gram(C):
    from danet_amd import ops
    rng = np.random.RandomState(40 + C)
    B, L = 300, 96                                                   # more utterances than the workgroup has threads
    perms = list(itertools.permutations(range(C)))
    s = rng.standard_normal((B, C, L))
    want = rng.randint(0, len(perms), B)
    level = 10.0 ** (-rng.uniform(-5, 30, (B, 1, 1)) / 20)
    e = np.zeros((B, C, L))
    for b in range(B):
        for i in range(C):
            e[b, perms[want[b]][i]] = s[b, i]                         # reference i is estimate p(i)
    e += level * rng.standard_normal((B, C, L))
    z = 10.0 ** (-rng.uniform(-5, 20, (B, 1, 1)) / 20) * rng.standard_normal((B, 1, L))
    s[6, 0] *= 0                                                     # one silent reference
    z[7] *= 0                                                        # one silent noise row
    (per_utt, perm, mean3), G = _finalize_both(np.concatenate([s, e, z], axis=1), C)
    clean = level[:, 0, 0] < 0.1                                     # (20 dB and better: the drawn permutation wins)
    clean[6] = False
    assert clean.sum() > 50 and np.array_equal(perm[clean], want[clean])
    assert per_utt[:, 0].min() < 0 and per_utt[:, 0].max() > 25 and np.isfinite(mean3).all()
    assert per_utt[7, 2] == 100.0 and -10 < np.delete(per_utt[:, 2], 7).min() and np.delete(per_utt[:, 2], 7).max() < 35
    # a silent noise row: the two figures of the clean metric on the sub-block, as values
    sub = G[7:8, :2 * C, :2 * C].contiguous()
    _m2, pu2, pi2 = ops.metric_finalize(sub)
    assert per_utt[7, 0] == float(pu2[0, 0]) and per_utt[7, 1] == float(pu2[0, 1]) and perm[7] == int(pi2[0])
    # and a batch of them
    wav0 = np.concatenate([s, e, np.zeros_like(z)], axis=1)
    (pu0, pi0, m0), G0 = _finalize_both(wav0, C)
    m2, pu2, pi2 = ops.metric_finalize(G0[:, :2 * C, :2 * C].contiguous())
    assert np.array_equal(pu0[:, :2], pu2.cpu().numpy()) and np.array_equal(pi0, pi2.cpu().numpy())
    has = np.abs(s).sum(axis=(1, 2)) > 0                              # (C = 1: utterance 6 has no live reference)
    assert np.array_equal(m0[:2], m2.cpu().numpy()) and np.array_equal(pu0[:, 2], np.where(has, 100.0, 0.0))
    assert m0[2] == 100.0


def test_finalize_clamps_ties_silence_and_an_empty_batch():
    rng = np.random.RandomState(9)
    L = 96
    a, b, n = np.zeros(L), np.zeros(L), np.zeros(L)
    a[:32], b[32:64], n[64:] = (rng.standard_normal(32) for _ in range(3))    # disjoint support: exactly orthogonal
    a, b, n = a / np.linalg.norm(a), b / np.linalg.norm(b), n / np.linalg.norm(n)
    z = np.zeros(L)
    wav = np.stack([np.stack([a, b, a, b, n]),            # identical: 100 dB, identity
                    np.stack([a, b, b, a, n]),            # identical, swapped: 100 dB, permutation 1
                    np.stack([a, z, b, b, n]),            # orthogonal to the one live reference: -100
                    np.stack([a, b, a + b, a + b, n]),    # a tie: the first permutation
                    np.stack([z, z, a, b, n]),            # no live reference
                    np.stack([z, b, a, b + 0.1 * a, z]),  # one silent reference, silent noise: nSNR +100
                    np.stack([a, -a, a, a, n]),           # the references cancel: nSNR -100
                    np.stack([a, b, a, b, 1e-6 * n]),     # nSNR above the clamp: +100
                    np.stack([1e-6 * a, 1e-6 * b, a, b, n])])     # nSNR below the clamp: -100
    (per_utt, perm, mean3), _ = _finalize_both(wav, 2, margin=False)
    assert np.array_equal(per_utt[:3, 0], [100.0, 100.0, -100.0])
    assert np.array_equal(perm[:6], [0, 1, 0, 0, 0, 0])               # (3: the tie goes to the first permutation)
    assert np.array_equal(per_utt[4], [0.0, 0.0, 0.0]) and abs(per_utt[5, 0] - 20.0) < 1e-4
    assert np.array_equal(per_utt[5:, 2], [100.0, -100.0, 100.0, -100.0])
    assert abs(per_utt[0, 2] - 10.0 * np.log10(2.0)) < 1e-5
    live = [0, 1, 2, 3, 5, 6, 7, 8]
    assert np.abs(mean3 - per_utt[live].mean(axis=0)).max() <= 1e-9
    # an all-silent batch: zeros
    (per_utt, perm, mean3), _ = _finalize_both(wav[4:5].repeat(3, axis=0), 2, margin=False)
    assert np.array_equal(mean3, [0.0, 0.0, 0.0]) and not per_utt.any() and not perm.any()
    (per_utt, perm, mean3), _ = _finalize_both(np.zeros((2, 5, L)), 2, margin=False)
    assert not mean3.any() and not per_utt.any() and not perm.any()


# ----------------------------------------------------------------------------------- end to end
def test_si_sdr_noisy_end_to_end_against_the_restatement(hp):
    from danet_amd import ops
    hp.load(dict(FFT_SIZE=256, FFT_STRIDE=64))
    hp.digest()
    rng = np.random.RandomState(11)
    B, C, T, N, S = 8, 2, 40, 256, 64
    F = N // 2 + 1
    w = np.asarray(hp.FFT_WND)
    src = _spectra(rng, B, C, T, F)
    db = np.linspace(-5, 30, B)
    est = (src[:, ::-1] + 10.0 ** (-db[:, None, None, None] / 20) * _spectra(rng, B, C, T, F)).astype(np.complex64)
    noise = _spectra(rng, B, T, F)
    # gains for about -5..20 dB of sources over noise: both have 3^2 * 2 per bin, the sources C of them
    gain = (np.sqrt(C) * 10.0 ** (-np.linspace(20, -5, B) / 20)).astype(np.float32)
    ref = NV.si_sdr_noisy(src, est, noise, gain, w, S)
    # the ranges asked for, by the restatement
    assert ref[0][:, 0].min() < -2 and ref[0][:, 0].max() > 27 and np.all(np.diff(ref[0][:, 0]) > 0), ref[0][:, 0]
    assert ref[0][:, 2].min() < -3 and ref[0][:, 2].max() > 18 and np.all(np.diff(ref[0][:, 2]) < 0), ref[0][:, 2]
    assert (NV.perm_margin(MR.gram(NV.synth(src, est, noise, gain, w, S)), C) > 1e-6).all()
    args = [torch.from_numpy(a).cuda() for a in (src, est, noise, gain)]
    a, b, c, per_utt, perm = ops.si_sdr_noisy(*args)
    got = per_utt.cpu().numpy()
    err = np.abs(got - ref[0])
    print('end to end: worst |kernel - float64| per utterance %.3g dB (SI-SDR %.3g, SI-SDRi %.3g, nSNR %.3g)'
          % (err.max(), err[:, 0].max(), err[:, 1].max(), err[:, 2].max()))
    assert (err <= 1e-3).all(), err
    assert np.abs(np.array([float(a), float(b), float(c)]) - ref[2]).max() <= 1e-3
    assert np.array_equal(perm.cpu().numpy(), ref[1]) and np.array_equal(ref[1], [1] * B)
    assert a.dtype == torch.float64 and a.dim() == 0 and per_utt.shape == (B, 3) and perm.dtype == torch.int32
    # the baseline is the NOISY mixture: SI-SDRi differs from the clean metric's, SI-SDR does not
    clean = ops.si_sdr(args[0], args[1])
    assert np.array_equal(clean[2].cpu().numpy()[:, 0], got[:, 0])
    assert np.abs(clean[2].cpu().numpy()[:, 1] - got[:, 1]).min() > 1e-3
    # the outputs are the caller's own: the next call, of another batch, leaves them alone
    keep, keep_a = per_utt.clone(), float(a)
    ops.si_sdr_noisy(args[1], args[0], args[2], None)
    torch.cuda.synchronize()
    assert torch.equal(keep, per_utt) and float(a) == keep_a


# ---------------------------------------------------------------------------------------- model
_MODEL_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import __graft_entry__ as g
g.load_package()
import neval_ref as NV
from danet_amd import _lib, ops
from danet_amd.hparams import hparams
from danet_amd.model import Model
base = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
            NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
            INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig')
rng = np.random.RandomState(0)
src_h = ((rng.randn(2, 2, 6, 33) + 1j * rng.randn(2, 2, 6, 33)) * 3).astype(np.complex64)
noise_h = ((rng.randn(2, 6, 33) + 1j * rng.randn(2, 6, 33)) * 3).astype(np.complex64)
gain_h = np.asarray([0.37, 1.9], np.float32)
src, noise, gain = (torch.as_tensor(a).cuda() for a in (src_h, noise_h, gain_h))
res = {}
def mapped():
    return 'libdanet_neval' in open('/proc/self/maps').read()
def put(tag, out):
    torch.cuda.synchronize()
    res[tag] = {k: float(v) for k, v in out.items()}
    res[tag + '_hex'] = {k: float(v).hex() for k, v in out.items()}
    res[tag + '_keys'] = list(out)
    res[tag + '_mapped'] = mapped()
def build(**keys):
    hparams.reset(); hparams.load(dict(base, **keys)); hparams.digest()
    return Model('neval', device='cuda:0', seed=3).build()
# EVAL_SI_SDR null
model = build()
put('clean0', model.valid_step(src))
put('noisy_null', model.valid_step(src, s_noise=noise, s_noise_gain=gain))
put('clean1', model.valid_step(src))                      # a call made after: bit-identical to the one before
# the same through the core front-end fed C + 1 rows, the targets cut back to C
def oracle(s, n, g=None, want_mix=False):
    B, C, T, F = s.shape
    last = torch.view_as_real(n)
    if g is not None:
        last = last * g.view(B, 1, 1, 1)
    rows = torch.cat([s, torch.view_as_complex(last.contiguous())[:, None]], dim=1).contiguous()
    fe = ops.frontend(rows, want_mix=True)
    return dict(src_pwr=fe['src_pwr'][:, :C].contiguous(), mix_pwr=fe['mix_pwr'], mix_log=fe['mix_log'],
                phasor=fe['phasor'])
real = ops.noise_frontend
ops.noise_frontend = oracle
with torch.no_grad():
    o = model.forward_noisy(src, noise, gain, with_valid=True, with_train=False)
ops.noise_frontend = real
put('core', dict(loss=o['valid_loss'], SNR=o['valid_SNR']))
# EVAL_SI_SDR true
model = build(EVAL_SI_SDR=True)
put('clean_on', model.valid_step(src))
put('noisy_on', model.valid_step(src, s_noise=noise, s_noise_gain=gain))
put('noisy_nogain', model.valid_step(src, s_noise=noise))
put('gain0', model.valid_step(src, s_noise=noise, s_noise_gain=torch.zeros(2, device='cuda')))
with torch.no_grad():
    o = model.forward_noisy(src, noise, gain, with_valid=True, with_train=False)
    est = ops.reattach_phase(o['sep_pwr_valid'], o['phasor']).cpu().numpy()
    o1 = model.forward_noisy(src, noise, None, with_valid=True, with_train=False)
    est1 = ops.reattach_phase(o1['sep_pwr_valid'], o1['phasor']).cpu().numpy()
torch.cuda.synchronize()
res['ok'] = bool(ops.lstm_status_ok())
w = np.asarray(hparams.FFT_WND)
res['ref'] = [float(v) for v in NV.si_sdr_noisy(src_h, est, noise_h, gain_h, w, 16)[2]]
res['ref_nogain'] = [float(v) for v in NV.si_sdr_noisy(src_h, est1, noise_h, None, w, 16)[2]]
print('RESULT ' + json.dumps(res))
'''


def test_valid_step_with_and_without_noise():
    code = _MODEL_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split('RESULT ')[1])
    assert r['ok']
    # without noise arguments: today's step, bit-identical to a call made before, the library never mapped
    assert r['clean0_keys'] == r['clean1_keys'] == ['loss', 'SNR'] and r['clean0_hex'] == r['clean1_hex']
    assert not r['clean0_mapped'] and not r['clean1_mapped']
    # noise with the key null: exactly loss and SNR, those of the core front-end on C + 1 rows; nothing mapped
    assert r['noisy_null_keys'] == ['loss', 'SNR'] and not r['noisy_null_mapped'] and not r['core_mapped']
    assert r['noisy_null_hex'] == r['core_hex'] and r['noisy_null_hex']['loss'] != r['clean0_hex']['loss']
    # the key true
    assert r['clean_on_keys'] == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi'] and not r['clean_on_mapped']
    assert r['clean_on_hex']['loss'] == r['clean0_hex']['loss']
    for tag, ref in (('noisy_on', r['ref']), ('noisy_nogain', r['ref_nogain'])):
        assert r[tag + '_keys'] == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi', 'nSNR'] and r[tag + '_mapped']
        assert all(np.isfinite(v) for v in r[tag].values())
        for k, want in zip(('SI-SDR', 'SI-SDRi', 'nSNR'), ref):
            print('%s %s %.6f (float64 restatement %.6f)' % (tag, k, r[tag][k], want))
            assert abs(r[tag][k] - want) <= 1e-3, (tag, k, r[tag][k], want)
    assert r['noisy_on_hex']['loss'] == r['noisy_null_hex']['loss']
    # gain 0: the clean step's figures
    assert r['gain0']['SI-SDR'] == r['clean_on']['SI-SDR'] and r['gain0']['SI-SDRi'] == r['clean_on']['SI-SDRi']
    assert r['gain0']['nSNR'] == 100.0 and r['gain0_hex']['loss'] == r['clean0_hex']['loss']


# -------------------------------------------------------------------------------------- dataset
def _config(hp, root, **kw):
    base = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(root), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
                BATCH_SIZE=4, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=48)
    base.update(kw)
    hp.reset()
    hp.load(base)
    hp.digest()


def _dataset(hp, root, **kw):
    from danet_amd import datasets
    _config(hp, root, **kw)
    ds = datasets.WavDirData()
    ds.load_host(out=open(os.devnull, 'w'))
    ds.is_loaded = True
    return ds


def _same(a, b):
    bits = lambda t: (torch.view_as_real(t) if t.is_complex() else t).detach().cpu().contiguous().numpy().view(np.uint32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('neval') / 'tree'
    SR.write_tree(root, seed=4, n_per_subset=14)                     # train / test: `valid` is aliased to `test`
    return root


@pytest.fixture(scope='module')
def eval_noise(tmp_path_factory):
    '''held-out recordings: one below FFT_SIZE (skipped), two shorter than any batch, three longer than every batch'''
    d = tmp_path_factory.mktemp('neval') / 'held_out'
    lengths = [200, 700, 1500, 20000, 9000, 12000]
    NR.write_noise(d, lengths, seed=17)
    return str(d), lengths


SNR = (0.0, 15.0)


def _sweep_device(ds, subset, bs=8):
    from danet_amd import feed
    random.seed(4)
    out = []
    for b in ds.epoch_device(subset, bs, False, 'cuda', None):
        out.append(feed.NoisyBatch(b.src.clone(), b.noise.clone(), b.gain.clone())
                   if isinstance(b, feed.NoisyBatch) else b.clone())
    return out


@pytest.mark.parametrize('mix', [False, True])
def test_valid_and_test_carry_the_restated_noise_on_both_routes(hp, tree, eval_noise, mix):
    from danet_amd import feed, ops
    folder, lengths = eval_noise
    more = dict(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0) if mix else {}
    keys = dict(more, NOISE_EVAL_DIR=folder, NOISE_EVAL_SNR_MIN=SNR[0], NOISE_EVAL_SNR_MAX=SNR[1])
    bs, C = 8, 2
    ds = _dataset(hp, tree, **keys)
    assert ds.noise_eval_skipped == 1 and sorted(int(n) for n in ds.noise_eval_lengths) == sorted(lengths[1:])
    assert ds.noise_eval_power is None and ds._noise_eval_pool_dev == {}      # nothing before the first noisy batch
    ds_off = _dataset(hp, tree, **more)
    _config(hp, tree, **keys)
    window, cuts, wholes = cu(_window(256)), 0, 0
    for subset in ('valid', 'test'):
        dev = _sweep_device(ds, subset)
        assert len(dev) == 2 and all(isinstance(b, feed.NoisyBatch) for b in dev)
        ref_pw = np.asarray([M.mean_power(ds.noise_eval_pool_host[o:o + n])
                             for o, n in zip(ds.noise_eval_offsets, ds.noise_eval_lengths)])
        assert np.abs(ds.noise_eval_power - ref_pw).max() <= 1e-12 * ref_pw.max()
        # two sweeps give identical batches
        for a, b in zip(dev, _sweep_device(ds, subset)):
            assert _same(a.src, b.src) and _same(a.noise, b.noise) and _same(a.gain, b.gain)
        # the sources are the batches of the run without the keys
        clean = _sweep_device(ds_off, subset)
        assert len(clean) == 2
        for a, b in zip(dev, clean):
            assert torch.is_tensor(b) and _same(a.src, b) and tuple(a.src.shape[:2]) == (4, C)
        # noise and gains by their definition: the plan of the run without the keys, then tests/noise_ref.py
        ds_off.power = ds.power
        random.seed(4)
        items = list(ds_off.plan_epoch_reverb(subset, bs, False, None, crop=True))
        rng = np.random.RandomState([1337, ('train', 'valid', 'test').index(subset), 4])
        pool = cu(ds.noise_eval_pool_host)
        for a, (idx, T_max, _pads, beg, cnt, gains) in zip(dev, [it[:6] for it in items]):
            assert (gains is not None) == mix and (beg, cnt) == (0, T_max)
            ref = NR.plan(ds.power['test'][idx], gains, rng, C, ds.noise_eval_offsets, ds.noise_eval_lengths,
                          ds.noise_eval_power, T_max, SNR[0], SNR[1], 256, 64)
            assert np.array_equal(a.gain.cpu().numpy().view(np.uint32), ref['gains'].view(np.uint32))
            desc = ops.prep_desc(ref['offsets'], ref['lengths'], ref['pads'], T_max, pool.numel(), 256, 64)
            X = ops.stft_batch(pool, desc, T_max, window, 256, 64, t_begin=0, t_count=T_max)
            assert tuple(a.noise.shape) == (4, T_max, 129) and _same(a.noise, X) and float(a.noise.abs().max()) > 0
            cuts += int((ref['lengths'] == NR.full_length(T_max, 64)).sum())
            wholes += int((ref['lengths'] < NR.full_length(T_max, 64)).sum())
        # epoch() through BatchFeed (no crop): the noise arrives scaled, and the front-end gives the same bits
        random.seed(4)
        src = feed.EpochSource(ds, subset, bs, shuffle=False)
        src.device = torch.device('cuda', 0)
        host = []
        for b in feed.BatchFeed(src, 'cuda', None):
            assert isinstance(b, feed.NoisyBatch) and b.gain is None
            host.append(ops.noise_frontend(b.src, b.noise, None, want_mix=True))
        assert len(host) == len(dev)
        for a, fe_host in zip(dev, host):
            fe_dev = ops.noise_frontend(a.src, a.noise, a.gain, want_mix=True)
            for k in ('src_pwr', 'mix_pwr', 'mix_log', 'phasor', 'mix'):
                assert _same(fe_dev[k], fe_host[k]), k
            assert not _same(fe_dev['mix_pwr'], ops.frontend(a.src)['mix_pwr'])
    assert cuts and wholes                    # both segment cases were drawn
    # `valid` (aliased to `test`) draws from its own subset index
    v, t = _sweep_device(ds, 'valid'), _sweep_device(ds, 'test')
    # (with the MIX_* keys the mix stream has the subset index too: the sources then differ as well)
    assert _same(v[0].src, t[0].src) == (not mix) and not _same(v[0].gain, t[0].gain)
    assert not _same(v[0].noise, t[0].noise)
    assert ds._noise_pool_dev == {} and ds.noise_power is None and ds._noise_rng == {}      # the train pool: untouched


def test_keys_null_launch_nothing_and_train_is_unchanged_by_the_eval_keys(hp, tree, eval_noise, monkeypatch):
    from danet_amd import feed, ops
    folder, _lengths = eval_noise
    keys = dict(NOISE_EVAL_DIR=folder, NOISE_EVAL_SNR_MIN=SNR[0], NOISE_EVAL_SNR_MAX=SNR[1])
    launches = []
    real = ops.stft_batch
    monkeypatch.setattr(ops, 'stft_batch', lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    ds_off = _dataset(hp, tree)
    got = {s: _sweep_device(ds_off, s) for s in ('valid', 'test')}
    assert len(launches) == 4 and all(torch.is_tensor(b) for s in got for b in got[s])     # one launch per batch
    assert ds_off.noise_eval_pool_host is None and ds_off._noise_eval_pool_dev == {} and ds_off.noise_eval_power is None
    assert all(len(pt) == 1 for pt in ds_off.epoch('valid', 8, shuffle=False))

    def train(ds):
        random.seed(21)
        np.random.seed(22)
        return [b.clone() for b in ds.epoch_device('train', 8, True, 'cuda', 48)], random.getstate(), \
            np.random.get_state()[1].copy()
    a, r0, n0 = train(ds_off)
    del launches[:]
    b, r1, n1 = train(_dataset(hp, tree, **keys))
    assert len(a) == len(b) == 2 and all(torch.is_tensor(y) and _same(x, y) for x, y in zip(a, b))
    assert r0 == r1 and np.array_equal(n0, n1) and len(launches) == 2                       # no noise launch in train


# ------------------------------------------------------------------------------------------ CLI
def test_command_line_valid_prints_nsnr_and_a_bad_value_names_the_key(tmp_path):
    P.write_tree(tmp_path / 'tree', seed=7, n_per_subset=8, subsets=('train', 'test'), seconds=(0.2, 0.4))
    NR.write_noise(tmp_path / 'held_out', [40, 900, 6000, 2500])
    base = dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2,
                LSTM_HDIM=8, NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
                INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64,
                DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'), EVAL_SI_SDR=True,
                NOISE_EVAL_DIR=str(tmp_path / 'held_out'), NOISE_EVAL_SNR_MIN=5, NOISE_EVAL_SNR_MAX=5)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)

    def main(**keys):
        cfg = tmp_path / 'cfg.json'
        cfg.write_text(json.dumps(dict(base, **keys)))
        return subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'neval', '-m', 'valid', '-ds',
                               'wavdir', '-c', str(cfg)], cwd=str(tmp_path), capture_output=True, text=True,
                              timeout=600, env=env)

    out = main()
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'NOISE_EVAL_DIR' in out.stdout and '3 files, 1 shorter than FFT_SIZE skipped' in out.stdout
    line = out.stdout.split('Valid: ')[1].splitlines()[0]
    assert line.index('loss=') < line.index('SNR=') < line.index('SI-SDR=') < line.index('SI-SDRi=') < line.index('nSNR=')
    for k in ('SI-SDR=', 'SI-SDRi=', 'nSNR='):
        assert np.isfinite(float(line.split(k)[1].split()[0])), line
    bad = main(NOISE_EVAL_SNR_MAX=75)
    assert bad.returncode != 0 and 'NOISE_EVAL_SNR_MAX' in bad.stderr, bad.stdout[-2000:] + bad.stderr[-2000:]
