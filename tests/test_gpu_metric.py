'''
GPU tests of the waveform metric of valid / test (run with -m gpu): the three kernels of libdanet_metric_hip.so,
each against the output it can be pinned on -- waveforms against the float64 restatement tests/metric_ref.py,
Gram matrices against math.fsum of the kernel's own waveforms, decibels against the restatement on the kernel's
own Gram matrices -- then ops.si_sdr end to end, Model.valid_step with the key off and on, and the command line.

Bars.  Synthesis: the project's 1e-5 STFT bar or twice the error of the float32 restatement, whichever is
larger, relative to each signal's max|y|.  Gram: 1e-9 of sqrt(G_ii G_jj), the bar of danet_mix_power.  Finalize:
1e-9 dB.  End to end: 1e-3 dB or twice |float32 restatement - float64 restatement|.
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
import prep_ref as P
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
    buf = torch.full((n + 2 * GUARD,), POISON if dtype.is_floating_point else -77, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, n):
    bad = POISON if buf.dtype.is_floating_point else -77
    return bool((buf[:GUARD] == bad).all()) and bool((buf[GUARD + n:] == bad).all())


# ------------------------------------------------------------------------------------ synthesis
@pytest.mark.parametrize('N,S', [(64, 16), (64, 32), (256, 64), (1024, 256)])
def test_synthesis_against_the_float64_restatement(N, S):
    from danet_amd import ops
    rng = np.random.RandomState(N + S)
    w = _window(N)
    wd = torch.from_numpy(w).cuda()
    worst = worst32 = 0.0
    for T in sorted({2, 3, N // S, N // S + 1, 9, 130}):
        for B, C in ((1, 1), (3, 2), (2, 4)):
            src, est = _spectra(rng, B, C, T, N), _spectra(rng, B, C, T, N, scale=0.5)
            assert np.abs(src[..., 0].imag).min() > 0 and np.abs(est[..., N // 2].imag).min() > 0
            Ls = (T - 1) * S
            buf, out = _guarded((B, 2 * C, Ls), torch.float32)
            got = ops.metric_synth(torch.from_numpy(src).cuda(), torch.from_numpy(est).cuda(), S, wd, out=out)
            first = got.cpu().numpy().copy()
            assert _guards_intact(buf, B * 2 * C * Ls), (T, B, C)
            X = np.concatenate([src, est], axis=1)
            ref = MR.synth(X, w, S)
            ref32 = MR.synth(X, w, S, np.float32)
            peak = np.abs(ref).max(axis=-1, keepdims=True)
            err = (np.abs(first - ref) / peak).max()
            err32 = (np.abs(ref32 - ref) / peak).max()
            worst, worst32 = max(worst, err), max(worst32, err32)
            assert np.isfinite(first).all() and err <= max(1e-5, 2 * err32), (T, B, C, err, err32)
            out.fill_(POISON)
            again = ops.metric_synth(torch.from_numpy(src).cuda(), torch.from_numpy(est).cuda(), S, wd, out=out)
            assert np.array_equal(again.cpu().numpy().view(np.uint32), first.view(np.uint32)), (T, B, C)
    print('N %d S %d: worst error %.3g of max|y| (float32 restatement %.3g)' % (N, S, worst, worst32))


def test_synthesis_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    wd = torch.from_numpy(_window(64)).cuda()
    x = torch.from_numpy(_spectra(np.random.RandomState(0), 1, 1, 1, 64)).cuda()
    buf, out = _guarded((1, 2, 0), torch.float32)
    with pytest.raises(_lib.DanetHipError, match='T must be >= 2'):
        ops.metric_synth(x, x, 16, wd, out=out)
    F = 49                                                           # N = 96: not a power of two
    x = torch.zeros(1, 1, 5, F, dtype=torch.complex64, device='cuda')
    buf2, out2 = _guarded((1, 2, 4 * 24), torch.float32)
    with pytest.raises(_lib.DanetHipError, match='power of two'):
        ops.metric_synth(x, x, 24, torch.ones(96, device='cuda'), out=out2)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all()) and bool((buf2 == POISON).all())


# ----------------------------------------------------------------------------------------- Gram
@pytest.mark.parametrize('Ls', [1, 63, 64, 65, 4097, 33024])
def test_gram_against_fsum(Ls):
    from danet_amd import ops
    rng = np.random.RandomState(Ls)
    for M in (2, 4, 8):
        for B in (1, 5):
            wav = (rng.standard_normal((B, M, Ls)) * 10.0 ** rng.uniform(-2, 2, (B, M, 1))).astype(np.float32)
            wd = torch.from_numpy(wav).cuda()
            buf, out = _guarded((B, M, M), torch.float64)
            G = ops.metric_gram(wd, out=out).cpu().numpy().copy()
            assert _guards_intact(buf, B * M * M)
            ref = MR.gram_fsum(wd.cpu().numpy())
            d = np.sqrt(np.einsum('bii->bi', ref))
            err = (np.abs(G - ref) / (d[:, :, None] * d[:, None, :])).max()
            assert err <= 1e-9, (M, B, err)
            assert np.array_equal(G.view(np.uint64), np.swapaxes(G, 1, 2).copy().view(np.uint64))
            out.fill_(POISON)
            again = ops.metric_gram(wd, out=out).cpu().numpy()
            assert np.array_equal(again.view(np.uint64), G.view(np.uint64))


# ------------------------------------------------------------------------------------- finalize
def _finalize_both(wav, C):
    '''the kernel and the restatement on the kernel's own Gram matrices of `wav` [B, 2C, L]'''
    from danet_amd import ops
    G = ops.metric_gram(torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).cuda())
    B = G.shape[0]
    bufs = [_guarded((B, 2), torch.float64), _guarded((B,), torch.int32), _guarded((2,), torch.float64)]
    mean2, per_utt, perm = ops.metric_finalize(G, out=tuple(v for _, v in bufs))
    got = per_utt.cpu().numpy().copy(), perm.cpu().numpy().copy(), mean2.cpu().numpy().copy()
    for (buf, _), n in zip(bufs, (2 * B, B, 2)):
        assert _guards_intact(buf, n)
    ref = MR.finalize(G.cpu().numpy(), C)
    assert np.abs(got[0] - ref[0]).max() <= 1e-9, (got[0], ref[0])
    assert np.array_equal(got[1], ref[1]), (got[1], ref[1])
    assert np.abs(got[2] - ref[2]).max() <= 1e-9
    return got


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_finalize_against_the_restatement_on_the_kernels_own_gram(C):
    rng = np.random.RandomState(C)
    B, L = 300, 96                                                   # more utterances than the workgroup has threads
    perms = list(itertools.permutations(range(C)))
    s = rng.standard_normal((B, C, L))
    want = rng.randint(0, len(perms), B)
    noise = 10.0 ** (-rng.uniform(-5, 30, (B, 1, 1)) / 20)
    e = np.zeros((B, C, L))
    for b in range(B):
        for i in range(C):
            e[b, perms[want[b]][i]] = s[b, i]                         # reference i is estimate p(i)
    e += noise * rng.standard_normal((B, C, L))
    s[5] *= 0                                                        # no live reference
    s[6, 0] *= 0                                                     # one silent reference
    per_utt, perm, mean2 = _finalize_both(np.concatenate([s, e], axis=1), C)
    assert np.array_equal(per_utt[5], [0.0, 0.0]) and perm[5] == 0
    clean = noise[:, 0, 0] < 0.1                                     # (20 dB and better: the drawn permutation wins)
    clean[[5, 6]] = False
    assert clean.sum() > 50 and np.array_equal(perm[clean], want[clean])
    assert per_utt[:, 0].min() < 0 and per_utt[:, 0].max() > 25 and np.isfinite(mean2).all()


def test_finalize_clamps_ties_silence_and_an_empty_batch():
    rng = np.random.RandomState(9)
    L = 64
    a, b = np.zeros(L), np.zeros(L)
    a[:32], b[32:] = rng.standard_normal(32), rng.standard_normal(32)        # disjoint support: exactly orthogonal
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)                      # (equal energy: +0.1 of the other is 20 dB)
    z = np.zeros(L)
    wav = np.stack([np.stack([a, b, a, b]),          # identical: 100 dB, identity
                    np.stack([a, b, b, a]),          # identical, swapped: 100 dB, permutation 1
                    np.stack([a, z, b, b]),          # orthogonal to the one live reference: -100
                    np.stack([a, b, a + b, a + b]),  # a tie: the first permutation
                    np.stack([z, z, a, b]),          # no live reference
                    np.stack([z, b, a, b + 0.1 * a])])   # one silent reference: 20 dB from the live one
    per_utt, perm, mean2 = _finalize_both(wav, 2)
    assert np.array_equal(per_utt[:3, 0], [100.0, 100.0, -100.0]) and np.array_equal(perm, [0, 1, 0, 0, 0, 0])
    assert np.array_equal(per_utt[4], [0.0, 0.0]) and abs(per_utt[5, 0] - 20.0) < 1e-4
    assert abs(mean2[0] - per_utt[[0, 1, 2, 3, 5], 0].mean()) <= 1e-9
    # a batch with no live utterance: 0
    per_utt, perm, mean2 = _finalize_both(wav[4:5].repeat(3, axis=0), 2)
    assert np.array_equal(mean2, [0.0, 0.0]) and not per_utt.any() and not perm.any()
    # C = 1: the mixture IS the reference, so the baseline is the +100 clamp
    per_utt, perm, _ = _finalize_both(np.stack([a, a + 0.1 * b])[None], 1)
    assert abs(per_utt[0, 0] - 20.0) < 1e-4 and abs(per_utt[0, 1] - (per_utt[0, 0] - 100.0)) <= 1e-9


# ----------------------------------------------------------------------------------- end to end
def _noisy_estimates(rng, src, db):
    '''estimates = references (swapped) + noise at about `db` [B] dB below them'''
    noise = _spectra(rng, *src.shape[:3], 2 * (src.shape[3] - 1))
    return (src[:, ::-1] + 10.0 ** (-np.asarray(db)[:, None, None, None] / 20) * noise).astype(np.complex64)


def _end_to_end_bar(src, est, w, S, got_per_utt, got_mean):
    ref, ref32 = MR.si_sdr(src, est, w, S), MR.si_sdr(src, est, w, S, np.float32)
    bar = np.maximum(1e-3, 2 * np.abs(ref32[0] - ref[0]))
    err = np.abs(got_per_utt - ref[0])
    assert (err <= bar).all(), (err, bar)
    assert (np.abs(got_mean - ref[2]) <= np.maximum(1e-3, 2 * np.abs(ref32[2] - ref[2]))).all()
    return ref, err.max(), np.abs(ref32[0] - ref[0]).max()


def test_si_sdr_end_to_end_against_the_restatement(hp):
    from danet_amd import ops
    hp.load(dict(FFT_SIZE=256, FFT_STRIDE=64))
    hp.digest()
    rng = np.random.RandomState(11)
    B, C, T, N, S = 8, 2, 40, 256, 64
    src = _spectra(rng, B, C, T, N)
    est = _noisy_estimates(rng, src, np.linspace(-5, 30, B))
    a, b, per_utt, perm = ops.si_sdr(torch.from_numpy(src).cuda(), torch.from_numpy(est).cuda())
    got_mean = np.array([float(a), float(b)])
    ref, worst, floor = _end_to_end_bar(src, est, np.asarray(hp.FFT_WND), S, per_utt.cpu().numpy(), got_mean)
    assert ref[0][:, 0].min() < -2 and ref[0][:, 0].max() > 27, ref[0][:, 0]       # the spread asked for
    assert np.all(np.diff(ref[0][:, 0]) > 0)
    assert np.array_equal(perm.cpu().numpy(), ref[1]) and np.array_equal(ref[1], [1] * B)
    assert a.dtype == torch.float64 and a.dim() == 0 and per_utt.shape == (B, 2)
    print('end to end: worst |kernel - float64| %.3g dB (float32 restatement %.3g dB)' % (worst, floor))
    # the outputs are the caller's own: the next call, of another batch, leaves them alone
    keep, keep_a = per_utt.clone(), float(a)
    ops.si_sdr(torch.from_numpy(est).cuda(), torch.from_numpy(src).cuda())
    torch.cuda.synchronize()
    assert torch.equal(keep, per_utt) and float(a) == keep_a


# ---------------------------------------------------------------------------------------- model
_MODEL_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import __graft_entry__ as g
g.load_package()
import metric_ref as MR
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
    model = Model('metric', device='cuda:0', seed=3).build()
    out = model.valid_step(src)
    torch.cuda.synchronize()
    res[tag] = {k: float(v) for k, v in out.items()}
    res[tag + '_hex'] = {k: float(v).hex() for k, v in out.items()}
    res[tag + '_keys'] = list(out)
    res[tag + '_mapped'] = 'libdanet_metric' in open('/proc/self/maps').read()
    return model
run('never')
run('null', EVAL_SI_SDR=None)
run('false', EVAL_SI_SDR=False)
model = run('on', EVAL_SI_SDR=True)
with torch.no_grad():
    o = model.forward(src, with_valid=True, with_train=False)
    est = ops.reattach_phase(o['sep_pwr_valid'], o['phasor']).cpu().numpy()
torch.cuda.synchronize()
res['ok'] = bool(ops.lstm_status_ok())
for tag, dt in (('ref', np.float64), ('ref32', np.float32)):
    res[tag] = [float(v) for v in MR.si_sdr(src_h, est, np.asarray(hparams.FFT_WND), 16, dt)[2]]
print('RESULT ' + json.dumps(res))
'''


def test_valid_step_with_the_key_off_and_on():
    code = _MODEL_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split('RESULT ')[1])
    assert r['ok']
    for tag in ('never', 'null', 'false'):
        assert r[tag + '_keys'] == ['loss', 'SNR'] and not r[tag + '_mapped'], tag
        assert r[tag + '_hex'] == r['never_hex'], tag                 # bit for bit
    assert r['on_keys'] == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi'] and r['on_mapped']
    assert all(np.isfinite(v) for v in r['on'].values())
    assert r['on_hex']['loss'] == r['never_hex']['loss'] and r['on_hex']['SNR'] == r['never_hex']['SNR']
    for k, ref, ref32 in zip(('SI-SDR', 'SI-SDRi'), r['ref'], r['ref32']):
        print('%s %.6f (float64 restatement %.6f, float32 %.6f)' % (k, r['on'][k], ref, ref32))
        assert abs(r['on'][k] - ref) <= max(1e-3, 2 * abs(ref32 - ref)), (k, r['on'][k], ref, ref32)


# ------------------------------------------------------------------------------------------ CLI
def test_command_line_valid_prints_the_metric_and_a_bad_value_names_the_key(tmp_path):
    P.write_tree(tmp_path / 'tree', seed=7, n_per_subset=8, subsets=('train', 'test'), seconds=(0.2, 0.4))
    base = dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2,
                LSTM_HDIM=8, NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
                INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64,
                DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)

    def main(value):
        cfg = tmp_path / 'cfg.json'
        cfg.write_text(json.dumps(dict(base, EVAL_SI_SDR=value)))
        return subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'metric', '-m', 'valid', '-ds',
                               'wavdir', '-c', str(cfg)], cwd=str(tmp_path), capture_output=True, text=True,
                              timeout=600, env=env)

    out = main(True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = out.stdout.split('Valid: ')[1].splitlines()[0]
    assert line.index('loss=') < line.index('SNR=') < line.index('SI-SDR=') < line.index('SI-SDRi=')
    for k in ('SI-SDR=', 'SI-SDRi='):
        assert np.isfinite(float(line.split(k)[1].split()[0])), line
    bad = main('yes')
    assert bad.returncode != 0 and 'EVAL_SI_SDR' in bad.stderr, bad.stdout[-2000:] + bad.stderr[-2000:]
