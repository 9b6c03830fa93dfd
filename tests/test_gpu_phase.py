'''
GPU tests of the MISI phase refinement (PHASE_REFINE_ITERS, include/danet_phase_hip.h) against the float64 restatement
of tests/phase_ref.py.  Every output and the workspace lie between poisoned guard bands.

(a) one danet_phase_project call from the GPU's own waveforms against float64, over the envelope: the transform (z_out)
    within 1e-5 of that signal's max |Z| (the project's standing bar for the synthesis), the normalisation within
    8 * 2^-24 * A per part of A Z / |Z| formed in float64 from the KERNEL's z_out (one rounding each for the two
    products and the sum of m2, the square root, the division and the product: 6 * 2^-25, doubled for slack, rounded
    up); the float32 restatement's own transform error is printed beside the kernel's;
(b) danet_phase_init: A within 2 * 2^-24 * A, x and the mixture sum bit for bit, y within the synthesis bar;
(c) a chain of K = 3 checked one step at a time, each against one float64 step from the GPU's own previous x;
(d) invariants of ops.phase_refine; (e) descent of the objective on the GPU's iterates; (f) the SI-SDR rise with
oracle magnitudes; (g) Model.infer / infer_long / valid_step / `main.py -m demo` with the key null and set.
'''
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metric_ref as MR
import phase_ref as PR
from gpu_helpers import ROOT, check_lstm_status

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
POISON = -7.25e33
GUARD = 1024
BYTE_POISON = 0xA5
GRID = [(64, 8), (64, 16), (64, 32), (256, 64), (1024, 256), (1024, 512)]
BC = [(1, 1), (3, 2), (2, 4)]


def _guarded_c64(shape):
    '''(whole float32 buffer, the complex64 view of `shape` in its middle): everything poisoned'''
    n = 2 * int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device='cuda')
    return buf, torch.view_as_complex(buf[GUARD:GUARD + n].view(tuple(shape) + (2,)))


def _guarded_ws(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), BYTE_POISON, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf):
    poison = BYTE_POISON if buf.dtype == torch.uint8 else POISON
    return bool((buf[:GUARD] == poison).all()) and bool((buf[-GUARD:] == poison).all())


def _bits(t):
    a = torch.view_as_real(t) if t.is_complex() else t
    return a.detach().cpu().contiguous().numpy().view(np.uint32).copy()


def _host_bits(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.uint32).reshape(a.shape + (2,))


def _put(view, host):
    view.copy_(torch.as_tensor(np.ascontiguousarray(host)).cuda())


def _times(N, S):
    return sorted({2, 3, N // S, N // S + 1, 9, 40} - {1})


def _spectra(B, C, Cm, T, N, S, seed):
    '''random spectra that are no consistent STFTs -> (est0 [B, C, T, F], mixrows [B, Cm, T, F], blank).  With T > N/S
    the first N/S frames of utterance 0 are blank in every row -- zero, but for the imaginary parts of bins 0 and N/2
    of frame 0 (real parts -0), which the synthesis ignores -- so that all its waveforms are zero over more than the
    window of frame 0 and Z[0, :, 0, :] is exactly 0 while A is not, in every iteration (the other blank frames have
    A = 0 and stay zero); a few bins elsewhere have A = 0 too'''
    rng = np.random.RandomState(seed)
    F = N // 2 + 1
    est0 = (rng.standard_normal((B, C, T, F)) + 1j * rng.standard_normal((B, C, T, F))).astype(np.complex64)
    mixrows = (rng.standard_normal((B, Cm, T, F)) + 1j * rng.standard_normal((B, Cm, T, F))).astype(np.complex64)
    est0[rng.random_sample(est0.shape) < 0.02] = 0
    nz = N // S
    blank = T > nz
    if blank:
        est0[0, :, :nz] = 0
        mixrows[0, :, :nz] = 0
        edge = (1j * (0.5 + rng.random_sample((C, 2)))).astype(np.complex64)
        edge.real[...] = -0.0
        est0[0, :, 0, 0], est0[0, :, 0, F - 1] = edge[:, 0], edge[:, 1]
    return est0, mixrows, blank


class _Run(object):
    '''est0, mixrows on the device between guards, a guarded workspace and x: init done'''

    def __init__(self, est0, mixrows, w, S, alias=False):
        from danet_amd import ops
        self.ops, self.S = ops, S
        B, C, T, F = est0.shape
        self.shape = (B, C, T, 2 * (F - 1), S)
        self.w = torch.as_tensor(w).cuda()
        self.est_buf, self.est0 = _guarded_c64(est0.shape)
        _put(self.est0, est0)
        self.mix_buf, self.mixrows = _guarded_c64(mixrows.shape)
        _put(self.mixrows, mixrows)
        self.ws_buf, self.ws = _guarded_ws(ops.phase_workspace_bytes(*self.shape))
        if alias:
            self.x_buf, self.x = self.est_buf, self.est0
        else:
            self.x_buf, self.x = _guarded_c64(est0.shape)
        self.z_buf, self.z = _guarded_c64(est0.shape)
        got = ops.phase_init(self.est0, self.mixrows, self.w, self.ws, S, x=self.x)
        assert got is self.x

    def parts(self):
        return [p.cpu().numpy() for p in self.ops.phase_parts(self.ws, *self.shape)]

    def step(self, z_out=True):
        self.ops.phase_synth(self.x, self.w, self.ws, self.S)
        self.ops.phase_project(self.x, self.w, self.ws, self.S, z_out=self.z if z_out else None)

    def intact(self):
        return all(_intact(b) for b in (self.est_buf, self.mix_buf, self.ws_buf, self.x_buf, self.z_buf))


def _check_projection(run, x_old, blank, where, constructed=True):
    '''after run.step(): z_out against float64 from the GPU's own waveforms, x against its own z_out -> the largest
    transform error of the kernel and of the float32 restatement, over the signal's max |Z|'''
    B, C, T, N, S = run.shape
    w = run.w.cpu().numpy()
    A, _, wav = run.parts()
    z = PR.redistribute(wav[:, :C], wav[:, C])
    Z = PR.analyse(z, w, S, T)
    top = np.abs(Z).max(axis=(-2, -1), keepdims=True)
    assert (top > 0).all(), where
    mag = np.abs(Z)
    # (a) constructs its inputs so that |Z| is exactly 0 or well away from it; the iterates of (c) are what they are
    assert not constructed or ((mag == 0) | (mag > 1e-6 * top)).all(), (where, float((mag[mag > 0] / np.broadcast_to(top, mag.shape)[mag > 0]).min()))
    if blank:
        assert not Z[0, :, 0].any() and A[0, :, 0, 0].all(), where
    got_z = run.z.cpu().numpy()
    err = float((np.abs(got_z - Z) / top).max())
    z32 = PR.analyse(PR.redistribute(wav[:, :C], wav[:, C], np.float32), w, S, T, np.float32)
    err32 = float((np.abs(z32 - Z) / top).max())
    assert err <= 1e-5, (where, err, err32)
    # the normalisation, from the kernel's own transform
    zr, zi = got_z.real, got_z.imag
    m2 = zr * zr + zi * zi
    assert m2.dtype == np.float32
    new = (m2 > 0) & np.isfinite(m2)
    assert np.array_equal(new, mag > 0), where
    got_x = run.x.cpu().numpy()
    want, _ = PR.project(got_z, A, x_old)
    x32 = PR.project(got_z, A, x_old, np.float32)[0]          # the float32 restatement's own normalisation error
    live = new & (A > 0)
    norm = [0.0, 0.0]                                         # the kernel's, the restatement's, in units of 2^-24 A
    for part in ('real', 'imag'):
        d = np.abs(getattr(got_x, part).astype(np.float64) - getattr(want, part))
        d32 = np.abs(getattr(x32, part).astype(np.float64) - getattr(want, part))
        if live.any():
            norm = [max(norm[0], float((d[live] / A[live]).max() / U)), max(norm[1], float((d32[live] / A[live]).max() / U))]
        assert (d <= 8 * U * A)[new].all(), (where, part, norm)
    assert norm[1] <= 4.0, (where, norm)                      # (beyond half the bar the bar would have to be re-derived)
    # the old value where the transform is exactly zero, and +0 where A is
    assert np.array_equal(_bits(run.x)[~new], _host_bits(x_old)[~new]), where
    assert not _bits(run.x)[new & (A == 0)].any(), where
    if blank:
        assert (~new[0, :, 0]).all() and (A == 0).any(), where
    return err, err32, norm[0], norm[1]


# ------------------------------------------------------------------------------------ (a) project
@pytest.mark.parametrize('N,S', GRID)
def test_project_against_float64(N, S):
    w = PR.window('sqrt_hann', N)
    worst = (0.0, 0.0, 0.0, 0.0)
    for T in _times(N, S):
        for i, (B, C) in enumerate(BC):
            Cm = (1, C, 4)[(T + i) % 3]
            est0, mixrows, blank = _spectra(B, C, Cm, T, N, S, seed=1000 * N + 10 * T + i)
            run = _Run(est0, mixrows, w, S)
            run.step()
            first = (_bits(run.x), _bits(run.z))
            err = _check_projection(run, est0, blank, (N, S, T, B, C))
            worst = tuple(max(a, b) for a, b in zip(worst, err))
            # a second call from the same start: bit for bit
            _put(run.x, est0)
            run.step()
            assert np.array_equal(first[0], _bits(run.x)) and np.array_equal(first[1], _bits(run.z)), (N, S, T, B, C)
            assert run.intact(), (N, S, T, B, C)
    print('project (N, S) = (%d, %d): transform error / max |Z|: kernel %.3g, float32 restatement %.3g; normalisation '
          'error / (2^-24 A): kernel %.2f, float32 restatement %.2f' % ((N, S) + worst))


# --------------------------------------------------------------------------------------- (b) init
@pytest.mark.parametrize('N,S,T,B,C,Cm,alias', [(64, 16, 9, 3, 2, 1, False), (64, 8, 2, 1, 1, 4, True),
                                                (256, 64, 40, 2, 4, 4, False), (1024, 512, 3, 2, 3, 2, True),
                                                (1024, 256, 40, 1, 2, 2, False)])
def test_init_against_float64(N, S, T, B, C, Cm, alias):
    w = PR.window('sqrt_hann' if N != 256 else 'hamming', N)
    est0, mixrows, _ = _spectra(B, C, Cm, T, N, S, seed=N + T)
    run = _Run(est0, mixrows, w, S, alias=alias)
    A, mix, wav = run.parts()
    A_ref, _, _, _ = PR.start(est0, mixrows, w, S)
    assert (np.abs(A - A_ref) <= 2 * U * A_ref).all() and not A[est0 == 0].any()
    assert np.array_equal(_bits(run.x), _host_bits(est0))
    want_mix = PR.mixture(mixrows, np.float32)
    assert want_mix.dtype == np.complex64
    assert np.array_equal(mix.view(np.float32).view(np.uint32), want_mix.view(np.float32).view(np.uint32))
    y_ref = MR.synth(mix, w, S)                              # from the GPU's own (bit-checked) mixture sum
    top = np.abs(y_ref).max(axis=-1, keepdims=True)
    err = float((np.abs(wav[:, C] - y_ref) / top).max())
    err32 = float((np.abs(MR.synth(mix, w, S, np.float32) - y_ref) / top).max())
    print('init y: error / max |y|: kernel %.3g, float32 restatement %.3g' % (err, err32))
    assert err <= 1e-5
    # rows 0..C-1 of wav and the padding between the parts are nobody's to write yet
    raw = run.ws.cpu().numpy()
    F, Ls = N // 2 + 1, (T - 1) * S
    sizes = [B * C * T * F * 4, B * T * F * 8, B * (C + 1) * Ls * 4]
    off = 0
    for n in sizes:
        end = off + ((n + 255) & ~255)
        assert (raw[off + n:end] == BYTE_POISON).all()
        off = end
    assert off == raw.size
    rows = raw[off - ((sizes[2] + 255) & ~255):][:sizes[2]].reshape(B, C + 1, Ls * 4)
    assert (rows[:, :C] == BYTE_POISON).all()
    assert run.intact()


# -------------------------------------------------------------------------------------- (c) chain
@pytest.mark.parametrize('N,S,T,B,C', [(64, 16, 9, 3, 2), (256, 64, 40, 2, 4), (1024, 512, 10, 1, 3), (64, 8, 9, 2, 1)])
def test_a_chain_of_three_one_step_at_a_time(N, S, T, B, C):
    w = PR.window('sqrt_hann', N)
    est0, mixrows, blank = _spectra(B, C, C, T, N, S, seed=7 * N + T)
    run = _Run(est0, mixrows, w, S)
    A = run.parts()[0]
    y = MR.synth(PR.mixture(mixrows, np.float32), w, S)
    sum_w = float(w.astype(np.float64).sum())
    for k in range(3):
        x_old = run.x.cpu().numpy()
        run.step()
        # (1) the kernel's step against ONE float64 step from the GPU's own previous x: the synthesis bar on every
        # waveform (own row + (y + C rows) / C: at most 3e-5 of the largest sample), carried through the analysis
        # (|dZ| <= sum(w) max |dz|), plus the transform's own bar
        Z = PR.analysis_of(x_old, y, w, S)
        x64 = MR.synth(x_old, w, S)
        big = max(np.abs(x64).max(axis=(1, 2)).max(), np.abs(y).max())
        top = np.abs(Z).max(axis=(-2, -1), keepdims=True)
        err = np.abs(run.z.cpu().numpy() - Z)
        print('chain step %d: |dZ| / max |Z| = %.3g' % (k, float((err / top).max())))
        assert (err <= 1e-5 * top + 3e-5 * sum_w * big).all(), (k, float((err / top).max()))
        # (2) and against float64 from its own waveforms and transform, at the bars of (a)
        _check_projection(run, x_old, blank, (N, S, T, B, C, k), constructed=k == 0)
    assert np.array_equal(run.parts()[0], A) and run.intact()


# --------------------------------------------------------------------------------- (d) invariants
@pytest.mark.parametrize('N,S,T,B,C,Cm', [(64, 16, 9, 3, 2, 1), (256, 64, 40, 2, 4, 4), (1024, 256, 5, 1, 3, 3)])
def test_invariants_of_phase_refine(N, S, T, B, C, Cm):
    from danet_amd import ops
    w = torch.as_tensor(PR.window('sqrt_hann', N)).cuda()
    est0_h, mixrows_h, blank = _spectra(B, C, Cm, T, N, S, seed=N + 3 * T)
    est0, mixrows = torch.as_tensor(est0_h).cuda(), torch.as_tensor(mixrows_h).cuda()
    in_bits = _bits(est0)
    A = PR.magnitudes(est0_h, np.float32).astype(np.float64)
    for K in (0, 1, 5):
        x = ops.phase_refine(est0, mixrows, K, fft_stride=S, window=w)
        assert x.data_ptr() != est0.data_ptr() and x.dtype == torch.complex64 and x.shape == est0.shape
        got = x.cpu().numpy().astype(np.complex128)
        assert (np.abs(np.abs(got) - A) <= 4 * U * A).all(), K
        assert np.array_equal(_bits(est0), in_bits)                              # the input is never written
        if K == 0:
            assert np.array_equal(_bits(x), in_bits)
        else:
            assert not np.array_equal(_bits(x), in_bits)
            assert (A == 0).any() and not _bits(x)[A == 0].any()                 # A = 0: both parts +0
            if blank:                                                           # exactly-zero bins keep the old value
                assert A[0, :, 0, 0].all() and np.array_equal(_bits(x)[0, :, 0], in_bits[0, :, 0])
        again = ops.phase_refine(est0, mixrows, K, fft_stride=S, window=w)
        assert np.array_equal(_bits(again), _bits(x)), K


def test_launch_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    N, S, T, B, C = 64, 16, 9, 2, 2
    est0, mixrows, _ = _spectra(B, C, 1, T, N, S, seed=5)
    run = _Run(est0, mixrows, PR.window('sqrt_hann', N), S)
    run.step()
    before = [b.clone() for b in (run.est_buf, run.mix_buf, run.ws_buf, run.x_buf, run.z_buf)]
    lib, st, p = _lib.load_phase(), _lib.stream(), _lib.ptr
    x, z, ws, wd = (p(torch.view_as_real(run.x)), p(torch.view_as_real(run.z)), p(run.ws), p(run.w))
    e0, mr = p(torch.view_as_real(run.est0)), p(torch.view_as_real(run.mixrows))
    for rc in (lib.danet_phase_project(st, B, C, T, N, S, wd, ws, x, x), lib.danet_phase_project(st, B, C, T, N, 4, wd, ws, x, z),
               lib.danet_phase_project(st, B, 5, T, N, S, wd, ws, x, z), lib.danet_phase_project(st, B, C, T, N, S, wd, ws, x + 4, z),
               lib.danet_phase_project(st, B, C, T, N, S, wd, None, x, z), lib.danet_phase_project(st, B, C, 1, N, S, wd, ws, x, z),
               lib.danet_phase_synth(st, B, C, T, 96, S, x, wd, ws), lib.danet_phase_synth(st, B, C, T, N, S, x, wd + 2, ws),
               lib.danet_phase_synth(st, 0, C, T, N, S, x, wd, ws), lib.danet_phase_init(st, B, C, 5, T, N, S, e0, mr, wd, ws, x),
               lib.danet_phase_init(st, B, C, 1, T, N, S, e0, None, wd, ws, x),
               lib.danet_phase_init(st, B, C, 1, T, N, 40, e0, mr, wd, ws, x)):
        assert rc == -1
    with pytest.raises(_lib.DanetHipError):
        ops.phase_workspace_bytes(B, 5, T, N, S)
    torch.cuda.synchronize()
    for a, b in zip(before, (run.est_buf, run.mix_buf, run.ws_buf, run.x_buf, run.z_buf)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------------ (e) descent
@pytest.mark.parametrize('N,S,T,C,wname', PR.DESCENT_CASES)
def test_the_objective_falls_on_the_gpus_iterates(N, S, T, C, wname):
    est0, src, w = PR.oracle_case(1, C, T, N, S, wname, seed=3)
    A, _, y, _ = PR.start(est0, src, w, S)
    run = _Run(est0, src, w, S)
    J = [PR.objective_of(est0, A, y, w, S)]
    for k in range(12):
        run.step(z_out=False)
        J.append(PR.objective_of(run.x.cpu().numpy(), A, y, w, S))
    print('J_k / J_0: %s' % np.round(np.asarray(J) / J[0], 5).tolist())
    assert all(J[k + 1] < J[k] for k in range(12)), J
    assert run.intact()


# ------------------------------------------------------------------------------------- (f) oracle
def test_si_sdr_rises_with_oracle_magnitudes(hp):
    from danet_amd import ops
    hp.digest()
    N, S, T, B, C, K = 256, 64, 40, 2, 2, 8
    assert (hp.FFT_SIZE, hp.FFT_STRIDE) == (N, S)
    est0_h, src_h, w = PR.oracle_case(B, C, T, N, S, seed=0)
    assert np.array_equal(w, np.asarray(hp.FFT_WND, np.float32))
    want = [MR.si_sdr(src_h, PR.refine(est0_h, src_h, w, S, k), w, S)[2][0] for k in (0, K)]
    est0, src = torch.as_tensor(est0_h).cuda(), torch.as_tensor(src_h).cuda()
    got = [float(ops.si_sdr(src, ops.phase_refine(est0, src, k))[0]) for k in (0, K)]
    print('SI-SDR with oracle magnitudes, K = 0 -> %d: GPU %.3f -> %.3f dB, float64 %.3f -> %.3f dB'
          % (K, got[0], got[1], want[0], want[1]))
    assert want[1] - want[0] > 6.0 and got[1] - got[0] >= 0.5 * (want[1] - want[0])


# -------------------------------------------------------------------------------------- (g) model
_MODEL_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import __graft_entry__ as g
g.load_package()
from danet_amd import _lib, ops
from danet_amd.hparams import hparams
from danet_amd.model import Model
base = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
            NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
            INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig')
rng = np.random.RandomState(0)
src = torch.as_tensor(((rng.randn(2, 2, 6, 33) + 1j * rng.randn(2, 2, 6, 33)) * 3).astype(np.complex64)).cuda()
mix = src.sum(1)
long_mix = torch.as_tensor(((rng.randn(1, 50, 33) + 1j * rng.randn(1, 50, 33)) * 3).astype(np.complex64)).cuda()
bits = lambda t: torch.view_as_real(t).cpu().numpy().view(np.uint32).tolist()
mapped = lambda: 'libdanet_phase' in open('/proc/self/maps').read()
res = {}
def build(**keys):
    hparams.reset(); hparams.load(dict(base, **keys)); hparams.digest()
    return Model('phase', device='cuda:0', seed=3).build()
def run(tag, **keys):
    model = build(**keys)
    res[tag + '_infer'] = bits(model.infer(mix))
    res[tag + '_valid'] = {k: float(v).hex() for k, v in model.valid_step(src).items()}
    torch.cuda.synchronize()
    res[tag + '_mapped'] = mapped()
    return model
run('never')
run('never_si', EVAL_SI_SDR=True)
run('null', PHASE_REFINE_ITERS=None)
model = run('null_si', PHASE_REFINE_ITERS=None, EVAL_SI_SDR=True)
with torch.no_grad():
    o = model.forward(src, with_valid=True, with_train=False)
    est = ops.reattach_phase(o['sep_pwr_valid'], o['phasor'])
null_infer = model.infer(mix)
res['state_null'] = model.phase_refine is None
model = build(BATCH_SIZE=1, INFER_CHUNK_LEN=16, INFER_CHUNK_OVERLAP=4)
null_long = model.infer(long_mix)
res['long_shape'] = list(null_long.shape)
res['unmapped_before_the_key'] = not mapped() and _lib._phase is None
run('on', PHASE_REFINE_ITERS=2)
model = run('on_si', PHASE_REFINE_ITERS=2, EVAL_SI_SDR=True)
res['state_on'] = model.phase_refine
res['want_infer'] = bits(ops.phase_refine(null_infer, mix[:, None], 2))
res['want_si'] = [float(v).hex() for v in ops.si_sdr(src, ops.phase_refine(est, src, 2))[:2]]
res['unrefined_si'] = [float(v).hex() for v in ops.si_sdr(src, est)[:2]]
model = build(BATCH_SIZE=1, INFER_CHUNK_LEN=16, INFER_CHUNK_OVERLAP=4, PHASE_REFINE_ITERS=2)
res['long_equal'] = bits(model.infer(long_mix)) == bits(ops.phase_refine(null_long, long_mix[:, None], 2))
res['long_differs'] = bits(model.infer(long_mix)) != bits(null_long)
torch.cuda.synchronize()
res['ok'] = bool(ops.lstm_status_ok())
print('RESULT ' + json.dumps(res))
'''


@functools.lru_cache(maxsize=None)
def _run_model():
    code = _MODEL_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split('RESULT ')[1])
    assert r['ok']
    return r


def test_model_with_the_key_null():
    '''infer and valid_step return what they returned before the key was ever set, bit for bit, and the library is
    never mapped'''
    r = _run_model()
    assert r['state_null'] and r['unmapped_before_the_key']
    for tag, never in (('null', 'never'), ('null_si', 'never_si')):
        assert not r[never + '_mapped'] and not r[tag + '_mapped']
        assert r[tag + '_infer'] == r[never + '_infer'] == r['never_infer']
        assert r[tag + '_valid'] == r[never + '_valid']
    assert list(r['never_valid']) == ['loss', 'SNR'] and list(r['never_si_valid']) == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi']


def test_model_with_the_key_set():
    r = _run_model()
    assert r['state_on'] == 2 and r['on_mapped'] and r['on_si_mapped']
    # valid_step: loss and SNR are the unrefined output's; with no waveform metric on, nothing else is there
    assert r['on_valid'] == r['never_valid']
    assert list(r['on_si_valid']) == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi']
    for k in ('loss', 'SNR'):
        assert r['on_si_valid'][k] == r['never_si_valid'][k], k
    assert [r['on_si_valid'][k] for k in ('SI-SDR', 'SI-SDRi')] == r['want_si'] != r['unrefined_si']
    assert [r['never_si_valid'][k] for k in ('SI-SDR', 'SI-SDRi')] == r['unrefined_si']
    # infer: the refinement of what the key-null model returns, against the mixture
    assert r['on_infer'] == r['on_si_infer'] == r['want_infer'] != r['never_infer']
    # infer_long: the stitched recording refined as a whole
    assert r['long_shape'] == [1, 2, 50, 33] and r['long_equal'] and r['long_differs']


def test_demo_mode_writes_what_infer_computes(hp, tmp_path, monkeypatch):
    import scipy.io.wavfile
    from danet_amd import cli, datasets, ops, utils
    monkeypatch.chdir(tmp_path)
    cfg = dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
               NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
               INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig', DATASET_TYPE='synth',
               PHASE_REFINE_ITERS=3)
    (tmp_path / 'cfg.json').write_text(json.dumps(cfg))
    wave = (datasets.speech_shaped_wave(np.random.RandomState(2), 8000, 8000)).astype(np.int16)
    scipy.io.wavfile.write('mix.wav', 8000, wave)
    out = io.StringIO()
    model = cli.main(['-n', 'refined', '-m', 'demo', '-if', 'mix.wav', '-c', 'cfg.json'], out=out)
    assert model.phase_refine == 3 and hp.BATCH_SIZE == 1
    x = torch.as_tensor(utils.load_wavfile('mix.wav').astype(np.complex64)).to(model.device)[None]
    sep = model.infer(x)
    model.phase_refine = None
    plain = model.infer(x)
    model.phase_refine = 3
    assert np.array_equal(_bits(sep), _bits(ops.phase_refine(plain, x[:, None], 3))) and not np.array_equal(_bits(sep), _bits(plain))
    model.check_status()
    for i in (1, 2):
        sr, y = scipy.io.wavfile.read('mix_separated_%d.wav' % i)
        assert sr == 8000 and np.isfinite(y).all() and np.abs(y).max() > 0
        utils.save_wavfile('direct_%d.wav' % i, sep[0, i - 1].cpu().numpy())
        assert open('direct_%d.wav' % i, 'rb').read() == open('mix_separated_%d.wav' % i, 'rb').read()
    check_lstm_status()
