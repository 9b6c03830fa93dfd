'''
GPU tests (run with -m gpu) of global-norm gradient clipping (GRAD_CLIP_NORM): danet_gclip_sumsq against math.fsum of
the exact float64 squares and the restatement tests/gclip_ref.py, danet_gclip_adam_step bit for bit against the core
library's danet_adam_clip_step launched with the factor the new kernel formed, the model with the key null / active
/ inert, the data-parallel scale, the gradient schedules, the early optimizer piece, SGD, and the command line.
'''
import functools
import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gclip_ref as GR
from oracle import torch_ref as R
from gpu_helpers import cfg_of, check_lstm_status, rand_src, small_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -7.25e33
GUARD = 1024                     # elements; a multiple of 4 (and of 2), so a view's residue is its offset's
ADAM_SWEEP = 2048 * 256 * 4      # elements one sweep of the optimizer kernel's grid covers on the 16-byte path
SUMSQ_SWEEP = GR.MAX_PARTIALS * GR.MIN_SLICE       # the largest n with slices of the minimum length
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, ADAM_SWEEP - 1, ADAM_SWEEP, ADAM_SWEEP + 1,
         SUMSQ_SWEEP - 1, SUMSQ_SWEEP, SUMSQ_SWEEP + 1, 1000003]
STEP_SIZES = [1, 5, 257, 1025, 1000003, ADAM_SWEEP + 1]


@functools.lru_cache(maxsize=None)
def _values():
    '''the gradient every kernel test takes a prefix of: magnitudes 1e-6 .. 1e4, both signs'''
    rng = np.random.RandomState(11)
    n = SUMSQ_SWEEP + 1
    return (10.0 ** rng.uniform(-6, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _fsum_squares(n):
    return math.fsum((_values()[:n].astype(np.float64) ** 2).tolist())


@functools.lru_cache(maxsize=None)
def _restated_partials(n, residue):
    p = GR.sumsq_partials(_values()[:n], residue)
    p.setflags(write=False)
    return p


def _guarded(n, dtype=torch.float32, offset=0, fill=None):
    '''(whole buffer, its view of n elements that starts `offset` elements behind an aligned address)'''
    buf = torch.full((n + 2 * GUARD + 4,), POISON, dtype=dtype, device='cuda')
    view = buf[GUARD + offset:GUARD + offset + n]
    assert view.data_ptr() % 16 == (offset * view.element_size()) % 16
    if fill is not None:
        view.copy_(torch.as_tensor(fill))
    return buf, view


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == POISON).all()) and bool((buf[lo + view.numel():] == POISON).all())


def _same_bits(a, b):
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------- sum of squares
@pytest.mark.parametrize('n', SIZES)
def test_sumsq_against_fsum_at_every_residue(n):
    from danet_amd import ops
    g = _values()[:n]
    want = _fsum_squares(n)
    P = GR.partials_of(n)
    assert ops.gclip_partials(n) == P
    bar = GR.sum_bar(n)
    for residue in range(4):
        gbuf, gv = _guarded(n, offset=residue, fill=g)
        pbuf, pv = _guarded(P, torch.float64)
        assert ops.grad_sumsq(gv, pv) is pv
        first = pv.clone()
        ops.grad_sumsq(gv, pv)
        torch.cuda.synchronize()
        assert _same_bits(first, pv), residue                        # repeats are bit-identical
        assert _guards_intact(pbuf, pv) and _guards_intact(gbuf, gv) and _same_bits(gv, torch.as_tensor(g).cuda())
        got = pv.cpu().numpy()
        err = abs(math.fsum(got.tolist()) - want) / want
        tot = abs(GR.total(got) - want) / want
        print('n %d residue %d: %d partials, relative error %.3g (fixed-tree total %.3g), bar %.3g'
              % (n, residue, P, err, tot, bar))
        assert err <= bar and tot <= bar, (n, residue)
        if n <= 1025 or n == 1000003:
            # the restatement's tree is the kernel's: a partial depends on (values, n, residue) and nothing else
            assert np.array_equal(got, _restated_partials(n, residue)), (n, residue)
    # a fresh allocation (another address, the same residue) gives the same bits
    again = ops.grad_sumsq(torch.as_tensor(g).cuda())
    gbuf, gv = _guarded(n, offset=0, fill=g)
    assert _same_bits(again, ops.grad_sumsq(gv))


# ------------------------------------------------------------------------------------- the fused step
HYPER = dict(lr_t=2.5e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def _state(n):
    rng = np.random.RandomState(n % 9973)
    theta = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.uniform(0, 1e-2, n)).astype(np.float32)
    return theta, m, v


def _run_both(g, theta, m, v, offsets, M, s, clip, zero_grad):
    '''the new kernel on guarded buffers and the core kernel on copies with the factor the new kernel formed
    -> (norm, coef, guards ok, {name: (new, core)})'''
    from danet_amd import ops
    n = g.size
    bufs = {}
    for name, a, off in (('theta', theta, offsets[0]), ('grad', g, offsets[1]), ('m', m, offsets[2]),
                         ('v', v, offsets[3])):
        bufs[name] = _guarded(n, offset=off, fill=a)
    P = GR.partials_of(n)
    bufs['partials'] = _guarded(P, torch.float64)
    bufs['norm_out'] = _guarded(2, torch.float64)
    pv, ov = bufs['partials'][1], bufs['norm_out'][1]
    ops.grad_sumsq(bufs['grad'][1], pv)
    ops.adam_gclip_step(bufs['theta'][1], bufs['grad'][1], bufs['m'][1], bufs['v'][1], clip=clip, grad_scale=s,
                        zero_grad=zero_grad, max_norm=M, partials=pv, norm_out=ov, **HYPER)
    norm, coef = ov.cpu().tolist()
    core = {name: _guarded(n, offset=off, fill=a)[1]
            for name, a, off in (('theta', theta, offsets[0]), ('grad', g, offsets[1]), ('m', m, offsets[2]),
                                 ('v', v, offsets[3]))}
    ops.adam_clip_step(core['theta'], core['grad'], core['m'], core['v'], clip=clip,
                       grad_scale=float(np.float32(s * coef)), zero_grad=zero_grad, **HYPER)
    torch.cuda.synchronize()
    ok = all(_guards_intact(b, w) for b, w in bufs.values())
    return norm, coef, ok, {name: (bufs[name][1], core[name]) for name in core}


@pytest.mark.parametrize('n', STEP_SIZES)
def test_fused_step_is_the_core_step_with_the_clip_factor(n):
    g = _values()[:n]
    theta, m, v = _state(n)
    bar = GR.sum_bar(n)
    for offsets in ((0, 0, 0, 0), (0, 1, 2, 3)):                     # the 16-byte path, and the scalar one
        S = GR.total(_restated_partials(n, offsets[1]))
        for s in (1.0, 0.5):
            norm_ref = GR.norm_coef(S, s, 1e30)[0]
            for M, clip, zero_grad in itertools.product((1e30, 0.25 * norm_ref), (0.0, 100.0), (0, 1)):
                want_norm, want_coef = GR.norm_coef(S, s, M)
                assert (want_coef < 1.0) == (M < 1e30)              # active / inactive by the restatement
                norm, coef, guards, pairs = _run_both(g, theta, m, v, offsets, M, s, clip, zero_grad)
                tag = (n, offsets, s, M, clip, zero_grad)
                assert guards, tag
                assert abs(norm - want_norm) <= (bar + GR.U) * want_norm, (tag, norm, want_norm)
                own = M / (norm + 1e-6) if norm + 1e-6 > M else 1.0
                assert abs(coef - own) <= GR.U * own, (tag, coef, own)           # the rule on its own norm
                assert abs(coef - want_coef) <= (bar + 3 * GR.U) * want_coef, (tag, coef, want_coef)
                assert (coef == 1.0) if M == 1e30 else (coef < 1.0), tag
                for name, (new, core) in pairs.items():
                    assert _same_bits(new, core), (tag, name)
                if zero_grad:
                    assert not bool(pairs['grad'][0].any()), tag
                assert not _same_bits(pairs['theta'][0], torch.as_tensor(theta).cuda()), tag
    print('n %d: norm %.17g against the restatement %.17g, bar %.3g' % (n, norm, want_norm, bar))


def test_a_nan_gradient_element_stays_in_its_element():
    n = 1030
    g = _values()[:n].copy()
    g[7] = np.nan
    theta, m, v = _state(n)
    norm, coef, guards, pairs = _run_both(g, theta, m, v, (0, 0, 0, 0), 1.0, 1.0, 100.0, 1)
    assert guards and math.isnan(norm) and coef == 1.0               # a NaN norm compares false
    t = pairs['theta'][0].cpu().numpy()
    assert np.isnan(t[7]) and np.isfinite(np.delete(t, 7)).all()
    for name, (new, core) in pairs.items():
        keep = torch.ones(n, dtype=torch.bool, device='cuda')
        keep[7] = False
        assert _same_bits(new[keep], core[keep]), name
    assert not bool(pairs['grad'][0].any())                          # zeroed after use


def test_an_infinite_gradient_element_gives_coefficient_zero():
    n = 1030
    g = _values()[:n].copy()
    g[3] = np.inf
    theta, m, v = _state(n)
    norm, coef, guards, pairs = _run_both(g, theta, m, v, (0, 0, 0, 0), 1.0, 1.0, 100.0, 0)
    assert guards and math.isinf(norm) and coef == 0.0
    for name, (new, core) in pairs.items():
        assert _same_bits(new, core), name
    got_m = pairs['m'][0].cpu().numpy()
    assert np.isnan(got_m[3]) and np.array_equal(np.delete(got_m, 3), np.delete(np.float32(0.9) * m, 3))


def test_argument_errors_launch_nothing():
    from danet_amd import _lib
    lib = _lib.load_gclip()
    n = 10000
    P = GR.partials_of(n)
    bufs = [torch.full((n,), POISON, device='cuda') for _ in range(4)]
    part = torch.full((P,), POISON, dtype=torch.float64, device='cuda')
    out = torch.full((2,), POISON, dtype=torch.float64, device='cuda')
    st = _lib.stream()
    ok = dict(stream=st, n=n, theta=bufs[0].data_ptr(), grad=bufs[1].data_ptr(), m=bufs[2].data_ptr(),
              v=bufs[3].data_ptr(), lr_t=1e-3, b1=0.9, b2=0.999, eps=1e-8, clip=100.0, grad_scale=1.0, zero_grad=1,
              max_norm=5.0, partials=part.data_ptr(), n_partials=P, norm_out=out.data_ptr())
    cases = [dict(n=0), dict(n=-5), dict(max_norm=0.0), dict(max_norm=-2.0), dict(max_norm=float('inf')),
             dict(max_norm=float('nan')), dict(n_partials=P + 1), dict(n_partials=P - 1), dict(n=n + 4096)]
    cases += [{k: None} for k in ('theta', 'grad', 'm', 'v', 'partials', 'norm_out')]
    for kw in cases:
        assert lib.danet_gclip_adam_step(*dict(ok, **kw).values()) == -1, kw
        assert lib.danet_gclip_last_error(), kw
    ok = dict(stream=st, n=n, grad=bufs[1].data_ptr(), partials=part.data_ptr(), n_partials=P)
    for kw in (dict(n=0), dict(grad=None), dict(partials=None), dict(n_partials=P + 1), dict(n=n + 4096)):
        assert lib.danet_gclip_sumsq(*dict(ok, **kw).values()) == -1, kw
        assert lib.danet_gclip_last_error(), kw
    torch.cuda.synchronize()
    for t in bufs + [part, out]:
        assert bool((t == POISON).all())


# ------------------------------------------------------------------------------------------ the model
SHAPE = dict(BATCH_SIZE=2, FFT_SIZE=16, FFT_STRIDE=4, EMBED_SIZE=3, NUM_LSTM_LAYERS=1, LSTM_HDIM=4,
             TRAIN_ESTIMATOR_METHOD='truth-weighted', SEPARATOR_TYPE='dot-sigmoid-orig')     # test_adam_parameters_to_1e5


@pytest.fixture
def lstm_status():
    yield
    check_lstm_status()


def _oracle_grads(src, tp, cfg):
    for k in tp:
        tp[k].grad = None
    R.model_forward(torch.tensor(src.astype(np.complex128)), tp, cfg)['loss'].backward()
    grads = {k: tp[k].grad for k in tp}
    sq = sum(float((g.double() ** 2).sum()) for g in grads.values() if g is not None)
    return grads, math.sqrt(sq)


def test_three_clipped_steps_against_float64_autograd(hp, lstm_status):
    '''the key at a quarter of the oracle's first-step norm: three steps against float64 autograd, the restated clip
    and the oracle's TF1 Adam; every parameter within 1e-5 of the tensor's maximum (the existing optimizer test's
    bar), grad_norm within 1e-5 relative of the oracle's, clip_coef below 1'''
    hp.load(dict(LR=3e-4))
    first = small_model(hp, **SHAPE)
    src = rand_src(hp, 6, 8, scale=6.0)
    cfg = cfg_of(hp)
    p0 = first.param_dict()
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p0.items()}
    M = 0.25 * _oracle_grads(src, tp, cfg)[1]
    hp.load(dict(GRAD_CLIP_NORM=M))
    model = small_model(hp, **SHAPE)
    assert model.grad_clip_norm == M
    for k in p0:
        assert np.array_equal(model.param_dict()[k], p0[k]), k
    m = {k: torch.zeros_like(v) for k, v in tp.items()}
    v = {k: torch.zeros_like(v_) for k, v_ in tp.items()}
    for t in (1, 2, 3):
        out = model.train_step(torch.as_tensor(src).cuda())
        assert list(out) == ['loss', 'SNR', 'LR', 'grad_norm', 'clip_coef']
        grads, norm = _oracle_grads(src, tp, cfg)
        assert norm + 1e-6 > M                                        # clipping is active, by the oracle
        coef = M / (norm + 1e-6)
        scaled = {k: (None if g is None else g * coef) for k, g in grads.items()}
        R.tf_adam_step_(tp, scaled, m, v, t, hp.LR, clip=hp.GRAD_CLIP_THRES)
        got_norm, got_coef = float(out['grad_norm']), float(out['clip_coef'])
        print('step %d: grad_norm %.9g, oracle %.9g (relative %.3g); clip_coef %.9g, oracle %.9g'
              % (t, got_norm, norm, abs(got_norm - norm) / norm, got_coef, coef))
        assert out['grad_norm'].dtype == torch.float64 and out['grad_norm'].is_cuda
        assert abs(got_norm - norm) <= 1e-5 * norm
        assert got_coef < 1.0 and abs(got_coef - coef) <= 2e-5 * coef
    p3 = model.param_dict()
    for k in p0:
        want = tp[k].detach().numpy()
        if tp[k].grad is None:
            assert np.array_equal(p3[k], p0[k]), k
            continue
        assert np.abs(p3[k] - want).max() <= 1e-5 * max(np.abs(want).max(), 1e-3), k


_NULL_SCRIPT = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import __graft_entry__ as g; g.load_package()
from danet_amd.hparams import hparams
from danet_amd import ops
from gpu_helpers import rand_src, small_model
SHAPE = %(shape)r
res = {}
def mapped():
    return 'libdanet_gclip' in open('/proc/self/maps').read()
def run(tag, **keys):
    hparams.reset()
    hparams.load(dict(LR=3e-4))
    hparams.load(keys)
    model = small_model(hparams, **SHAPE)
    src = torch.as_tensor(rand_src(hparams, 6, 8, scale=6.0)).cuda()
    outs = [model.train_step(src) for _ in range(3)]
    torch.cuda.synchronize()
    res[tag + '_keys'] = list(outs[-1])
    res[tag] = [[float(o['loss']).hex(), float(o['SNR']).hex()] for o in outs]
    res[tag + '_flat'] = model._flat.cpu().numpy().view(np.uint32).tolist()
    res[tag + '_norm'] = model.grad_clip_norm
    res[tag + '_mapped'] = mapped()
    return outs
run('never')                                  # built before the key is ever set
run('null', GRAD_CLIP_NORM=None)
outs = run('inert', GRAD_CLIP_NORM=1e30)
res['inert_coef'] = [float(o['clip_coef']) for o in outs]
res['inert_grad_norm'] = [float(o['grad_norm']) for o in outs]
res['ok'] = bool(ops.lstm_status_ok())
print('RESULT ' + json.dumps(res))
'''


def test_the_key_null_is_todays_step_and_the_key_at_1e30_moves_nothing():
    code = _NULL_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), shape=SHAPE)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split('RESULT ')[1])
    assert r['ok']
    for tag in ('never', 'null'):
        assert r[tag + '_keys'] == ['loss', 'SNR', 'LR'] and r[tag + '_norm'] is None, tag
        assert not r[tag + '_mapped'], tag                           # the library is never loaded
        assert r[tag] == r['never'] and r[tag + '_flat'] == r['never_flat'], tag          # bit for bit
    assert r['inert_keys'] == ['loss', 'SNR', 'LR', 'grad_norm', 'clip_coef'] and r['inert_mapped']
    assert r['inert_norm'] == 1e30 and r['inert_coef'] == [1.0, 1.0, 1.0]
    assert all(math.isfinite(x) and x > 0 for x in r['inert_grad_norm'])
    assert r['inert'] == r['never'] and r['inert_flat'] == r['never_flat']               # k = s exactly


def _three_steps(hp, monkeypatch=None, schedule='0', early=False, M=1e-2, **keys):
    if monkeypatch is not None:
        monkeypatch.setenv('DANET_OVERLAP_ALLREDUCE', schedule)
    hp.reset()
    hp.load(dict(LR=3e-4, GRAD_CLIP_NORM=M))
    hp.load(keys)
    model = small_model(hp, BATCH_SIZE=3, FFT_SIZE=16, FFT_STRIDE=4, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8)
    assert model.grad_schedule == schedule
    if early:
        model._early_adam = True
    src = torch.as_tensor(rand_src(hp, 6, 8, scale=6.0)).cuda()
    outs = [model.train_step(src) for _ in range(3)]
    torch.cuda.synchronize()
    return model, [float(o['grad_norm']).hex() for o in outs], [float(o['clip_coef']) for o in outs]


def test_schedules_and_the_early_piece_give_the_same_step(hp, monkeypatch, lstm_status):
    base, norms, coefs = _three_steps(hp, monkeypatch, '0')
    assert all(c < 1.0 for c in coefs)
    flat = base._flat.clone()
    for schedule in ('tail', '1'):
        model, n2, c2 = _three_steps(hp, monkeypatch, schedule)
        assert model._buckets is not None
        assert n2 == norms and c2 == coefs and _same_bits(model._flat, flat), schedule
    model, n2, c2 = _three_steps(hp, monkeypatch, '0', early=True)
    assert model.early_steps == 0 and model._early_adam
    assert n2 == norms and c2 == coefs and _same_bits(model._flat, flat)


def test_the_data_parallel_scale_is_part_of_the_norm(hp, monkeypatch, lstm_status):
    from danet_amd import dist
    monkeypatch.setenv('DANET_OVERLAP_ALLREDUCE', '0')
    _, norms, _ = _three_steps(hp, M=1e30)
    monkeypatch.setattr(dist, 'allreduce_grads_', lambda bucket: 0.5)           # the bucket untouched
    _, halved, coefs = _three_steps(hp, M=1e30)
    assert float.fromhex(halved[0]) == 0.5 * float.fromhex(norms[0]) and coefs[0] == 1.0


def test_sgd_one_step_against_numpy(hp, lstm_status):
    hp.load(dict(LR=1e-2, OPTIMIZER_TYPE='sgd'))
    first = small_model(hp, **SHAPE)
    first.keep_grads = True
    src = torch.as_tensor(rand_src(hp, 6, 8, scale=6.0)).cuda()
    assert list(first.train_step(src)) == ['loss', 'SNR', 'LR']
    g = first._flat_grad.cpu().numpy()
    norm = math.sqrt(math.fsum((g.astype(np.float64) ** 2).tolist()))
    M = 0.25 * norm
    # a value clip (read at every step) at the median magnitude of the SCALED gradient: it bites on half of it
    thres = float(np.float32(np.median(np.abs(g[g != 0])) * 0.25))
    hp.load(dict(GRAD_CLIP_NORM=M, GRAD_CLIP_THRES=thres))
    model = small_model(hp, **SHAPE)
    theta0 = model._flat.cpu().numpy()
    out = model.train_step(src)
    assert abs(float(out['grad_norm']) - norm) <= 1e-12 * norm
    coef = M / (norm + 1e-6)
    assert abs(float(out['clip_coef']) - coef) <= 1e-12 * coef
    gp = GR.scaled_value_clip(g, GR.factor(1.0, coef), thres)
    assert (np.abs(gp) == thres).any() and (np.abs(gp) < thres).any()            # the value clip bites after the scaling
    want = theta0.astype(np.float64) - 1e-2 * gp
    assert np.abs(model._flat.cpu().numpy() - want).max() <= 2e-7 * np.abs(want).max()
    assert not bool(model._flat_grad.any())


# ------------------------------------------------------------------------------------------ CLI
def test_command_line_prints_the_norm_and_the_coefficient(tmp_path):
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

    out = main('gc', dict(GRAD_CLIP_NORM=0.5))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('Epoch 1/1')][0]
    fields = dict(f.split('=') for f in line.split()[2:])
    assert list(fields) == ['loss', 'SNR', 'LR', 'grad_norm', 'clip_coef'], line
    assert math.isfinite(float(fields['grad_norm'])) and float(fields['grad_norm']) > 0
    assert 0.0 < float(fields['clip_coef']) <= 1.0
    plain, null = main('plain', {}), main('null', dict(GRAD_CLIP_NORM=None))
    assert plain.returncode == 0 and null.returncode == 0, plain.stderr[-2000:] + null.stderr[-2000:]
    lines = [[l for l in o.stdout.splitlines() if l.startswith(('Epoch 1/1', 'Valid  1/1'))] for o in (plain, null)]
    assert len(lines[0]) == 2 and lines[0] == lines[1]
    assert 'grad_norm' not in plain.stdout and 'clip_coef' not in plain.stdout
    bad = main('bad', dict(GRAD_CLIP_NORM=-1.0))
    assert bad.returncode != 0 and 'GRAD_CLIP_NORM' in bad.stderr, bad.stdout[-2000:] + bad.stderr[-2000:]
