'''
GPU tests of the truth-online estimator and the trajectory separator's backward (libdanet_tonline_hip.so,
include/danet_tonline_hip.h) against the float64 restatement of tests/tonline_ref.py.  Every output and the saved
denominators lie between poisoned guard bands.

(a) frame_sums + scan over the F x E case table: every attractor inside the header's derived ERROR BOUND of float64
(test_tonline_cpu.py shows on the same cases that the float32 restatement stays inside it and that it is below 1e-5
of max |attr|); (b) the three backward kernels against float64, each output to 1e-5 of its own maximum
(tonline_ref.BAR, the bar of tests/test_gpu_lstm_envelope.py; the float32 restatement is under half of it on every
case); (c) bit for bit: repeats, rows of a batch of 33; the silent prefix; argument errors; ties; (d) against
ops.TruthAttractorFn and ops.SeparateFn; (e) the heads end to end through autograd; (f) the model.

E not a multiple of 4 runs with embed and dembed at an address that is 4-byte aligned only.
'''
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tonline_ref as TR
from gpu_helpers import ROOT, check_lstm_status

pytestmark = pytest.mark.gpu

POISON = -7.25e33
GUARD = 1024


def _guarded(shape, dtype=torch.float32, fill=None, skew=0):
    '''(whole buffer, the view of `shape` in its middle, `skew` elements past the guard): everything poisoned, or the
    middle set to `fill`'''
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + skew,), POISON, dtype=dtype, device='cuda')
    view = buf[GUARD + skew:GUARD + skew + n].view(tuple(shape))
    if fill is not None:
        view.copy_(torch.as_tensor(np.ascontiguousarray(fill)).to(dtype))
    return buf, view


def _intact(*bufs):
    return all(bool((b[:GUARD] == POISON).all()) and bool((b[-GUARD:] == POISON).all()) for b in bufs)


def _cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _skew(E):
    return 1 if E % 4 else 0


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _forward(V, W, P, lam, T0=TR.T0, eps=TR.EPS):
    '''frame_sums + scan between guard bands -> (attr float32, den float64) read back'''
    from danet_amd import ops
    B, T, F, E = V.shape
    C = P.shape[1]
    _, v = _guarded(V.shape, fill=V, skew=_skew(E))
    sb, s = _guarded((B, T, C, E))
    qb, q = _guarded((B, T, C))
    ab, attr = _guarded((B, T, C, E))
    db, den = _guarded((B, T, C), torch.float64)
    ops.tonline_frame_sums(v, _cu(P), _cu(W), out=(s, q))
    got = ops.tonline_scan(s, q, lam, T0, eps, out=(attr, den))
    assert got[0] is attr and got[1] is den
    torch.cuda.synchronize()
    assert _intact(sb, qb, ab, db)
    return attr.cpu().numpy(), den.cpu().numpy()


def _estimator_bwd(G, den, W, P, lam, E, T0=TR.T0):
    '''scan_bwd + sums_bwd between guard bands -> dV float32'''
    from danet_amd import ops
    B, C, T, F = P.shape
    rb, r = _guarded((B, T, C, E))
    vb, dv = _guarded((B, T, F, E), skew=_skew(E))
    ops.tonline_scan_bwd(_cu(G), _cu(den), lam, T0, out=r)
    assert ops.tonline_sums_bwd(_cu(P), _cu(W), r, out=dv) is dv
    torch.cuda.synchronize()
    assert _intact(rb, vb)
    return dv.cpu().numpy()


def _separate_bwd(V, W, attr, D, act):
    '''separate_bwd between guard bands -> (dV, dattr) float32'''
    from danet_amd import ops
    B, T, F, E = V.shape
    C = attr.shape[2]
    _, v = _guarded(V.shape, fill=V, skew=_skew(E))
    vb, dv = _guarded((B, T, F, E), skew=_skew(E))
    ab, da = _guarded((B, T, C, E))
    ops.tonline_separate_bwd(_cu(W), _cu(attr), v, _cu(D), act, out=(dv, da))
    torch.cuda.synchronize()
    assert _intact(vb, ab)
    return dv.cpu().numpy(), da.cpu().numpy()


# ------------------------------------------------------------------------------------ (a) the trajectory
@pytest.mark.parametrize('i', range(len(TR.CASES)))
def test_trajectory_inside_the_headers_bound(i):
    B, T, F, E, C, lam = TR.CASES[i]
    V, W, P = TR.case(B, T, F, E, C, seed=i)
    attr, den = _forward(V, W, P, lam)
    want, wden = TR.attractors(V, W, P, lam, TR.T0, TR.EPS)
    bound = TR.attr_bound(V, W, P, lam, TR.T0, TR.EPS)
    err = np.abs(attr - want)
    print('case %d B %d T %d F %d E %d C %d lambda %.3f: kernel %.3g of max |attr|, %.3g of the bound (bound %.3g)'
          % (i, B, T, F, E, C, lam, err.max() / np.abs(want).max(), (err / np.maximum(bound, 1e-300)).max(), bound.max() / np.abs(want).max()))
    assert (err <= bound).all()
    assert TR.rel(den, wden) <= (TR.depth_q(F) + 2) * TR.U
    hold = min(T, TR.T0)
    assert _same(attr[:, :hold], np.broadcast_to(attr[:, hold - 1:hold], attr[:, :hold].shape))       # the hold shares


# ------------------------------------------------------------------------------------ (b) the backward kernels
@pytest.mark.parametrize('i', range(len(TR.CASES)))
def test_backward_kernels_against_float64(i):
    B, T, F, E, C, lam = TR.CASES[i]
    V, W, P = TR.case(B, T, F, E, C, seed=i)
    G, D = TR.grads(B, T, F, E, C, seed=i)
    attr, den = _forward(V, W, P, lam)
    errs = {'dV estimator': TR.rel(_estimator_bwd(G, den, W, P, lam, E), TR.attractors_bwd(G, den, W, P, lam, TR.T0))}
    for act in (0, 1):
        dV, dA = _separate_bwd(V, W, attr, D, act)
        wV, wA = TR.separate_bwd(V, W, attr, D, act)
        errs['dV act %d' % act], errs['dattr act %d' % act] = TR.rel(dV, wV), TR.rel(dA, wA)
    print('case %d B %d T %d F %d E %d C %d: %s of each maximum'
          % (i, B, T, F, E, C, ', '.join('%s %.3g' % kv for kv in errs.items())))
    assert max(errs.values()) <= TR.BAR, errs


# ------------------------------------------------------------------------------------ (c) bit for bit and edges
@pytest.mark.parametrize('F,E,C', [(129, 20, 2), (5, 3, 4)])
def test_repeats_and_rows_of_a_batch_agree_bit_for_bit(F, E, C):
    B, T, lam = 33, 12, TR.LAMBDAS[1]
    V, W, P = TR.case(B, T, F, E, C, seed=50)
    G, D = TR.grads(B, T, F, E, C, seed=50)

    def run(rows):
        attr, den = _forward(V[rows], W[rows], P[rows], lam)
        dV, dA = _separate_bwd(V[rows], W[rows], attr, D[rows], 0)
        return attr, _estimator_bwd(G[rows], den, W[rows], P[rows], lam, E), dV, dA

    whole, again = run(slice(None)), run(slice(None))
    assert all(_same(a, b) for a, b in zip(whole, again))
    for b in (0, 17, 32):
        alone = run(slice(b, b + 1))
        assert all(_same(a[0], w[b]) for a, w in zip(alone, whole)), b


def test_a_silent_prefix_gives_exact_zeros_and_a_finite_gradient_that_ignores_it():
    B, T, F, E, C, p, lam = 2, 20, 9, 4, 3, 12, 0.9
    V, W, P = TR.case(B, T, F, E, C, seed=7, silent=p)
    G, _ = TR.grads(B, T, F, E, C, seed=7)
    attr, den = _forward(V, W, P, lam)
    assert not attr[:, :p, C - 1].any() and np.abs(attr[:, p:, C - 1]).min() > 0.01
    assert np.array_equal(den[:, :p, C - 1], np.full((B, p), TR.EPS))
    dV = _estimator_bwd(G, den, W, P, lam, E)
    assert np.isfinite(dV).all() and TR.rel(dV, TR.attractors_bwd(G, den, W, P, lam, TR.T0)) <= TR.BAR
    G2 = G.copy()
    G2[:, :p, C - 1] *= -5
    assert _same(_estimator_bwd(G2, den, W, P, lam, E), dV)
    # eps = 0: a source without a bin has A = 0 and a zero denominator, and nothing becomes non-finite
    attr0, den0 = _forward(V, W, P, lam, eps=0.0)
    assert not attr0[:, :p, C - 1].any() and not den0[:, :p, C - 1].any() and np.isfinite(attr0).all()
    assert np.isfinite(_estimator_bwd(G, den0, W, P, lam, E)).all()


def test_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    B, T, F, E, C = 2, 5, 9, 4, 2
    V, W, P = TR.case(B, T, F, E, C, seed=8)
    G, D = TR.grads(B, T, F, E, C, seed=8)
    v, w, pp, g, d = _cu(V), _cu(W), _cu(P), _cu(G), _cu(D)
    outs = [_guarded(s, dt) for s, dt in (((B, T, C, E), torch.float32), ((B, T, C), torch.float32),
                                          ((B, T, C), torch.float64), ((B, T, F, E), torch.float32))]
    (_, s), (_, q), (_, den), (_, dv) = outs
    s2, q2 = torch.zeros_like(s), torch.zeros_like(q)
    den2 = torch.ones(B, T, C, dtype=torch.float64, device='cuda')
    lib, st = _lib.load_tonline(), _lib.stream()
    calls = [lambda: ops.tonline_scan(s2, q2, 0.0, 4, 1e-7, out=(s, den)),
             lambda: ops.tonline_scan(s2, q2, 0.9, 0, 1e-7, out=(s, den)),
             lambda: ops.tonline_scan(s2, q2, 0.9, 4, -1.0, out=(s, den)),
             lambda: ops.tonline_scan_bwd(g, den2, 1.5, 4, out=s),
             lambda: ops.tonline_scan_bwd(g, den2, 0.9, 0, out=s),
             lambda: ops.tonline_separate_bwd(w, g, v, d, 2, out=(dv, s)),
             lambda: _lib.tonline_check(lib.danet_tonline_frame_sums(st, B, 5, T, F, E, v.data_ptr(), pp.data_ptr(),
                                                                     w.data_ptr(), s.data_ptr(), q.data_ptr())),
             lambda: _lib.tonline_check(lib.danet_tonline_sums_bwd(st, B, C, T, 1026, E, pp.data_ptr(), w.data_ptr(),
                                                                   g.data_ptr(), dv.data_ptr())),
             lambda: _lib.tonline_check(lib.danet_tonline_frame_sums(st, B, C, T, F, E, v.data_ptr() + 4, pp.data_ptr(),
                                                                     w.data_ptr(), s.data_ptr(), q.data_ptr()))]
    for call in calls:
        with pytest.raises(_lib.DanetHipError):
            call()
    torch.cuda.synchronize()
    for buf, _ in outs:
        assert bool((buf == POISON).all())


def _tied_case(B, T, F, E, C, seed):
    V, W, P = TR.case(B, T, F, E, C, seed=seed)
    rng = np.random.RandomState(seed)
    top = P.max(axis=1, keepdims=True)
    tie = rng.random_sample(P.shape) < 0.5                     # about half of the other sources tie with the largest
    return V, W, np.where(tie, top, P).astype(np.float32)


def test_ties_take_the_label_of_the_truth_weighted_kernel():
    from danet_amd import ops
    B, T, F, E, C = 2, 6, 65, 8, 3
    V, W, P = _tied_case(B, T, F, E, C, seed=9)
    assert ((P == P.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.3
    attr, _ = _forward(V, W, P, 1.0, T0=T)
    one = ops.TruthAttractorFn.apply(_cu(V), _cu(P), _cu(W), ops.TRUTH_MODES['truth-weighted'], TR.EPS).cpu().numpy()
    want = TR.attractors(V, W, P, 1.0, T, TR.EPS)[0]                 # np.argmax: the lowest c
    assert TR.rel(attr, want) <= TR.BAR and TR.rel(one, want[:, 0]) <= TR.BAR
    # the other tie rule is far away: the two kernels cannot agree with float64 unless they share the rule
    other = TR.attractors(V, W, P[:, ::-1], 1.0, T, TR.EPS)[0][:, :, ::-1]
    assert TR.rel(other, want) > 1e-2


# ------------------------------------------------------------------------------------ (d) against the older kernels
def test_lambda_one_and_a_hold_over_everything_is_truth_weighted():
    from danet_amd import ops
    B, T, F, E, C = 3, 11, 129, 20, 2
    V, W, P = TR.case(B, T, F, E, C, seed=10)
    one = ops.TruthAttractorFn.apply(_cu(V), _cu(P), _cu(W), ops.TRUTH_MODES['truth-weighted'], TR.EPS).cpu().numpy()
    for T0 in (T, T + 1, 500):
        attr, _ = _forward(V, W, P, 1.0, T0=T0)
        want = TR.attractors(V, W, P, 1.0, T0, TR.EPS)[0]
        assert np.abs(want - want[:, :1]).max() == 0                                     # one attractor set
        assert TR.rel(attr, want) <= TR.BAR and TR.rel(one, want[:, 0]) <= TR.BAR


@pytest.mark.parametrize('act', [0, 1])
def test_online_separate_fn_with_one_attractor_set_is_separate_fn(act):
    from danet_amd import ops
    B, T, F, E, C = 2, 7, 129, 20, 3
    V, W, P = TR.case(B, T, F, E, C, seed=11 + act)
    _, D = TR.grads(B, T, F, E, C, seed=11)
    A = TR.attractors(V, W, P, 1.0, T, TR.EPS, np.float32)[0][:, 0].astype(np.float32)           # [B, C, E]
    v1, a1 = _cu(V).requires_grad_(), _cu(np.repeat(A[:, None], T, axis=1)).requires_grad_()
    out1 = ops.OnlineSeparateFn.apply(_cu(W), a1, v1.view(B, T * F, E), act)
    out1.backward(_cu(D))
    v2, a2 = _cu(V).requires_grad_(), _cu(A).requires_grad_()
    out2, _ = ops.SeparateFn.apply(_cu(W), a2, v2.view(B, T * F, E), act, False)
    out2.backward(_cu(D))
    wV, wA = TR.separate_bwd(V, W, np.repeat(A[:, None], T, axis=1), D, act)
    assert TR.rel(out1.detach().cpu().numpy(), out2.detach().cpu().numpy()) <= TR.BAR
    assert TR.rel(v1.grad.cpu().numpy(), wV) <= TR.BAR and TR.rel(v2.grad.cpu().numpy(), wV) <= TR.BAR
    assert TR.rel(a1.grad.sum(dim=1).cpu().numpy(), wA.sum(axis=1)) <= TR.BAR
    assert TR.rel(a2.grad.cpu().numpy(), wA.sum(axis=1)) <= TR.BAR


# ------------------------------------------------------------------------------------ (e) the heads end to end
def _ref_heads(V, W, P, src, phasor, act, lam, T0, eps):
    '''float64 autograd of the restated heads on the embedding V -> (loss, dL/dV)'''
    from oracle import torch_ref as R
    v = torch.tensor(np.asarray(V), dtype=torch.float64, requires_grad=True)
    sep = TR.torch_separate(v, W, TR.torch_attractors(v, W, P, lam, T0, eps), act)
    ph = torch.as_tensor(np.asarray(phasor), dtype=torch.float64)
    sepc = torch.complex(ph[..., 0][:, None] * sep, ph[..., 1][:, None] * sep)
    loss = R.pit_mse_loss(torch.as_tensor(np.asarray(src)).to(torch.complex128), sepc)[0]
    loss.backward()
    return float(loss.detach()), v.grad.numpy()


@pytest.mark.parametrize('act', [0, 1])
def test_heads_end_to_end_against_float64_autograd(act):
    from danet_amd import ops
    B, T, F, E, C, lam, T0 = 2, 20, 33, 4, 2, TR.LAMBDAS[1], 4
    rng = np.random.RandomState(12)
    src = (rng.standard_normal((B, C, T, F)) + 1j * rng.standard_normal((B, C, T, F))).astype(np.complex64) * 3
    fe = ops.frontend(_cu(src))
    W, P = fe['mix_pwr'].cpu().numpy(), fe['src_pwr'].cpu().numpy()
    V = TR.case(B, T, F, E, C, seed=12)[0]
    embed = _cu(V).requires_grad_()
    attr = ops.TruthOnlineAttractorFn.apply(embed, fe['src_pwr'], fe['mix_pwr'], lam, T0, TR.EPS)
    assert tuple(attr.shape) == (B, T, C, E)
    sep = ops.OnlineSeparateFn.apply(fe['mix_pwr'], attr, embed.reshape(B, -1, E), act)
    loss = ops.pit_mse_loss(_cu(src), sep, fe['phasor'], mode=0, eps=TR.EPS)[0]
    loss.backward()
    want_loss, want = _ref_heads(V, W, P, src, fe['phasor'].cpu().numpy(), act, lam, T0, TR.EPS)
    err = TR.rel(embed.grad.cpu().numpy(), want)
    print('heads act %d: loss %.6g against %.6g, dembed %.3g of its maximum' % (act, float(loss.detach()), want_loss, err))
    assert abs(float(loss.detach()) - want_loss) <= 1e-5 * abs(want_loss) and err <= TR.BAR


# ------------------------------------------------------------------------------------ (f) the model
TINY = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
            NUM_ANCHOR=4, ENCODER_TYPE='lstm-causal', TRAIN_ESTIMATOR_METHOD='truth-online',
            INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=4, SEPARATOR_TYPE='dot-softmax-orig')
T = 40


def _model(hp, **keys):
    from danet_amd.model import Model
    hp.reset()
    hp.load(dict(TINY, **keys))
    hp.digest()
    return Model('tonline', device='cuda:0', seed=5).build()


def _signals(T, seed=0):
    rng = np.random.RandomState(seed)
    return _cu((rng.standard_normal((2, 2, T, 33)) + 1j * rng.standard_normal((2, 2, T, 33))).astype(np.complex64) * 3)


def test_build_and_one_train_step(hp):
    from danet_amd import _lib, modules
    model = _model(hp)
    assert isinstance(model.estimator, modules.TruthOnlineEstimator) and model.online == (4, 1.0)
    assert _lib._tonline is not None                           # the dry forward of build() ran the train branch
    src = _signals(T)
    res = model.train_step(src)
    assert list(res) == ['loss', 'SNR', 'LR'] and np.isfinite(float(res['loss'])) and np.isfinite(float(res['SNR']))
    with torch.no_grad():
        out = model.forward(src)
    assert tuple(out['attrs'].shape) == (2, T, 2, 4) and tuple(out['sep_pwr'].shape) == (2, 2, T, 33)
    res = model.valid_step(src)
    assert list(res) == ['loss', 'SNR'] and all(np.isfinite(float(v)) for v in res.values())
    check_lstm_status()


@pytest.mark.parametrize('sep,tau', [('dot-softmax-orig', None), ('dot-sigmoid-orig', 8)])
def test_parameter_gradients_against_float64_autograd_of_the_heads(hp, sep, tau):
    '''the embedding gradient of float64 autograd through the restated heads, fed back through the encoder's own
    backward, against the gradients one train_step leaves'''
    from danet_amd import ops
    model = _model(hp, SEPARATOR_TYPE=sep, ONLINE_MEMORY_FRAMES=tau)
    T0, lam = model.online
    src = _signals(T, seed=1)
    fe = ops.frontend(src)
    emb = model.encoder(fe['mix_log'])
    want_loss, dembed = _ref_heads(emb.detach().cpu().numpy(), fe['mix_pwr'].cpu().numpy(), fe['src_pwr'].cpu().numpy(),
                                   src.cpu().numpy(), fe['phasor'].cpu().numpy(), model.separator.ACT, lam, T0,
                                   float(hp.EPS))
    model.zero_grad()
    emb.backward(_cu(dembed.astype(np.float32)))
    torch.cuda.synchronize()
    want = model.grad_dict()
    model.zero_grad()
    model.keep_grads = True
    res = model.train_step(src)
    torch.cuda.synchronize()
    got = model.grad_dict()
    assert abs(float(res['loss']) - want_loss) <= 1e-5 * abs(want_loss)
    worst, checked = {}, 0
    for k in want:
        if not np.any(want[k]):                    # the inference estimator's anchors
            assert not np.any(got[k]), k
            continue
        worst[k] = TR.rel(got[k], want[k])
        checked += 1
    print('worst gradient error: %r' % (max(worst.items(), key=lambda kv: kv[1]),))
    assert checked == 5 and max(worst.values()) <= TR.BAR, worst
    check_lstm_status()


def test_the_loss_falls_over_30_steps_on_one_batch(hp):
    model = _model(hp, LR=3e-3)
    src = _signals(T, seed=2)
    losses = [float(model.train_step(src)['loss']) for _ in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    check_lstm_status()


@pytest.mark.parametrize('keys,extra', [(dict(TRAIN_LOSS='si-sdr'), []), (dict(DPCL_WEIGHT=0.1), ['DPCL']),
                                        (dict(GRAD_CLIP_NORM=0.5, DROPOUT_KEEP_PROB=0.8), ['grad_norm', 'clip_coef'])])
def test_the_step_runs_with_the_other_training_keys(hp, keys, extra):
    model = _model(hp, **keys)
    res = model.train_step(_signals(T, seed=3))
    assert list(res) == ['loss', 'SNR', 'LR'] + extra and all(np.isfinite(float(v)) for v in res.values())
    check_lstm_status()


def test_a_model_with_truth_weighted_never_maps_the_library():
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib\n"
        "from danet_amd.hparams import hparams\n"
        "from danet_amd.model import Model\n"
        "hparams.load(%r); hparams.digest()\n"
        "model = Model('other', device='cuda:0', seed=5).build()\n"
        "rng = np.random.RandomState(0)\n"
        "src = torch.as_tensor((rng.standard_normal((2, 2, 40, 33)) + 1j * rng.standard_normal((2, 2, 40, 33)))"
        ".astype(np.complex64)).cuda()\n"
        "res = model.train_step(src); out = model.infer(src.sum(1)); val = model.valid_step(src)\n"
        "torch.cuda.synchronize()\n"
        "print('RAN:', np.isfinite(float(res['loss'])) and tuple(out.shape) == (2, 2, 40, 33) and sorted(val) == ['SNR', 'loss'])\n"
        "print('UNMAPPED:', _lib._tonline is None and 'libdanet_tonline' not in open('/proc/self/maps').read())\n"
        "print('ONLINE:', 'libdanet_online' in open('/proc/self/maps').read())\n"
    ) % (ROOT, dict(TINY, TRAIN_ESTIMATOR_METHOD='truth-weighted'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('RAN: True', 'UNMAPPED: True', 'ONLINE: True'):
        assert words in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_command_line_trains_one_epoch(tmp_path):
    cfg = tmp_path / 'cfg.json'
    cfg.write_text(json.dumps(dict(TINY, MAX_TRAIN_LEN=128)))     # the toy dataset's own length: no crop
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'to', '-m', 'train', '-ds', 'toy',
                          '-c', str(cfg), '-ne', '1', '-bs', '2'], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert np.isfinite(float(out.stdout.split('Epoch 1/1 loss=')[1].split()[0])) and 'Valid  1/1 loss=' in out.stdout
    assert (tmp_path / 'saves' / 'to_e1.npz').exists()
