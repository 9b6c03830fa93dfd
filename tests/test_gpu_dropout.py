'''
GPU tests of DROPOUT_KEEP_PROB (run with -m gpu): the apply kernel of libdanet_dropout_hip.so across
its header envelope against the numpy restatement of the mask contract (bit for bit), the BiLSTM
layer / encoder functions and whole train steps against float64 autograd with the same masks
injected at the reference's positions (tests/dropout_ref.py), and the model-level properties:
determinism, seed / step dependence, evaluation paths that never drop, a keep-1.0 step that never
loads the library, and a resumed run that continues the mask sequence.
'''
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import dropout_ref as D
from gpu_helpers import (GTOL, ROOT, TOL, cfg_of, check_lstm_status, cu, oracle_threads, rand_src, relerr,
                         small_model)

pytestmark = pytest.mark.gpu

KEY = dict(key0=1337, key1=2, stream_id=1, step=3)
GUARD = 64          # floats in front of and behind every buffer


def _apply(x, ldx, y, ldy, rows, cols, thr, scale, key0=0, key1=0, stream_id=0, step=0):
    from danet_amd import _lib
    return _lib.load_dropout().danet_dropout_apply(
        torch.cuda.current_stream().cuda_stream, rows, cols, x.data_ptr(), ldx, y.data_ptr(), ldy, thr, scale,
        key0, key1, stream_id, step)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _pitched(vals, ld, off):
    '''a NaN-filled device buffer [GUARD | off | rows x ld | GUARD] with `vals` at the logical positions;
    returns (whole buffer, view that starts at the matrix's first element)'''
    rows, cols = vals.shape
    host = np.full(GUARD + off + rows * ld + GUARD, np.nan, np.float32)
    body = host[GUARD + off:GUARD + off + rows * ld].reshape(rows, ld)
    body[:, :cols] = vals
    buf = cu(host)
    return buf, buf[GUARD + off:]


def _check_out(buf, off, rows, cols, ld, want, what):
    '''logical positions == want bit for bit; pitch gaps and guard bands still NaN'''
    host = buf.cpu().numpy()
    body = host[GUARD + off:GUARD + off + rows * ld].reshape(rows, ld)
    assert np.array_equal(_bits(body[:, :cols]), _bits(want)), what
    assert np.isnan(body[:, cols:]).all(), what + ': pitch gap written'
    assert np.isnan(host[:GUARD + off]).all() and np.isnan(host[GUARD + off + rows * ld:]).all(), \
        what + ': guard band written'


@pytest.mark.parametrize('rows', [1, 7, 4096])
@pytest.mark.parametrize('cols', [1, 3, 5, 132, 600, 1200])
def test_kernel_envelope_matches_numpy_mask_exactly(rows, cols):
    keep = 0.8
    thr, scale = D.threshold_of(keep), D.scale_of(keep)
    rng = np.random.RandomState(rows * 10007 + cols)
    x = rng.randn(rows, cols).astype(np.float32)
    x[0, 0] = np.float32(np.inf)               # a kept inf stays inf, a dropped one becomes +0
    mask = D.keep_mask(rows, cols, thr, **KEY)
    want = np.where(mask, x * scale, np.float32(0)).astype(np.float32)
    assert np.array_equal(want, D.apply_np(x, thr, scale, **KEY))
    assert not np.isnan(want).any()
    # (ldx, ldy, base offset in floats, in place): dense; pitched fast-path candidates; odd pitches;
    # a base pointer that is 4- but not 16-byte aligned (element-wise path, same result)
    variants = [(cols, cols, 0, False), (cols + 4, cols + 8, 0, False), (cols + 3, cols + 5, 0, False),
                (cols, cols, 1, False), (cols + 4, cols + 4, 3, False),
                (cols, cols, 0, True), (cols + 4, cols + 4, 0, True), (cols + 1, cols + 1, 2, True)]
    for ldx, ldy, off, inplace in variants:
        what = 'rows %d cols %d ldx %d ldy %d off %d inplace %d' % (rows, cols, ldx, ldy, off, inplace)
        xbuf, xv = _pitched(x, ldx, off)
        if inplace:
            ybuf, yv = xbuf, xv
        else:
            ybuf, yv = _pitched(np.full((rows, cols), np.nan, np.float32), ldy, off)
        assert _apply(xv, ldx, yv, ldy, rows, cols, thr, float(scale), **KEY) == 0, what
        torch.cuda.synchronize()
        _check_out(ybuf, off, rows, cols, ldy, want, what)
        if not inplace:                        # the input, gaps included, is untouched
            _check_out(xbuf, off, rows, cols, ldx, x, what + ' (input)')
    kept = float(mask.mean())
    if rows * cols >= 4096:
        assert abs(kept - keep) < 6 * np.sqrt(keep * (1 - keep) / (rows * cols)), kept


def test_extreme_thresholds_and_what_changes_the_mask():
    rows, cols = 33, 132
    x = np.random.RandomState(0).randn(rows, cols).astype(np.float32) + 3
    xd = cu(x)

    def run(thr, scale=1.0, **kw):
        y = torch.full((rows, cols), float('nan'), device='cuda')
        k = dict(KEY, **kw)
        assert _apply(xd, cols, y, cols, rows, cols, thr, scale, **k) == 0
        got = y.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(D.apply_np(x, thr, np.float32(scale), **k))), (thr, kw)
        return got

    lo = run(1)                                  # keeps a word only if it is 0
    assert not lo.any()
    hi = run(0xffffffff)                         # drops a word only if it is 0xffffffff
    assert np.array_equal(_bits(hi), _bits(x))
    half = D.threshold_of(0.5)
    base = run(half, 2.0)
    for kw in (dict(step=4), dict(stream_id=2), dict(key0=1338), dict(key1=3)):
        other = run(half, 2.0, **kw)
        assert ((other != 0) != (base != 0)).mean() > 0.3, kw
    again = run(half, 2.0)
    assert np.array_equal(_bits(again), _bits(base))


def test_bad_arguments_return_an_error_and_leave_the_output_untouched():
    from danet_amd import _lib
    lib = _lib.load_dropout()
    x = torch.ones(8, 16, device='cuda')
    y = torch.full((8, 16), 7.0, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    good = [s, 8, 16, x.data_ptr(), 16, y.data_ptr(), 16, 1 << 31, 2.0, 0, 0, 0, 0]
    for i, v in ((1, 0), (2, 0), (3, None), (5, None), (4, 15), (6, 12), (7, 0), (3, x.data_ptr() + 2),
                 (5, y.data_ptr() + 1), (8, float('inf'))):
        a = list(good)
        a[i] = v
        assert lib.danet_dropout_apply(*a) == -1, (i, v)
        assert lib.danet_dropout_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert lib.danet_dropout_apply(*good) == 0
    torch.cuda.synchronize()
    assert set(np.unique(y.cpu().numpy())) <= {0.0, 2.0}


# ------------------------------------------------------------------ layer and encoder functions
def _lstm_params(rng, D_, H, ndir=2):
    from oracle import danet_oracle as O
    r = 0.75 / np.sqrt(H)
    out = []
    for _ in range(ndir):
        out.append(rng.uniform(-r, r, (D_ + H, 4 * H)).astype(np.float32))
        out.append((O.lstm_bias_init(H) + 0.1 * rng.randn(4 * H)).astype(np.float32))
    return out


@pytest.mark.parametrize('B,T,Din,H,gtol', [(3, 9, 10, 16, TOL), (32, 128, 600, 300, GTOL)])
def test_bilstm_layer_fn_vs_float64_with_injected_mask(B, T, Din, H, gtol):
    from danet_amd import ops
    rng = np.random.RandomState(B)
    x = rng.randn(B, T, Din).astype(np.float32)
    dy = rng.randn(B, T, 2 * H).astype(np.float32)
    P = _lstm_params(rng, Din, H)
    spec = ops.DropoutSpec(0.8, 1337, 1, 6)
    xc = cu(x).requires_grad_(True)
    Pc = [cu(p).requires_grad_(True) for p in P]
    with ops.dropout_scope(spec):
        y = ops.LstmLayerFn.apply(xc, H, *Pc)
    y.backward(cu(dy))
    check_lstm_status()
    rs = D.Spec(0.8, 1337, 1, 6)
    assert (spec.threshold, spec.scale) == (rs.threshold, float(rs.scale))
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    Pt = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in P]
    with oracle_threads():
        yr = D.bilstm_layer(xt, *Pt, H, rs, 0)
        (yr * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    got = y.detach().cpu().numpy()
    # the dropped positions are exact zeros, and exactly the contract's
    m = D.keep_mask(T * B, 2 * H, rs.threshold, 1337, 1, 0, 6).reshape(T, B, 2 * H).transpose(1, 0, 2)
    assert not got[~m].any()
    errs = dict(y=relerr(got, yr.detach().numpy()), dx=relerr(xc.grad.cpu().numpy(), xt.grad.numpy()))
    for i, (a, b) in enumerate(zip(Pc, Pt)):
        errs['p%d' % i] = relerr(a.grad.cpu().numpy(), b.grad.numpy())
    print('layer B %d T %d D %d H %d: %s' % (B, T, Din, H, errs))
    assert errs.pop('y') < TOL
    assert all(v < gtol for v in errs.values()), errs
    # without a scope: no dropout (nothing is exactly zero)
    y1 = ops.LstmLayerFn.apply(cu(x), H, *[cu(p) for p in P])
    assert bool((y1 != 0).all())


@pytest.mark.parametrize('B,T,nfft,H,E,gtol', [(3, 10, 16, 8, 3, TOL), (32, 128, 256, 300, 20, GTOL)])
def test_three_layer_encoder_fn_vs_float64_with_injected_masks(B, T, nfft, H, E, gtol):
    from danet_amd import ops
    L, F = 3, nfft // 2 + 1
    rng = np.random.RandomState(T)
    x = np.abs(rng.randn(B, T, F)).astype(np.float32)
    names, P, Din = [], [], F
    for l in range(L):
        lp = _lstm_params(rng, Din, H)
        for d, dn in enumerate(('fwd', 'bwd')):
            names += ['global/encoder/lstm%d_%s/LSTM/linear/%s' % (l, dn, v) for v in ('W', 'B')]
            P += lp[2 * d:2 * d + 2]
        Din = 2 * H
    names.append('global/encoder/output/W')
    P.append(rng.uniform(-1.85, 1.85, (2 * H, F * E)).astype(np.float32))
    dembed = rng.randn(B, T, F * E).astype(np.float32)
    spec = ops.DropoutSpec(0.8, 99, 0, 2)
    Pc = [cu(p).requires_grad_(True) for p in P]
    with ops.dropout_scope(spec):
        embed = ops.RnnEncoderFn.apply(cu(x), H, L, 2, *Pc)
    embed.backward(cu(dembed))
    check_lstm_status()
    assert spec.take() == L                          # one stream id per layer
    Pt = {n: torch.tensor(p, dtype=torch.float64, requires_grad=True) for n, p in zip(names, P)}
    t0 = time.time()
    with oracle_threads():
        ref = D.bilstm_encoder(torch.tensor(x, dtype=torch.float64), Pt, H, L, E, D.Spec(0.8, 99, 0, 2))
        (ref.reshape(B, T, F * E) * torch.tensor(dembed, dtype=torch.float64)).sum().backward()
    print('float64 encoder forward+backward: %.1f s' % (time.time() - t0))
    e_out = relerr(embed.detach().cpu().numpy(), ref.detach().reshape(B, T, F * E).numpy())
    errs = {n: relerr(a.grad.cpu().numpy(), Pt[n].grad.numpy()) for n, a in zip(names, Pc)}
    print('encoder B %d T %d H %d: embed %.3g, worst gradient %s' % (
        B, T, H, e_out, max(errs.items(), key=lambda kv: kv[1])))
    assert e_out < TOL
    bad = {k: v for k, v in errs.items() if not v < gtol}
    assert not bad, bad
    # the unmasked oracle is far away: the test can tell dropout from none
    from oracle import torch_ref as R
    with torch.no_grad(), oracle_threads():
        plain = R.bilstm_encoder(torch.tensor(x, dtype=torch.float64), Pt, H, L, E)
    assert relerr(embed.detach().cpu().numpy(), plain.reshape(B, T, F * E).numpy()) > 100 * TOL
    # lstm-orig (ndir == 1) ignores an active scope
    P1 = []
    Din = F
    for l in range(2):
        P1 += _lstm_params(rng, Din, H, ndir=1)
        Din = H
    P1.append(rng.uniform(-1, 1, (H, F * E)).astype(np.float32))
    with torch.no_grad():
        a = ops.RnnEncoderFn.apply(cu(x), H, 2, 1, *[cu(p) for p in P1])
        with ops.dropout_scope(ops.DropoutSpec(0.5, 1, 0, 0)):
            b = ops.RnnEncoderFn.apply(cu(x), H, 2, 1, *[cu(p) for p in P1])
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- whole model steps
def _masked_step_vs_oracle(hp, model, src, oracle, cfg, seed, min_checked):
    '''gpu_helpers.train_step_vs_oracle with the masked oracle: loss and SNR at 1e-4, every parameter
    gradient at GTOL'''
    model.keep_grads = True
    params = model.param_dict()
    step = model.step_base + model.step_count
    out = model.train_step(src)
    torch.cuda.synchronize()
    check_lstm_status()
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    t0 = time.time()
    with oracle_threads():
        ref = oracle(src.cpu().to(torch.complex128), tp, cfg,
                     D.Spec(float(hp.DROPOUT_KEEP_PROB), seed & 0xffffffff, 0, step))
        ref['loss'].backward()
    print('float64 masked oracle forward+backward: %.1f s' % (time.time() - t0))
    e_loss = relerr(float(out['loss']), float(ref['loss'].detach()))
    e_snr = relerr(float(out['SNR']), float(ref['SNR'].detach()))
    g = model.grad_dict()
    worst = {k: relerr(g[k], tp[k].grad.numpy()) for k in tp if tp[k].grad is not None}
    print('loss %.3g SNR %.3g worst gradient %s' % (e_loss, e_snr, max(worst.items(), key=lambda kv: kv[1])))
    assert e_loss < 1e-4 and e_snr < 1e-4, (e_loss, e_snr)
    bad = {k: v for k, v in worst.items() if not v < GTOL}
    assert not bad, bad
    assert len(worst) >= min_checked, len(worst)
    return out, ref


def test_cfg2_b32_train_step_keep_08_vs_masked_oracle(hp):
    '''BASELINE configs[1] as bench.py runs it, with DROPOUT_KEEP_PROB = 0.8: loss, SNR and all 14
    trained tensors' gradients; and the keep-1.0 loss of the same model is a different number'''
    from test_gpu_fullsize import _cfg, _setup, _synth
    model = _setup(hp, BATCH_SIZE=32, DROPOUT_KEEP_PROB=0.8)
    src = _synth(hp, 32, 128, 1337)
    with torch.no_grad():
        plain = float(model.forward(src, fuse_heads=True)['loss'])
    out, ref = _masked_step_vs_oracle(hp, model, src, D.model_forward, _cfg(hp), 7, min_checked=14)
    assert relerr(float(out['loss']), plain) > 1e-3, (float(out['loss']), plain)


def test_small_model_steps_vs_masked_oracle_over_three_steps(hp):
    '''the mask follows step_count: three consecutive steps, each against the oracle at that step'''
    model = small_model(hp, seed=3, NUM_LSTM_LAYERS=3, DROPOUT_KEEP_PROB=0.8)
    src = torch.as_tensor(rand_src(hp, 12, seed=1)).cuda()
    for _ in range(3):
        _masked_step_vs_oracle(hp, model, src, D.model_forward, cfg_of(hp), 3, min_checked=14)
    assert model.step_count == 3


def test_conv_bilstm_v1_train_step_keep_08_vs_masked_oracle(hp):
    '''conv-bilstm-v1 at its existing small test shape (tests/test_gpu_conv_encoder.py: FFT 64, B 4,
    16 frames, seed 4 of its truth-weighted case) and bar'''
    model = small_model(hp, ENCODER_TYPE='conv-bilstm-v1', FFT_SIZE=64, EMBED_SIZE=4, BATCH_SIZE=4,
                        MAX_N_SIGNAL=3, TRAIN_ESTIMATOR_METHOD='truth-weighted', DROPOUT_KEEP_PROB=0.8)
    src = torch.as_tensor(rand_src(hp, 16, seed=4)).cuda()
    cfg = dict(nfft=hp.FFT_SIZE, E=hp.EMBED_SIZE, C=hp.MAX_N_SIGNAL, alpha=hp.RELU_LEAKAGE,
               train_est=hp.TRAIN_ESTIMATOR_METHOD, separator=hp.SEPARATOR_TYPE)
    params = model.param_dict()
    _masked_step_vs_oracle(hp, model, src, D.conv_model_forward, cfg, 3, min_checked=25)
    # the comparison can tell dropout from none: the unmasked restatement's LSTM gradients are far away
    # (masking a fifth of a layer's outputs and scaling the rest by 1.25 moves them by tens of percent)
    import conv_ref
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    with oracle_threads():
        conv_ref.model_forward(src.cpu().to(torch.complex128), tp, cfg)['loss'].backward()
    g = model.grad_dict()
    for k in ('global/encoder/lstm0_fwd/LSTM/linear/W', 'global/encoder/lstm1_bwd/LSTM/linear/W'):
        far = relerr(g[k], tp[k].grad.numpy())
        print('%s against the unmasked oracle: %.3g' % (k, far))
        assert far > 1e-2, (k, far)


def _three_steps(hp, seed, keep=0.8, start=0):
    model = small_model(hp, seed=seed, NUM_LSTM_LAYERS=3, DROPOUT_KEEP_PROB=keep)
    model.step_base = start
    src = torch.as_tensor(rand_src(hp, 12, seed=2)).cuda()
    losses = [float(model.train_step(src)['loss']) for _ in range(3)]
    torch.cuda.synchronize()
    return model, losses


def test_same_seed_is_bit_identical_and_seed_or_step_change_the_loss(hp):
    a, la = _three_steps(hp, 5)
    pa = a.param_dict()
    b, lb = _three_steps(hp, 5)
    assert la == lb
    for k, v in b.param_dict().items():
        assert np.array_equal(_bits(v), _bits(pa[k])), k
    # same parameters (seed 5 initialises both), same data, different mask key or step
    c = small_model(hp, seed=5, NUM_LSTM_LAYERS=3, DROPOUT_KEEP_PROB=0.8)
    src = torch.as_tensor(rand_src(hp, 12, seed=2)).cuda()
    with torch.no_grad():
        l_step0 = float(c.forward(src, s_dropout_keep=0.8)['loss'])
        c.step_base = 1
        l_step1 = float(c.forward(src, s_dropout_keep=0.8)['loss'])
        c.step_base, c.seed = 0, 6
        l_seed6 = float(c.forward(src, s_dropout_keep=0.8)['loss'])
        l_plain = float(c.forward(src)['loss'])
    assert l_step0 == la[0] or relerr(l_step0, la[0]) < 1e-6     # (fused vs unfused heads)
    assert len({l_step0, l_step1, l_seed6, l_plain}) == 4, (l_step0, l_step1, l_seed6, l_plain)


def test_evaluation_paths_never_drop(hp):
    outs = []
    for keep in (1.0, 0.5):
        model = small_model(hp, seed=9, DEBUG=True, DROPOUT_KEEP_PROB=keep)
        src = torch.as_tensor(rand_src(hp, 12, seed=3)).cuda()
        v = model.valid_step(src)
        sep = model.infer(src.sum(dim=1))
        dbg = model.debug_fetch(src)
        outs.append([v['loss'], v['SNR'], torch.view_as_real(sep), dbg['embed'], dbg['attrs'],
                     torch.view_as_real(dbg['output'])])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_keep_one_step_loads_nothing_and_launches_what_it_did():
    '''fresh process: after a keep-1.0 train step the dropout library is still unloaded; a keep-0.8
    step of the same model adds exactly 2 L launches, all of them `dropout`'''
    code = '''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import __graft_entry__ as g; g.load_package()
import torch
from danet_amd import _lib
from danet_amd.hparams import hparams as hp
from gpu_helpers import small_model, rand_src
model = small_model(hp, seed=3, NUM_LSTM_LAYERS=3)
assert hp.DROPOUT_KEEP_PROB == 1.0
src = torch.as_tensor(rand_src(hp, 12, seed=1)).cuda()
def counted():
    model.train_step(src)
    _lib.profile_start()
    model.train_step(src)
    return {k: n for k, (n, ms) in _lib.profile_stop().items()}
a = counted()
print('UNLOADED', _lib._dropout is None, 'dropout' not in a)
hp.DROPOUT_KEEP_PROB = 0.8
b = counted()
extra = b.pop('dropout')
print('EXTRA', extra, b == a, _lib._dropout is not None)
''' % (ROOT, ROOT + '/tests')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert 'UNLOADED True True' in out.stdout, out.stdout + out.stderr
    assert 'EXTRA 6 True True' in out.stdout, out.stdout + out.stderr


def test_resumed_run_continues_the_mask_sequence(hp, tmp_path):
    '''save after two steps, reload into a fresh model: its next step draws the masks of step index 2,
    like the uninterrupted run's third step (a step's loss is a function of the parameters before it
    and of its masks; Adam's moments are not in a parameter file, so the comparison is that step's
    loss and SNR, bit for bit)'''
    a = small_model(hp, seed=5, NUM_LSTM_LAYERS=3, DROPOUT_KEEP_PROB=0.8)
    src = torch.as_tensor(rand_src(hp, 12, seed=2)).cuda()
    for _ in range(2):
        a.train_step(src)
    fn = str(tmp_path / 'resume')
    a.save_params(fn)
    assert int(np.load(fn + '.npz')['step_count']) == 2
    o3 = a.train_step(src)
    b = small_model(hp, seed=5, NUM_LSTM_LAYERS=3, DROPOUT_KEEP_PROB=0.8)
    b.load_params(fn)
    b.weights_written()
    assert b.step_base + b.step_count == 2
    r3 = b.train_step(src)
    assert float(r3['loss']) == float(o3['loss']) and float(r3['SNR']) == float(o3['SNR'])
    # a model that restarts the sequence at 0 draws other masks
    c = small_model(hp, seed=5, NUM_LSTM_LAYERS=3, DROPOUT_KEEP_PROB=0.8)
    c.load_params(fn)
    c.weights_written()
    c.step_base = 0
    assert float(c.train_step(src)['loss']) != float(o3['loss'])
