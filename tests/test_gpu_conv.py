'''
GPU tests of the convolution operators of libdanet_conv_hip.so (include/danet_conv_hip.h): every
conv layer of the conv-bilstm-v1 encoder (app/modules.py:263-379) at the cfg-2 shapes in the
layouts the encoder chains them with, forward / data gradient / weight and bias gradients against
float64 torch.nn.functional autograd; pool ties, the dropped odd column, the gradient at exactly
zero pre-activation, T = 4, and run-to-run bit equality of the weight gradients.

Where fp32 and float64 may legitimately disagree on a discrete choice -- which of two values within
rounding of each other is a window's maximum, whether a pre-activation within rounding of 0 is
positive -- the backward reference takes that choice from the kernel's own forward (its argmax and
the sign of its output), and the forward check makes sure the choice was a valid one.  Shapes
whose activations are exactly tied or exactly zero use the plain float64 reference throughout.
'''
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from conv_layer import _data, _scatter, _span, _out_shape, _windows, reference, run_layer
from gpu_helpers import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5
ALPHA = 0.3


def _ops():
    from danet_amd import ops
    return ops


def check_layer(d, x, w, b, dy, nfft, plain=False):
    y, am, dx, dw, db = run_layer(d, x, w, b, dy)
    ry, rdx, rdw, rdb = reference(d, x, w, b, dy, None if plain else y, None if plain else am, nfft)
    errs = dict(y=relerr(y, ry), dw=relerr(dw, rdw), db=relerr(db, rdb))
    if d.Cin > 1 or plain:
        errs['dx'] = relerr(dx, rdx)
    if am is not None:
        # the kernel's choice is a maximum of its window (to fp32 rounding)
        with torch.no_grad():
            z = Fn.leaky_relu(Fn.conv2d(x.double(), w.double().permute(3, 2, 0, 1), b.double(),
                                        padding=d.k // 2), ALPHA)
            win = _windows(z, d.T // 2, d.F // 2)
            picked = win.gather(-1, am.long()[..., None]).squeeze(-1)
            errs['argmax'] = float((win.max(-1).values - picked).abs().max() / win.abs().max())
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, (bad, errs)
    return y, am


def _descs(B, T, nfft):
    return _ops().conv_encoder_descs(B, T, nfft, ALPHA)


# ------------------------------------------------------------------ every layer at the cfg-2 shape
@pytest.mark.parametrize('layer', range(8))
def test_layer_cfg2_shape(layer):
    d = _descs(2, 128, 256)[layer]
    check_layer(d, *_data(d, 100 + layer), nfft=256)


@pytest.mark.parametrize('layer', [1, 6])
def test_layer_full_batch(layer):
    d = _descs(32, 128, 256)[layer]
    check_layer(d, *_data(d, 200 + layer), nfft=256)


# ------------------------------------------------------------------ the corner cases
@pytest.mark.parametrize('layer', [1, 3])
def test_pool_ties_in_constant_regions(layer):
    '''zero frames (what LENGTH_ALIGN pads) and zero bias: whole windows of exactly equal values;
    the gradient goes to the first maximum in row-major order, as F.max_pool2d's does'''
    d = _descs(2, 16, 64)[layer]
    x, w, b, dy = _data(d, 300 + layer)
    x[:, :, d.T // 2:] = 0.            # the second half of the frames: constant
    x[:, :, :, :5] = 0.
    b.zero_()
    y, am = check_layer(d, x, w, b, dy, nfft=64, plain=True)
    with torch.no_grad():
        z = Fn.leaky_relu(Fn.conv2d(x.double(), w.double().permute(3, 2, 0, 1), b.double(),
                                    padding=d.k // 2), ALPHA)
        win = _windows(z, d.T // 2, d.F // 2)
    tied = (win == win[..., :1]).all(-1)
    assert int(tied.sum()) > 100
    assert bool((am[tied] == 0).all())


def test_odd_width_drops_last_column():
    '''F = 33 (nfft 64): the 'valid' pool drops column 32, whose gradient is zero'''
    d = _descs(2, 16, 64)[1]
    assert d.F == 33 and d.F // 2 == 16
    x, w, b, dy = _data(d, 400)
    check_layer(d, x, w, b, dy, nfft=64, plain=True)
    # the last input column still reaches kept outputs (5x5 kernel: columns 30, 31 of the pre-pool grid)
    y0 = run_layer(d, x, w, b, dy)[0]
    x2 = x.clone()
    x2[:, :, :, 32] += 1000.
    y2 = run_layer(d, x2, w, b, dy)[0]
    assert y2.shape[-1] == 16
    assert not torch.equal(y0[..., 15], y2[..., 15])


def test_gradient_at_exact_zero_preactivation():
    '''x = 0 and bias = 0: every pre-activation is exactly 0, lrelu' = alpha there'''
    d = _descs(2, 16, 64)[2]
    x, w, b, dy = _data(d, 500)
    x.zero_()
    b.zero_()
    y, _, dx, dw, db = run_layer(d, x, w, b, dy)
    assert not bool(y.any())
    np.testing.assert_allclose(db.numpy(), ALPHA * dy.double().sum(dim=(0, 2, 3)).numpy(), rtol=1e-5, atol=1e-5)
    _, rdx, rdw, rdb = reference(d, x, w, b, dy, nfft=64)
    assert relerr(dx, rdx) < TOL and relerr(db, rdb) < TOL
    assert not bool(dw.any())


@pytest.mark.parametrize('layer', range(8))
def test_layers_at_T4(layer):
    '''T = 4: the LSTM-side layers run on T/4 = 1 frame'''
    d = _descs(2, 4, 64)[layer]
    check_layer(d, *_data(d, 600 + layer), nfft=64)


def test_weight_gradients_bit_identical_run_to_run():
    ops = _ops()
    d = _descs(8, 128, 256)[1]
    x, w, b, dy = _data(d, 700)
    xs, ys = tuple(d.x_stride), tuple(d.y_stride)
    xbuf, _ = _scatter(x.cuda(), xs)
    ybuf = torch.zeros(_span(_out_shape(d), ys), device='cuda')
    am = torch.zeros(d.B, d.Cout, d.T // 2, d.F // 2, dtype=torch.uint8, device='cuda')
    wg, bg = w.cuda(), b.cuda()
    ops.conv_fwd(d, xbuf, wg, bg, ybuf, am)
    dybuf, _ = _scatter(dy.cuda(), ys)
    outs = []
    for _ in range(2):
        dw, db = torch.empty_like(wg), torch.empty_like(bg)
        ops.conv_bwd_weight(d, xbuf, dybuf, ybuf, am, dw, db)
        dx = torch.empty_like(xbuf)
        ops.conv_bwd_data(d, dybuf, ybuf, am, wg, dx)
        outs.append((dw, db, dx))
    torch.cuda.synchronize()
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)
    # accumulate = 1 adds onto what is there
    dw, db = outs[0][0].clone(), outs[0][1].clone()
    ops.conv_bwd_weight(d, xbuf, dybuf, ybuf, am, dw, db, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(dw, outs[0][0] + outs[0][0]) and torch.equal(db, outs[0][1] + outs[0][1])
