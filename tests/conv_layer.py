'''
Layer harness of the GPU tests of libdanet_conv_hip.so (include/danet_conv_hip.h), shared by
tests/test_gpu_conv.py and tests/test_gpu_conv_envelope.py: stored-output shapes, scatter into a
strided buffer, one call of each entry point, the float64 torch.nn.functional reference of one
layer of any shape, mode and layout the header admits, and seeded data.  Test infrastructure only.

The reference reads everything from the descriptor (shape, k, alpha, pool / depth-to-space), so it
serves the encoder's own descriptors (ops.conv_encoder_descs) and any ops._conv_desc alike.
'''
import torch
import torch.nn.functional as Fn

from conv_ref import depth_to_space


def _ops():
    from danet_amd import ops
    return ops


def _span(shape, strides):
    return sum((n - 1) * s for n, s in zip(shape, strides)) + 1


def _out_shape(d):
    if d.pool:
        return (d.B, d.Cout, d.T // 2, d.F // 2)
    if d.d2s:
        return (d.B, d.Cout // 4, 2 * d.T, 2 * d.F)
    return (d.B, d.Cout, d.T, d.F)


def _scatter(t, strides, dtype=torch.float32):
    '''a zero buffer holding the NCHW tensor t at `strides`, and that view'''
    buf = torch.zeros(_span(t.shape, strides), dtype=dtype, device='cuda')
    v = buf.as_strided(tuple(t.shape), tuple(strides))
    v.copy_(t)
    return buf, v


def run_layer(d, x, w, b, dy):
    '''the three entry points on layer d; x, dy NCHW (dy in the stored output's shape) float32 CPU.
    Returns y, argmax, dx, dw, db as CPU tensors (NCHW).'''
    ops = _ops()
    xs, ys = tuple(d.x_stride), tuple(d.y_stride)
    yshape = _out_shape(d)
    xbuf, _ = _scatter(x.cuda(), xs)
    ybuf = torch.zeros(_span(yshape, ys), device='cuda')
    am = torch.zeros(d.B, d.Cout, d.T // 2, d.F // 2, dtype=torch.uint8, device='cuda') if d.pool else None
    wg, bg = w.cuda(), b.cuda()
    ops.conv_fwd(d, xbuf, wg, bg, ybuf, am)
    dybuf, _ = _scatter(dy.cuda(), ys)
    dxbuf = torch.full_like(xbuf, float('nan'))
    ops.conv_bwd_data(d, dybuf, ybuf, am, wg, dxbuf)
    dw, db = torch.full_like(wg, float('nan')), torch.full_like(bg, float('nan'))
    ops.conv_bwd_weight(d, xbuf, dybuf, ybuf, am, dw, db)
    torch.cuda.synchronize()
    y = ybuf.as_strided(yshape, ys).cpu()
    dx = dxbuf.as_strided(tuple(x.shape), xs).cpu()
    return y, (am.cpu() if am is not None else None), dx, dw.cpu(), db.cpu()


def _windows(z, Tp, Fp):
    B, C = z.shape[:2]
    return z[:, :, :2 * Tp, :2 * Fp].reshape(B, C, Tp, 2, Fp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Tp, Fp, 4)


def reference(d, x, w, b, dy, gpu_y=None, gpu_am=None, nfft=None):
    '''float64 forward (plain) and backward of layer d; with gpu_y the backward takes the pool
    choice and the leaky-ReLU branch from the kernel's forward (tests/test_gpu_conv.py's module
    docstring says why).  alpha is the descriptor's (the fp32 value the kernel uses).  nfft, when
    given for a depth-to-space layer of the encoder, must be the FFT size its shape implies.'''
    assert nfft is None or not d.d2s or 8 * d.F == nfft, (nfft, d.F)
    alpha = d.alpha
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    k = d.k
    z = Fn.conv2d(x64, w64.permute(3, 2, 0, 1), b64, padding=k // 2)
    with torch.no_grad():
        yp = Fn.leaky_relu(z, alpha)
        if d.pool:
            yp = Fn.max_pool2d(yp, 2, 2)
        if d.d2s:
            yp = depth_to_space(yp)
    if gpu_y is None:
        y = Fn.leaky_relu(z, alpha)
        if d.pool:
            y = Fn.max_pool2d(y, 2, 2)
        if d.d2s:
            y = depth_to_space(y)
    else:
        if d.pool:
            z = _windows(z, d.T // 2, d.F // 2).gather(-1, gpu_am.long()[..., None]).squeeze(-1)
        if d.d2s:
            z = depth_to_space(z)
        y = z * torch.where(gpu_y > 0, 1.0, alpha).double()
    (y * dy.double()).sum().backward()
    return yp, x64.grad, w64.grad, b64.grad


def _data(d, seed, scale_x=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(d.B, d.Cin, d.T, d.F, generator=g) * scale_x
    lim = (6. / (d.k * d.k * (d.Cin + d.Cout))) ** 0.5
    w = (torch.rand(d.k, d.k, d.Cin, d.Cout, generator=g) * 2 - 1) * lim
    b = torch.randn(d.Cout, generator=g) * 0.1
    dy = torch.randn(*_out_shape(d), generator=g)
    return x, w, b, dy
