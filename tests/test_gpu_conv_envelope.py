'''
GPU tests of libdanet_conv_hip.so across the whole envelope include/danet_conv_hip.h promises, not
only the encoder's eight layers: every <KS, NT> instantiation of the forward, data-gradient and
weight-gradient kernels, pool and depth-to-space at every tile count, channel counts that make the
implicit GEMM's K walk wrap more than once per step, T and F down to 1, alpha at 0 and near 1,
layouts with f-strides other than 1 and gaps between rows and channels, the weight-gradient slab
plan at its extremes, danet_conv_add, pool ties at NT > 1 and NaN in the input.

Every case runs fwd, bwd_data and bwd_weight through `run_guarded`, which poisons what the kernels
must not read and watches what they must not write: the x, dy and saved-y buffers hold a NaN in
every element their views do not address; y, argmax, dx, dw and db sit between guard elements in
buffers pre-filled with a sentinel bit pattern that must survive, bit for bit, wherever the view
does not point; bwd_weight gets exactly danet_conv_workspace_bytes(...) bytes, followed by a NaN
tail that must survive.  y, dx, dw and db are compared with float64 torch.nn.functional autograd
(tests/conv_layer.py) at TOL relative to each tensor's maximum, and y and dx once more on their
border band alone (the first and last k//2 rows and columns), relative to the band's own maximum,
so that a padding error is not diluted by the interior.  The backward reference takes the pool
choice and the leaky-ReLU branch from the kernel's forward; a separate check confirms that each
pool choice is a maximum of its window.
'''
import ctypes

import pytest
import torch
import torch.nn.functional as Fn

from conv_layer import _data, _out_shape, _span, _windows, reference
from gpu_helpers import oracle_threads, relerr

pytestmark = pytest.mark.gpu

# fp32 products are exact (v_mfma_f32_16x16x4_f32) and only the sums round.  The deepest K here is
# Cin k k = 64 * 25 = 1600 terms; with random signs the rounding error of such a sum grows like
# sqrt(K) eps = 40 * 6e-8 = 2.4e-6 of its scale, which TOL covers without loosening.
TOL = 1e-5
SENT = 0x7FC5A5A5          # a quiet NaN with a payload: poison wherever a kernel would read it
SENT_U8 = 0xA5
G = 37                     # guard elements before and after every buffer
WS_TAIL = 64               # NaN floats after the workspace


# ------------------------------------------------------------------ layouts of a [B][C][H][W] tensor
def _layout(name, shape):
    B, C, H, W = shape
    if name == 'nchw':
        return (C * H * W, H * W, W, 1)
    if name == 'nhwc':                     # channels-last: f-stride C
        return (H * W * C, 1, W * C, C)
    if name == 'tm':                       # time-major [H][B][C][W], like ops.conv_encoder_descs's TM
        return (C * W, W, B * C * W, 1)
    if name == 'pad':                      # slack after every row, channel and batch item
        cp = H * (W + 3) + 5
        return (C * cp + 7, cp, W + 3, 1)
    if name == 'fmajor':                   # [B][C][W][H]: t-stride 1, f-stride H
        return (C * H * W, H * W, 1, H)
    raise KeyError(name)


LAYOUTS = ('nchw', 'nhwc', 'tm', 'pad', 'fmajor')


def desc(B, Cin, Cout, T, F, k, mode='plain', alpha=0.3, xl='nhwc', yl='pad'):
    from danet_amd import ops
    pool, d2s = mode == 'pool', mode == 'd2s'
    d = ops._conv_desc(B, Cin, Cout, T, F, k, alpha, (0,) * 4, (0,) * 4, pool, d2s)
    xs, ys = _layout(xl, (B, Cin, T, F)), _layout(yl, _out_shape(d))
    return ops._conv_desc(B, Cin, Cout, T, F, k, alpha, xs, ys, pool, d2s)


# ------------------------------------------------------------------ the guarded harness
def _dense(shape):
    s, out = 1, []
    for n in reversed(shape):
        out.append(s)
        s *= n
    return tuple(reversed(out))


def _buffer(shape, strides, dtype=torch.float32):
    '''G guard elements, the span of the view, G guard elements, all holding the sentinel.
    Returns (buffer, view, mask of the elements the view addresses).'''
    n = _span(shape, strides) + 2 * G
    if dtype == torch.uint8:
        buf = torch.full((n,), SENT_U8, dtype=torch.uint8, device='cuda')
    else:
        buf = torch.full((n,), SENT, dtype=torch.int32, device='cuda').view(torch.float32)
    view = buf.as_strided(tuple(shape), tuple(strides), G)
    mask = torch.zeros(n, dtype=torch.bool, device='cuda')
    mask.as_strided(tuple(shape), tuple(strides), G).fill_(True)
    return buf, view, mask


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _kept(buf, mask):
    '''every element outside the view still holds the sentinel, bit for bit'''
    s = SENT if buf.dtype == torch.float32 else SENT_U8
    return bool((_bits(buf)[~mask] == s).all())


class Result(object):
    pass


def run_guarded(d, x, w, b, dy, dw0=None, db0=None):
    '''fwd, bwd_data, bwd_weight (accumulate = 1 onto dw0, db0 when given) on layer d in poisoned,
    guarded buffers; asserts that nothing outside the outputs' views changed and that no input
    changed.  Returns y, am, dx, dw, db as CPU tensors (NCHW).'''
    from danet_amd import _lib, ops
    xs, ys = tuple(d.x_stride), tuple(d.y_stride)
    yshape = _out_shape(d)
    xbuf, xv, _ = _buffer(x.shape, xs)
    xv.copy_(x.cuda())
    dybuf, dyv, _ = _buffer(yshape, ys)
    dyv.copy_(dy.cuda())
    ybuf, yv, ym = _buffer(yshape, ys)
    abuf = av = None
    if d.pool:
        ashape = (d.B, d.Cout, d.T // 2, d.F // 2)
        abuf, av, am_mask = _buffer(ashape, _dense(ashape), torch.uint8)
    dxbuf, dxv, dxm = _buffer(x.shape, xs)
    dwbuf, dwv, dwm = _buffer(w.shape, _dense(w.shape))
    dbbuf, dbv, dbm = _buffer(b.shape, (1,))
    accumulate = dw0 is not None
    if accumulate:
        dwv.copy_(dw0.cuda())
        dbv.copy_(db0.cuda())
    nbytes = _lib.conv_ws_bytes(_lib.CONV_WS_BWD_WEIGHT, d)
    assert nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + WS_TAIL,), SENT, dtype=torch.int32, device='cuda').view(torch.float32)
    wg, bg = w.cuda(), b.cuda()
    inputs = [_bits(t).clone() for t in (xbuf, dybuf, wg, bg)]

    ops.conv_fwd(d, xv, wg, bg, yv, av)
    torch.cuda.synchronize()
    assert _kept(ybuf, ym), 'fwd wrote outside y'
    if d.pool:
        assert _kept(abuf, am_mask), 'fwd wrote outside argmax'
    ysaved = _bits(ybuf).clone()        # its unaddressed elements: the sentinel, a NaN
    ops.conv_bwd_data(d, dyv, yv, av, wg, dxv)
    _lib.conv_check(_lib.load_conv().danet_conv_bwd_weight(
        _lib.stream(), ctypes.byref(d), xv.data_ptr(), dyv.data_ptr(), yv.data_ptr(),
        av.data_ptr() if av is not None else None, dwv.data_ptr(), dbv.data_ptr(), int(accumulate),
        ws.data_ptr(), nbytes))
    torch.cuda.synchronize()
    assert _kept(dxbuf, dxm), 'bwd_data wrote outside dx'
    assert _kept(dwbuf, dwm) and _kept(dbbuf, dbm), 'bwd_weight wrote outside dw / db'
    assert bool((_bits(ws)[nbytes // 4:] == SENT).all()), 'bwd_weight wrote past its workspace'
    for before, after in zip(inputs + [ysaved], (xbuf, dybuf, wg, bg, ybuf)):
        assert torch.equal(before, _bits(after)), 'an input buffer changed'
    r = Result()
    r.y, r.dx, r.dw, r.db = yv.cpu(), dxv.cpu(), dwv.cpu(), dbv.cpu()
    r.am = av.cpu() if av is not None else None
    return r


# ------------------------------------------------------------------ checks
def _band(n_out, n, P, mode):
    '''output rows (or columns) within P of the pre-pool / pre-depth-to-space border'''
    r = torch.arange(n_out)
    if mode == 'pool':
        lo, hi = 2 * r, 2 * r + 1
    elif mode == 'd2s':
        lo = hi = r // 2
    else:
        lo = hi = r
    return (lo < P) | (hi >= n - P)


def _mode(d):
    return 'pool' if d.pool else ('d2s' if d.d2s else 'plain')


def _z64(d, x, w, b):
    return Fn.conv2d(x.double(), w.double().permute(3, 2, 0, 1), b.double(), padding=d.k // 2)


def check(d, x, w, b, dy, r):
    '''r against float64; returns the reference (y, dx, dw, db)'''
    with oracle_threads():
        ref = reference(d, x, w, b, dy, r.y, r.am)
    ry, rdx, rdw, rdb = ref
    for name, t in (('y', r.y), ('dx', r.dx), ('dw', r.dw), ('db', r.db)):
        assert bool(torch.isfinite(t).all()), name + ' is not finite'
    errs = dict(y=relerr(r.y, ry), dx=relerr(r.dx, rdx), dw=relerr(r.dw, rdw), db=relerr(r.db, rdb))
    P, mode = d.k // 2, _mode(d)
    yb = _band(r.y.shape[2], d.T, P, mode)[:, None] | _band(r.y.shape[3], d.F, P, mode)[None, :]
    xb = _band(d.T, d.T, P, 'plain')[:, None] | _band(d.F, d.F, P, 'plain')[None, :]
    errs['y_border'] = relerr(r.y[..., yb], ry[..., yb])
    errs['dx_border'] = relerr(r.dx[..., xb], rdx[..., xb])
    if d.pool:
        assert int(r.am.max()) <= 3
        with torch.no_grad():
            win = _windows(Fn.leaky_relu(_z64(d, x, w, b), d.alpha), d.T // 2, d.F // 2)
            picked = win.gather(-1, r.am.long()[..., None]).squeeze(-1)
            errs['argmax'] = float((win.max(-1).values - picked).abs().max() / (win.abs().max() + 1e-30))
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, (bad, errs)
    return ref


def run_and_check(d, seed, **kw):
    x, w, b, dy = _data(d, seed, **kw)
    r = run_guarded(d, x, w, b, dy)
    check(d, x, w, b, dy, r)
    return r


# ------------------------------------------------------------------ (a) the instantiation matrix
# (Cin, Cout, k, mode).  fwd and wgrad run <k, ntiles(Cout)>, dgrad <k, ntiles(Cin)>, with
# ntiles(n) = 1 for n <= 16, 2 for n <= 32, else 4.  tests/test_conv_envelope_cpu.py checks that
# the table runs all 18 kernels, pool at every NT, depth-to-space at every NT with both k, and
# channel counts that are not multiples of 4 (and below 4) on both K walks.
MATRIX = (
    (1, 7, 3, 'plain'),      # fwd <3,1>  dgrad <3,1>; Cin = 1: one K step wraps 4 times
    (2, 17, 5, 'plain'),     # fwd <5,2>  dgrad <5,1>
    (3, 33, 3, 'pool'),      # fwd <3,4>  pool NT 4
    (5, 31, 3, 'pool'),      # fwd <3,2>  pool NT 2
    (17, 5, 5, 'pool'),      # fwd <5,1>  pool NT 1  dgrad <5,2>
    (33, 2, 3, 'plain'),     # dgrad <3,4>; Cout = 2: the dgrad walk wraps twice
    (64, 63, 5, 'plain'),    # fwd <5,4>  dgrad <5,4>; the deepest K = 1600
    (31, 1, 3, 'plain'),     # dgrad <3,2>; Cout = 1
    (16, 3, 5, 'plain'),     # dgrad <5,1>; Cout = 3 at k = 5
    (7, 12, 3, 'd2s'),       # d2s <3,1>
    (12, 16, 5, 'd2s'),      # d2s <5,1>
    (20, 20, 3, 'd2s'),      # d2s <3,2>  dgrad <3,2>
    (3, 32, 5, 'd2s'),       # d2s <5,2>
    (16, 48, 3, 'd2s'),      # d2s <3,4>
    (32, 64, 5, 'd2s'),      # d2s <5,4>  dgrad <5,2>
)
_GEO = ((2, 9, 17), (3, 6, 15), (2, 5, 33), (4, 8, 20), (3, 11, 9))


@pytest.mark.parametrize('i', range(len(MATRIX)), ids=['%d-%d-k%d-%s' % c for c in MATRIX])
def test_instantiation_matrix(i):
    Cin, Cout, k, mode = MATRIX[i]
    B, T, F = _GEO[i % len(_GEO)]
    d = desc(B, Cin, Cout, T, F, k, mode, xl=LAYOUTS[i % 5], yl=LAYOUTS[(i + 2) % 5])
    run_and_check(d, 1000 + i)


# ------------------------------------------------------------------ (b) geometry edges
@pytest.mark.parametrize('T', [1, 2, 3, 17])
@pytest.mark.parametrize('F', [1, 2, 15, 16, 17, 33])
def test_geometry_plain(T, F):
    d = desc(2, 3, 20, T, F, 5, 'plain', xl='pad', yl='nhwc')
    run_and_check(d, 2000 + 50 * T + F)


@pytest.mark.parametrize('T', [2, 3, 17])
@pytest.mark.parametrize('F', [2, 15, 16, 17, 33])
def test_geometry_pool(T, F):
    d = desc(3, 6, 40, T, F, 3, 'pool', xl='tm', yl='fmajor')
    run_and_check(d, 3000 + 50 * T + F)


@pytest.mark.parametrize('T,F', [(1, 1), (1, 17), (17, 1), (3, 16)])
def test_geometry_d2s(T, F):
    d = desc(2, 5, 28, T, F, 5, 'd2s', xl='nchw', yl='tm')
    run_and_check(d, 4000 + 50 * T + F)


@pytest.mark.parametrize('Cin,Cout,k', [(3, 12, 3), (9, 40, 5)])
def test_pool_odd_T_and_F(Cin, Cout, k):
    '''T = 7, F = 9: the 'valid' pool drops row 6 and column 8.  g is zero there, so with only the
    centre tap of w non-zero dx is exactly 0 on that row and column; with the whole kernel the
    dropped inputs still reach the last kept outputs'''
    d = desc(2, Cin, Cout, 7, 9, k, 'pool', xl='nhwc', yl='pad')
    x, w, b, dy = _data(d, 5000 + k)
    r = run_guarded(d, x, w, b, dy)
    check(d, x, w, b, dy, r)
    x2 = x.clone()
    x2[:, :, 6, :] += 100.
    x2[:, :, :, 8] += 100.
    y2 = run_guarded(d, x2, w, b, dy).y
    assert not torch.equal(r.y[:, :, 2, :], y2[:, :, 2, :])
    assert not torch.equal(r.y[:, :, :, 3], y2[:, :, :, 3])
    wc = torch.zeros_like(w)
    wc[k // 2, k // 2] = w[k // 2, k // 2]
    rc = run_guarded(d, x, wc, b, dy)
    check(d, x, wc, b, dy, rc)
    assert bool((rc.dx[:, :, 6, :] == 0).all()) and bool((rc.dx[:, :, :, 8] == 0).all())
    assert bool((rc.dx[:, :, :6, :8] != 0).any())


# ------------------------------------------------------------------ (c) alpha
@pytest.mark.parametrize('alpha', [0.0, 0.3, 0.99])
@pytest.mark.parametrize('mode', ['plain', 'pool', 'd2s'])
def test_alpha(alpha, mode):
    d = desc(2, 5, 24, 6, 13, 3, mode, alpha=alpha, xl='fmajor', yl='nchw')
    x, w, b, dy = _data(d, 6000 + int(alpha * 100))
    r = run_guarded(d, x, w, b, dy)
    check(d, x, w, b, dy, r)
    if alpha == 0.0:
        # negative z gives y = 0 * z = -0.0 (tf.maximum(0 * z, z) likewise) and lrelu' = 0
        with torch.no_grad():
            z = _z64(d, x, w, b)
        margin = 1e-4 * float(z.abs().max())
        if d.pool:
            neg = (_windows(z, d.T // 2, d.F // 2) < -margin).all(-1)
        else:
            neg = z < -margin
            if d.d2s:
                from conv_ref import depth_to_space
                neg = depth_to_space(neg.double()) > 0
        assert int(neg.sum()) > 20
        yn = r.y[neg]
        assert bool((yn == 0).all()) and bool(torch.signbit(yn).all())


# ------------------------------------------------------------------ (d) layouts
@pytest.mark.parametrize('xl,yl', [(a, b) for a in LAYOUTS for b in LAYOUTS if a != b])
def test_layouts(xl, yl):
    i = LAYOUTS.index(xl) * 5 + LAYOUTS.index(yl)
    mode = ('plain', 'pool', 'd2s')[i % 3]
    d = desc(3, 7, 20, 10, 11, (3, 5)[i % 2], mode, xl=xl, yl=yl)
    run_and_check(d, 7000 + i)


# ------------------------------------------------------------------ (e) the weight-gradient slab plan
# wgrad_plan (csrc/conv/conv.hip): Ktot = Cin k k, Mtot = Ktot + 1 (the row of db), nmt =
# ceil(Mtot / 16) row tiles, target = 4096 // nmt slabs, R = B T rows, rows_per_slab =
# ceil(R / target), nslab = ceil(R / rows_per_slab).  The reduce sums slabs g, g+16, .. per group.
#   one slab:   Cin 16, k 5: Mtot 401, nmt 26, target 157; R = 1 is the only way to one slab
#               (nslab = 1 needs rows_per_slab >= R, i.e. target = 1 or R = 1), so B = 1 here.
#   16 slabs:   Cin 5, k 5: Mtot 126, nmt 8, target 512; R = 2 * 8 = 16 -> 1 row each, 16 slabs.
#   > 16 slabs: Cin 1, k 3: Mtot 10, nmt 1, target 4096; R = 17 * 241 = 4097 -> 2 rows each,
#               2049 slabs (128 per group + 1 in group 0), the last one a single row.
#   large nmt:  Cin 64, k 5: Mtot 1601, nmt 101, target 40; R = 5 * 17 = 85 -> 3 rows each,
#               29 slabs (groups of 2 and 1), the last one a single row.
# (Cin, Cout, k, mode, B, T, F, nslab); the slab cases may exceed the other tests' B, T bounds.
SLABS = (
    (16, 17, 5, 'plain', 1, 1, 40, 1),
    (5, 32, 5, 'd2s', 2, 8, 24, 16),
    (1, 8, 3, 'pool', 17, 241, 3, 2049),
    (64, 20, 5, 'plain', 5, 17, 9, 29),
)


@pytest.mark.parametrize('case', SLABS, ids=['nslab%d' % c[-1] for c in SLABS])
def test_wgrad_slab_plan(case):
    Cin, Cout, k, mode, B, T, F, nslab = case
    d = desc(B, Cin, Cout, T, F, k, mode, xl='nchw', yl='nhwc')
    x, w, b, dy = _data(d, 8000 + nslab)
    r = run_guarded(d, x, w, b, dy)
    _, _, rdw, rdb = check(d, x, w, b, dy, r)
    # accumulate = 1 adds the gradient onto what dw, db hold
    g = torch.Generator().manual_seed(8100 + nslab)
    dw0 = torch.randn(w.shape, generator=g) * float(rdw.abs().max())
    db0 = torch.randn(b.shape, generator=g) * float(rdb.abs().max())
    ra = run_guarded(d, x, w, b, dy, dw0, db0)
    assert relerr(ra.dw, dw0.double() + rdw) < TOL
    assert relerr(ra.db, db0.double() + rdb) < TOL


# fwd and wgrad <k, ntiles(Cout)>: the six weight-gradient kernels, each run twice
@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('Cout', [7, 31, 63])
def test_bit_identical_run_to_run(k, Cout):
    d = desc(4, 5, Cout, 40, 37, k, 'pool' if k == 5 else 'plain', xl='pad', yl='tm')
    x, w, b, dy = _data(d, 8200 + k * 100 + Cout)
    r1 = run_guarded(d, x, w, b, dy)
    check(d, x, w, b, dy, r1)
    r2 = run_guarded(d, x, w, b, dy)
    for name in ('y', 'dx', 'dw', 'db'):
        assert torch.equal(_bits(getattr(r1, name)), _bits(getattr(r2, name))), name
    if d.pool:
        assert torch.equal(r1.am, r2.am)


# ------------------------------------------------------------------ (f) danet_conv_add
@pytest.mark.parametrize('n', [1, 255, 257, 4096 * 256 + 3])
@pytest.mark.parametrize('alias', ['a', 'b', None])
def test_conv_add(n, alias):
    '''bit-equal to torch's a + b; n = 4096 * 256 + 3 needs the grid-stride loop (the grid stops at
    4096 blocks of 256); out may be a or b; nothing past out[n - 1] is written'''
    from danet_amd import ops
    g = torch.Generator().manual_seed(n)
    a0, b0 = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    want = a0 + b0
    a, b = a0.clone(), b0.clone()
    if alias is None:
        buf = torch.full((n + G,), SENT, dtype=torch.int32, device='cuda').view(torch.float32)
        out = buf[:n]
    else:
        out = a if alias == 'a' else b
    ops.conv_add(a, b, out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    if alias is None:
        assert bool((_bits(buf)[n:] == SENT).all())
        assert torch.equal(a, a0) and torch.equal(b, b0)
    else:
        assert torch.equal(b if alias == 'a' else a, b0 if alias == 'a' else a0)


# ------------------------------------------------------------------ (g) pool ties at NT > 1
@pytest.mark.parametrize('Cout,k', [(24, 3), (63, 5)])
def test_pool_ties_multi_tile(Cout, k):
    '''zero input and zero bias make whole windows exactly equal: argmax is 0 there, the first
    maximum in row-major order (F.max_pool2d's choice too)'''
    d = desc(2, 6, Cout, 16, 20, k, 'pool', xl='nhwc', yl='nchw')
    x, w, b, dy = _data(d, 9000 + Cout)
    x[:, :, 8:] = 0.
    x[:, :, :, :6] = 0.
    b.zero_()
    r = run_guarded(d, x, w, b, dy)
    check(d, x, w, b, dy, r)
    with torch.no_grad():
        win = _windows(Fn.leaky_relu(_z64(d, x, w, b), d.alpha), d.T // 2, d.F // 2)
    tied = (win == win[..., :1]).all(-1)
    assert int(tied.sum()) > 100
    assert bool((r.am[tied] == 0).all())
    assert int(r.am.max()) <= 3


# ------------------------------------------------------------------ (h) NaN in x, plain layer
@pytest.mark.parametrize('Cin,Cout,k', [(3, 8, 3), (20, 40, 5)])
def test_nan_in_x_plain(Cin, Cout, k):
    '''y is NaN exactly where float64's is (every output whose window holds a NaN); dx stays
    finite (g comes from dy and the sign of y, and NaN > 0 is false) exactly as float64's does'''
    d = desc(2, Cin, Cout, 12, 19, k, 'plain', xl='tm', yl='pad')
    x, w, b, dy = _data(d, 9100 + k)
    x[0, Cin - 1, 3, 4] = float('nan')
    x[1, 0, 11, 18] = float('nan')
    x[1, Cin // 2, 0, 9] = float('nan')
    r = run_guarded(d, x, w, b, dy)
    with oracle_threads():
        ry, rdx, rdw, rdb = reference(d, x, w, b, dy, r.y, r.am)
    for got, want in ((r.y, ry), (r.dx, rdx), (r.dw, rdw), (r.db, rdb)):
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        ok = ~torch.isnan(want)
        assert relerr(got[ok], want[ok]) < TOL
    assert bool(torch.isnan(r.y).any())
