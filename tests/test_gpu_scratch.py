'''
GPU tests of the per-shape scratch cache behind the cached chains of ops.py (ops._scratch): ops.si_sdr,
ops.si_sdr_noisy, ops.bss_eval, ops.stoi_eval, ops.phase_refine and ops.stitch.  A repeat reuses the cached views; a
shape that regrows the scratch of _lib.workspace does not leave a stale view behind for the shapes cached before;
another stream carves from a buffer of its own; the cache evicts at 64 entries.  Every result is compared bit for bit.
'''
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOOR = 1 << 20                                          # _lib.workspace never allocates less
SMALL = dict(FFT_SIZE=64, FFT_STRIDE=16)                 # F = 33
STOI = dict(FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000)   # F = 129, U / D = 5 / 4
STITCH = (2, 16, 33, 4)                                  # C, L, F, V


def _c64(g, *shape):
    return torch.view_as_complex(torch.randn(*shape, 2, generator=g, device='cuda') * 3)


def _gen(seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return g


class Chain(object):
    '''one cached chain at shapes (B, C, T): its inputs, its call, and what its cache and its scratch are called'''
    hp, grow_dim = SMALL, 2

    def __init__(self, ops, _lib):
        self.ops, self._lib = ops, _lib
        self.dev = torch.device('cuda', torch.cuda.current_device())

    def grow(self, shape):
        return tuple(2 * n if d == self.grow_dim else n for d, n in enumerate(shape))

    def spectra(self, shape, F, seed=0):
        B, C, T = shape
        g = _gen(seed + T)
        src = _c64(g, B, C, T, F)
        return src, (0.8 * src + 0.3 * src.flip(1) + 0.5 * _c64(g, B, C, T, F)).contiguous()


class SiSdr(Chain):
    tag, cache, small = 'metric', '_metric_ws', (2, 2, 6)

    def inputs(self, shape):
        return self.spectra(shape, 33)

    def call(self, x):
        return self.ops.si_sdr(x[0], x[1], 16)

    def dims(self, shape):
        return shape + (64, 16)

    def nbytes(self, shape):
        return self._lib.load_metric().danet_metric_workspace_bytes(*self.dims(shape))

    def workspace(self, shape):
        B, C, T = shape
        return self.ops._wave_workspace('metric', self.ops._metric_ws, 2 * C, 2, B, C, T, 64, 16, self.dev)


class SiSdrNoisy(SiSdr):
    tag, cache = 'neval', '_neval_ws'

    def inputs(self, shape):
        B, C, T = shape
        g = _gen(7 + T)
        return self.spectra(shape, 33) + (_c64(g, B, T, 33), torch.rand(B, generator=g, device='cuda') + 0.5)

    def call(self, x):
        return self.ops.si_sdr_noisy(x[0], x[1], x[2], x[3], 16)

    def nbytes(self, shape):
        return self._lib.load_neval().danet_neval_workspace_bytes(*self.dims(shape))

    def workspace(self, shape):
        B, C, T = shape
        return self.ops._wave_workspace('neval', self.ops._neval_ws, 2 * C + 1, 3, B, C, T, 64, 16, self.dev)


class Bss(Chain):
    tag, cache, small, grow_dim = 'bss', '_bss_ws', (2, 2, 6), 0          # the scratch grows with the group, not with T

    def inputs(self, shape):
        return self.spectra(shape, 33)

    def call(self, x):
        return self.ops.bss_eval(x[0], x[1], filter_len=8, fft_stride=16)

    def dims(self, shape):
        return (shape[0], shape[1], 8)

    def nbytes(self, shape):
        return self.ops.bss_workspace_bytes(*self.dims(shape))

    def workspace(self, shape):
        return self.ops._bss_workspace(shape[0], shape[1], 8, self.dev)


class Stoi(Chain):
    tag, cache, small, grow_dim, hp = 'stoi', '_stoi_ws', (2, 2, 52), 0, STOI      # 52 frames: 30 segments and more

    def inputs(self, shape):
        return self.spectra(shape, 129)

    def call(self, x):
        return self.ops.stoi_eval(x[0], x[1], fft_stride=64, smprate=8000, with_count=True)

    def dims(self, shape):
        return (shape[0], shape[1], (shape[2] - 1) * 64, 5, 4)

    def nbytes(self, shape):
        return self.ops.stoi_workspace_bytes(*self.dims(shape))

    def workspace(self, shape):
        return self.ops._stoi_workspace(*(self.dims(shape) + (self.dev,)))


class Phase(Chain):
    tag, cache, small = 'phase', '_phase_ws', (2, 2, 9)

    def inputs(self, shape):
        src, est = self.spectra(shape, 33)
        return est, src

    def call(self, x):
        return (self.ops.phase_refine(x[0], x[1], 2, fft_stride=16),)

    def dims(self, shape):
        return shape + (64, 16)

    def nbytes(self, shape):
        return self.ops.phase_workspace_bytes(*self.dims(shape))

    def workspace(self, shape):
        return self.ops._phase_workspace(*(self.dims(shape) + (self.dev,)))


class Stitch(Chain):
    tag, cache, small, grow_dim = 'stitch', '_stitch_ws', (50,), 0          # the shape is (T,)

    def inputs(self, shape):
        C, L, F, V = STITCH
        n = self.ops.stitch_chunks(shape[0], L, V)
        g = _gen(shape[0])
        return (torch.rand(n, C, L, F, generator=g, device='cuda'), torch.randn(n, L, F, 2, generator=g, device='cuda'),
                shape[0], V)

    def call(self, x):
        return (self.ops.stitch(*x),)

    def dims(self, shape):
        C, L, F, V = STITCH
        return (self.ops.stitch_chunks(shape[0], L, V), C, L, F, V, shape[0])

    def nbytes(self, shape):
        n, C, L, F, V, T = self.dims(shape)
        return self.ops._carve(None, self.ops._stitch_parts(n, C, L, F, T, V))[1]      # the carve's own end

    def workspace(self, shape):
        n, C, L, F, V, T = self.dims(shape)
        return self.ops._stitch_workspace(n, C, L, F, T, V, self.dev)


CHAINS = [SiSdr, SiSdrNoisy, Bss, Stoi, Phase, Stitch]


@pytest.fixture(params=CHAINS, ids=lambda c: c.__name__)
def chain(request, hp):
    '''the chain, on a cache and a scratch nobody has used: the tests below depend on what was cached before'''
    from danet_amd import _lib, ops
    hp.load(request.param.hp)
    hp.digest()
    c = request.param(ops, _lib)
    torch.cuda.synchronize()
    getattr(ops, c.cache).clear()
    for key in [k for k in _lib._ws if k[2] == c.tag]:
        del _lib._ws[key]
    return c


def _bits(res):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in res]


def _key(c, shape, stream=None):
    stream = torch.cuda.current_stream() if stream is None else stream
    return (c.dev.index, stream.cuda_stream) + tuple(c.dims(shape))


def _entry(c, shape, stream=None):
    '''(buffer, [views]) the cache holds for this shape'''
    hit = getattr(c.ops, c.cache)[_key(c, shape, stream)]
    return hit[0], list(hit[1].values()) if isinstance(hit[1], dict) else list(hit[1:])


def _scratch_of(c, stream=None):
    stream = torch.cuda.current_stream() if stream is None else stream
    return c._lib._ws[(c.dev.index, stream.cuda_stream, c.tag)]


def _inside(views, buf):
    lo, hi = buf.data_ptr(), buf.data_ptr() + buf.numel()
    return all(lo <= v.data_ptr() and v.data_ptr() + v.numel() * v.element_size() <= hi for v in views)


def test_repeat_reuses_the_cached_views(chain):
    c = chain
    x = c.inputs(c.small)
    first = _bits(c.call(x))
    buf, views = _entry(c, c.small)
    ptrs = [v.data_ptr() for v in views]
    again = _bits(c.call(x))
    buf2, views2 = _entry(c, c.small)
    assert again == first
    assert buf2 is buf is _scratch_of(c) and [v.data_ptr() for v in views2] == ptrs and _inside(views2, buf)
    assert all(a is b for a, b in zip(views, views2)) and len(getattr(c.ops, c.cache)) == 1
    if c.tag in ('metric', 'neval'):                     # a hit hands out the cached tuple itself
        assert c.workspace(c.small) is c.workspace(c.small) is getattr(c.ops, c.cache)[_key(c, c.small)]


def test_a_regrown_scratch_leaves_no_stale_view(chain):
    c = chain
    assert c.nbytes(c.small) <= FLOOR
    large = c.small
    while c.nbytes(large) <= FLOOR:
        large = c.grow(large)
    x, xl = c.inputs(c.small), c.inputs(large)
    first = _bits(c.call(x))
    old = _scratch_of(c)
    assert old.numel() == FLOOR and _entry(c, c.small)[0] is old
    c.call(xl)
    grown = _scratch_of(c)
    assert grown is not old and grown.numel() == c.nbytes(large) > FLOOR
    stale = _entry(c, c.small)[0]
    assert stale is old                                  # still cached, and no longer what _lib.workspace holds
    del old, stale
    third = _bits(c.call(x))
    assert third == first
    buf, views = _entry(c, c.small)
    assert buf is grown is _scratch_of(c) and _inside(views, grown)
    assert _inside(_entry(c, large)[1], grown)


def test_a_side_stream_carves_from_its_own_buffer(chain):
    c = chain
    x = c.inputs(c.small)
    main = _bits(c.call(x))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = c.call(x)
        buf_side, views_side = _entry(c, c.small)
        assert buf_side is _scratch_of(c)
    side.synchronize()
    buf_main, views_main = _entry(c, c.small)
    assert _bits(res) == main
    assert buf_side is not buf_main and buf_side.data_ptr() != buf_main.data_ptr()
    assert _inside(views_side, buf_side) and _inside(views_main, buf_main) and not _inside(views_side[:1], buf_main)
    assert _key(c, c.small, side) != _key(c, c.small) and len(getattr(c.ops, c.cache)) == 2


def test_the_cache_evicts_at_64_entries(chain):
    c = chain
    cache = getattr(c.ops, c.cache)
    x = c.inputs(c.small)
    first = _bits(c.call(x))
    assert len(cache) == 1
    shape, seen = c.small, 1
    for i in range(65):
        shape = shape[:c.grow_dim] + (shape[c.grow_dim] + 1,) + shape[c.grow_dim + 1:]
        c.workspace(shape)                               # the workspace function alone: no launch
        seen += 1
        assert len(cache) == (seen if seen <= 64 else seen - 64), (i, len(cache))
        assert _key(c, shape) in cache
    assert seen == 66 and len(cache) == 2 and _key(c, c.small) not in cache
    assert _bits(c.call(x)) == first
    assert len(cache) == 3 and _inside(_entry(c, c.small)[1], _scratch_of(c))


def test_refused_arguments_raise_assertion_errors_and_launch_nothing():
    from danet_amd import ops
    empty = torch.zeros(1, 1, 0, 33, dtype=torch.complex64, device='cuda')          # T = 0
    w = torch.ones(64, device='cuda')
    with pytest.raises(AssertionError):
        ops.metric_synth(empty, empty, 16, w)
    with pytest.raises(AssertionError):
        ops.neval_synth(empty, empty, empty[:, 0], None, 16, w)
    f64 = dict(dtype=torch.float64, device='cuda')
    with pytest.raises(AssertionError, match='^R: want'):
        ops.bss_systems(torch.zeros(2, 2, 15, **f64), torch.zeros(2, 2, 2, 8, **f64))
    with pytest.raises(AssertionError, match='^T: want'):
        ops.stoi_segments(torch.zeros(2, 4, 15, 30, **f64), torch.zeros(2, 2, dtype=torch.int32, device='cuda'), 30)
