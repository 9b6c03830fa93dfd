'''
CPU tests (no GPU) of what the wrappers of the extension libraries share in ops.py: the carver that lays the parts of a
workspace into a buffer (against every library's own *_workspace_bytes, a host function), the tensor check, and the
group function behind ops.bss_group and ops.stoi_group.
'''
import numpy as np
import pytest
import torch

f32, f64, i32, c64, u8 = torch.float32, torch.float64, torch.int32, torch.complex64, torch.uint8
WAVE_SHAPES = ((32, 2, 128, 256, 64), (1, 1, 2, 64, 32), (3, 4, 130, 1024, 128))
PHASE_SHAPES = ((1, 1, 2, 64, 8), (3, 2, 9, 64, 16), (2, 4, 40, 256, 64), (32, 2, 128, 256, 64), (1, 2, 1251, 512, 128),
                (5, 3, 7, 1024, 512), (1, 4, 2, 1024, 128))
BSS_SHAPES = ((1, 1, 1), (3, 2, 8), (2, 4, 512), (32, 2, 512), (65535, 1, 1), (7, 3, 33))
STOI_SHAPES = ((1, 1, 1, 5, 4), (3, 2, 255, 1, 1), (2, 4, 8128, 5, 4), (32, 2, 8128, 5, 8), (16383, 1, 300, 100, 441),
               (7, 3, 2049, 100, 819))


def _layouts():
    '''(label, parts, the library's size) of every library's layout at the shapes its own CPU test asks the size of'''
    from danet_amd import _lib, ops
    for B, C, T, N, S in WAVE_SHAPES:
        yield 'metric', ops._wave_parts(2 * C, 2, B, T, S), _lib.load_metric().danet_metric_workspace_bytes(B, C, T, N, S)
        yield 'neval', ops._wave_parts(2 * C + 1, 3, B, T, S), _lib.load_neval().danet_neval_workspace_bytes(B, C, T, N, S)
    for shape in PHASE_SHAPES:
        yield 'phase', ops._phase_layout(*shape), ops.phase_workspace_bytes(*shape)
    for shape in BSS_SHAPES:
        yield 'bss', ops.bss_parts(*shape), ops.bss_workspace_bytes(*shape)
    for shape in STOI_SHAPES:
        yield 'stoi', ops.stoi_parts(*shape), ops.stoi_workspace_bytes(*shape)


def _check_carve(parts, want_end, label=''):
    from danet_amd import ops
    assert ops._carve(None, parts) == ({}, want_end), label
    buf = torch.empty(want_end, dtype=u8)
    views, end = ops._carve(buf, parts)
    assert end == want_end and list(views) == [p[0] for p in parts], label
    off = 0
    for name, shape, dtype in parts:
        v = views[name]
        assert v.dtype == dtype and tuple(v.shape) == tuple(shape) and v.is_contiguous(), (label, name)
        assert off % 256 == 0 and v.data_ptr() - buf.data_ptr() == off, (label, name, off)
        nbytes = v.numel() * v.element_size()
        assert nbytes == int(np.prod(shape)) * dtype.itemsize
        off += -(-nbytes // 256) * 256                 # the next part starts behind this one: in order and disjoint
    assert off == end


def test_carve_is_every_librarys_layout():
    n = 0
    for label, parts, nbytes in _layouts():
        _check_carve(parts, nbytes, label)
        n += 1
    assert n == 2 * len(WAVE_SHAPES) + len(PHASE_SHAPES) + len(BSS_SHAPES) + len(STOI_SHAPES)


def test_carve_sizes_elements_by_their_dtype():
    parts = [('a', (3,), c64), ('b', (257,), u8), ('c', (5, 7), f64), ('d', (1,), torch.int16), ('e', (2, 3), i32)]
    _check_carve(parts, 256 + 512 + 512 + 256 + 256)
    from danet_amd import ops
    buf = torch.arange(2048, dtype=torch.int64).to(u8)
    views, end = ops._carve(buf, parts)
    assert views['b'].numel() == 257 and torch.equal(views['b'], buf[256:513])         # an odd byte count
    assert views['a'].data_ptr() == buf.data_ptr() and views['d'].data_ptr() - buf.data_ptr() == 1280
    views['a'].fill_(1 + 2j)
    assert torch.equal(buf[:24].view(f32), torch.tensor([1., 2.] * 3)) and int(buf[24]) == 24
    assert ops._carve(None, []) == ({}, 0)


def test_phase_parts_are_the_carve_of_the_phase_layout():
    from danet_amd import ops
    shape = (3, 2, 9, 64, 16)
    buf = torch.empty(ops.phase_workspace_bytes(*shape) + 100, dtype=u8)      # at least as long: a tail is ignored
    got = ops.phase_parts(buf, *shape)
    want = ops._carve(buf, ops._phase_layout(*shape))[0]
    assert list(want) == ['A', 'mix', 'wav']
    for g, w in zip(got, want.values()):
        assert g.data_ptr() == w.data_ptr() and g.dtype == w.dtype and g.shape == w.shape


# ------------------------------------------------------------------------------------ tensor check
def test_chk_accepts_what_matches():
    from danet_amd import ops
    t = torch.zeros(2, 3, dtype=f64)
    assert ops._chk('t', t, f64, cuda=False) is t
    assert ops._chk('t', t, f64, (2, 3), numel=6, dim=2, dev=t.device, cuda=False) is t
    assert ops._chk('t', t, f64, [2, 3], cuda=False) is t and ops._chk('t', t, f64, t.shape, cuda=False) is t
    assert ops._chk('t', t.t(), f64, (3, 2), contiguous=False, cuda=False).shape == (3, 2)
    assert ops._chk('t', torch.zeros((), dtype=f32), f32, numel=1, cuda=False).dim() == 0
    assert ops._chk('t', None, f64, (2, 3), optional=True) is None
    fresh = ops._out('o', None, (4, 5), i32, 'cpu')
    assert fresh.dtype == i32 and tuple(fresh.shape) == (4, 5)


@pytest.mark.parametrize('kw,words', [
    (dict(dtype=f32), 'torch.float32'), (dict(shape=(3, 2)), 'shape (3, 2)'), (dict(shape=(2, 3, 1)), 'shape (2, 3, 1)'),
    (dict(numel=7), 'numel 7'), (dict(dim=3), 'dim 3'), (dict(dev=torch.device('cuda', 0)), 'on cuda:0'),
    (dict(cuda=True), 'on a GPU')])
def test_chk_refuses_and_names_the_argument(kw, words):
    from danet_amd import ops
    t = torch.zeros(2, 3, dtype=f64)
    kw = dict(dict(dtype=f64, cuda=False), **kw)
    with pytest.raises(AssertionError) as e:
        ops._chk('the_arg', t, kw.pop('dtype'), **kw)
    assert str(e.value).startswith('the_arg: want ') and words in str(e.value) and 'got torch.float64 (2, 3)' in str(e.value)


def test_chk_refuses_views_cpu_tensors_and_none():
    from danet_amd import ops
    t = torch.zeros(4, 6, dtype=f32)
    for bad in (t.t(), t[:, ::2], t[:, :3]):
        with pytest.raises(AssertionError, match='^x: want torch.float32, contiguous, got .* strides'):
            ops._chk('x', bad, f32, cuda=False)
        assert ops._chk('x', bad, f32, contiguous=False, cuda=False) is bad
    with pytest.raises(AssertionError, match='^x: want .*on a GPU, got .* on cpu'):
        ops._chk('x', t, f32)                                      # a device tensor is the default
    with pytest.raises(AssertionError, match='^out: want .*on a GPU'):
        ops._out('out', t, (4, 6), f32, t.device)
    with pytest.raises(AssertionError, match='^x: want .* got None'):
        ops._chk('x', None, f32, cuda=False)                       # None only where the call says optional
    with pytest.raises(AssertionError, match="^x: want .* got 'no tensor'"):
        ops._chk('x', 'no tensor', f32, cuda=False, optional=True)
    with pytest.raises(AssertionError, match='^perm_idx: want torch.int32'):
        ops._check_result(torch.zeros(3, 4, dtype=f64), torch.zeros(3, dtype=f64), torch.zeros(3, dtype=i32),
                          torch.zeros(4, dtype=f64), 4)
    assert ops._check_result(torch.zeros(3, 4, dtype=f64), torch.zeros(3, dtype=i32), torch.zeros(3, dtype=i32),
                             torch.zeros(2, 2, dtype=f64), 4) == 3


def test_result_allocates_the_finalize_tuple():
    from danet_amd import ops
    spec = lambda ts: [(t.dtype, tuple(t.shape)) for t in ts]
    assert spec(ops._result(5, 2, 'cpu')) == [(f64, (5, 2)), (i32, (5,)), (f64, (2,))]
    assert spec(ops._result(5, 4, 'cpu', flags=True)) == [(f64, (5, 4)), (i32, (5,)), (i32, (5,)), (f64, (4,))]
    assert spec(ops._result(1, 4, 'cpu', flags=True, count=True)) == [(f64, (1, 4)), (i32, (1,)), (i32, (1,)), (f64, (4,)),
                                                                      (i32, (1,))]


# ------------------------------------------------------------------------------------ group function
def _brute(B, limit, bytes_of):
    fit = [g for g in range(1, B + 1) if bytes_of(g) <= limit]
    return max(fit) if fit else 1


def test_group_is_the_largest_that_fits_and_at_least_one():
    from danet_amd import ops
    steps = lambda g: 1000 * g + (5000 if g % 7 == 0 else 0) + 3 * g * g        # not linear, at least g * steps(1)
    for B in (1, 2, 6, 7, 8, 50, 200):
        for limit in (1, 999, 1003, 10000, 61000, 62000, 10 ** 9):
            assert ops._group(B, limit, steps) == _brute(B, limit, steps), (B, limit)
    assert ops._group(9, 10, lambda g: 11 * g) == 1              # one utterance is over the limit: still one
    assert ops._group(9, 10 ** 6, lambda g: 11 * g) == 9         # never more than B
    # the search starts at limit // bytes_of(1), as bss_group and stoi_group always did: where g utterances need less
    # than g times the bytes of one, it stops short of the largest that fits
    fixed_cost = lambda g: 100 + 10 * g
    assert _brute(40, 300, fixed_cost) == 20 and ops._group(40, 300, fixed_cost) == 2


def test_group_is_bss_group_and_stoi_group():
    from danet_amd import ops
    for B, C, L in ((32, 4, 512), (32, 2, 512), (4, 2, 8), (1, 4, 512)):
        want = ops._group(B, ops.BSS_SCRATCH_BYTES, lambda g: ops.bss_workspace_bytes(g, C, L))
        assert ops.bss_group(B, C, L) == want == _brute(B, ops.BSS_SCRATCH_BYTES, lambda g: ops.bss_workspace_bytes(g, C, L))
    assert [ops.bss_group(32, 4, 512), ops.bss_group(32, 2, 512), ops.bss_group(4, 2, 8), ops.bss_group(1, 4, 512)] \
        == [6, 21, 4, 1]
    for B, C, Ls, U, D in ((32, 2, 8128, 5, 4), (1, 4, 100, 5, 4)):
        want = ops._group(B, ops.STOI_SCRATCH_BYTES, lambda g: ops.stoi_workspace_bytes(g, C, Ls, U, D))
        assert ops.stoi_group(B, C, Ls, U, D) == want == B
