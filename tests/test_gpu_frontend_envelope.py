'''
frontend_kernel and reattach_kernel (csrc/pointwise.hip) through ops.frontend / ops.reattach_phase:
C = 1 .. 4 sources, a second trip of the grid-stride loop (the grid is capped at 2048 x 256
threads), inputs on which hypotf / atan2f / log1pf have something to get wrong, per-ELEMENT bars,
and every permutation of nth_permutation.

Reference: oracle.danet_oracle.frontend in float64.  The mixture itself must be bitwise the float32
channel sum (accumulated left to right from +0, as any accumulator is); every other reference is
computed FROM that float32 mixture upcast to float64, so the cancellation of the channel sum does
not enter the bars.  Bars, per element: 16 float32 ulp = 2^-20 -- relative for src_pwr, mix_pwr and
mix_log, 2^-20 * pi absolute for phase, 2^-20 absolute for the phasor against cos / sin of the
float64 phase.  Each output is at most three float32 library calls deep.  ops.reattach_phase is
one float32 multiply per component: bitwise.
'''
import itertools

import numpy as np
import pytest
import torch

from oracle import danet_oracle as O

from gpu_helpers import cu
from prep_ref import bits

pytestmark = pytest.mark.gpu

ULP16 = 2.0 ** -20


def _mix32(src):
    '''float32 channel sum, left to right from +0 (main.py:233-234), re and im apart'''
    re = np.zeros(src.shape[:1] + src.shape[2:], np.float32)
    im = np.zeros_like(re)
    for c in range(src.shape[1]):
        re = re + src[:, c].real
        im = im + src[:, c].imag
        assert re.dtype == im.dtype == np.float32
    mix = np.empty(re.shape, np.complex64)
    mix.real, mix.imag = re, im
    return mix


def _source(B, C, T, F, seed, special=False):
    rng = np.random.RandomState(seed)
    src = ((rng.randn(B, C, T, F) + 1j * rng.randn(B, C, T, F)) * 50).astype(np.complex64)
    marks = {}
    if special:
        assert (B, T, F) == (3, 7, 33)
        src[0, :, 0, :4] = 0                                       # all-zero bins
        marks['zero'] = (0, 0, slice(0, 4))
        # the negative real axis: every channel on it, im = +0 / im = -0 / im just below 0
        src[0, :, 1, 0:3] = np.complex64(complex(-3.0, 0.0))
        src[0, :, 1, 3:6] = np.complex64(complex(-3.0, -0.0))
        src[0, :, 1, 6:9] = np.complex64(complex(-3.0, -1e-30))
        assert np.all(np.signbit(src[0, :, 1, 3:6].imag)) and not np.any(np.signbit(src[0, :, 1, 0:3].imag))
        marks['neg_pos0'], marks['neg_neg0'], marks['neg_below'] = (0, 1, slice(0, 3)), (0, 1, slice(3, 6)), (0, 1, slice(6, 9))
        # magnitudes whose squares overflow / flush to zero in float32
        u = np.exp(1j * rng.uniform(-np.pi, np.pi, (C, 6))) * rng.uniform(1.0, 2.0, (C, 6))
        src[1, :, 2, 0:6] = (u * 1e30).astype(np.complex64)
        src[1, :, 3, 0:6] = (u * 1e-30).astype(np.complex64)
        marks['big'], marks['small'] = (1, 2, slice(0, 6)), (1, 3, slice(0, 6))
        if C >= 2:                                                 # channels that cancel exactly
            src[2, 1:, 4, 0:5] = 0
            src[2, 1, 4, 0:5] = -src[2, 0, 4, 0:5]
            marks['cancel'] = (2, 4, slice(0, 5))
    return src, marks


def _reference(src):
    mix = _mix32(src)
    ref = O.frontend(mix[:, None].astype(np.complex128))          # one "channel": the float32 mixture
    ref['src_pwr'] = np.abs(src.astype(np.complex128))
    ref['mix32'] = mix
    return ref


def _check(fe, src, what):
    '''-> worst error of every output in float32 ulp (2^-24 of the value; of pi for phase; of 1 for the phasor)'''
    ref = _reference(src)
    worst = {}
    assert np.array_equal(bits(fe['mix'].cpu().numpy()), bits(ref['mix32'])), what
    for k in ('src_pwr', 'mix_pwr', 'mix_log'):
        got = fe[k].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ref[k].shape, (what, k)
        err = np.abs(got.astype(np.float64) - ref[k])
        worst[k] = float((err / np.where(ref[k] != 0, ref[k], 1.0)).max() / 2.0 ** -24)
        bad = err > ULP16 * np.abs(ref[k])                        # a zero reference must be met exactly
        assert not bad.any(), (what, k, worst[k], got[bad][:4], ref[k][bad][:4])
    ph = fe['phase'].cpu().numpy().astype(np.float64)
    err = np.abs(ph - ref['phase'])
    worst['phase'] = float(err.max() / (2.0 ** -24 * np.pi))
    assert err.max() <= ULP16 * np.pi, (what, 'phase', worst['phase'])
    pr = fe['phasor'].cpu().numpy().astype(np.float64)
    assert pr.shape == ref['phase'].shape + (2,)
    err = np.maximum(np.abs(pr[..., 0] - np.cos(ref['phase'])), np.abs(pr[..., 1] - np.sin(ref['phase'])))
    worst['phasor'] = float(err.max() / 2.0 ** -24)
    assert err.max() <= ULP16, (what, 'phasor', worst['phasor'])
    return worst


def _frontend(src, **kw):
    from danet_amd import ops
    return ops.frontend(torch.as_tensor(src).cuda(), **kw)


# -------------------------------------------------------------------------------- frontend
@pytest.mark.parametrize('C', [1, 2, 3, 4])
@pytest.mark.parametrize('B,T,F', [(1, 1, 1), (3, 7, 33), (2, 5, 129)])
def test_frontend_per_element(B, T, F, C):
    src, marks = _source(B, C, T, F, seed=B * 100 + C, special=(B, T, F) == (3, 7, 33))
    fe = _frontend(src, want_phase=True, want_mix=True)
    worst = _check(fe, src, (B, C, T, F))
    print('ENVELOPE frontend B=%d C=%d T=%d F=%d worst ulp: %s' % (
        B, C, T, F, ' '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    if not marks:
        return
    out = {k: v.cpu().numpy() for k, v in fe.items()}
    at = lambda k, m: out[k][marks[m][0], marks[m][1], marks[m][2]]
    for m in ('zero', 'cancel') if C >= 2 else ('zero',):
        assert not at('phase', m).any() and not at('mix_log', m).any() and not at('mix_pwr', m).any(), m
        assert np.all(at('phasor', m)[..., 0] == 1) and not at('phasor', m)[..., 1].any(), m
    b, t, f = marks['cancel'] if C >= 2 else marks['zero']
    assert C < 2 or np.all(out['src_pwr'][b, 0, t, f] > 0)           # cancelled, not absent
    # phase = +-pi by the sign of the mixture's imaginary part; a sum that starts at +0 turns -0 into +0
    assert not np.any(np.signbit(at('mix', 'neg_neg0').imag))
    assert np.all(np.signbit(at('mix', 'neg_below').imag))
    for m, sign in (('neg_pos0', 1), ('neg_neg0', 1), ('neg_below', -1)):
        assert np.all(np.abs(at('phase', m).astype(np.float64) - sign * np.pi) <= ULP16 * np.pi), (m, at('phase', m))
        assert np.all(np.abs(at('phasor', m)[..., 0] + 1) <= ULP16), m
    for m in ('neg_pos0', 'neg_neg0'):
        assert np.all(at('mix_pwr', m) == np.float32(3.0 * C)), m      # hypot(x, +-0) = |x|
    # hypotf: no overflow at 1e30, no flush at 1e-30, where sqrt(re^2 + im^2) in float32 gives inf / 0
    for m, lo, hi in (('big', 1e27, 1e33), ('small', 1e-33, 1e-27)):
        v = at('mix_pwr', m)
        assert np.isfinite(v).all() and np.all((v > lo) & (v < hi)), (m, v)
        s = out['src_pwr'][marks[m][0], :, marks[m][1], marks[m][2]]
        assert np.isfinite(s).all() and np.all((s > lo) & (s < hi)), (m, s)
        with np.errstate(over='ignore', under='ignore'):
            naive = np.sqrt(at('mix', m).real ** 2 + at('mix', m).imag ** 2)
        assert naive.dtype == np.float32 and (np.isinf(naive).all() if m == 'big' else not naive.any())


def test_frontend_grid_stride_second_trip():
    '''B * T * F = 525 009 > 2048 * 256 = 524 288: the grid-stride loop of frontend_kernel goes round again'''
    B, C, T, F = 3, 2, 1, 175003
    assert B * T * F == 525009 > 2048 * 256
    src, _ = _source(B, C, T, F, seed=9)
    worst = _check(_frontend(src, want_phase=True, want_mix=True), src, 'grid stride')
    print('ENVELOPE frontend grid-stride worst ulp: %s' % ' '.join('%s %.2f' % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize('C', [1, 3])
def test_frontend_optional_outputs(C):
    src, _ = _source(3, C, 7, 33, seed=C, special=True)
    full = _frontend(src, want_phase=True, want_mix=True)
    for kw in (dict(), dict(want_phase=True), dict(want_mix=True)):
        part = _frontend(src, **kw)
        assert set(part) == {'src_pwr', 'mix_pwr', 'mix_log', 'phasor'} | {k[5:] for k in kw}
        for k in part:
            a, b = part[k], full[k]
            assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), (kw, k)


# ---------------------------------------------------------------------------- reattach_phase
def _reattach_want(pw, phasor, perm_idx):
    '''float32(ph) * float32(pw) per component after the permutation gather (main.py:293-306, :282-284)'''
    C = pw.shape[1]
    if perm_idx is not None:
        perms = np.asarray(list(itertools.permutations(range(C))), dtype=np.int64)
        pw = O.perm_gather(pw, perms, perm_idx)
    re = phasor[:, None, ..., 0] * pw
    im = phasor[:, None, ..., 1] * pw
    assert re.dtype == im.dtype == np.float32
    return re, im


def _reattach_check(pw, phasor, perm_idx, what):
    from danet_amd import ops
    idx = None if perm_idx is None else torch.as_tensor(np.asarray(perm_idx, np.int32)).cuda()
    got = ops.reattach_phase(cu(pw), cu(phasor), idx).cpu().numpy()
    assert got.dtype == np.complex64 and got.shape == pw.shape, what
    re, im = _reattach_want(pw, phasor, perm_idx)
    assert np.array_equal(bits(np.ascontiguousarray(got.real)), bits(re)), what
    assert np.array_equal(bits(np.ascontiguousarray(got.imag)), bits(im)), what


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_reattach_every_permutation(C):
    '''B = C! utterances, one per permutation in itertools.permutations order, then shuffled, then none'''
    B, T, F = len(list(itertools.permutations(range(C)))), 3, 17
    rng = np.random.RandomState(C)
    pw = (rng.rand(B, C, T, F) * 40).astype(np.float32)
    phasor = rng.randn(B, T, F, 2).astype(np.float32)
    _reattach_check(pw, phasor, np.arange(B), (C, 'arange'))
    _reattach_check(pw, phasor, rng.permutation(B), (C, 'shuffled'))
    _reattach_check(pw, phasor, None, (C, 'none'))
    if C > 1:                                                      # the check can tell permutations apart
        a = _reattach_want(pw, phasor, np.arange(B))[0]
        assert not np.array_equal(a[1:], _reattach_want(pw, phasor, None)[0][1:])


def test_reattach_grid_stride_second_trip():
    '''B * C * T * F past 2048 * 256 at C = 2: 524 289 is odd, so 524 290 -- two elements on the second trip'''
    B, C, T, F = 5, 2, 1, 52429
    assert B * C * T * F == 2048 * 256 + 2
    rng = np.random.RandomState(52429)
    pw = (rng.rand(B, C, T, F) * 40).astype(np.float32)
    phasor = rng.randn(B, T, F, 2).astype(np.float32)
    _reattach_check(pw, phasor, np.array([1, 0, 1, 1, 0]), 'grid stride')
    _reattach_check(pw, phasor, None, 'grid stride, no permutation')


def test_reattach_rejects_five_sources():
    from danet_amd import ops, _lib
    pw = torch.rand(2, 5, 3, 17, device='cuda')
    phasor = torch.randn(2, 3, 17, 2, device='cuda')
    with pytest.raises(_lib.DanetHipError):
        ops.reattach_phase(pw, phasor, torch.zeros(2, dtype=torch.int32, device='cuda'))
    with pytest.raises(_lib.DanetHipError):
        ops.reattach_phase(pw, phasor)
    torch.cuda.synchronize()
    rng = np.random.RandomState(5)
    _reattach_check((rng.rand(2, 2, 3, 17) * 40).astype(np.float32), rng.randn(2, 3, 17, 2).astype(np.float32),
                    np.array([1, 0]), 'after a rejection')
