'''
danet_stft and danet_istft (csrc/stft.hip) over their whole envelope, through ops.stft / ops.istft,
against the references and case tables of tests/stft_ref.py (which tests/test_stft_cpu.py checks on
the host): every FFT size the entry points accept (64 threads on 32 butterflies at N = 64, more
than one butterfly per thread from N = 1024, the 48 KiB of dynamic LDS at the largest size),
strides that divide N, do not, S = N and S = 1, the five signal lengths around the frame
boundaries, and a window without any symmetry next to the project's sqrt-Hann.

Bars.  STFT: per FRAME max|X_t - ref_t| / max|ref_t| < 1e-5 (the BAR of tests/test_gpu_prep.py, per
frame instead of per tensor; a float32 scipy pipeline is at 2.5e-7, test_stft_cpu.py); frames whose
reference is identically zero are +-0 bitwise.  iSTFT: the float64 kernel against the float64
restatement of utils.istft with the reference's FLOAT32 window squares (app/utils.py:72), error of
the overlap-added accumulator relative to its maximum (stft_ref.weighted_error) < 1e-12 -- about
1000 x the rounding of a float64 radix-2 transform (log2 N * 2^-53 ~ 1.2e-15 times the <= N/S
overlap-added terms), four orders below what float64 squares would do (1.6e-8 .. 5.1e-8).
'''
import numpy as np
import pytest
import torch

import stft_ref as SR
from prep_ref import bits

pytestmark = pytest.mark.gpu

BAR = 1e-5
ISTFT_BAR = 1e-12
STFT_CASES = [(N, S, w) for N, S in SR.STFT_ENVELOPE for w in SR.WINDOWS]
ISTFT_CASES = [(N, S, w) for N, S in SR.ISTFT_ENVELOPE for w in SR.WINDOWS]


def _ids(cases):
    return ['N%d-S%d-%s' % c for c in cases]


def _errors():
    from danet_amd import _lib
    return (ValueError, _lib.DanetHipError)


def cu(a):
    '''a COPY on the device: the arrays stft_ref shares between tests are read-only'''
    return torch.from_numpy(np.array(a)).cuda()


def _stft(x, w, N, S):
    from danet_amd import ops
    return ops.stft(x, w, N, S).cpu().numpy()


def _check_frames(X, ref, what):
    assert X.shape == ref.shape and X.dtype == np.complex64, (what, X.shape, ref.shape)
    err, zero = SR.frame_errors(X, ref)
    assert not np.any(bits(X[zero]) & 0x7fffffff), what          # +-0, bitwise
    assert err.max() < BAR, (what, float(err.max()), int(err.argmax()))
    return float(err.max())


# ------------------------------------------------------------------------------------ STFT
@pytest.mark.parametrize('N,S,wname', STFT_CASES, ids=_ids(STFT_CASES))
def test_stft_parity_per_frame(N, S, wname):
    w = cu(SR.window(wname, N))
    worst = 0.0
    for Ls in SR.lengths(N, S):
        x, ref = SR.stft_case(wname, N, S, Ls)
        worst = max(worst, _check_frames(_stft(cu(x[0]), w, N, S), ref[0], (N, S, wname, Ls)))
    print('ENVELOPE stft N=%d S=%d %s worst per-frame error %.3g' % (N, S, wname, worst))


@pytest.mark.parametrize('N,S,wname', STFT_CASES, ids=_ids(STFT_CASES))
def test_stft_reads_nothing_outside_the_signal(N, S, wname):
    '''the signal is a slice (storage_offset != 0) of a buffer that is NaN on both sides, alone and as three
    rows: finite, and the bits of the run on a buffer of its own'''
    w = cu(SR.window(wname, N))
    for Ls in SR.lengths(N, S):
        x = cu(SR.signal(N, S, Ls, 3))
        pad = 2 * N + 5
        one = torch.full((Ls + 2 * pad,), float('nan'), device='cuda')
        one[pad:pad + Ls] = x[0]
        view = one[pad:pad + Ls]
        assert view.storage_offset() == pad and view.is_contiguous()
        got = _stft(view, w, N, S)
        assert np.isfinite(got.view(np.float32)).all(), (N, S, Ls)
        assert np.array_equal(bits(got), bits(_stft(x[0].clone(), w, N, S))), (N, S, Ls)
        flat = torch.full((3 * Ls + 2 * pad,), float('nan'), device='cuda')
        flat[pad:pad + 3 * Ls] = x.reshape(-1)
        rows = flat[pad:pad + 3 * Ls].view(3, Ls)
        assert rows.storage_offset() == pad and rows.is_contiguous()
        got = _stft(rows, w, N, S)
        assert np.isfinite(got.view(np.float32)).all(), (N, S, Ls)
        assert np.array_equal(bits(got), bits(_stft(x.clone(), w, N, S))), (N, S, Ls)


@pytest.mark.parametrize('N,S,wname', STFT_CASES, ids=_ids(STFT_CASES))
def test_stft_batch_consistency(N, S, wname):
    '''three signals in one call = three calls, bit for bit, and within the bar of the reference; a second run
    returns the same bits'''
    w = cu(SR.window(wname, N))
    for Ls in SR.lengths(N, S):
        x, ref = SR.stft_case(wname, N, S, Ls, 3)
        xg = cu(x)
        got = _stft(xg, w, N, S)
        _check_frames(got, ref, (N, S, wname, Ls))
        for r in range(3):
            assert np.array_equal(bits(got[r]), bits(_stft(xg[r], w, N, S))), (N, S, Ls, r)
        assert np.array_equal(bits(got), bits(_stft(xg, w, N, S))), (N, S, Ls)


@pytest.mark.parametrize('wname', list(SR.WINDOWS))
def test_stft_widest_batch(wname):
    '''n_sig = 65535 = the limit of grid.y, at N = S = Ls = 64 (T = 2, a 35 MB output): every row against the
    reference; one more signal is refused'''
    from danet_amd import ops
    N = S = Ls = 64
    w = SR.window(wname, N)
    x = (np.random.RandomState(65535).randn(65536, Ls) * 500).astype(np.float32)
    xg = cu(x)
    got = _stft(xg[:65535], cu(w), N, S)
    assert got.shape == (65535, 2, 33)
    worst = _check_frames(got, SR.stft_ref(x[:65535], w, N, S), 'n_sig 65535')
    print('ENVELOPE stft n_sig=65535 %s worst per-frame error %.3g' % (wname, worst))
    with pytest.raises(_errors()):
        ops.stft(xg, cu(w), N, S)
    torch.cuda.synchronize()


@pytest.mark.parametrize('N,S,Ls', [(32, 8, 200), (96, 24, 400), (8192, 2048, 20000), (256, 0, 1000), (256, 257, 1000),
                                    (256, 64, 255), (4096, 1024, 4095)])
def test_stft_rejections(N, S, Ls):
    '''outside the envelope the call raises and launches nothing; the next valid call is unharmed'''
    from danet_amd import ops
    x = torch.randn(Ls, device='cuda')
    w = torch.ones(N, device='cuda')
    with pytest.raises(_errors()):
        ops.stft(x, w, N, S)
    torch.cuda.synchronize()
    xv, ref = SR.stft_case('asym', 256, 97, 256 + 2 * 97 + 3)
    _check_frames(_stft(cu(xv[0]), cu(SR.window('asym', 256)), 256, 97), ref[0], 'after a rejection')


# ----------------------------------------------------------------------------------- iSTFT
def _istft(X, S, w):
    from danet_amd import ops
    y = ops.istft(X, S, w)
    assert y.dtype == torch.float64
    return y.cpu().numpy()


@pytest.mark.parametrize('N,S,wname', ISTFT_CASES, ids=_ids(ISTFT_CASES))
def test_istft_parity(N, S, wname):
    '''a spectrum that is no STFT of a real signal (DC and Nyquist carry imaginary parts, which irfft ignores),
    used = 5 frames: the weighted error of stft_ref.weighted_error against utils.istft restated in float64 with
    its float32 window squares.

    Measured on an MI355X over the table: 1.6e-16 .. 4.4e-16.  While istft_ola_kernel squared (double)window[m]
    instead of the float32 window: 1.6e-8 .. 3.7e-8.'''
    T = SR.parity_frames(N, S)
    X, ref, wsum = SR.istft_case(wname, N, S, T)
    y = _istft(cu(X[0]), S, cu(SR.window(wname, N)))
    assert y.shape == ref[0].shape == (T * S,)
    assert np.isfinite(y).all()
    err = SR.weighted_error(y, ref[0], wsum)
    print('ENVELOPE istft N=%d S=%d %s T=%d weighted error %.3g' % (N, S, wname, T, err))
    assert err < ISTFT_BAR, (N, S, wname, err)


@pytest.mark.parametrize('N,S,wname', ISTFT_CASES, ids=_ids(ISTFT_CASES))
def test_istft_frame_truncation(N, S, wname):
    '''T with T*S - N just below 0, 0 and just above (used = 0, 0, 1) and used = 5: nothing at all when no frame
    fits, exact zeros past the last used frame, and frames >= used -- which utils.istft never reads -- filled
    with NaN change no bit'''
    w = cu(SR.window(wname, N))
    for T in SR.istft_frames(N, S):
        X, ref, wsum = SR.istft_case(wname, N, S, T)
        used = SR.istft_used(T, N, S)
        assert used < T
        y = _istft(cu(X[0]), S, w)
        assert y.shape == (T * S,)
        if used == 0:
            assert not y.any(), (N, S, T)
        else:
            assert SR.weighted_error(y, ref[0], wsum) < ISTFT_BAR, (N, S, T)
            end = (used - 1) * S + N
            assert end < T * S and not y[end:].any(), (N, S, T)
        Xn = X[0].copy()
        Xn[used:] = complex(float('nan'), float('nan'))
        yn = _istft(cu(Xn), S, w)
        assert np.isfinite(yn).all(), (N, S, T)
        assert np.array_equal(yn.view(np.uint64), y.view(np.uint64)), (N, S, T)


@pytest.mark.parametrize('N', [64, 256])
def test_istft_zero_pattern_of_wsum(N):
    '''S = N: one frame per sample, so wsum is one window square.  A window entry of 0 and one of 1e-25f both
    square to 0 in float32 (app/utils.py:72 squares the float32 window), so utils.istft leaves those samples
    UNDIVIDED (:73-74); in float64 the second squares to 1e-50 and would be divided by.'''
    S, T = N, 6
    w = SR.window('asym', N).copy()
    i0, i1 = 5, N - 11
    w[i0], w[i1] = 0.0, np.float32(1e-25)
    X = SR.spectrum(N, T)[0]
    ref, wsum = SR.istft_ref(X, S, w)
    used = SR.istft_used(T, N, S)
    assert used == 5
    at0, at1 = i0 + S * np.arange(used), i1 + S * np.arange(used)
    assert not wsum[at0].any() and not wsum[at1].any()
    assert np.count_nonzero(wsum == 0) == 2 * used + S
    assert not ref[at0].any() and np.all(ref[at1] != 0) and np.abs(ref[at1]).max() < 1e-22    # the accumulators
    y = _istft(cu(X), S, cu(w))
    assert not y[at0].any(), y[at0]
    acc_max = (np.abs(ref) * np.where(wsum != 0, wsum, 1.0)).max()               # largest accumulator: irfft * w
    assert np.all(np.abs(y[at1] - ref[at1]) <= ISTFT_BAR * acc_max * 1e-25), (y[at1], ref[at1])
    assert SR.weighted_error(y, ref, wsum) < ISTFT_BAR


@pytest.mark.parametrize('N,S,wname', ISTFT_CASES, ids=_ids(ISTFT_CASES))
def test_istft_batch_consistency(N, S, wname):
    w = cu(SR.window(wname, N))
    T = SR.parity_frames(N, S)
    X, ref, wsum = SR.istft_case(wname, N, S, T, 3)
    Xg = cu(X)
    y = _istft(Xg, S, w)
    assert y.shape == (3, T * S)
    for r in range(3):
        assert SR.weighted_error(y[r], ref[r], wsum) < ISTFT_BAR, (N, S, r)
        assert np.array_equal(_istft(Xg[r], S, w).view(np.uint64), y[r].view(np.uint64)), (N, S, r)
    assert np.array_equal(_istft(Xg, S, w).view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize('N,S', [(4096, 1024), (256, 257), (32, 8), (96, 24)])
def test_istft_rejections(N, S):
    from danet_amd import ops
    X = torch.zeros(12, N // 2 + 1, dtype=torch.complex64, device='cuda')
    with pytest.raises(_errors()):
        ops.istft(X, S, torch.ones(N, device='cuda'))
    torch.cuda.synchronize()
    Xv, ref, wsum = SR.istft_case('asym', 128, 49, SR.parity_frames(128, 49))
    y = _istft(cu(Xv[0]), 49, cu(SR.window('asym', 128)))
    assert SR.weighted_error(y, ref[0], wsum) < ISTFT_BAR
