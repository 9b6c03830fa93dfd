'''
References and case tables of the STFT / iSTFT envelope tests (tests/test_stft_cpu.py,
tests/test_gpu_stft_envelope.py): danet_stft and danet_istft (csrc/stft.hip) over every FFT size
the entry points accept, strides that do and do not divide N, a window that is NOT symmetric, and
the float32 window squares of the reference's utils.istft (app/utils.py:72).

stft_ref is scipy.signal.stft on a float64 copy (what the reference calls, app/utils.py:117-122);
istft_ref restates utils.istft (app/utils.py:53-75) line by line with the spectrum upcast to
complex128 and the window KEPT float32, so `window ** 2.` rounds to float32 as it does there.
Signals, spectra and references are made once per case and shared (lru_cache); callers must not
write to them.
'''
import functools

import numpy as np
import scipy.signal

from oracle import danet_oracle as O

STFT_SIZES = (64, 128, 256, 512, 1024, 2048, 4096)       # danet_stft: 2^6 .. 2^12
ISTFT_SIZES = STFT_SIZES[:-1]                             # danet_istft: 2^6 .. 2^11


def strides(N):
    '''S = N/4 and N/2 divide N; S = N: no overlap; N-1 and 3N/8+1 do not divide N; S = 1 at the
    smallest size only (T ~ Ls frames)'''
    s = [N // 4, N // 2, N, N - 1, 3 * N // 8 + 1]
    if N == 64:
        s.append(1)
    return s


STFT_ENVELOPE = [(N, S) for N in STFT_SIZES for S in strides(N)]
ISTFT_ENVELOPE = [(N, S) for N in ISTFT_SIZES for S in strides(N)]


def lengths(N, S):
    '''signal lengths of one (N, S): the shortest legal one, one more, and both sides of the next
    two frame boundaries (duplicates at S = 1 dropped, order kept)'''
    return list(dict.fromkeys([N, N + 1, N + S - 1, N + S, N + 2 * S + 3]))


# --------------------------------------------------------------------------------- windows
def sqrt_hann(N):
    '''the project's FFT_WND (default.json:7): symmetric, endpoints exactly 0'''
    return O.fft_window(N)


def asym_window(N):
    '''no symmetry at all: w[i] != w[N-1-i] for every i, all entries in [0.1, 1)'''
    w = np.random.RandomState(N).uniform(0.1, 1.0, N).astype(np.float32)
    assert np.all(w[:N // 2] != w[::-1][:N // 2]), N
    return w


WINDOWS = {'sqrt_hann': sqrt_hann, 'asym': asym_window}


@functools.lru_cache(maxsize=None)
def window(name, N):
    w = WINDOWS[name](N)
    assert w.dtype == np.float32 and w.shape == (N,)
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------------------------ STFT
def stft_ref(x, window, N, S):
    '''the reference's call (app/utils.py:117-122) on a float64 copy of x[..., Ls]
    -> complex128 [..., T, F]'''
    Z = scipy.signal.stft(np.asarray(x, dtype=np.float64), window=np.asarray(window), nperseg=N,
                          noverlap=N - S)[2]
    assert Z.dtype == np.complex128
    return np.swapaxes(Z, -1, -2)


def num_frames(Ls, N, S):
    '''frames scipy makes of Ls samples (boundary='zeros': N//2 zeros each side; padded=True: a
    zero tail up to the next whole frame)'''
    ext = Ls + 2 * (N // 2)
    nadd = (-(ext - N) % S) % N
    return (ext + nadd - N) // S + 1


@functools.lru_cache(maxsize=None)
def signal(N, S, Ls, rows=1):
    '''float32 randn * 500 (int16-scale audio), [rows, Ls]'''
    x = (np.random.RandomState((N * 8191 + S * 131 + Ls) % (2 ** 31)).randn(rows, Ls) * 500).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def stft_case(wname, N, S, Ls, rows=1):
    '''(x float32 [rows, Ls], reference complex128 [rows, T, F]) of one table entry'''
    x = signal(N, S, Ls, rows)
    ref = stft_ref(x, window(wname, N), N, S)
    ref.setflags(write=False)
    return x, ref


def frame_errors(X, ref):
    '''per frame max|X_t - ref_t| / max|ref_t| over the frames whose reference is not identically
    zero, and the mask of those that are -> (ratios [..., T] with 0 at the zero frames, zero mask)'''
    X = np.asarray(X).astype(np.complex128)
    top = np.abs(ref).max(axis=-1)
    zero = top == 0
    err = np.abs(X - ref).max(axis=-1)
    return np.where(zero, 0.0, err / np.where(zero, 1.0, top)), zero


# ----------------------------------------------------------------------------------- iSTFT
def istft_ref(X, S, window):
    '''utils.istft (app/utils.py:53-75) restated: X complex [T, F] upcast to complex128, float64
    accumulators, window float32 -> (y float64 [T*S], wsum float64 [T*S]); wsum is the
    overlap-added FLOAT32 squares of the window, y is left undivided where wsum == 0'''
    X = np.asarray(X).astype(np.complex128)
    window = np.asarray(window)
    N = (X.shape[1] - 1) * 2
    assert window.shape == (N,)
    sq = window ** 2.                                       # app/utils.py:72
    assert sq.dtype == window.dtype                         # float32 squares of a float32 window
    x = np.zeros(X.shape[0] * S)
    wsum = np.zeros(X.shape[0] * S)
    for n, i in enumerate(range(0, len(x) - N, S)):
        x[i:i + N] += np.real(np.fft.irfft(X[n])) * window  # app/utils.py:71
        wsum[i:i + N] += sq
    pos = wsum != 0
    x[pos] /= wsum[pos]
    return x, wsum


def istft_used(T, N, S):
    '''leading frames app/utils.py:70 consumes'''
    return len(range(0, T * S - N, S))


def istft_frames(N, S):
    '''frame counts of one (N, S), by T*S - N: the largest below 0 (-1 where S divides N - 1),
    0 where S divides N, the smallest above 0 (1 where S divides N + 1) -- used = 0, 0, 1 -- and
    the T of used = 5, the parity case.  T >= 1, duplicates dropped.'''
    ts = [(N - 1) // S, N // S if N % S == 0 else 0, N // S + 1, N // S + 5]
    return list(dict.fromkeys(t for t in ts if t >= 1))


def parity_frames(N, S):
    return N // S + 5


@functools.lru_cache(maxsize=None)
def spectrum(N, T, rows=1):
    '''random complex64 [rows, T, F] that is NOT the STFT of anything real: the imaginary parts of
    DC and Nyquist are as large as every other'''
    F = N // 2 + 1
    rng = np.random.RandomState(N * 31 + T)
    X = ((rng.randn(rows, T, F) + 1j * rng.randn(rows, T, F)) * 10).astype(np.complex64)
    assert np.all(X[..., 0].imag != 0) and np.all(X[..., F - 1].imag != 0)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def istft_case(wname, N, S, T, rows=1):
    '''(X complex64 [rows, T, F], y float64 [rows, T*S], wsum float64 [T*S]) of one table entry'''
    X = spectrum(N, T, rows)
    w = window(wname, N)
    ys, wsum = zip(*[istft_ref(X[r], S, w) for r in range(rows)])
    y = np.stack(ys)
    y.setflags(write=False)
    return X, y, wsum[0]


def weighted_error(y, ref, wsum):
    '''max_i |y_i - ref_i| wsum_i / max_i |ref_i| wsum_i with wsum taken as 1 where it is 0: the
    error of the overlap-added accumulator.  A tiny wsum next to the signal's edges makes max|ref|
    several hundred times the interior's, and an error relative to THAT would hide the interior.'''
    w = np.where(wsum != 0, wsum, 1.0)
    den = (np.abs(ref) * w).max()
    num = (np.abs(np.asarray(y, np.float64) - ref) * w).max()
    return float(num / den) if den > 0 else float(num)
