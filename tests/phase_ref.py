'''
Restatement of the MISI phase refinement (include/danet_phase_hip.h, THE RULE) in numpy float64, written from the rule
and independently of csrc/phase/phase.hip.  The synthesis is tests/metric_ref.synth; the analysis is written out
directly (scipy.signal.stft refuses a signal shorter than its window, and T >= 2 allows Ls < N).  `dtype=np.float32`
runs every step in single precision in the order the rule gives: the noise floor of float32 arithmetic that the
tests report beside the kernel's error.
'''
import numpy as np
import scipy.fft

import metric_ref as MR

MAX_C = 4
# (N, S, T, C, window name): the cases on which every one of 12 iterations lowers the objective by > 1e-4 J_0
DESCENT_CASES = ((64, 16, 9, 2, 'sqrt_hann'), (64, 32, 5, 3, 'sqrt_hann'), (64, 8, 12, 4, 'sqrt_hann'),
                 (128, 32, 3, 2, 'sqrt_hann'), (64, 16, 2, 2, 'sqrt_hann'), (64, 16, 9, 2, 'hamming'),
                 (64, 32, 9, 3, 'hann'))


def window(name, N):
    '''float32 [N]; sqrt_hann is hparams' default FFT_WND'''
    import scipy.signal.windows as W
    w = {'sqrt_hann': lambda: np.sqrt(W.hann(N)), 'hann': lambda: W.hann(N), 'hamming': lambda: W.hamming(N)}[name]()
    return w.astype(np.float32)


def _ctype(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def analyse(z, w, S, T, dtype=np.float64):
    '''z [..., Ls] -> complex [..., T, F]: the UNSCALED windowed real FFT of frame t = samples [tS - N/2, tS + N/2),
    zero outside [0, Ls)'''
    z = np.asarray(z, dtype)
    w = np.asarray(w).astype(dtype)
    N = len(w)
    Ls = (T - 1) * S
    assert z.shape[-1] == Ls
    pad = np.zeros(z.shape[:-1] + (Ls + N,), dtype)
    pad[..., N // 2:N // 2 + Ls] = z
    frames = np.stack([pad[..., t * S:t * S + N] * w for t in range(T)], axis=-2)
    Z = (scipy.fft.rfft(frames, axis=-1) if dtype == np.float32 else np.fft.rfft(frames, axis=-1))
    assert Z.dtype == _ctype(dtype)
    return Z


def magnitudes(est0, dtype=np.float64):
    '''|est0| taken in float64 and rounded once to `dtype`: the rule's hypot form'''
    e = np.asarray(est0).astype(np.complex128)
    return np.hypot(e.real, e.imag).astype(dtype)


def mixture(mixrows, dtype=np.float64):
    '''[B, Cm, T, F] -> [B, T, F]: the rows summed in ascending order starting from row 0'''
    m = np.asarray(mixrows).astype(_ctype(dtype))
    acc = m[:, 0].copy()
    for c in range(1, m.shape[1]):
        acc = acc + m[:, c]
    return acc


def redistribute(x, y, dtype=np.float64):
    '''x [B, C, Ls], y [B, Ls] -> z [B, C, Ls] = x_c + (y - sum_c' x_c') / C, the sum ascending from x_0'''
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    C = x.shape[1]
    s = x[:, 0].copy()
    for c in range(1, C):
        s = s + x[:, c]
    return x + ((y - s) / dtype(C))[:, None]


def project(Z, A, X_old, dtype=np.float64):
    '''step 4: A Z / |Z| where |Z|^2 > 0 and finite (+0 there where A = 0), the old value elsewhere'''
    Z = np.asarray(Z).astype(_ctype(dtype))
    A = np.asarray(A, dtype)
    out = np.array(X_old).astype(_ctype(dtype))
    with np.errstate(over='ignore', invalid='ignore'):
        m2 = Z.real * Z.real + Z.imag * Z.imag
    ok = (m2 > 0) & np.isfinite(m2)
    r = np.sqrt(m2[ok])
    new = A[ok] * (Z.real[ok] / r) + 1j * (A[ok] * (Z.imag[ok] / r))
    new[A[ok] == 0] = 0.0
    out[ok] = new.astype(out.dtype)
    return out, ok


def analysis_of(X, y, w, S, dtype=np.float64):
    '''steps 1-3 of one iteration: X [B, C, T, F], y [B, Ls] -> Z [B, C, T, F]'''
    T = np.asarray(X).shape[-2]
    x = MR.synth(X, w, S, dtype)
    return analyse(redistribute(x, y, dtype), w, S, T, dtype)


def step(X, A, y, w, S, dtype=np.float64):
    '''one iteration -> (X_new, Z, the mask of the bins that took a new value)'''
    Z = analysis_of(X, y, w, S, dtype)
    X_new, ok = project(Z, A, X, dtype)
    return X_new, Z, ok


def start(est0, mixrows, w, S, dtype=np.float64):
    '''-> (A, mix, y, X^0)'''
    mix = mixture(mixrows, dtype)
    return magnitudes(est0, dtype), mix, MR.synth(mix, w, S, dtype), np.asarray(est0).astype(_ctype(dtype))


def refine(est0, mixrows, w, S, K, dtype=np.float64):
    '''-> X^K'''
    A, _, y, X = start(est0, mixrows, w, S, dtype)
    for _ in range(K):
        X = step(X, A, y, w, S, dtype)[0]
    return X


def objective(A, Z):
    '''J = sum_c || A_c - |Z_c| ||^2 in float64'''
    return float(((np.asarray(A, np.float64) - np.abs(np.asarray(Z).astype(np.complex128))) ** 2).sum())


def objective_of(X, A, y, w, S):
    '''J of the iterate X: its analysis taken in float64'''
    return objective(A, analysis_of(np.asarray(X).astype(np.complex128), y, w, S))


def make_sources(B, C, T, N, S, seed):
    '''C random waveforms per utterance (low-passed noise of different colours) -> float64 [B, C, (T - 1) * S + N]'''
    rng = np.random.RandomState(seed)
    L = (T - 1) * S + N
    x = rng.standard_normal((B, C, L))
    for c in range(C):
        k = 2 + 3 * c
        x[:, c] = np.apply_along_axis(lambda v: np.convolve(v, np.ones(k) / k, mode='same'), -1, x[:, c])
    return x * (1.0 + 0.5 * np.arange(C))[:, None]


def spectra_of(wavs, w, S, T):
    '''the consistent complex64 spectra [..., T, F] of waveforms [..., (T - 1) * S] at the scale of the reference's
    STFT (the unscaled analysis / sum(w)): what a dataset feeds the model'''
    return (analyse(wavs, w, S, T) / np.asarray(w, np.float64).sum()).astype(np.complex64)


def oracle_case(B, C, T, N, S, wname='sqrt_hann', seed=0):
    '''sources complex64 [B, C, T, F], and est0 = their magnitudes with the MIXTURE's phase -> (est0, src, w)'''
    w = window(wname, N)
    src = spectra_of(make_sources(B, C, T, N, S, seed)[..., :(T - 1) * S], w, S, T)
    mix = mixture(src, np.float32)
    ph = np.where(np.abs(mix) > 0, mix / np.maximum(np.abs(mix), 1e-30), 1.0)
    return (np.abs(src) * ph[:, None]).astype(np.complex64), src, w


def si_sdr_db(ref, est):
    '''plain SI-SDR of waveforms [..., L], no permutation search, mean over the leading axes, dB'''
    ref, est = np.asarray(ref, np.float64), np.asarray(est, np.float64)
    a = (ref * est).sum(-1, keepdims=True) / (ref * ref).sum(-1, keepdims=True)
    t = a * ref
    return float(np.mean(10 * np.log10((t * t).sum(-1) / ((est - t) ** 2).sum(-1))))
