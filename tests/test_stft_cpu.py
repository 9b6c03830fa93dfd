'''
CPU checks (no GPU) behind tests/test_gpu_stft_envelope.py: the host-side frame count and iSTFT
scratch size of csrc/stft.hip against scipy / the reference's range(), the coverage the case tables
of tests/stft_ref.py must keep, and the resolving power of the two bars -- a float32 FFT pipeline
sits well inside the STFT's per-frame 1e-5, and squaring the window in float64 instead of float32
(app/utils.py:72) moves the iSTFT reference by far more than the 1e-12 the kernel is held to.
'''
import numpy as np
import scipy.fft
import scipy.signal

from oracle import danet_oracle as O

import stft_ref as SR

BAR = 1e-5


def _lib_core():
    from danet_amd import _lib
    return _lib, _lib.load()


def _scipy_frames(Ls, N, S, w):
    return scipy.signal.stft(np.zeros(Ls), window=w, nperseg=N, noverlap=N - S)[2].shape[-1]


# ---------------------------------------------------------------------------- frame count
def _sweep_strides(N):
    '''every S in 1 .. N below 1024; from there a few hundred: every table stride, 1 .. 64, the last 33, the
    neighbours of N/2 and N/4 and a seeded draw'''
    if N < 1024:
        return list(range(1, N + 1))
    s = set(SR.strides(N)) | set(range(1, 65)) | set(range(N - 32, N + 1))
    s |= {N // 2 + d for d in (-1, 1)} | {N // 4 + d for d in (-1, 1)} | {N // 3, N // 3 + 1, 2 * N // 3}
    s |= set(int(v) for v in np.random.RandomState(N).randint(1, N + 1, size=200))
    return sorted(s)


def test_restated_frame_count_is_scipys():
    '''SR.num_frames, which the full sweep below compares with, IS the frame count of the real
    scipy.signal.stft output: every (S, Ls in N .. N+2S) at N = 64 and 128, and at every larger N the table
    strides, their neighbours and S = 1, 2, 3 at the lengths on both sides of each frame boundary (a scipy call for
    each of the sweep's two million triples would take minutes)'''
    calls = 0
    for N in SR.STFT_SIZES:
        w = np.ones(N, np.float32)
        if N <= 128:
            cases = [(S, Ls) for S in range(1, N + 1) for Ls in range(N, N + 2 * S + 1)]
        else:
            ss = set(SR.strides(N)) | {1, 2, 3, N // 4 + 1, N // 2 - 1, N - 2}
            cases = [(S, Ls) for S in sorted(ss)
                     for Ls in sorted({N, N + 1, N + S - 1, N + S, N + S + 1, N + 2 * S - 1, N + 2 * S, N + 2 * S + 3})
                     if S > 3 or N <= 256 or Ls <= N + 1]        # S <= 3 at a large N: thousands of frames a call
        for S, Ls in cases:
            assert SR.num_frames(Ls, N, S) == _scipy_frames(Ls, N, S, w), (N, S, Ls)
            calls += 1
    assert calls > 20000
    # the table lengths themselves, with the table windows (the count does not depend on the window)
    for N, S in SR.STFT_ENVELOPE:
        for Ls in SR.lengths(N, S):
            assert SR.stft_case('asym', N, S, Ls)[1].shape == (1, SR.num_frames(Ls, N, S), N // 2 + 1)
            assert SR.num_frames(Ls, N, S) == O.stft_frame_count(Ls, N, S)


def test_num_frames_sweep():
    '''danet_stft_num_frames over every N of the envelope, S in 1 .. N (thinned from N = 1024) and every
    Ls in N .. N+2S -- all residues of the tail padding (`nadd`) for strides that do not divide N'''
    _, L = _lib_core()
    f = L.danet_stft_num_frames
    n = 0
    for N in SR.STFT_SIZES:
        ss = _sweep_strides(N)
        assert set(SR.strides(N)) <= set(ss) and {N - 1, N} <= set(ss)
        assert N < 1024 or 200 < len(ss) < 500
        for S in ss:
            for Ls in range(N, N + 2 * S + 1):
                assert f(Ls, N, S) == SR.num_frames(Ls, N, S), (N, S, Ls)
            n += 2 * S + 1
    print('frame counts compared: %d' % n)
    for N in SR.STFT_SIZES:
        for S in SR.strides(N):
            assert f(N - 1, N, S) < 0 and f(0, N, S) < 0 and f(-3, N, S) < 0     # Ls < N: scipy raises
        assert f(4 * N, N, 0) < 0 and f(4 * N, N, N + 1) < 0 and f(4 * N, N, -1) < 0
    assert f(1000, 0, 1) < 0 and f(1000, 0, 0) < 0 and f(1000, -64, 16) < 0


def test_num_frames_rejections_are_err_arg():
    _, L = _lib_core()
    for Ls, N, S in [(63, 64, 16), (256, 256, 0), (256, 256, 257), (1000, 0, 16)]:
        assert L.danet_stft_num_frames(Ls, N, S) == -1, (Ls, N, S)             # DANET_ERR_ARG


# ------------------------------------------------------------------------- workspace size
def test_istft_workspace_bytes():
    '''danet_workspace_bytes(DANET_WS_ISTFT) = n_sig * max(used, 1) * N * 8 with used the reference's
    len(range(0, T*S - N, S)), incl. T*S - N in {-1, 0, 1}'''
    _lib, _ = _lib_core()
    seen = set()
    for N, S in SR.ISTFT_ENVELOPE:
        ts = set(SR.istft_frames(N, S)) | {1, 2, N // S + 2, N // S + 17}
        for T in sorted(ts):
            used = len(range(0, T * S - N, S))
            assert used == SR.istft_used(T, N, S) == O.istft_num_frames_used(T, N, S)
            for n_sig in (1, 3, 65535):
                assert _lib.ws_bytes(_lib.WS_ISTFT, n_sig, T, N, S) == n_sig * max(used, 1) * N * 8, (n_sig, T, N, S)
            if T * S - N in (-1, 0, 1):
                seen.add(T * S - N)
                assert used == (1 if T * S - N == 1 else 0)
    assert seen == {-1, 0, 1}


# ------------------------------------------------------------------------- table coverage
def test_tables_keep_their_coverage():
    assert {int(np.log2(N)) for N, _ in SR.STFT_ENVELOPE} == set(range(6, 13))
    assert {int(np.log2(N)) for N, _ in SR.ISTFT_ENVELOPE} == set(range(6, 12))
    for sizes, table in ((SR.STFT_SIZES, SR.STFT_ENVELOPE), (SR.ISTFT_SIZES, SR.ISTFT_ENVELOPE)):
        for N in sizes:
            ss = [S for n, S in table if n == N]
            assert N in ss and N - 1 in ss                      # no overlap; one sample of overlap
            assert sum(1 for S in ss if N % S) >= 2             # strides that do not divide N
            assert sum(1 for S in ss if N % S == 0 and S < N) >= 2
            assert all(1 <= S <= N for S in ss)
    assert (64, 1) in SR.STFT_ENVELOPE and (64, 1) in SR.ISTFT_ENVELOPE
    # N >= 1024: more butterflies than threads (256); N = 64: fewer (32 on 64 threads)
    assert 64 // 2 < 64 and 4096 // 2 > 256
    for N in SR.STFT_SIZES:
        a, h = SR.window('asym', N), SR.window('sqrt_hann', N)
        assert np.all(a[:N // 2] != a[::-1][:N // 2])
        assert np.array_equal(h, h[::-1])                       # why the second window exists
        assert a.min() >= 0.1 and h[0] == 0 and h[-1] == 0
    for N, S in SR.STFT_ENVELOPE:
        ls = SR.lengths(N, S)
        assert ls[0] == N and len(set(ls)) == len(ls) >= (3 if S == 1 else 5)
        assert len({SR.num_frames(Ls, N, S) for Ls in ls}) >= 2
    for N, S in SR.ISTFT_ENVELOPE:
        ts = SR.istft_frames(N, S)
        useds = [SR.istft_used(T, N, S) for T in ts]
        assert 0 in useds
        assert 1 in useds and max(useds) >= 5
        assert SR.istft_used(SR.parity_frames(N, S), N, S) >= 5
        if N % S == 0:
            assert any(T * S == N for T in ts)
        for T in ts:
            used = SR.istft_used(T, N, S)
            assert T - used >= 1                                # a frame the reference never reads
            for wname in SR.WINDOWS:
                wsum = SR.istft_case(wname, N, S, T)[2]
                assert np.any(wsum == 0)                        # a sample it never divides
                assert used == 0 or np.any(wsum != 0)
    assert any((T * S - N) == -1 for N, S in SR.ISTFT_ENVELOPE for T in SR.istft_frames(N, S))
    assert any((T * S - N) == 1 for N, S in SR.ISTFT_ENVELOPE for T in SR.istft_frames(N, S))


def test_references_agree_with_the_oracle():
    '''stft_ref (scipy) against oracle.danet_oracle.stft (explicit framing + numpy rfft) and istft_ref against
    oracle.danet_oracle.istft on a complex128 spectrum: two independent restatements each'''
    for N, S in [(64, 1), (64, 27), (256, 64), (512, 511), (1024, 385), (4096, 4096)]:
        for wname in SR.WINDOWS:
            Ls = SR.lengths(N, S)[-1]
            x, ref = SR.stft_case(wname, N, S, Ls)
            o = O.stft(x[0], SR.window(wname, N), N, S, out_dtype='complex128')
            assert o.shape == ref[0].shape
            assert np.abs(o - ref[0]).max() < 1e-12 * np.abs(ref).max()
    for N, S in [(64, 1), (64, 25), (256, 64), (2048, 2047)]:
        for wname in SR.WINDOWS:
            X, y, wsum = SR.istft_case(wname, N, S, SR.parity_frames(N, S))
            o = O.istft(X[0].astype(np.complex128), S, SR.window(wname, N))
            assert np.array_equal(o, y[0])


# ------------------------------------------------------------------- the bars can resolve
def test_float32_pipeline_is_inside_the_stft_bar():
    '''the reference alone: float32 frames through scipy.fft.rfft (which stays float32) times float32(1 / sum(w))
    is within 1e-5 PER FRAME of stft_ref over the whole table, so the bar leaves a correct float32 kernel room;
    frames whose reference is identically zero are exactly zero'''
    worst = 0.0
    for N, S in SR.STFT_ENVELOPE:
        for wname in SR.WINDOWS:
            w = SR.window(wname, N)
            scale = np.float32(1.0 / w.astype(np.float64).sum())
            for Ls in SR.lengths(N, S):
                x, ref = SR.stft_case(wname, N, S, Ls)
                T = ref.shape[1]
                ext = np.zeros(N + (T - 1) * S, np.float32)
                ext[N // 2:N // 2 + Ls] = x[0]
                frames = ext[np.arange(N)[None] + S * np.arange(T)[:, None]] * w[None]
                X = scipy.fft.rfft(frames, axis=-1)
                assert X.dtype == np.complex64
                err, zero = SR.frame_errors(X * scale, ref[0])
                assert np.all(X[zero] == 0)
                assert err.max() < BAR, (N, S, wname, Ls, err.max())
                worst = max(worst, err.max())
    print('float32 pipeline, worst per-frame error: %.3g' % worst)
    assert worst < BAR / 10


def test_float32_window_squares_are_visible_in_the_istft_reference():
    '''the effect test_gpu_stft_envelope must catch: dividing by float64 squares of the window instead of the
    reference's float32 squares moves the result by more than 1e-8 in the weighted measure on every table case
    that divides at all -- four orders above the 1e-12 the kernel is held to'''
    lo, hi = np.inf, 0.0
    for N, S in SR.ISTFT_ENVELOPE:
        for wname in SR.WINDOWS:
            for T in SR.istft_frames(N, S):
                X, y, wsum = SR.istft_case(wname, N, S, T)
                y64, wsum64 = SR.istft_ref(X[0], S, SR.window(wname, N).astype(np.float64))
                if SR.istft_used(T, N, S) == 0:
                    assert not y.any() and not y64.any()
                    continue
                d = SR.weighted_error(y64, y[0], wsum)
                assert d > 1e-8, (N, S, wname, T, d)
                assert SR.weighted_error(y[0], y[0], wsum) == 0.0
                lo, hi = min(lo, d), max(hi, d)
    print('float64 squares vs float32 squares: %.3g .. %.3g' % (lo, hi))
    assert hi < 1e-6


def test_tiny_window_entry_squares_to_zero_in_float32_only():
    w = np.array([1e-25, 0.0, 0.5], np.float32)
    assert (w ** 2.).dtype == np.float32 and (w ** 2.)[0] == 0 and (w.astype(np.float64) ** 2.)[0] > 0
