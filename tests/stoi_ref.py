'''
The STOI / ESTOI rule of include/danet_stoi_hip.h restated in numpy, stage by stage: resampling to 10 kHz, silent
frames, compaction, one-third-octave band magnitudes, the 30-frame segments and the finalize step.  float64 is the
reference; dtype=np.float32 runs the band and segment stages in single precision, which is how the GPU tests derive
their bar (four times the worst deviation of that run from the float64 one).
'''
import itertools
from math import gcd

import numpy as np

FS = 10000
FRAME, HOP, NFFT, BANDS, SEG = 256, 128, 512, 15, 30
CLIP = 6.623413251903491            # 1 + 10 ** (15 / 20), as the header writes it out
DYN = 1e-4                          # 40 dB under the loudest frame, as an energy ratio
MAX_C, MAX_TABLE, MIN_RATE, MAX_BATCH = 4, 16384, 8000, 16383
FLAG_SHORT, FLAG_SILENT = 1, 2
# [lo, hi) of the fifteen one-third-octave bands on the grid 10000 k / 512 (the header's table)
BAND_BINS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69),
             (69, 87), (87, 109), (109, 138), (138, 174), (174, 219))


# ------------------------------------------------------------------------------------------ 1. resample
def rate(smprate):
    '''(U, D, H) of a sample rate: H = 0 (the stage is a copy) when it is 10 kHz already'''
    g = gcd(FS, int(smprate))
    U, D = FS // g, int(smprate) // g
    return U, D, (0 if U == D == 1 else 10 * max(U, D))


def table(smprate):
    '''h, float64 [2H + 1]'''
    import scipy.signal
    U, D, H = rate(smprate)
    if H == 0:
        return np.ones(1)
    return U * scipy.signal.firwin(2 * H + 1, 1.0 / max(U, D), window=('kaiser', 5.0))


def out_len(Ls, U, D):
    return -(-int(Ls) * U // D)


def resample(x, U, D, H, h, with_bound=False):
    '''y[n] = sum_k h[n D + H - k U] x[k] along the last axis in float64, the terms of an output in ascending k;
    with_bound: also (taps [L10], sum |h x|) per output'''
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    Ls = x.shape[-1]
    L10 = out_len(Ls, U, D)
    c = np.arange(L10, dtype=np.int64) * D + H
    klo = np.maximum(0, -((2 * H - c) // U))
    khi = np.minimum(Ls - 1, c // U)
    y, a = np.zeros(x.shape[:-1] + (L10,)), np.zeros(x.shape[:-1] + (L10,))
    for t in range(int((khi - klo).max()) + 1 if L10 else 0):
        k = klo + t
        ok = k <= khi
        k = np.where(ok, k, 0)
        p = np.where(ok, h[np.where(ok, c - k * U, 0)] * x[..., k], 0.0)
        y += p
        a += np.abs(p)
    if with_bound:
        return y, np.maximum(khi - klo + 1, 0), a
    return y


def mixture(refs):
    '''the float32 sum of the float32 references, in their order'''
    m = np.array(refs[0], np.float32)
    for r in refs[1:]:
        m = (m + np.asarray(r, np.float32)).astype(np.float32)
    return m


# ------------------------------------------------------------------------------------ 2. silent frames
def window():
    return np.hanning(FRAME + 2)[1:-1].astype(np.float32)


def num_frames(L10):
    return (L10 - FRAME) // HOP + 1 if L10 >= FRAME else 0


def _frames(x, idx):
    return x[HOP * np.asarray(idx, np.int64)[:, None] + np.arange(FRAME)]


def frame_energies(x, w):
    nf = num_frames(len(x))
    fr = np.asarray(w, np.float64) * _frames(np.asarray(x, np.float64), np.arange(nf))
    return (fr * fr).sum(axis=1)


def kept(x, w):
    '''(mask [nf], k [M], E [nf]) of a reference'''
    E = frame_energies(x, w)
    mask = E > DYN * E.max() if len(E) else np.zeros(0, bool)
    return mask, np.flatnonzero(mask), E


def margin_db(E):
    '''the least distance, in dB, of a frame energy from the threshold (inf without a frame or without energy)'''
    E = np.asarray(E, np.float64)
    if not len(E) or not E.max() > 0:
        return np.inf
    with np.errstate(divide='ignore'):
        return float(np.abs(10 * np.log10(E / (DYN * E.max()))).min())


# ---------------------------------------------------------------------------------------- 3. compaction
def compact(z, w, k):
    '''the compacted frames c_q [M, 256] of signal z under the kept frames k: a gather'''
    z, w, k = np.asarray(z, np.float64), np.asarray(w, np.float64), np.asarray(k, np.int64)
    M = len(k)
    if M == 0:
        return np.zeros((0, FRAME))
    own = w * _frames(z, k)
    c = own.copy()
    c[1:, :HOP] += own[:-1, HOP:]
    c[:-1, HOP:] += own[1:, :HOP]
    return c


def compact_loop(z, w, mask):
    '''the same, literally: overlap-add the kept windowed frames one by one, then cut frames at the same hop'''
    z, w = np.asarray(z, np.float64), np.asarray(w, np.float64)
    ks = [f for f in range(len(mask)) if mask[f]]
    if not ks:
        return np.zeros((0, FRAME))
    ola = np.zeros((len(ks) - 1) * HOP + FRAME)
    for q, f in enumerate(ks):
        for n in range(FRAME):
            ola[HOP * q + n] += w[n] * z[HOP * f + n]
    return np.stack([ola[HOP * q:HOP * q + FRAME] for q in range(len(ks))])


def band_table():
    grid = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    out = []
    for b in range(BANDS):
        lo = 150.0 * 2.0 ** ((2 * b - 1) / 6.0)
        hi = 150.0 * 2.0 ** ((2 * b + 1) / 6.0)
        out.append((int(np.argmin(np.abs(grid - lo))), int(np.argmin(np.abs(grid - hi)))))
    return tuple(out)


def band_mags(c, w, bins=BAND_BINS, dtype=np.float64):
    '''T [15, M] of the compacted frames c [M, 256]'''
    fr = (np.asarray(w, dtype) * np.asarray(c, dtype)).astype(dtype)
    if not len(fr):
        return np.zeros((BANDS, 0), dtype)
    Z = np.fft.rfft(fr, NFFT, axis=1)
    P = (Z.real * Z.real + Z.imag * Z.imag).astype(dtype)
    return np.stack([np.sqrt(P[:, lo:hi].sum(axis=1, dtype=dtype)) for lo, hi in bins]).astype(dtype)


# ------------------------------------------------------------------------------------------ 4. segments
def _safe_div(a, b):
    out = np.zeros_like(a)
    np.divide(a, b, out=out, where=b > 0)
    return out


def segment_values(X, Y, dtype=np.float64):
    '''(d_q of STOI, d_q of ESTOI), each [M - 29], of the band magnitudes X (reference) and Y, [15, M]'''
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    M = X.shape[1]
    if M < SEG:
        return np.zeros(0, dtype), np.zeros(0, dtype)
    Xs = np.lib.stride_tricks.sliding_window_view(X, SEG, axis=1).transpose(1, 0, 2)      # [nseg, 15, 30]
    Ys = np.lib.stride_tricks.sliding_window_view(Y, SEG, axis=1).transpose(1, 0, 2)
    nx = np.sqrt((Xs * Xs).sum(-1, dtype=dtype))
    ny = np.sqrt((Ys * Ys).sum(-1, dtype=dtype))
    alpha = _safe_div(nx, ny)
    Yp = np.minimum(alpha[..., None] * Ys, dtype(CLIP) * Xs)
    xc = Xs - Xs.mean(-1, dtype=dtype, keepdims=True)
    yc = Yp - Yp.mean(-1, dtype=dtype, keepdims=True)
    den = np.sqrt((xc * xc).sum(-1, dtype=dtype)) * np.sqrt((yc * yc).sum(-1, dtype=dtype))
    r = _safe_div((xc * yc).sum(-1, dtype=dtype), np.where(ny > 0, den, 0).astype(dtype))
    d_stoi = r.sum(-1, dtype=dtype) / dtype(BANDS)

    def normed(A):
        a = A - A.mean(-1, dtype=dtype, keepdims=True)
        a = _safe_div(a, np.broadcast_to(np.sqrt((a * a).sum(-1, dtype=dtype, keepdims=True)), a.shape))
        a = a - a.mean(1, dtype=dtype, keepdims=True)
        return _safe_div(a, np.broadcast_to(np.sqrt((a * a).sum(1, dtype=dtype, keepdims=True)), a.shape))
    d_estoi = (normed(Xs) * normed(Ys)).sum((1, 2), dtype=dtype) / dtype(SEG)
    return d_stoi.astype(dtype), d_estoi.astype(dtype)


def segments(X, Y, dtype=np.float64):
    '''(STOI, ESTOI) of a pair: the means of d_q over the M - 29 segments, (0, 0) when M < 30'''
    a, e = segment_values(X, Y, dtype)
    if not len(a):
        return 0.0, 0.0
    return float(a.sum(dtype=dtype) / dtype(len(a))), float(e.sum(dtype=dtype) / dtype(len(e)))


# ------------------------------------------------------------------------------------------ 5. finalize
def search(st, live):
    '''(index, permutation) maximising the sum of st[i][p[i]] over the live references; ties: the first'''
    C = len(st)
    best, best_v, best_p = 0, None, tuple(range(C))
    for idx, p in enumerate(itertools.permutations(range(C))):
        v = 0.0
        for i in range(C):
            if live[i]:
                v += st[i][p[i]]
        if best_v is None or v > best_v:
            best, best_v, best_p = idx, v, p
    return best, best_p


def search_gap(st, live):
    '''best minus second-best permutation sum (inf with one permutation)'''
    C = len(st)
    sums = sorted((sum(st[i][p[i]] for i in range(C) if live[i]) for p in itertools.permutations(range(C))),
                  reverse=True)
    return np.inf if len(sums) < 2 else sums[0] - sums[1]


def scores(st, es, M, live):
    '''st, es [C][C + 1] (column C: the mixture), M [C], live [C] -> (per_utt [4], perm index, flags)'''
    C = len(st)
    flag = FLAG_SHORT if any(live[i] and M[i] < SEG for i in range(C)) else 0
    n_live = sum(1 for v in live if v)
    if n_live == 0:
        return np.zeros(4), 0, flag | FLAG_SILENT
    if flag:
        return np.zeros(4), 0, flag
    idx, p = search(st, live)
    out = np.zeros(4)
    for i in range(C):
        if live[i]:
            out += [st[i][p[i]], es[i][p[i]], st[i][p[i]] - st[i][C], es[i][p[i]] - es[i][C]]
    return out / n_live, idx, 0


def batch_mean(per_utt, flags):
    '''(mean4, count) over the utterances with flags = 0'''
    per_utt, flags = np.asarray(per_utt, np.float64).reshape(-1, 4), np.asarray(flags)
    ok = flags == 0
    if not ok.any():
        return np.zeros(4), 0
    return per_utt[ok].sum(axis=0) / ok.sum(), int(ok.sum())


# --------------------------------------------------------------------------------------- the whole rule
def signals10(wav, U, D, H, h32):
    '''float32 [2C, Ls] -> the float32 rows [2C + 1, L10] the later stages read (rounded once, as the kernel does)'''
    wav = np.asarray(wav, np.float32)
    C = wav.shape[0] // 2
    rows = list(wav) + [mixture(wav[:C])]
    return np.stack([resample(r, U, D, H, h32).astype(np.float32) for r in rows])


def pair_tables(sig, w, dtype=np.float64, with_gap=False):
    '''sig float32 [2C + 1, L10] -> (st [C][C + 1], es [C][C + 1], M [C], live [C])'''
    C = (sig.shape[0] - 1) // 2
    nf = num_frames(sig.shape[1])
    st, es, Ms, live = np.zeros((C, C + 1)), np.zeros((C, C + 1)), [], []
    for i in range(C):
        mask, k, E = kept(sig[i], w)
        Ms.append(len(k))
        live.append(bool(nf == 0 or E.max() > 0))
        if len(k) < SEG:
            continue
        X = band_mags(compact(sig[i], w, k), w, dtype=dtype)
        for j in range(C + 1):
            Y = band_mags(compact(sig[C + j], w, k), w, dtype=dtype)
            st[i, j], es[i, j] = segments(X, Y, dtype)
    return st, es, Ms, live


def evaluate(wav, smprate, h32=None, dtype=np.float64):
    '''one utterance, float32 [2C, Ls] -> (per_utt [4], perm index, flags)'''
    U, D, H = rate(smprate)
    h32 = table(smprate).astype(np.float32) if h32 is None else h32
    st, es, Ms, live = pair_tables(signals10(wav, U, D, H, h32), window(), dtype)
    return scores(st, es, Ms, live)


def evaluate_batch(wav, smprate, h32=None, dtype=np.float64):
    '''float32 [B, 2C, Ls] -> (mean4, per_utt [B, 4], perm_idx [B], flags [B], count)'''
    res = [evaluate(u, smprate, h32, dtype) for u in wav]
    per = np.stack([r[0] for r in res])
    flags = np.array([r[2] for r in res], np.int32)
    mean4, count = batch_mean(per, flags)
    return mean4, per, np.array([r[1] for r in res], np.int32), flags, count


def stoi(x, y, smprate=FS):
    '''(STOI, ESTOI) of the estimate y against the reference x, two float32 signals (0, 0 when M < 30)'''
    U, D, H = rate(smprate)
    h32 = table(smprate).astype(np.float32)
    w = window()
    xs = resample(np.asarray(x, np.float32), U, D, H, h32).astype(np.float32)
    ys = resample(np.asarray(y, np.float32), U, D, H, h32).astype(np.float32)
    k = kept(xs, w)[1]
    return segments(band_mags(compact(xs, w, k), w), band_mags(compact(ys, w, k), w))


# ------------------------------------------------------------------------------------------ test signals
def make_signal(rng, n, period, floor_db=60.0):
    '''an AR(1) process gated by sin(2 pi n / period) > -0.3, the gated-off parts `floor_db` down'''
    import scipy.signal
    x = scipy.signal.lfilter([1.0], [1.0, -0.9], rng.standard_normal(n))
    gate = np.sin(2 * np.pi * np.arange(n) / period) > -0.3
    return (x * np.where(gate, 1.0, 10.0 ** (-floor_db / 20.0))).astype(np.float32)


def make_case(C, Ls, seed, noise=0.3, period=None):
    '''float32 [2C, Ls]: C gated AR(1) references and C estimates = reference + a little of the others + white noise'''
    rng = np.random.RandomState(seed)
    refs = [make_signal(rng, Ls, period or (1500 + 400 * i + 37 * (seed % 5))) for i in range(C)]
    ests = []
    for j in range(C):
        e = refs[j].astype(np.float64) + noise * (1 + 0.5 * j) * rng.standard_normal(Ls)
        for i in range(C):
            if i != j:
                e = e + 0.2 * refs[i]
        ests.append(e.astype(np.float32))
    return np.stack(refs + ests)
