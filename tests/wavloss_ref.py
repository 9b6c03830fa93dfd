'''
Restatement of the waveform training loss (include/danet_wavloss_hip.h, THE RULE) in numpy float64, written from
the rule and independently of csrc/wavloss/wavloss.hip: the forward finalize step on Gram matrices (loss, pairing,
gradient coefficients), the backward step on its own inputs (combination, window-sum division, windowed forward
FFT per frame, the phasor form), and the loss and its gradient from the spectra.  The synthesis and the Gram
matrices are those of tests/metric_ref.py.  The backward step has a float32 variant (single-precision window sums,
frames and FFT; the combination in float64 rounded once, as the rule says) that measures the noise floor of
float32 arithmetic -- the tests compare the kernel's error with it.
'''
import itertools
import math

import numpy as np
import scipy.fft

import metric_ref as MR

MAX_C = 4
K = 10.0 / math.log(10.0)


def tile_frames(N):
    '''DANET_WAVLOSS_TILE_FRAMES(N)'''
    return min(32, (16384 - 3 * N // 2) // (3 * N // 2))


def clamped(a, b, c):
    '''the rule's clamps of sdr(i, j): no gradient flows through them'''
    t = c * c / a
    r = b - t
    if not t > 0 or not r > 0:
        return True
    return abs(10.0 * math.log10(t / r)) >= 100.0


def fwd(G, C):
    '''G [B, 2C, 2C] -> dict(loss, per_utt [B], perm_idx [B], pair [B, C], coef [B, C, 2])'''
    G = np.asarray(G, dtype=np.float64)
    B = G.shape[0]
    assert G.shape == (B, 2 * C, 2 * C) and 1 <= C <= MAX_C
    perms = list(itertools.permutations(range(C)))
    per_utt, perm_idx = np.zeros(B), np.zeros(B, np.int32)
    pair, coef = np.full((B, C), -1, np.int32), np.zeros((B, C, 2))
    lives = []
    for u in range(B):
        g = [[float(v) for v in row] for row in G[u]]
        live = [i for i in range(C) if g[i][i] != 0.0]
        lives.append(live)
        if not live:
            continue
        s = {(i, j): MR.sdr(g[i][i], g[C + j][C + j], g[i][C + j]) for i in live for j in range(C)}
        best, best_v = 0, None
        for p, perm in enumerate(perms):
            v = 0.0
            for i in live:
                v += s[i, perm[i]]
            if best_v is None or v > best_v:            # ties: the first permutation
                best, best_v = p, v
        per_utt[u] = best_v / len(live)
        perm_idx[u] = best
    n_utt = sum(1 for live in lives if live)
    loss = -(sum(per_utt[u] for u in range(B) if lives[u]) / n_utt) if n_utt else 0.0
    for u in range(B):
        g = G[u]
        for i in lives[u]:
            j = perms[perm_idx[u]][i]
            pair[u, j] = i
            a, b, c = float(g[i, i]), float(g[C + j, C + j]), float(g[i, C + j])
            if clamped(a, b, c):
                continue
            r = b - c * c / a
            scale = -(1.0 / (len(lives[u]) * n_utt))
            coef[u, j] = scale * (2.0 * K * b / (c * r)), scale * (-2.0 * K / r)
    return dict(loss=loss, per_utt=per_utt, perm_idx=perm_idx, pair=pair, coef=coef)


def window_sum(window, S, T, dtype=np.float64):
    '''the synthesis rule's window sum over (T - 1) * S samples: the frames in ascending t, in `dtype`'''
    w = np.asarray(window).astype(dtype)
    N = len(w)
    Ls = (T - 1) * S
    wsum = np.zeros(Ls, dtype)
    for t in range(T):
        lo = t * S - N // 2
        a, b = max(lo, 0), min(lo + N, Ls)
        if a < b:
            wsum[a:b] += w[a - lo:b - lo] * w[a - lo:b - lo]
    return wsum


def adjoint(u, window, S, T, dtype=np.float64):
    '''u [..., Ls] (ALREADY divided by the window sum) -> complex [..., T, F]: (c_f / N) rfft_N(w * frame t of u)'''
    w = np.asarray(window).astype(dtype)
    N = len(w)
    Ls = (T - 1) * S
    u = np.asarray(u).astype(dtype)
    assert u.shape[-1] == Ls
    pad = np.zeros(u.shape[:-1] + (N // 2,), dtype)
    up = np.concatenate([pad, u, pad], axis=-1)                 # frame t covers up[t S : t S + N]
    frames = np.stack([w * up[..., t * S:t * S + N] for t in range(T)], axis=-2)
    if dtype == np.float32:
        X = scipy.fft.rfft(frames, axis=-1)
        assert X.dtype == np.complex64
    else:
        X = np.fft.rfft(frames, axis=-1)
    c = np.full(N // 2 + 1, 2.0, dtype)
    c[0] = c[-1] = 1.0
    X = X * (c / dtype(N))
    X[..., 0] = X[..., 0].real                                  # exactly real at bins 0 and N/2
    X[..., -1] = X[..., -1].real
    return X


def bwd(wav, pair, coef, window, S, dloss=1.0, phasor=None, dtype=np.float64):
    '''the backward step of the rule on ITS OWN inputs: wav [B, 2C, Ls], pair [B, C], coef [B, C, 2] ->
    complex dX [B, C, T, F], or with phasor [B, T, F, 2] the real dsep'''
    wav = np.asarray(wav)
    B, M, Ls = wav.shape
    C, T = M // 2, Ls // S + 1
    pair, coef = np.asarray(pair), np.asarray(coef, dtype=np.float64)
    wsum = window_sum(window, S, T, dtype)
    g = np.zeros((B, C, Ls))
    for b in range(B):
        for j in range(C):
            i = int(pair[b, j])
            if 0 <= i < C:
                g[b, j] = coef[b, j, 0] * wav[b, i].astype(np.float64) + coef[b, j, 1] * wav[b, C + j].astype(np.float64)
    ok = wsum > 0
    u = np.zeros((B, C, Ls))
    u[..., ok] = g[..., ok] / wsum[ok].astype(np.float64)
    dX = adjoint(u.astype(dtype), window, S, T, dtype) * dtype(dloss)
    if phasor is None:
        return dX
    ph = np.asarray(phasor).astype(dtype)
    return ph[:, None, :, :, 0] * dX.real + ph[:, None, :, :, 1] * dX.imag


def loss_and_grad(S_ref, E, window, stride, dtype=np.float64):
    '''references and (unpermuted) estimates complex [B, C, T, F] -> (fwd dict, dX [B, C, T, F]).  dtype float32:
    the synthesis and the backward step in single precision (Gram and finalize stay float64, as in the library)'''
    S_ref, E = np.asarray(S_ref), np.asarray(E)
    C = S_ref.shape[1]
    wav = MR.synth(np.concatenate([S_ref, E], axis=1), window, stride, dtype)
    # exactly rounded Gram matrices: r = b - c^2 / a amplifies their rounding by 10^(SDR/10) (a plain float64 dot
    # product of 2500 samples is already 1e-10 of the gradient at 50 dB)
    f = fwd(MR.gram_fsum(wav), C)
    return f, bwd(wav, f['pair'], f['coef'], window, stride, dtype=dtype)


def reattach(sep_pwr, phasor):
    '''separated magnitudes [B, C, T, F] with the mixture phase (cos, sin) [B, T, F, 2] -> complex'''
    sep_pwr, phasor = np.asarray(sep_pwr), np.asarray(phasor)
    return sep_pwr * (phasor[:, None, :, :, 0] + 1j * phasor[:, None, :, :, 1])


def loss_from_sep(S_ref, sep_pwr, phasor, window, stride, dtype=np.float64):
    '''-> (fwd dict, dsep [B, C, T, F]): the loss of ops.si_sdr_loss and its gradient, from the spectra'''
    E = reattach(np.asarray(sep_pwr, dtype=np.float64), np.asarray(phasor, dtype=np.float64))
    if dtype == np.float32:
        E = E.astype(np.complex64)
    f, dX = loss_and_grad(S_ref, E, window, stride, dtype)
    ph = np.asarray(phasor).astype(dtype)
    return f, ph[:, None, :, :, 0] * dX.real + ph[:, None, :, :, 1] * dX.imag
