'''
numpy float64 restatement of the additive noise of the wavdir dataset, written from the rule in
include/danet_noise_hip.h (not from datasets.py / noise.hip): the draw of a batch, the segment of every mixture, its
gain, and the helpers the noise tests share (a recording RandomState, a folder of noise recordings).
'''
import math
import os

import numpy as np


def stream(rank, subset):
    '''the RandomState of a subset's noise: seeded by (1337 + rank, index of the subset, 3)'''
    return np.random.RandomState([1337 + rank, ('train', 'valid', 'test').index(subset), 3])


def num_frames(L, N, S):
    return (L + (-L % S) % N) // S + 1


def full_length(T_max, S):
    '''Lfull: the waveform length of exactly T_max frames'''
    return (T_max - 1) * S


def segment(u, Ln, off, T_max, N, S):
    '''(offset, length, pad_left) of ONE mixture's noise row: a cut of Lfull samples out of a long file, or the
    whole of a short one placed like a short utterance'''
    Lfull = full_length(T_max, S)
    if Ln >= Lfull:
        start = min(int(u * (Ln - Lfull + 1)), Ln - Lfull)
        return off + start, Lfull, 0
    T_n = num_frames(Ln, N, S)
    return off, Ln, min(int(u * (T_max - T_n + 1)), T_max - T_n)


def gain64(P_rows, g_rows, P_n, snr):
    '''float64 gain of ONE mixture: P_rows the stored mean powers of its sources, g_rows their float32 mix gains
    (None: 1), P_n the noise file's mean power, snr the drawn dB'''
    P_s = 0.0
    for c in range(len(P_rows)):
        g = 1.0 if g_rows is None else float(np.float32(g_rows[c]))
        P_s += g * g * float(P_rows[c])
    if P_s == 0.0 or P_n == 0.0:
        return 0.0
    return math.sqrt(P_s / float(P_n)) * 10.0 ** (-float(snr) / 20.0)


def plan(powers, gains, rng, C, noise_offsets, noise_lengths, noise_powers, T_max, lo, hi, N, S):
    '''one batch of B = len(powers) / C mixtures: THREE calls, each of size B -- randint, random_sample, uniform ->
    dict(files, u, snr, offsets, lengths, pads, gains64, gains)'''
    powers = np.asarray(powers, dtype=np.float64)
    assert len(powers) % C == 0
    B = len(powers) // C
    f = rng.randint(0, len(noise_lengths), size=B)
    u = rng.random_sample(B)
    snr = rng.uniform(lo, hi, size=B)
    rows, g64 = [], []
    for b in range(B):
        rows.append(segment(float(u[b]), int(noise_lengths[f[b]]), int(noise_offsets[f[b]]), T_max, N, S))
        g64.append(gain64(powers[b * C:(b + 1) * C], None if gains is None else gains[b * C:(b + 1) * C],
                          noise_powers[f[b]], snr[b]))
    g64 = np.asarray(g64, dtype=np.float64)
    return dict(files=f, u=u, snr=snr, offsets=np.asarray([r[0] for r in rows], np.int64),
                lengths=np.asarray([r[1] for r in rows], np.int64), pads=np.asarray([r[2] for r in rows], np.int64),
                gains64=g64, gains=g64.astype(np.float32))


def realised_snr(P_rows, g_rows, P_n, g_n):
    '''10 log10(P_s / (g_n^2 P_n)), dB'''
    P_s = sum((1.0 if g_rows is None else float(np.float32(g_rows[c]))) ** 2 * float(P_rows[c])
              for c in range(len(P_rows)))
    return 10.0 * math.log10(P_s / (g_n * g_n * P_n))


class RecordingRandomState(object):
    '''a RandomState that records its calls: (name, size) in order; `fixed_u` replaces what random_sample returns
    (the draw is still made)'''

    def __init__(self, seed, fixed_u=None):
        self.rng, self.calls, self.fixed_u = np.random.RandomState(seed), [], fixed_u

    def randint(self, lo, hi, size=None):
        self.calls.append(('randint', size))
        return self.rng.randint(lo, hi, size=size)

    def random_sample(self, size=None):
        self.calls.append(('random_sample', size))
        v = self.rng.random_sample(size)
        return v if self.fixed_u is None else np.full_like(v, self.fixed_u)

    def uniform(self, lo, hi, size=None):
        self.calls.append(('uniform', size))
        return self.rng.uniform(lo, hi, size=size)


def write_noise(root, lengths, seed=5, rates=(8000, 16000, 11025), scales=(40.0, 900.0, 6000.0), silent=()):
    '''a folder of int16 noise recordings: file i has lengths[i] samples AT 8 kHz once resampled (a file at another
    rate is written with the number of samples that resamples to it), rates and stored scales cycling; indices in
    `silent` are all-zero -> [paths] in sorted order'''
    import scipy.io.wavfile
    rng = np.random.RandomState(seed)
    os.makedirs(str(root), exist_ok=True)
    out = []
    for i, L in enumerate(lengths):
        rate = rates[i % len(rates)]
        n = L
        if rate != 8000:
            n = int(L * rate / 8000.0)
            while int(math.ceil(n * 8000 / float(rate))) < L:
                n += 1
            while int(math.ceil(n * 8000 / float(rate))) > L:
                n -= 1
        w = rng.randn(n) * scales[i % len(scales)]
        if i in silent:
            w = np.zeros(n)
        fn = os.path.join(str(root), 'sub%d' % (i % 2), 'noise%02d.wav' % i)
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        scipy.io.wavfile.write(fn, rate, np.clip(w, -32768, 32767).astype(np.int16))
        out.append(fn)
    return sorted(out)
