'''
numpy float64 restatement of the active-speech-level rule of the wavdir dataset (MIX_LEVEL_MEASURE = "active"),
written from the rule in include/danet_level_hip.h (not from datasets.py / level.hip): the parameters, the
two-stage envelope (the sequential recurrence, through scipy's lfilter), the thresholds, the activity counts --
vectorised, and as the standard's literal counter loop -- the finish, and the gated-noise inputs the level tests
share.
'''
import math

import numpy as np
import scipy.signal

N_THR = 16
MARGIN_DB = 15.9


def params(fs):
    '''(g, k, I) at the sampling rate fs'''
    g = math.exp(-1.0 / (0.03 * fs))
    return g, 1.0 - g, int(math.ceil(0.2 * fs))


def envelope(x, g):
    '''q[n] of the rule: p[n] = g p[n-1] + k |x[n]|, q[n] = g q[n-1] + k p[n] from a zero state, float64, in
    sample order (lfilter's direct form is exactly this recurrence)'''
    a = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64))
    k = 1.0 - g
    p = scipy.signal.lfilter([k], [1.0, -g], a)
    return scipy.signal.lfilter([k], [1.0, -g], p)


def envelope_loop(x, g):
    '''the same recurrence as a plain loop (small inputs)'''
    k, p, q, out = 1.0 - g, 0.0, 0.0, []
    for v in np.asarray(x, dtype=np.float32).astype(np.float64):
        p = g * p + k * abs(v)
        q = g * q + k * p
        out.append(q)
    return np.asarray(out, dtype=np.float64)


def sum_squares(x):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return math.fsum((x * x).tolist())


def thresholds(P):
    '''c_j = sqrt(P) * 2^(j - 10), j = 0..15'''
    return np.asarray([math.sqrt(P) * 2.0 ** (j - 10) for j in range(N_THR)], dtype=np.float64)


def counts(q, thr, I):
    '''a_j for every threshold: the number of n for which some m <= n has q[m] >= c_j and n - m <= I'''
    q = np.asarray(q, dtype=np.float64)
    n = np.arange(len(q), dtype=np.int64)
    out = np.zeros(len(thr), dtype=np.int64)
    for j, c in enumerate(thr):
        last = np.maximum.accumulate(np.where(q >= c, n, -1))
        out[j] = int(np.count_nonzero((last >= 0) & (n - last <= I)))
    return out


def counts_literal(q, thr, I):
    '''the standard's counter loop, hangover counter started at I: a sample at or above the threshold is active
    and clears the counter; one below it is active while the counter is below I, and advances it'''
    out = np.zeros(len(thr), dtype=np.int64)
    for j, c in enumerate(thr):
        a, h = 0, I
        for v in q:
            if v >= c:
                a, h = a + 1, 0
            elif h < I:
                a, h = a + 1, h + 1
        out[j] = a
    return out


def min_margin(q, thr):
    '''the smallest |q[n] / c_j - 1| over every sample and threshold'''
    q = np.asarray(q, dtype=np.float64)
    return min(float(np.min(np.abs(q / c - 1.0))) for c in thr)


def finish(sumsq, L, a, thr):
    '''the active POWER from the counts: step 4 of the rule, scalar float64'''
    if not sumsq > 0.0:
        return 0.0
    A = [10.0 * math.log10(sumsq / a[j]) if a[j] > 0 else None for j in range(N_THR)]
    C = [20.0 * math.log10(thr[j]) for j in range(N_THR)]
    for j in range(N_THR):
        if a[j] > 0 and A[j] - C[j] <= MARGIN_DB:
            if j == 0:
                return 10.0 ** (A[0] / 10.0)
            d0, d1 = A[j - 1] - C[j - 1], A[j] - C[j]
            w = (d0 - MARGIN_DB) / (d0 - d1)
            return 10.0 ** ((A[j - 1] + w * (A[j] - A[j - 1])) / 10.0)
    return sumsq / L


def active_power(x, fs):
    '''the active power of one float32 waveform, start to end'''
    x = np.asarray(x, dtype=np.float32)
    g, _k, I = params(fs)
    s = sum_squares(x)
    if not s > 0.0:
        return 0.0
    thr = thresholds(s / len(x))
    return finish(s, len(x), counts(envelope(x, g), thr, I), thr)


def active_level_db(x, fs):
    return 10.0 * math.log10(active_power(x, fs))


def gated_noise(rng, n, fs, rms=1000.0, floor_db=-50.0, lo_ms=50, hi_ms=400, duty=None):
    '''float32 white noise of n samples in bursts and pauses of lo_ms..hi_ms each, on a noise floor floor_db below
    the bursts (duty: None = alternate drawn bursts and pauses; 1.0 = no pause; else ONE burst over that
    share of the file, then one pause: long against the hangover)'''
    gate = np.zeros(n, dtype=np.float64)
    if duty is None:
        at, on = 0, bool(rng.randint(0, 2))
        while at < n:
            span = int(rng.randint(lo_ms, hi_ms + 1) * fs // 1000)
            gate[at:at + span] = 10.0 ** (-rng.uniform(0.0, 20.0) / 20.0) if on else 0.0      # bursts over 20 dB
            at, on = at + span, not on
    elif duty >= 1.0:
        gate[:] = 1.0
    else:
        gate[:int(duty * n)] = 1.0
    amp = rms * np.maximum(gate, 10.0 ** (floor_db / 20.0))
    return (rng.randn(n) * amp).astype(np.float32)
