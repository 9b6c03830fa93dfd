'''
THE RULE of include/danet_gclip_hip.h (GRAD_CLIP_NORM) restated in numpy float64: the slicing, the fixed summation
tree of the sum of squares bit for bit, norm, coefficient, factor, and the scaled value clip + TF1-Adam element
update in float64.  The GPU tests compare the library with this file, the CPU tests this file with
torch.nn.utils.clip_grad_norm_.
'''
import numpy as np

MAX_PARTIALS = 1024
MIN_SLICE = 4096
THREADS = 256
U = 2.0 ** -53          # the unit roundoff of float64


def slice_of(n):
    '''slice(n): elements of one partial, a multiple of 4'''
    per = -(-n // MAX_PARTIALS)
    return max(MIN_SLICE, 4 * (-(-per // 4)))


def partials_of(n):
    '''partials(n)'''
    return -(-n // slice_of(n))


def serial_terms(n):
    '''terms(n): the most terms one thread adds serially'''
    return -(-slice_of(n) // 1024) + 2


def sum_bar(n):
    '''bound on the relative error of the sum of squares (positive terms, exact squares): the chain of additions
    is terms(n) + 22 long at the most; the header's bar is (terms(n) + 32) * 2^-53'''
    return (serial_terms(n) + 32) * U


def _block_sum(acc):
    '''the 256 accumulators -> their sum over the butterfly of a wave (partner lane ^ 32, 16, ..., 1) and
    (w0 + w1) + (w2 + w3)'''
    w = np.asarray(acc, np.float64).reshape(4, 64).copy()
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ m]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def _partial(x, head):
    '''one partial of the float32 span x whose first 16-byte boundary lies `head` elements in'''
    n = x.size
    head = min(n, head)
    nvec = (n - head) // 4
    tail = n - head - 4 * nvec
    sq = x.astype(np.float64) ** 2                        # exact
    acc = np.zeros(THREADS, np.float64)
    if nvec:
        v = sq[head:head + 4 * nvec].reshape(nvec, 4)
        v = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
        rows = -(-nvec // THREADS)
        v = np.concatenate([v, np.zeros(rows * THREADS - nvec)]).reshape(rows, THREADS)
        live = (np.arange(rows * THREADS) < nvec).reshape(rows, THREADS)
        for r in range(rows):                             # thread t: q = t, t + 256, ... in order
            acc = np.where(live[r], acc + v[r], acc)
    acc[:head] += sq[:head]
    acc[:tail] += sq[head + 4 * nvec:]
    return _block_sum(acc)


def sumsq_partials(g, residue=0):
    '''the partials of the float32 gradient g whose first element lies `residue` elements (0..3) behind a 16-byte
    boundary'''
    g = np.asarray(g, np.float32).reshape(-1)
    n, s = g.size, slice_of(g.size)
    head = (4 - residue) & 3
    return np.array([_partial(g[b:b + s], head) for b in range(0, n, s)], np.float64)


def total(partials):
    '''S: thread t adds the partials t, t + 256, t + 512, t + 768 in order, then the block sum'''
    p = np.zeros(MAX_PARTIALS, np.float64)
    live = np.arange(MAX_PARTIALS) < len(partials)
    p[:len(partials)] = partials
    acc = np.zeros(THREADS, np.float64)
    for q in range(MAX_PARTIALS // THREADS):
        sl = slice(q * THREADS, (q + 1) * THREADS)
        acc = np.where(live[sl], acc + p[sl], acc)
    return _block_sum(acc)


def norm_coef(S, s, M):
    '''-> (norm, coef) of THE RULE, float64'''
    with np.errstate(invalid='ignore', over='ignore'):
        norm = np.abs(np.float64(s)) * np.sqrt(np.float64(S))
        lim = norm + np.float64(1e-6)
        coef = np.float64(M) / lim if lim > M else np.float64(1.0)
    return norm, coef


def factor(s, coef):
    '''k: one rounding to float32'''
    return np.float32(np.float64(s) * np.float64(coef))


def clip(g, s, M, residue=0):
    '''-> dict(norm, coef, k) of the float32 gradient g'''
    norm, coef = norm_coef(total(sumsq_partials(g, residue)), s, M)
    return dict(norm=norm, coef=coef, k=factor(s, coef))


def scaled_value_clip(g, k, thres):
    '''g' of the update: g * k, then the value clip (0 / None: off); NaN stays NaN'''
    g = np.asarray(g, np.float64) * np.float64(k)
    if thres:
        g = np.where(np.isnan(g), g, np.clip(g, -thres, thres))
    return g
