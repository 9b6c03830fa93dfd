'''
THE RULE of include/danet_tonline_hip.h restated in numpy, with the element type as a parameter: float64 is the
reference the kernels are tested against; the float32 run walks the header's SUMMATION ORDER term by term and shows how
far float32 arithmetic alone moves the answer.  The forward, the closed-form backward and the separator's backward; the
same forward in torch float64 for autograd; the header's ERROR BOUND; the case generators.

Everything is batched: V [B, T, F, E], W [B, T, F], P [B, C, T, F]; attr, G, R [B, T, C, E]; den [B, T, C]; D [B, C, T, F].
'''
import numpy as np

import online_ref as OR

MAX_C, MAX_E, MAX_F, MAX_T = 4, 64, 1025, 65536
U = 2.0 ** -24                                        # the unit roundoff of float32
NT, BLOCK = 256, 16                                   # threads of a workgroup; partial sums per block
EPS = 1e-7
T0 = 8
BAR = 1e-5                                            # of each output's maximum (test_gpu_lstm_envelope.py's bar)


def fma(a, b, c, dtype):
    '''a * b + c rounded once to `dtype`.  float32: the product of two float32 is exact in float64 and the sum is
    rounded to float64 and then to float32, which differs from one rounding only on a tie of the second one'''
    if dtype == np.float64:
        return a * b + c
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def labels(P):
    '''step 1: the lowest c that maximises P[b, c, t, f] -> int [B, T, F]'''
    return np.argmax(np.asarray(P), axis=1)


def geometry(E):
    '''SUMMATION ORDER of s: (L values per lane, Q lanes per row, G rows in flight)'''
    L = 1 if E % 4 else 4
    Q = E // L
    return L, Q, NT // Q


def depth_s(F, E):
    '''N_s of the header: the float32 roundings a term of s passes through at most'''
    G = geometry(E)[2]
    return -(-F // G) + min(G, BLOCK) + -(-G // BLOCK)


def depth_q(F):
    return -(-F // NT) + 9


def contract(slot, V, dtype):
    '''sum_f slot[..., f, c] V[..., f, e] -> [..., C, E] in the header's order of s: G chains of fused multiply-adds
    over f = g, g + G, ... from +0, then the G partial sums in blocks of 16'''
    slot, V = np.asarray(slot, dtype), np.asarray(V, dtype)
    F, E = V.shape[-2:]
    C = slot.shape[-1]
    if dtype == np.float64:
        return np.einsum('...fc,...fe->...ce', slot, V)
    G = geometry(E)[2]
    n = -(-F // G)
    pad = [(0, 0)] * (V.ndim - 2) + [(0, n * G - F), (0, 0)]       # a padded bin adds 0 * 0: exact
    sl = np.pad(slot, pad).reshape(slot.shape[:-2] + (n, G, C))
    v = np.pad(V, pad).reshape(V.shape[:-2] + (n, G, E))
    acc = np.zeros(V.shape[:-2] + (G, C, E), dtype)
    for i in range(n):
        acc = fma(sl[..., i, :, :, None], v[..., i, :, None, :], acc, dtype)
    total = np.zeros(V.shape[:-2] + (C, E), dtype)
    for g0 in range(0, G, BLOCK):
        blk = np.zeros_like(total)
        for g in range(g0, min(g0 + BLOCK, G)):
            blk = (blk + acc[..., g, :, :]).astype(dtype)
        total = (total + blk).astype(dtype)
    return total


def wave_tree(x, dtype):
    '''SUMMATION ORDER of q over the 256 threads (last axis): the DPP butterfly is a balanced pairwise tree over the 64
    lanes of a wave; the four wave sums in ascending wave'''
    x = np.asarray(x, dtype).reshape(x.shape[:-1] + (NT // 64, 64))
    while x.shape[-1] > 1:
        x = (x[..., 0::2] + x[..., 1::2]).astype(dtype)
    x = x[..., 0]
    out = x[..., 0]
    for v in range(1, NT // 64):
        out = (out + x[..., v]).astype(dtype)
    return out


def frame_sums(V, W, P, dtype=np.float64):
    '''step 2 -> (s [B, T, C, E], q [B, T, C]) in `dtype`, in the header's order'''
    V, W = np.asarray(V, dtype), np.asarray(W, dtype)
    B, T, F, E = V.shape
    C = P.shape[1]
    slot = (np.eye(C, dtype=dtype)[labels(P)] * W[..., None]).astype(dtype)           # [B, T, F, C]
    s = contract(slot, V, dtype)
    if dtype == np.float64:
        return s, slot.sum(axis=2)
    n = -(-F // NT)
    sl = np.pad(slot, [(0, 0), (0, 0), (0, n * NT - F), (0, 0)]).reshape(B, T, n, NT, C)
    qa = np.zeros((B, T, NT, C), dtype)
    for j in range(n):
        qa = (qa + sl[:, :, j]).astype(dtype)
    return s, wave_tree(np.moveaxis(qa, 2, -1), dtype)


def tau(t, T, T0):
    return min(max(t, T0 - 1), T - 1)


def running(s, q, lam, T0):
    '''step 3, read at tau(t): (S_tau(t) [B, T, C, E], n_tau(t) [B, T, C]) in float64'''
    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    T = s.shape[1]
    S, n = np.zeros_like(s[:, 0]), np.zeros_like(q[:, 0])
    Ss, ns = [], []
    for t in range(T):
        S = lam * S + s[:, t]
        n = lam * n + q[:, t]
        Ss.append(S)
        ns.append(n)
    at = [tau(t, T, T0) for t in range(T)]
    return np.stack([Ss[u] for u in at], axis=1), np.stack([ns[u] for u in at], axis=1)


def scan(s, q, lam, T0, eps, dtype=np.float64):
    '''steps 3 to 5 -> (attr [B, T, C, E] float64 holding `dtype` values, den float64 [B, T, C])'''
    S, n = running(s, q, lam, T0)
    den = n + eps
    with np.errstate(all='ignore'):
        attr = np.where(den[..., None] != 0, S / den[..., None], 0.0)
    return attr.astype(dtype).astype(np.float64), den


def attractors(V, W, P, lam, T0, eps, dtype=np.float64):
    '''THE RULE -> (attr, den)'''
    return scan(*frame_sums(V, W, P, dtype), lam, T0, eps, dtype)


def scan_bwd(G, den, lam, T0, dtype=np.float64):
    '''Backward: G = dL/dattr [B, T, C, E] -> R [B, T, C, E], float64 holding `dtype` values'''
    G, den = np.asarray(G, np.float64), np.asarray(den, np.float64)
    B, T, C, E = G.shape
    u0 = min(T0, T) - 1
    R = np.zeros((B, T, C, E))
    run = np.zeros((B, C, E))
    for u in range(T - 1, -1, -1):
        if u > u0:
            top = G[:, u]
        elif u == u0:
            top = np.zeros((B, C, E))
            for t in range(u0 + 1):
                top = top + G[:, t]
        else:
            top = None
        if top is None:
            run = lam * run
        else:
            d = den[:, u, :, None]
            with np.errstate(all='ignore'):
                H = np.where(d != 0, top / d, 0.0)
            run = H + lam * run
        R[:, u] = run.astype(dtype).astype(np.float64)
    return R


def sums_bwd(R, W, P, dtype=np.float64):
    '''dV[b, t, f, e] = W[b, t, f] * R[b, t, k(t, f), e] in `dtype`'''
    R, W = np.asarray(R, dtype), np.asarray(W, dtype)
    k = labels(P)                                                             # [B, T, F]
    B, T, F = k.shape
    rows = R[np.arange(B)[:, None, None], np.arange(T)[None, :, None], k]     # [B, T, F, E]
    return (W[..., None] * rows).astype(dtype)


def attractors_bwd(G, den, W, P, lam, T0, dtype=np.float64):
    '''the closed-form backward of attractors(): dL/dattr -> dL/dV'''
    return sums_bwd(scan_bwd(G, den, lam, T0, dtype), W, P, dtype)


def separate_bwd(V, W, attr, D, act, dtype=np.float64):
    '''the backward of online_ref.separate: D = dL/dout [B, C, T, F] -> (dV [B, T, F, E], dattr [B, T, C, E])'''
    V, W, attr, D = (np.asarray(x, dtype) for x in (V, W, attr, D))
    C = attr.shape[2]
    m = OR.activation(OR.logits(V, attr, dtype), act)                      # [B, T, F, C]
    g = (W[..., None] * np.moveaxis(D, 1, -1)).astype(dtype)
    if act == 0:
        dot = np.zeros(m.shape[:-1], dtype)
        for c in range(C):
            dot = fma(m[..., c], g[..., c], dot, dtype)
        dl = (m * (g - dot[..., None]).astype(dtype)).astype(dtype)
    else:
        dl = ((m * (1 - m)).astype(dtype) * g).astype(dtype)
    dV = np.zeros(V.shape, dtype)
    for c in range(C):
        dV = fma(dl[..., c, None], attr[:, :, None, c, :], dV, dtype)
    return dV, contract(dl, V, dtype)


def attr_bound(V, W, P, lam, T0, eps):
    '''the header's ERROR BOUND of attr, per element [B, T, C, E]'''
    V, W = np.asarray(V, np.float64), np.asarray(W, np.float64)
    F, E = V.shape[2:]
    attr, den = attractors(V, W, P, lam, T0, eps)
    Sabs, nabs = running(*frame_sums(np.abs(V), np.abs(W), P), lam, T0)
    with np.errstate(all='ignore'):
        sums = U * ((depth_s(F, E) + 2) * Sabs + (depth_q(F) + 2) * np.abs(attr) * nabs[..., None]) / np.abs(den)[..., None]
    return np.where(den[..., None] != 0, sums, 0.0) + U * np.abs(attr)


# ------------------------------------------------------------------------------------------------ torch float64
def torch_attractors(V, W, P, lam, T0, eps):
    '''the forward in torch float64, differentiable in V: V [B, T, F, E] tensor, W, P arrays or tensors'''
    import torch
    W = torch.as_tensor(np.asarray(W), dtype=torch.float64)
    k = torch.as_tensor(labels(np.asarray(P)))
    C = P.shape[1]
    onehot = torch.nn.functional.one_hot(k, C).to(torch.float64) * W[..., None]          # [B, T, F, C]
    s = torch.einsum('btfc,btfe->btce', onehot, V)
    q = onehot.sum(dim=2)
    B, T = V.shape[:2]
    S, n = torch.zeros_like(s[:, 0]), torch.zeros_like(q[:, 0])
    Ss, ns = [], []
    for t in range(T):
        S = lam * S + s[:, t]
        n = lam * n + q[:, t]
        Ss.append(S)
        ns.append(n)
    return torch.stack([Ss[tau(t, T, T0)] / (ns[tau(t, T, T0)] + eps)[..., None] for t in range(T)], dim=1)


def torch_separate(V, W, attr, act):
    '''online_ref.separate in torch float64, differentiable in V and attr -> [B, C, T, F]'''
    import torch
    W = torch.as_tensor(np.asarray(W), dtype=torch.float64)
    l = torch.einsum('btfe,btce->btfc', V, attr)
    m = torch.softmax(l, dim=-1) if act == 0 else torch.sigmoid(l)
    return (W[..., None] * m).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ the cases
def case(B, T, F, E, C, seed=0, silent=0):
    '''C centres per utterance with entries +-(1 + U(0, 1)) * 0.655 / sqrt(E), so that a bin's logit against its own
    source is about 1 and neither activation saturates (where every bin saturates, m (1 - m) of the rule is a
    difference of nearly equal float32 numbers and no float32 evaluation is within 1e-5 of float64); every bin
    belongs to a source, its embedding is that source's centre plus 0.3 x noise of the same scale, and its P is largest
    for that source; W = 10 |N(0, 1)|.  silent: source C - 1 has no bin in the first `silent` frames and a bin in every
    later frame -> (V [B, T, F, E], W [B, T, F], P [B, C, T, F]) float32'''
    rng = np.random.RandomState(3000 + seed)
    centres = (1 + rng.random_sample((B, C, E))) * rng.choice([-1.0, 1.0], size=(B, C, E))
    which = rng.randint(C, size=(B, T, F))
    if silent:
        which[:, :silent] = rng.randint(max(C - 1, 1), size=(B, silent, F))
        which[:, silent:, 0] = C - 1
    V = (centres[np.arange(B)[:, None, None], which] + 0.3 * rng.standard_normal((B, T, F, E))) * (0.655 / np.sqrt(E))
    P = rng.random_sample((B, C, T, F)) + np.moveaxis(np.eye(C)[which], -1, 1)
    W = 10 * np.abs(rng.standard_normal((B, T, F)))
    return V.astype(np.float32), W.astype(np.float32), P.astype(np.float32)


def rel(got, want):
    '''the largest error of `got` as a fraction of the largest |want| (0 where both are all zero)'''
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def grads(B, T, F, E, C, seed=0):
    '''upstream gradients: G [B, T, C, E] and D [B, C, T, F], unit normal, float32'''
    rng = np.random.RandomState(4000 + seed)
    return (rng.standard_normal((B, T, C, E)).astype(np.float32), rng.standard_normal((B, C, T, F)).astype(np.float32))


SHAPE_F = (1, 3, 129, 257, 1025)
SHAPE_E = (1, 3, 4, 20, 64)
SHAPE_C = (1, 2, 3, 4)
SHAPE_T = (1, 2, T0 - 1, T0, T0 + 1, 70)
SHAPE_B = (1, 3)
LAMBDAS = (1.0, float(np.exp(-1.0 / 8)))
# (B, T, F, E, C, lambda): every F x E pair, with C, T, B and lambda taken in turn; T0 = 8 throughout
CASES = [(SHAPE_B[i % 2], SHAPE_T[i % 6], F, E, SHAPE_C[(i + i // 4) % 4], LAMBDAS[(i // 2) % 2])
         for i, (F, E) in enumerate((F, E) for F in SHAPE_F for E in SHAPE_E)]
