'''
THE RULE of include/danet_online_hip.h restated in numpy, with the element type as a parameter: float64 is the
reference the kernels are tested against, the float32 run shows how far float32 arithmetic alone moves the answer (the
input condition of the 1e-5 bar).  Plus the shared case table.

Everything is batched: V [B, T, F, E], W [B, T, F], state = (S [B, C, E], n [B, C], A [B, C, E]) in float64.
'''
import numpy as np

MAX_C, MAX_E, MAX_F, MAX_T = 4, 64, 1025, 65536
U = 2.0 ** -24                                        # the unit roundoff of float32


def state_doubles(C, E):
    '''the float64 words of one utterance's state: S [C][E], n [C], A [C][E]'''
    return 2 * C * E + C


def init(A0):
    '''danet_online_init: S = 0, n = 0, A = A0'''
    A0 = np.asarray(A0, np.float64)
    return np.zeros_like(A0), np.zeros(A0.shape[:2]), A0.copy()


def pack(state):
    '''(S, n, A) -> float64 [B, 2 C E + C], the header's layout'''
    S, n, A = state
    B = S.shape[0]
    return np.concatenate([S.reshape(B, -1), n.reshape(B, -1), A.reshape(B, -1)], axis=1).astype(np.float64)


def unpack(flat, C, E):
    flat = np.asarray(flat, np.float64)
    B, CE = flat.shape[0], C * E
    assert flat.shape == (B, state_doubles(C, E)), flat.shape
    return flat[:, :CE].reshape(B, C, E).copy(), flat[:, CE:CE + C].copy(), flat[:, CE + C:].reshape(B, C, E).copy()


def logits(V, A, dtype=np.float64):
    '''step 1: l[..., f, c] = V[..., f, :] . A[..., c, :], e ascending from +0, in `dtype`; V [..., F, E], A [..., C, E]'''
    V, A = np.asarray(V, dtype), np.asarray(A, dtype)
    l = np.zeros(V.shape[:-1] + (A.shape[-2],), dtype)
    for e in range(V.shape[-1]):
        l = (l + V[..., :, None, e] * A[..., None, :, e]).astype(dtype)
    return l


def activation(l, act):
    '''step 2: softmax over the last axis (act 0; the row maximum subtracted) or sigmoid (act 1), in l's type'''
    if act == 0:
        x = np.exp(l - l.max(axis=-1, keepdims=True))
        return (x / x.sum(axis=-1, keepdims=True)).astype(l.dtype)
    with np.errstate(over='ignore'):
        return (1 / (1 + np.exp(-l))).astype(l.dtype)


def scan(V, W, state, act, lam, T0, eps, t_first=0, dtype=np.float64):
    '''danet_online_scan: the frames t_first .. t_first + T - 1 from `state` -> (attr [B, T, C, E] in float64 holding
    `dtype` values, the state after the last frame).  Steps 1-3 run in `dtype`, step 4 in float64, the new attractor is
    rounded to `dtype`.  Nothing here is fused: the logits and step 4 round the product and the sum separately, where
    the header's rule (and the kernel) uses one fused multiply-add.  In step 4 that is at most one float64 unit in the
    last place per frame, nine orders of magnitude below the bar the kernel is held to.'''
    V, W = np.asarray(V, dtype), np.asarray(W, dtype)
    B, T, F, E = V.shape
    S, n, A = (np.array(x, np.float64) for x in state)
    C = A.shape[1]
    attr = np.empty((B, T, C, E), np.float64)
    for t in range(T):
        m = activation(logits(V[:, t], A, dtype), act)                     # [B, F, C]
        wm = (W[:, t, :, None] * m).astype(dtype)
        s = np.einsum('bfc,bfe->bce', wm, V[:, t]).astype(dtype)
        q = wm.sum(axis=1, dtype=dtype)
        S = lam * S + s.astype(np.float64)
        n = lam * n + q.astype(np.float64)
        if t_first + t >= T0:
            ok = n > eps
            with np.errstate(all='ignore'):
                new = (S / n[..., None]).astype(dtype).astype(np.float64)
            A = np.where(ok[..., None], new, A)
        attr[:, t] = A
    return attr, (S, n, A)


def attractors(V, W, A0, act, lam, T0, eps, dtype=np.float64):
    '''ops.online_attractors: init plus one scan -> attr [B, T, C, E]'''
    return scan(V, W, init(A0), act, lam, T0, eps, 0, dtype)[0]


def separate(V, W, attr, act, dtype=np.float64):
    '''danet_online_separate: out[b][c][t][f] = W[b][t][f] * act(V[b][t][f] . attr[b][t][c]); attr [B, T, C, E]'''
    m = activation(logits(V, attr, dtype), act)                           # [B, T, F, C]
    return np.moveaxis(np.asarray(W, dtype)[..., None] * m, -1, 1).astype(dtype)


def separate_bound(V, W, attr):
    '''the header's ERROR BOUND of danet_online_separate, per element of out [B, C, T, F] (the same for every c):
    |W| (max_c dl_c / 2 + 8 * 2^-24) with dl_c = (E + 1) 2^-24 sum_e |v_e a_e|'''
    V, W, attr = (np.asarray(x, np.float64) for x in (V, W, attr))
    E = V.shape[-1]
    dl = (E + 1) * U * np.einsum('btfe,btce->btfc', np.abs(V), np.abs(attr)).max(axis=-1)
    bound = np.abs(W) * (dl / 2 + 8 * U)
    return np.repeat(bound[:, None], attr.shape[2], axis=1)


# ------------------------------------------------------------------------------------------------ the cases
def clustered_case(B, T, F, E, C, seed=0):
    '''the inputs of a trajectory case: C centres of unit-normal entries per utterance, every bin a centre plus
    0.5 x noise, A0 = the centres plus 0.3 x noise, W = 10 |N(0, 1)|; on such inputs the update contracts
    -> (V [B, T, F, E], W [B, T, F], A0 [B, C, E]) float32'''
    rng = np.random.RandomState(1000 + seed)
    centres = rng.standard_normal((B, C, E))
    which = rng.randint(C, size=(B, T, F))
    V = centres[np.arange(B)[:, None, None], which] + 0.5 * rng.standard_normal((B, T, F, E))
    A0 = centres + 0.3 * rng.standard_normal((B, C, E))
    W = 10 * np.abs(rng.standard_normal((B, T, F)))
    return V.astype(np.float32), W.astype(np.float32), A0.astype(np.float32)


def random_case(B, T, F, E, C, seed=0):
    '''arbitrary data for single-frame calls: unit-normal embeddings and attractors, W = 10 |N(0, 1)|, and a random
    state with S normal and n in [1, 3) -> (V, W float32, state float64 (S, n, A))'''
    rng = np.random.RandomState(2000 + seed)
    V = rng.standard_normal((B, T, F, E)).astype(np.float32)
    W = (10 * np.abs(rng.standard_normal((B, T, F)))).astype(np.float32)
    A = rng.standard_normal((B, C, E)).astype(np.float32).astype(np.float64)
    S = 3 * rng.standard_normal((B, C, E))
    n = 1 + 2 * rng.random_sample((B, C))
    return V, W, (S, n, A)


# (T, F, E, C, lambda, act): the trajectory cases of the input condition (CPU) -- T0 = 8 throughout
TRAJECTORY_CASES = [
    (70, 3, 2, 2, 1.0, 0), (70, 3, 2, 2, 0.5, 1), (200, 33, 8, 2, 0.95, 1), (70, 129, 20, 2, 1.0, 1),
    (70, 257, 20, 2, 0.95, 0), (200, 65, 40, 3, 0.5, 0), (70, 65, 40, 3, 1.0, 1), (70, 17, 5, 4, 0.95, 0)]
T0 = 8
EPS = 1e-7
# (F, E, C, act) of the GPU trajectory cases, taken in turn over the T x B x lambda grid
TRAJECTORY_SHAPES = [(3, 2, 2, 0), (257, 20, 2, 1), (65, 40, 3, 0), (129, 20, 2, 0), (33, 7, 4, 1), (65, 64, 4, 1)]
TRAJECTORY_T = (1, 2, T0 - 1, T0, T0 + 1, 70)
TRAJECTORY_B = (1, 3, 33)
TRAJECTORY_LAMBDA = (1.0, 0.95, 0.5)
# the F x E x C set of the single-frame and separator cases
SHAPE_F = (1, 3, 63, 64, 65, 129, 256, 257, 513, 1025)
SHAPE_E = (1, 2, 20, 40, 64)
SHAPE_C = (1, 2, 3, 4)
BAR = 1e-5                                            # of each output's maximum (test_gpu_lstm_envelope.py's bar)
