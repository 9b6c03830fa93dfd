'''
Restatement of include/danet_causal_hip.h (THE RULE) in numpy, with the element type as a parameter: the causal
centring and its adjoint, the LSTM block from carried state, the projection and the whole `lstm-causal` encoder.
Test infrastructure only, shared by tests/test_causal_cpu.py and tests/test_gpu_causal.py.

dtype = np.float64 is the reference the kernels are held against; dtype = np.float32 is the "float32 restatement":
the same formulas with every product, sum and activation rounded to float32 (the row sums and the running sum of the
centring stay float64, as the rule has them), in numpy's own summation order -- its distance from the float64 run
shows what plain float32 rounding does to a case, whatever the order.  encoder_torch is the float64 twin of `encoder`
on torch tensors, for autograd.
'''
import numpy as np

BAR = 1e-5             # LSTM block, embedding: of each output's maximum (the bar of tests/test_gpu_lstm_envelope.py)
F32_BAR = 1e-5         # the float32 restatement against float64 on the GPU test's own LSTM cases (the input condition)
MAX_B, MAX_TB, MAX_H, MAX_D0, MAX_L, MAX_M = 16, 64, 608, 1028, 8, 1024
MAX_T, MAX_D = 65536, 4096
MAX_K = MAX_D0 + MAX_H

# the GPU test's LSTM block cases: (L, H, D0, B, Tb); every value of every axis of the issue's grid at least once, the
# large-H cases at Tb <= 5 only
LSTM_CASES = [(1, 4, 1, 1, 1), (1, 4, 1, 3, 2), (1, 4, 1, 16, 64), (2, 8, 33, 1, 64), (2, 8, 33, 3, 5), (2, 8, 33, 16, 2),
              (3, 64, 129, 1, 5), (3, 64, 129, 3, 64), (3, 64, 129, 16, 1), (1, 600, 257, 1, 2), (1, 600, 257, 3, 1),
              (1, 600, 257, 16, 5), (2, 608, 600, 1, 1), (2, 608, 600, 3, 5), (2, 608, 600, 16, 2), (8, 12, 5, 1, 5),
              (8, 12, 5, 3, 64), (8, 12, 5, 16, 2)]
CENTER_B, CENTER_T, CENTER_D = (1, 3, 33), (1, 2, 7, 64, 65, 300), (1, 3, 129, 600, 608)
PROJECT_M, PROJECT_KN = (1, 5, 16, 17, 1024), ((8, 33), (600, 2580), (608, 5140))


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


# ------------------------------------------------------------------------------------------ rule 1
def center_fwd(x, state=None, dtype=np.float64):
    '''x [B, T, D] -> (out [B, T, D] of `dtype`, mu [B, T] of `dtype`, the state after float64 [B, 2]); state float64
    [B, 2] = (S, n) or None = a fresh utterance.  The row sums and S are float64 whatever dtype.'''
    x = np.asarray(x)
    B, T, D = x.shape
    state = np.zeros((B, 2)) if state is None else np.array(state, np.float64)
    r = x.astype(np.float64).sum(axis=2)
    mu = np.empty((B, T), dtype)
    S, n = state[:, 0].copy(), state[:, 1].copy()
    for t in range(T):
        S = S + r[:, t]
        n = n + 1
        mu[:, t] = (S / (n * D)).astype(dtype)
    out = x.astype(dtype) - mu[:, :, None]
    return out, mu, np.stack([S, n], axis=1)


def center_bwd(g, dtype=np.float64):
    '''the adjoint of center_fwd over a whole utterance from a zero state: g [B, T, D] -> (din [B, T, D], s [B, T])'''
    g = np.asarray(g)
    B, T, D = g.shape
    r = g.astype(np.float64).sum(axis=2)
    s = np.empty((B, T), dtype)
    acc = np.zeros(B)
    for t in range(T - 1, -1, -1):
        acc = acc + r[:, t] / ((t + 1.0) * D)
        s[:, t] = acc.astype(dtype)
    return g.astype(dtype) - s[:, :, None], s


# ------------------------------------------------------------------------------------------ rules 2 and 3
def project(A, W, dtype=np.float64):
    return np.asarray(A, dtype) @ np.asarray(W, dtype)


def lstm_block(x, Ws, bs, h, c, dtype=np.float64):
    '''x [Tb, B, D0]; Ws[l] [D_l + H, 4H]; bs[l] [4H]; h, c [L, B, H] -> (y [Tb, B, H], h after, c after), all of
    `dtype`; gate order g | i | f | o, g linear'''
    cur = np.asarray(x, dtype)
    h, c = np.array(h, dtype), np.array(c, dtype)
    H = h.shape[2]
    for l, (W, b) in enumerate(zip(Ws, bs)):
        W, b = np.asarray(W, dtype), np.asarray(b, dtype)
        ys = np.empty(cur.shape[:2] + (H,), dtype)
        hl, cl = h[l], c[l]
        for t in range(cur.shape[0]):
            a = np.concatenate([cur[t], hl], axis=1) @ W + b
            g, i, f, o = a[:, :H], sigmoid(a[:, H:2 * H]), sigmoid(a[:, 2 * H:3 * H]), sigmoid(a[:, 3 * H:])
            cl = (i * g + f * cl).astype(dtype)
            hl = (o * np.tanh(cl)).astype(dtype)
            ys[t] = hl
        h[l], c[l] = hl, cl
        cur = ys
    return cur, h, c


def encoder(x, Ws, bs, Wout, dtype=np.float64):
    '''the whole `lstm-causal` encoder from a zero state: x [B, T, F] -> embed [B, T, Wout.shape[1]]'''
    B = x.shape[0]
    H = Ws[0].shape[1] // 4
    xc = center_fwd(x, None, dtype)[0]
    z = np.zeros((len(Ws), B, H), dtype)
    y = lstm_block(xc.transpose(1, 0, 2), Ws, bs, z, z, dtype)[0].transpose(1, 0, 2)
    return project(center_fwd(y, None, dtype)[0], Wout, dtype)


def encoder_torch(x, Ws, bs, Wout):
    '''`encoder` in float64 on torch tensors (autograd)'''
    import torch

    def centre(v):
        B, T, D = v.shape
        n = torch.arange(1, T + 1, dtype=v.dtype)[None, :] * D
        return v - (torch.cumsum(v.sum(dim=2), dim=1) / n)[:, :, None]

    cur = centre(x).transpose(0, 1)
    H = Ws[0].shape[1] // 4
    for W, b in zip(Ws, bs):
        h = cur.new_zeros(cur.shape[1], H)
        c = cur.new_zeros(cur.shape[1], H)
        ys = []
        for t in range(cur.shape[0]):
            a = torch.cat([cur[t], h], dim=1) @ W + b
            g, i, f, o = a[:, :H], torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c = i * g + f * c
            h = o * torch.tanh(c)
            ys.append(h)
        cur = torch.stack(ys)
    return centre(cur.transpose(0, 1)) @ Wout


# ------------------------------------------------------------------------------------------ inputs
def f32(a):
    return np.asarray(a, np.float32)


def lstm_case(L, H, D0, B, Tb, seed=None, sat=False):
    '''float32 inputs of an LSTM block case with a RANDOM carried state: dict(x [Tb, B, D0], Ws, bs, h, c)'''
    rng = np.random.RandomState(seed if seed is not None else L * 1009 + H * 101 + D0 * 13 + B * 7 + Tb)
    r = 1.5 / np.sqrt(H)
    Ws, bs, D = [], [], D0
    for _ in range(L):
        Ws.append(f32(rng.uniform(-r, r, size=(D + H, 4 * H))))
        b = np.zeros(4 * H)
        b[H:2 * H], b[2 * H:3 * H], b[3 * H:] = 1.5, -1.0, 1.0
        b = b + rng.randn(4 * H) * 0.1
        if sat:
            b = b + rng.choice([-30.0, 0.0, 30.0], size=4 * H)
        bs.append(f32(b))
        D = H
    return dict(x=f32(rng.randn(Tb, B, D0) * 0.7), Ws=Ws, bs=bs, h=f32(rng.uniform(-0.8, 0.8, size=(L, B, H))),
                c=f32(rng.randn(L, B, H)))


def relmax(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))
