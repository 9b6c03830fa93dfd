'''
The rule of include/danet_dpcl_hip.h restated in float64 numpy (one utterance at a time), the literal N x N loss in
torch float64 for the restatement's own check, and the stats pass's float32 order for orientation.

    embed    [N, E]   (any float dtype; taken as it is)
    src_pwr  [C, N]   float32: labels and weights compare and add THESE values
'''
import numpy as np

MAX_CHUNKS = 16          # DANET_DPCL_MAX_CHUNKS
TILE_ROWS = 128          # DANET_DPCL_TILE_ROWS
MAX_E, MAX_C = 64, 4


def chunk_rows(N):
    return TILE_ROWS * -(-(-(-N // MAX_CHUNKS)) // TILE_ROWS)


def chunks(N):
    return -(-N // chunk_rows(N))


def workspace_bytes(B, N, E, C):
    return B * chunks(N) * (E + 1) * (E + C + 1) * 4


def labels(src_pwr):
    '''the lowest c with src_pwr[c, i] = max_c src_pwr[c, i] (np.argmax returns the first maximum)'''
    return np.argmax(np.asarray(src_pwr), axis=0)


def sums(src_pwr):
    '''s_i = sum_c S_ci in float64 (exact for C <= 4 float32 values up to the last bit of the float32 sum)'''
    return np.asarray(src_pwr, np.float64).sum(axis=0)


def weights(src_pwr):
    s = sums(src_pwr)
    tot = s.sum()
    return s / tot if tot > 0 else np.zeros_like(s)


def stats(embed, src_pwr):
    '''-> dict(y, w, A [E, E], Bm [E, C], c [C], S) of one utterance'''
    V = np.asarray(embed, np.float64)
    C = np.asarray(src_pwr).shape[0]
    y, w = labels(src_pwr), weights(src_pwr)
    Y = np.eye(C)[y]                                     # [N, C]
    A = (V * w[:, None]).T @ V
    Bm = (V * w[:, None]).T @ Y
    c = w @ Y
    return dict(y=y, w=w, A=A, Bm=Bm, c=c, S=float(sums(src_pwr).sum()))


def loss_of(st):
    return float((st['A'] ** 2).sum() - 2.0 * (st['Bm'] ** 2).sum() + (st['c'] ** 2).sum())


def term_size(st):
    '''||A||^2 + 2 ||Bm||^2 + sum c^2: the size of the terms of L_b, not of the possibly cancelled result'''
    return float((st['A'] ** 2).sum() + 2.0 * (st['Bm'] ** 2).sum() + (st['c'] ** 2).sum())


def utterance(embed, src_pwr):
    '''-> (L_b, dL_b / dV [N, E], stats)'''
    V = np.asarray(embed, np.float64)
    st = stats(V, src_pwr)
    g = 4.0 * st['w'][:, None] * (V @ st['A'].T - st['Bm'][:, st['y']].T)
    return loss_of(st), g, st


def batch(embed, src_pwr, main=0.0, alpha=1.0, dloss=1.0):
    '''embed [B, N, E], src_pwr [B, C, N] -> dict(per_utt [B], dpcl, total, dembed [B, N, E], stats [B])'''
    B = len(embed)
    res = [utterance(embed[b], src_pwr[b]) for b in range(B)]
    per = np.array([r[0] for r in res])
    dpcl = per.sum() / B
    return dict(per_utt=per, dpcl=dpcl, total=float(main) + alpha * dpcl,
                dembed=np.stack([r[1] for r in res]) * (dloss * alpha / B), stats=[r[2] for r in res])


def grad_bar(embed, st):
    '''max_i 4 w_i (sum_f |A_ef v_if| + |Bm_e,y_i|): the size of the gradient's terms (over i and e)'''
    V = np.abs(np.asarray(embed, np.float64))
    t = V @ np.abs(st['A']).T + np.abs(st['Bm'][:, st['y']].T)
    return float((4.0 * st['w'][:, None] * t).max()) if t.size else 0.0


def literal(embed, src_pwr):
    '''torch float64 autograd of || W^1/2 (V V^T - Y Y^T) W^1/2 ||_F^2 with the N x N matrices -> (loss, grad)'''
    import torch
    V = torch.tensor(np.asarray(embed, np.float64), requires_grad=True)
    C = np.asarray(src_pwr).shape[0]
    Y = torch.tensor(np.eye(C)[labels(src_pwr)])
    r = torch.tensor(np.sqrt(weights(src_pwr)))
    D = (V @ V.T - Y @ Y.T) * r[:, None] * r[None, :]
    L = (D ** 2).sum()
    L.backward()
    return float(L.detach()), V.grad.numpy()


def stats_f32(embed, src_pwr):
    '''the unnormalised sums in the stats pass's float32 order, simplified: a tile of 128 rows in float32 (numpy's
    own order inside the tile), tiles and chunks in float64 -> (G_A [E, E], G_B [E, C], G_c [C], S) normalised'''
    V = np.asarray(embed, np.float32)
    sp = np.asarray(src_pwr, np.float32)
    C, N = sp.shape
    y = labels(sp)
    s = sp[0].copy()
    for c in range(1, C):
        s = s + sp[c]
    Q = np.concatenate([V, np.eye(C, dtype=np.float32)[y]], axis=1)
    P = np.concatenate([V * s[:, None], s[:, None]], axis=1)
    G = np.zeros((P.shape[1], Q.shape[1]), np.float64)
    for n0 in range(0, N, TILE_ROWS):
        G += (P[n0:n0 + TILE_ROWS].T @ Q[n0:n0 + TILE_ROWS]).astype(np.float64)
    E = V.shape[1]
    S = float(s.astype(np.float64).sum())
    if S <= 0:
        return np.zeros((E, E)), np.zeros((E, C)), np.zeros(C), 0.0
    return G[:E, :E] / S, G[:E, E:] / S, G[E, E:] / S, S
