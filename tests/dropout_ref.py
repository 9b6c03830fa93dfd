'''
Restatement of the dropout mask contract (include/danet_dropout_hip.h) in numpy, and the float64
torch-CPU encoders / model steps with those masks injected where the reference's graph has
`tf.nn.dropout` (app/modules.py:137: behind the concatenation of every `_lyr_bilstm`) -- the
authority the dropout tests compare with.  Test infrastructure only; wraps the restatements that
exist (oracle/torch_ref.py, tests/conv_ref.py) and changes none of them.
'''
import contextlib

import numpy as np
import torch

from oracle import torch_ref as R

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xffffffff


def philox4x32_10(ctr, key):
    '''ctr: 4 uint32 arrays (or ints) of one shape, key: 2 ints -> [4, ...] uint32 output words'''
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)
        p1 = c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c).astype(np.uint32)


def threshold_of(keep):
    '''min(2^32 - 1, floor(keep * 2^32)), in exact integer arithmetic on the double's value'''
    from fractions import Fraction
    return min(MASK32, int(Fraction(float(keep)) * (1 << 32)))


def scale_of(keep):
    return np.float32(np.float64(1.0) / np.float64(keep))


def words(n, key0, key1, stream_id, step):
    '''the 32-bit word of each of the logical elements 0..n-1'''
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((g & np.uint64(MASK32), g >> np.uint64(32), stream_id, step), (key0, key1))
    return w.T.reshape(-1)[:n]                 # element e = 4 g + j <- word j of group g


def keep_mask(rows, cols, threshold, key0, key1, stream_id, step):
    '''bool [rows, cols]: element kept'''
    return (words(rows * cols, key0, key1, stream_id, step) < np.uint32(threshold)).reshape(rows, cols)


def apply_np(x, threshold, scale, key0, key1, stream_id, step):
    '''float32 [rows, cols] -> what danet_dropout_apply writes'''
    m = keep_mask(x.shape[0], x.shape[1], threshold, key0, key1, stream_id, step)
    return np.where(m, x * np.float32(scale), np.float32(0)).astype(np.float32)


class Spec(object):
    '''the mask source of one model step, as ops.DropoutSpec derives it'''

    def __init__(self, keep, key0=0, key1=0, step=0):
        self.keep, self.key0, self.key1, self.step = keep, key0, key1, step
        self.threshold, self.scale = threshold_of(keep), scale_of(keep)

    def factor(self, stream_id, T, B, W):
        '''float64 tensor [B, T, W]: scale (as the float32 the kernel multiplies by) where kept, 0 where
        dropped; the mask is indexed over the TIME-MAJOR [T][B][W] buffer the kernels work on'''
        m = keep_mask(T * B, W, self.threshold, self.key0, self.key1, stream_id, self.step)
        f = m.reshape(T, B, W).astype(np.float64) * np.float64(self.scale)
        return torch.tensor(f).transpose(0, 1)


def bilstm_layer(x, Wf, bf, Wb, bb, H, spec, stream_id):
    '''_lyr_bilstm, app/modules.py:120-137, batch-major [B, T, D] -> [B, T, 2H]'''
    y = torch.cat([R.lstm_scan(x, Wf, bf, H), R.lstm_scan(x, Wb, bb, H, reverse=True)], dim=-1)
    if spec is not None and spec.keep < 1:
        y = y * spec.factor(stream_id, y.shape[1], y.shape[0], 2 * H)
    return y


def bilstm_encoder(x, params, H, L, E, spec):
    '''oracle.torch_ref.bilstm_encoder with layer l's output dropped by stream l'''
    B, T, F = x.shape
    x = x - x.mean(dim=(1, 2), keepdim=True)
    for l in range(L):
        p = 'global/encoder/lstm%d_%s/LSTM/linear/%s'
        x = bilstm_layer(x, params[p % (l, 'fwd', 'W')], params[p % (l, 'fwd', 'B')],
                         params[p % (l, 'bwd', 'W')], params[p % (l, 'bwd', 'B')], H, spec, l)
    y = x - x.mean(dim=(1, 2), keepdim=True)
    return (y @ params['global/encoder/output/W']).reshape(B, T, F, E)


@contextlib.contextmanager
def _patched(obj, name, fn):
    old = getattr(obj, name)
    setattr(obj, name, fn)
    try:
        yield
    finally:
        setattr(obj, name, old)


def model_forward(src, params, cfg, spec):
    '''oracle.torch_ref.model_forward (bilstm-orig) with the masked encoder in place of its own'''
    assert cfg.get('encoder', 'bilstm-orig') == 'bilstm-orig'
    with _patched(R, 'bilstm_encoder', lambda x, p, H, L, E: bilstm_encoder(x, p, H, L, E, spec)):
        return R.model_forward(src, params, cfg)


def conv_model_forward(src, params, cfg, spec):
    '''tests/conv_ref.model_forward with both BiLSTM layers of the conv-bilstm-v1 encoder dropped:
    conv_ref.encoder concatenates the two scans of a layer with torch.cat(dim=-1) and nothing else
    does, so the mask rides on that call (layer index = call index)'''
    import conv_ref
    calls = [0]
    real_cat = torch.cat

    def cat(ts, dim=0):
        y = real_cat(ts, dim=dim)
        if dim == -1 and len(ts) == 2:
            y = y * spec.factor(calls[0], y.shape[1], y.shape[0], y.shape[2])
            calls[0] += 1
        return y

    with _patched(conv_ref.torch, 'cat', cat):
        out = conv_ref.model_forward(src, params, cfg)
    assert calls[0] == 2, calls
    return out
