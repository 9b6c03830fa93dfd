'''
GPU tests of the causal encoder and block-wise streaming inference (libdanet_causal_hip.so,
include/danet_causal_hip.h) against the float64 restatement of tests/causal_ref.py.  Every output and every state lies
between poisoned guard bands; the gaps of padded leading dimensions hold a NaN on the input side and must keep their
poison on the output side wherever the rule does not write.

(a) the causal centring, forward and adjoint, within the header's derived bound 2^-23 (|x| + |mu|) on every written
element, over B x T x D x the four layout pairs; bit for bit: cuts, rows of a batch, repeats; (b) the LSTM block from a
RANDOM carried state within 1e-5 of each output's maximum (causal_ref.BAR, the bar of test_gpu_lstm_envelope.py;
test_causal_cpu.py shows that the float32 restatement alone stays within 1e-5 on these cases), bit for bit over cuts,
rows and repeats; (c) the projection within (K + 1) 2^-24 sum_k |a_k w_k|, row r bit-identical whatever M; (d) the
`lstm-causal` encoder: embedding, causality on the device, one train step's gradients, training, parameter files;
(e) the session: block sizes, the hold, flush, reset, batches, INFER_STREAM_BLOCK, the demo mode; (f) the untouched path.

Measured on an MI355X (this file's prints; also in README, "Streaming inference"): centring forward at most 0.95 and
adjoint 0.96 of the derived bound, adjoint identity to 5.0e-7; LSTM block at most 4.8e-7 of an output's maximum where
the float32 restatement reaches 1.4e-6; projection at most 0.25 of its bound; embedding 2.3e-7; worst gradient 1.0e-6;
session embedding 2.0e-7 and infer's 2.2e-7 of float64, 2.6e-7 of each other.

The gradient bar of (d) is TOL = 1e-4 of each gradient's maximum, the bar of the BiLSTM encoder's gradient tests in
tests/test_gpu_lstm.py (gpu_helpers.TOL; the whole-model successor gpu_helpers.train_step_vs_oracle allows 2e-4 at full
size, which this small model does not need).

The adjoint identity of (a), "to 1e-5 relative": relative to sum |fwd(x) g|, the sum of the magnitudes of the terms of
the inner product, not to the inner product itself -- on random data the inner product cancels to about 1 / sqrt(B T D)
of that sum, so that its own relative error says how much it cancelled, not how well the kernels agree.

flush() against infer with the key null is asserted to FLUSH_BAR = 2e-5 of the output's maximum, the bar the issue sets
between the session's embedding and infer's: the two paths differ in the embedding only (A0 and the separator are the
same calls on it), A0 is a weighted mean of embedding rows, a logit is an E-term product of an embedding row and an
attractor, both of order one here, and the softmax moves by at most half the largest logit change, so the relative
change of |out| = |mix| * mask is of the order of the embedding's.  (The anchor estimator also picks one of its anchor
subsets by an argmin; two embeddings 2e-5 apart pick the same one unless two subsets tie to that precision.)
'''
import io
import json
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

import causal_ref as CR
import online_ref as OR
from gpu_helpers import ROOT, TOL, check_lstm_status, cfg_of, oracle_step, oracle_threads, relerr

pytestmark = pytest.mark.gpu

POISON = -7.25e33
GUARD = 1024
EPS23, EPS24 = 2.0 ** -23, 2.0 ** -24
FLUSH_BAR = 2e-5       # flush() against infer with the key null, of the output's maximum (the module docstring)


def _guarded(shape, dtype=torch.float32, fill=None):
    '''(whole buffer, the view of `shape` in its middle): everything poisoned, or the middle set to `fill`'''
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=dtype, device='cuda')
    view = buf[GUARD:GUARD + n].view(tuple(shape))
    if fill is not None:
        view.copy_(torch.as_tensor(np.ascontiguousarray(fill)).to(dtype))
    return buf, view


def _intact(*bufs):
    return all(bool((b[:GUARD] == POISON).all()) and bool((b[-GUARD:] == POISON).all()) for b in bufs)


def _cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------ (a) the centring
def _laid_out(x, layout, ld):
    '''x [B, T, D] float32 -> a device buffer [rows, ld] in `layout` (0 batch-major, 1 time-major), NaN in the gaps'''
    B, T, D = x.shape
    rows = x if layout == 0 else x.transpose(1, 0, 2)
    buf = torch.full((B * T, ld), float('nan'), device='cuda')
    buf[:, :D] = _cu(rows.reshape(B * T, D))
    return buf


def _read_back(view, B, T, D, layout):
    '''(the [B, T, D] columns, the [B, T, ld - D] gap) of an output buffer [rows, ld] in `layout`'''
    a = view.cpu().numpy()
    a = a.reshape(B, T, -1) if layout == 0 else a.reshape(T, B, -1).transpose(1, 0, 2)
    return a[:, :, :D], a[:, :, D:]


def _center(x, lin, lout, state=None, bwd=False, pad=(3, 5)):
    '''one centring launch on x [B, T, D]: forward from the numpy state [B, 2] (None: zeros) or the adjoint ->
    (out [B, T, D], the gap columns, the state after or None); guard bands checked'''
    from danet_amd import ops
    B, T, D = x.shape
    ldi, ldo = D + pad[0], D + pad[1]
    src = _laid_out(x, lin, ldi)
    obuf, out = _guarded((B * T, ldo))
    if bwd:
        ops.causal_center_bwd(src, B, T, D, lin, ldi, out, lout, ldo)
        torch.cuda.synchronize()
        assert _intact(obuf)
        return _read_back(out, B, T, D, lout) + (None,)
    sbuf, st = _guarded((B, 2), torch.float64, np.zeros((B, 2)) if state is None else state)
    ops.causal_center_fwd(src, B, T, D, lin, ldi, out, lout, ldo, st)
    torch.cuda.synchronize()
    assert _intact(obuf, sbuf)
    return _read_back(out, B, T, D, lout) + (st.cpu().numpy(),)


def _center_input(B, T, D, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((B, T, D)) * 2 + rng.standard_normal((B, 1, 1)) * 3).astype(np.float32)


@pytest.mark.parametrize('D', CR.CENTER_D)
def test_center_forward_against_float64_within_the_derived_bound(D):
    worst = 0.0
    for B in CR.CENTER_B:
        for T in CR.CENTER_T:
            x = _center_input(B, T, D, B * 1000 + T * 10 + D)
            want, mu, wstate = CR.center_fwd(x)
            bound = EPS23 * (np.abs(x) + np.abs(mu)[:, :, None])
            for lin in (0, 1):
                for lout in (0, 1):
                    got, gap, state = _center(x, lin, lout)
                    ratio = float((np.abs(got - want) / bound).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1, (B, T, D, lin, lout, ratio)
                    assert not gap.any() and not np.signbit(gap).any()           # the pad columns are zero-filled
                    assert np.array_equal(state[:, 1], np.full(B, T))
                    assert np.abs(state[:, 0] - wstate[:, 0]).max() <= 1e-12 * np.abs(x.astype(np.float64)).sum(axis=(1, 2)).max()
    print('centring forward D %d: worst error %.3g of the derived bound' % (D, worst))


@pytest.mark.parametrize('D', CR.CENTER_D)
def test_center_backward_against_float64_and_the_adjoint_identity(D):
    worst, worst_adj = 0.0, 0.0
    for B in CR.CENTER_B:
        for T in CR.CENTER_T:
            g = _center_input(B, T, D, B * 1000 + T * 10 + D + 1)
            x = _center_input(B, T, D, B * 1000 + T * 10 + D)
            want, s = CR.center_bwd(g)
            bound = EPS23 * (np.abs(g) + np.abs(s)[:, :, None])
            fwd = _center(x, 0, 0)[0].astype(np.float64)
            for lin in (0, 1):
                for lout in (0, 1):
                    got, gap, _ = _center(g, lin, lout, bwd=True)
                    ratio = float((np.abs(got - want) / bound).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1, (B, T, D, lin, lout, ratio)
                    assert (gap == np.float32(POISON)).all()                    # the adjoint writes the columns < D only
            # <fwd(x), g> = <x, bwd(g)> on the kernels' own outputs, relative to sum |fwd(x) g| (the module docstring
            # says why not to the inner product itself)
            # (T = 1, D = 1: fwd(x) is exactly zero and so is bwd(g); both sides are 0)
            lhs, rhs, scale = (fwd * g).sum(), (x.astype(np.float64) * got).sum(), np.abs(fwd * g).sum()
            assert abs(lhs - rhs) <= 1e-5 * scale, (B, T, D, lhs, rhs, scale)
            if scale > 0:
                worst_adj = max(worst_adj, abs(lhs - rhs) / scale)
    print('centring backward D %d: worst error %.3g of the derived bound, adjoint identity to %.3g' % (D, worst, worst_adj))


@pytest.mark.parametrize('B,T,D,lin,lout', [(3, 300, 129, 0, 1), (2, 70, 600, 1, 0), (1, 130, 3, 0, 0)])
def test_cut_centrings_equal_the_whole_bit_for_bit(B, T, D, lin, lout):
    x = _center_input(B, T, D, 5)
    whole, _, end = _center(x, lin, lout)
    again, _, end_again = _center(x, lin, lout)
    assert _same(whole, again) and _same(end, end_again)                          # repeated calls agree
    for cut in (1, 7, 64):
        a, _, mid = _center(x[:, :cut], lin, lout)
        b, _, end2 = _center(x[:, cut:], lin, lout, state=mid)
        assert _same(np.concatenate([a, b], axis=1), whole) and _same(end2, end), cut
    a, _, s1 = _center(x[:, :9], lin, lout)
    b, _, s2 = _center(x[:, 9:10], lin, lout, state=s1)
    c, _, s3 = _center(x[:, 10:], lin, lout, state=s2)
    assert _same(np.concatenate([a, b, c], axis=1), whole) and _same(s3, end)
    # the adjoint: repeats agree too
    assert _same(_center(x, lin, lout, bwd=True)[0], _center(x, lin, lout, bwd=True)[0])


def test_a_centred_row_alone_equals_the_row_inside_a_launch_of_33():
    B, T, D = 33, 65, 129
    x = _center_input(B, T, D, 33)
    whole, _, end = _center(x, 0, 1)
    back = _center(x, 1, 0, bwd=True)[0]
    for b in (0, 7, 32):
        one, _, end1 = _center(x[b:b + 1], 0, 1)
        assert _same(one[0], whole[b]) and _same(end1[0], end[b]), b
        assert _same(_center(x[b:b + 1], 1, 0, bwd=True)[0][0], back[b]), b


def test_center_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    B, T, D = 2, 5, 7
    src = _laid_out(_center_input(B, T, D, 0), 0, D)
    obuf, out = _guarded((B * T, D))
    sbuf, st = _guarded((B, 2), torch.float64, np.ones((B, 2)))
    for kw in (dict(T=0), dict(D=0), dict(lin=2), dict(lout=3), dict(ldi=D - 1), dict(ldo=D - 1)):
        a = dict(dict(T=T, D=D, lin=0, ldi=D, lout=0, ldo=D), **kw)
        with pytest.raises(_lib.DanetHipError) as e:
            ops.causal_center_fwd(src, B, a['T'], a['D'], a['lin'], a['ldi'], out, a['lout'], a['ldo'], st)
        assert 'libdanet_causal_hip error -1: center_fwd: ' in str(e.value), kw
        with pytest.raises(_lib.DanetHipError) as e:
            ops.causal_center_bwd(src, B, a['T'], a['D'], a['lin'], a['ldi'], out, a['lout'], a['ldo'])
        assert 'libdanet_causal_hip error -1: center_bwd: ' in str(e.value), kw
    torch.cuda.synchronize()
    assert bool((obuf == POISON).all()) and _intact(sbuf) and bool((st == 1).all())


# ------------------------------------------------------------------------------------ (b) the LSTM block
def _lstm(d, x=None, h=None, c=None, pad=(3, 5)):
    '''one danet_causal_lstm_block on the inputs of causal_ref.lstm_case (x, h, c overridable) -> (y [Tb, B, H], h, c
    after) read back; NaN in the gap of x, poisoned ws, guards around y, h, c and ws, poison kept in the gap of y'''
    from danet_amd import ops
    x = d['x'] if x is None else x
    h0 = d['h'] if h is None else h
    c0 = d['c'] if c is None else c
    Tb, B, D0 = x.shape
    L, _, H = h0.shape
    ldx, ldy = D0 + pad[0], H + pad[1]
    xb = torch.full((Tb, B, ldx), float('nan'), device='cuda')
    xb[:, :, :D0] = _cu(x)
    Ws, bs = [_cu(W) for W in d['Ws']], [_cu(b) for b in d['bs']]
    hbuf, hv = _guarded((L, B, H), fill=h0)
    cbuf, cv = _guarded((L, B, H), fill=c0)
    ybuf, yv = _guarded((Tb, B, ldy))
    n = ops.causal_lstm_ws_bytes(L, B, Tb, H) // 4
    wbuf = torch.full((n + 2 * GUARD,), float('nan'), device='cuda')
    wbuf[:GUARD] = POISON
    wbuf[-GUARD:] = POISON
    got = ops.causal_lstm_block(xb, ldx, D0, Ws, bs, hv, cv, y=yv, ldy=ldy, ws=wbuf[GUARD:GUARD + n])
    assert got is yv
    torch.cuda.synchronize()
    assert _intact(hbuf, cbuf, ybuf, wbuf)
    y = yv.cpu().numpy()
    assert (y[:, :, H:] == np.float32(POISON)).all()
    return y[:, :, :H], hv.cpu().numpy(), cv.cpu().numpy()


@pytest.mark.parametrize('case', range(len(CR.LSTM_CASES)))
def test_lstm_block_from_a_random_state_against_float64(case):
    L, H, D0, B, Tb = CR.LSTM_CASES[case]
    d = CR.lstm_case(L, H, D0, B, Tb)
    got = _lstm(d)
    r64 = CR.lstm_block(d['x'], d['Ws'], d['bs'], d['h'], d['c'])
    r32 = CR.lstm_block(d['x'], d['Ws'], d['bs'], d['h'], d['c'], np.float32)
    errs = [CR.relmax(a, b) for a, b in zip(got, r64)]
    f32 = [CR.relmax(a, b) for a, b in zip(r32, r64)]
    print('LSTM block L %d H %d D0 %d B %d Tb %d: kernel y %.3g h %.3g c %.3g, float32 restatement %.3g %.3g %.3g, '
          'worst ratio %.2f' % ((L, H, D0, B, Tb) + tuple(errs) + tuple(f32) + (max(e / max(f, 1e-30) for e, f in zip(errs, f32)),)))
    assert all(np.isfinite(a).all() for a in got)
    assert max(errs) <= CR.BAR, errs
    assert _same(got[1][-1], got[0][-1])                      # the top layer's state is its last output
    assert np.abs(got[1] - d['h']).max() > 1e-3


@pytest.mark.parametrize('L,H,D0,B', [(2, 8, 33, 3), (3, 64, 129, 16), (8, 12, 5, 1)])
def test_cut_lstm_blocks_equal_the_whole_bit_for_bit(L, H, D0, B):
    d = CR.lstm_case(L, H, D0, B, 64)
    whole = _lstm(d)
    again = _lstm(d)
    assert all(_same(a, b) for a, b in zip(whole, again))                        # repeated calls agree
    for cuts in ((1, 7, 56), (1,) * 64):
        ys, h, c, t = [], d['h'], d['c'], 0
        for n in cuts:
            y, h, c = _lstm(d, x=d['x'][t:t + n], h=h, c=c)
            ys.append(y)
            t += n
        assert _same(np.concatenate(ys), whole[0]) and _same(h, whole[1]) and _same(c, whole[2]), cuts[:3]


@pytest.mark.parametrize('L,H,D0,Tb', [(2, 8, 33, 5), (1, 600, 257, 2), (3, 64, 129, 64)])
def test_an_lstm_row_alone_equals_the_row_among_16(L, H, D0, Tb):
    d = CR.lstm_case(L, H, D0, 16, Tb)
    whole = _lstm(d)
    for b, n in ((0, 1), (5, 1), (15, 1), (4, 3)):             # rows alone (B = 1) and three rows (the B <= 4 kernel)
        y, h, c = _lstm(d, x=d['x'][:, b:b + n], h=d['h'][:, b:b + n], c=d['c'][:, b:b + n])
        assert _same(y, whole[0][:, b:b + n]) and _same(h, whole[1][:, b:b + n]) and _same(c, whole[2][:, b:b + n]), (b, n)


def test_saturated_gates_stay_finite():
    for L, H, D0, B, Tb in ((2, 8, 33, 3, 5), (1, 600, 257, 16, 2)):
        d = CR.lstm_case(L, H, D0, B, Tb, sat=True)
        got = _lstm(d)
        r64 = CR.lstm_block(d['x'], d['Ws'], d['bs'], d['h'], d['c'])
        assert all(np.isfinite(a).all() for a in got)
        assert max(CR.relmax(a, b) for a, b in zip(got, r64)) <= CR.BAR


def test_lstm_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    d = CR.lstm_case(2, 8, 33, 3, 5)
    Ws, bs = [_cu(W) for W in d['Ws']], [_cu(b) for b in d['bs']]
    hbuf, hv = _guarded((2, 3, 8), fill=d['h'])
    cbuf, cv = _guarded((2, 3, 8), fill=d['c'])
    ybuf, yv = _guarded((5, 3, 8))
    x = _cu(d['x'])
    with pytest.raises(_lib.DanetHipError) as e:
        ops.causal_lstm_block(x, 33, 33, Ws, bs, hv, cv, y=yv, ldy=8, ws=torch.empty(2 * 3 * 5 * 8 - 1, device='cuda'))
    assert 'lstm_block: workspace too small' in str(e.value)
    with pytest.raises(_lib.DanetHipError):
        ops.causal_lstm_block(x, 33, 33, Ws, bs, hv, cv, y=yv, ldy=7)
    wp = (_lib.c_p * 2)(Ws[0].data_ptr(), Ws[1].data_ptr() + 4)
    bp = (_lib.c_p * 2)(*[b.data_ptr() for b in bs])
    ws = torch.empty(2 * 3 * 5 * 8, device='cuda')
    assert _lib.load_causal().danet_causal_lstm_block(_lib.stream(), 2, 3, 5, 33, 8, x.data_ptr(), 33, wp, bp, hv.data_ptr(),
                                                     cv.data_ptr(), yv.data_ptr(), 8, ws.data_ptr(), ws.numel() * 4) == -1
    torch.cuda.synchronize()
    assert bool((ybuf == POISON).all()) and _intact(hbuf, cbuf)
    assert _same(hv.cpu().numpy(), d['h']) and _same(cv.cpu().numpy(), d['c'])


# ------------------------------------------------------------------------------------ (c) the projection
@pytest.mark.parametrize('K,N', CR.PROJECT_KN)
def test_projection_against_float64_and_row_r_whatever_m(K, N):
    from danet_amd import ops
    rng = np.random.RandomState(K + N)
    Mmax = max(CR.PROJECT_M)
    A = rng.standard_normal((Mmax, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    with oracle_threads():
        want = torch.as_tensor(A).double() @ torch.as_tensor(W).double()
        bound = (K + 1) * EPS24 * (torch.as_tensor(A).double().abs() @ torch.as_tensor(W).double().abs())
    want, bound = want.numpy(), bound.numpy()
    lda, ldw, ldo = K + 1, N + (4 if N % 4 == 0 else 3), N + 3
    Ab = torch.full((Mmax, lda), float('nan'), device='cuda')
    Ab[:, :K] = _cu(A)
    Wb = torch.full((K, ldw), float('nan'), device='cuda')
    Wb[:, :N] = _cu(W)
    rows, worst = {}, 0.0
    for M in CR.PROJECT_M:
        obuf, out = _guarded((M, ldo))
        ops.causal_project(Ab, M, K, N, lda, Wb, ldw, out=out, ldo=ldo)
        torch.cuda.synchronize()
        assert _intact(obuf)
        got = out.cpu().numpy()
        assert (got[:, N:] == np.float32(POISON)).all()
        got = got[:, :N]
        ratio = float((np.abs(got - want[:M]) / bound[:M]).max())
        worst = max(worst, ratio)
        assert ratio <= 1, (M, ratio)
        rows[M] = got
    for M in CR.PROJECT_M:
        assert _same(rows[M], rows[Mmax][:M]), M                                  # row r does not depend on M
    # an unpadded, 16-byte aligned W (the 16-byte loads) gives the same bits as the padded one
    if N % 4 == 0:
        assert _same(ops.causal_project(_cu(A[:17]), 17, K, N, K, _cu(W), N).cpu().numpy(), rows[17])
    print('projection K %d N %d: worst error %.3g of the derived bound' % (K, N, worst))


# ------------------------------------------------------------------------------------ (d) the encoder
TINY = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
            NUM_ANCHOR=4, ENCODER_TYPE='lstm-causal', TRAIN_ESTIMATOR_METHOD='truth-weighted',
            INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=8, SEPARATOR_TYPE='dot-softmax-orig')
T = 40


def _model(hp, **keys):
    from danet_amd.model import Model
    hp.reset()
    hp.load(dict(TINY, **keys))
    hp.digest()
    return Model('causal', device='cuda:0', seed=5).build()


def _signals(T, seed=0, B=2):
    rng = np.random.RandomState(seed)
    src = (rng.standard_normal((B, 2, T, 33)) + 1j * rng.standard_normal((B, 2, T, 33))).astype(np.complex64) * 3
    return _cu(src), _cu(src.sum(1))


def _cbits(t):
    return torch.view_as_real(t).cpu().numpy().view(np.uint32)


def _encoder_params(model, L=2):
    p = model.param_dict()
    return ([p['global/encoder/lstm%d/LSTM/linear/W' % l] for l in range(L)],
            [p['global/encoder/lstm%d/LSTM/linear/B' % l] for l in range(L)], p['global/encoder/output/W'])


def _embedding(model, mix):
    '''(infer's embedding [B, T, F, E], the float64 restatement's on the same log-magnitudes)'''
    from danet_amd import ops
    with torch.no_grad():
        fe = ops.frontend(mix[:, None].contiguous())
        emb = model.encoder(fe['mix_log'])
    Ws, bs, Wout = _encoder_params(model)
    want = CR.encoder(fe['mix_log'].cpu().numpy(), Ws, bs, Wout).reshape(emb.shape)
    return emb, want, fe


def test_the_embedding_against_float64_and_causality_on_the_device(hp):
    model = _model(hp)
    src, mix = _signals(T)
    emb, want, _ = _embedding(model, mix)
    assert tuple(emb.shape) == (2, T, 33, 4)
    err = CR.relmax(emb.cpu().numpy(), want)
    print('lstm-causal embedding against float64: %.3g of the maximum' % err)
    assert err <= CR.BAR
    mix2 = mix.clone()
    mix2[:, 20:] = mix2[:, 20:] * (-2.5) + 1
    emb2, _, _ = _embedding(model, mix2)
    assert _same(emb2[:, :20].cpu().numpy(), emb[:, :20].cpu().numpy())
    assert not _same(emb2[:, 20:].cpu().numpy(), emb[:, 20:].cpu().numpy())
    # lstm-orig on the same parameters is NOT causal: the test can tell
    orig = _model(hp, ENCODER_TYPE='lstm-orig', INFER_ESTIMATOR_METHOD='anchor', ONLINE_INIT_FRAMES=None)
    a, b = _embedding(orig, mix)[0], _embedding(orig, mix2)[0]
    assert not _same(a[:, :20].cpu().numpy(), b[:, :20].cpu().numpy())
    check_lstm_status()


def test_one_train_step_against_float64_autograd(hp, monkeypatch):
    from oracle import torch_ref as R
    model = _model(hp)
    src, _ = _signals(T, seed=3)
    model.keep_grads = True
    params = model.param_dict()

    def causal_encoder(x, p, H, L, E):
        out = CR.encoder_torch(x, [p['global/encoder/lstm%d/LSTM/linear/W' % l] for l in range(L)],
                               [p['global/encoder/lstm%d/LSTM/linear/B' % l] for l in range(L)],
                               p['global/encoder/output/W'])
        return out.reshape(x.shape[0], x.shape[1], x.shape[2], E)
    monkeypatch.setattr(R, 'lstm_encoder', causal_encoder)
    out = model.train_step(src)
    torch.cuda.synchronize()
    with oracle_threads():
        ref, tp = oracle_step(src, params, cfg_of(hp))
    assert relerr(float(out['loss']), float(ref['loss'].detach())) < 1e-4
    g = model.grad_dict()
    worst, checked = {}, 0
    for k in tp:
        if tp[k].grad is None:                 # the inference estimator's anchors
            assert not np.any(g[k]), k
            continue
        worst[k] = relerr(g[k], tp[k].grad.numpy())
        checked += 1
    print('worst gradient error: %r' % (max(worst.items(), key=lambda kv: kv[1]),))
    assert checked == 5 and all(v < TOL for v in worst.values()), worst
    check_lstm_status()


def test_the_loss_decreases_over_20_steps_and_lstm_orig_files_load(hp, tmp_path):
    model = _model(hp, LR=3e-3)
    src, _ = _signals(T, seed=4)
    losses = [float(model.train_step(src)['loss']) for _ in range(20)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    res = model.valid_step(src)
    assert list(res) == ['loss', 'SNR'] and all(np.isfinite(float(v)) for v in res.values())
    orig = _model(hp, ENCODER_TYPE='lstm-orig', INFER_ESTIMATOR_METHOD='anchor', ONLINE_INIT_FRAMES=None)
    orig.train_step(src)
    path = str(tmp_path / 'orig.npz')
    orig.save_params(path)
    causal = _model(hp)
    causal.load_params(path)
    a, b = orig.param_dict(), causal.param_dict()
    assert sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    assert np.isfinite(causal.infer(_signals(T)[1]).abs().cpu().numpy()).all()
    check_lstm_status()


# ------------------------------------------------------------------------------------ (e) the session
def _push_all(stream, mix, blocks):
    '''push `mix` [B, T, F] in consecutive blocks of the given sizes (cycled) -> (the outputs per call, the
    concatenated embedding and trajectory of the blocks as the session saw them)'''
    outs, embs, t, i = [], [], 0, 0
    while t < mix.shape[1]:
        n = blocks[i % len(blocks)]
        outs.append(stream.push(mix[:, t:t + n]))
        embs.append(stream.embed)
        t, i = t + n, i + 1
    return outs, torch.cat(embs, dim=1)


@pytest.mark.parametrize('sep,tau', [('dot-softmax-orig', None), ('dot-sigmoid-orig', -1.0 / math.log(0.9))])
def test_block_sizes_give_bit_identical_outputs_and_the_restatement(hp, sep, tau):
    from danet_amd import ops
    T0 = 8
    model = _model(hp, SEPARATOR_TYPE=sep, ONLINE_MEMORY_FRAMES=tau)
    lam = 1.0 if tau is None else 0.9
    assert model.online[0] == T0 and abs(model.online[1] - lam) <= 1e-15
    src, mix = _signals(T, seed=1)
    stream = model.open_stream(2)
    whole_outs, whole_emb = _push_all(stream, mix, (T,))
    whole = whole_outs[0]
    assert tuple(whole.shape) == (2, 2, T, 33) and whole.dtype == torch.complex64
    traj = stream.attr.cpu().numpy()
    assert tuple(stream.flush().shape) == (2, 2, 0, 33)
    for blocks in ((1,), (3,), (5, 35)):
        outs, emb = _push_all(stream, mix, blocks)
        assert np.array_equal(_cbits(torch.cat(outs, dim=2)), _cbits(whole)), blocks
        assert _same(emb.cpu().numpy(), whole_emb.cpu().numpy()), blocks
        # nothing before frame T0 - 1, then T0 frames at once (blocks of one frame), then every frame as it comes
        seen, want_m = 0, []
        for o in outs:
            n = min(blocks[len(want_m) % len(blocks)], T - seen)      # (the last block of 3 holds one frame)
            seen += n
            want_m.append(0 if seen < T0 else (seen if seen - n < T0 else n))
        assert [o.shape[2] for o in outs] == want_m, (blocks, [o.shape[2] for o in outs])
        if blocks == (1,):
            assert want_m[:T0] == [0] * (T0 - 1) + [T0] and set(want_m[T0:]) == {1}
        stream.reset()
    # the session's embedding against infer's and against float64
    emb_i, want, fe = _embedding(model, mix)
    V = whole_emb.cpu().numpy()
    e_s, e_i = CR.relmax(V, want), CR.relmax(emb_i.cpu().numpy(), want)
    e_si = CR.relmax(V, emb_i.cpu().numpy())
    print('session embedding %.3g, infer embedding %.3g of float64; session against infer %.3g' % (e_s, e_i, e_si))
    assert e_s <= CR.BAR and e_i <= CR.BAR and e_si <= 2e-5
    # the trajectory and |out| against the online restatement fed the session's own embedding
    with torch.no_grad():
        a0, _, _ = ops.AnchorAttractorFn.apply(whole_emb[:, :T0].contiguous(), model.vars['global/infer_estimator/anchors'], 2)
    W, A0, act = fe['mix_pwr'].cpu().numpy(), a0.cpu().numpy(), model.separator.ACT
    want_traj = OR.attractors(V, W, A0, act, lam, T0, float(hp.EPS))
    assert tuple(traj.shape) == (2, T, 2, 4) and CR.relmax(traj, want_traj) <= OR.BAR
    assert CR.relmax(whole.abs().cpu().numpy(), OR.separate(V, W, want_traj, act)) <= OR.BAR
    check_lstm_status()


def test_flush_reset_batches_and_the_key(hp):
    '''flush on a recording no longer than the hold "equals infer bit for bit": infer of the model with
    INFER_STREAM_BLOCK set, which is what makes infer take the session's arithmetic -- with the key null, infer's
    encoder runs on the core's recurrent kernels, whose embedding differs from the block kernel's in the last bits
    (the 2e-5 test above), so there flush is held to infer within FLUSH_BAR = 2e-5 of the maximum of the complex
    output (the module docstring derives it; measured 1.2e-7), which is what ties flush to infer's own path for a
    recording within the hold; the plain separator on the session's own embedding is compared bit for bit as well'''
    from danet_amd import ops
    model = _model(hp)
    src, mix = _signals(T, seed=2)
    stream = model.open_stream(2)
    short = mix[:, :5].contiguous()
    assert stream.push(short).shape[2] == 0
    emb = stream.embed.clone()
    got = stream.flush()
    assert tuple(got.shape) == (2, 2, 5, 33) and stream.t == 0 and stream.state is None and not stream.held
    with torch.no_grad():
        fe = ops.frontend(short[:, None].contiguous())
        a0, _, _ = ops.AnchorAttractorFn.apply(emb, model.vars['global/infer_estimator/anchors'], 2)
        want = ops.reattach_phase(model.separator(fe['mix_pwr'], a0, emb.reshape(2, -1, 4)), fe['phasor'])
    assert np.array_equal(_cbits(got), _cbits(want))
    plain = model.infer(short)                                 # the whole-utterance encoder: close, not the same bits
    assert tuple(plain.shape) == tuple(got.shape)
    err = float((got - plain).abs().max() / plain.abs().max())
    print('flush against infer with the key null: %.3g of the maximum' % err)
    assert err <= FLUSH_BAR
    # reset, then the same pushes repeat bit for bit; without reset the state goes on
    first = torch.cat(_push_all(stream, mix, (7,))[0], dim=2)
    stream.reset()
    second = torch.cat(_push_all(stream, mix, (7,))[0], dim=2)
    assert np.array_equal(_cbits(first), _cbits(second)) and stream.t == T
    third = stream.push(mix[:, :7])
    assert third.shape[2] == 7 and not np.array_equal(_cbits(third), _cbits(first[:, :, :7]))
    # batch = 3: row 1 is a batch = 1 session on that recording
    src3, mix3 = _signals(T, seed=6, B=3)
    three = torch.cat(_push_all(model.open_stream(3), mix3, (6,))[0], dim=2)
    one = torch.cat(_push_all(model.open_stream(1), mix3[1:2].contiguous(), (6,))[0], dim=2)
    assert tuple(three.shape) == (3, 2, T, 33) and np.array_equal(_cbits(three[1:2]), _cbits(one))
    # the key: infer IS the session, whatever the block size; and on the short recording it is flush
    for n in (4, 64):
        keyed = _model(hp, INFER_STREAM_BLOCK=n)
        assert keyed.stream_block == n
        assert np.array_equal(_cbits(keyed.infer(mix)), _cbits(first)), n
        assert np.array_equal(_cbits(keyed.infer(short)), _cbits(got)), n
    with pytest.raises(ValueError):
        stream.push(mix[:1])
    check_lstm_status()


def test_demo_mode_with_the_key_writes_what_the_session_computes(hp, tmp_path, monkeypatch):
    import scipy.io.wavfile
    from danet_amd import _lib, cli, datasets, utils
    monkeypatch.chdir(tmp_path)
    cfg = dict(TINY, BATCH_SIZE=4, DATASET_TYPE='synth', ONLINE_MEMORY_FRAMES=50, INFER_STREAM_BLOCK=4)
    (tmp_path / 'cfg.json').write_text(json.dumps(cfg))
    wave = (datasets.speech_shaped_wave(np.random.RandomState(2), 8000, 8000)).astype(np.int16)
    scipy.io.wavfile.write('mix.wav', 8000, wave)
    model = cli.main(['-n', 'streamed', '-m', 'demo', '-if', 'mix.wav', '-c', 'cfg.json'], out=io.StringIO())
    assert model.stream_block == 4 and hp.BATCH_SIZE == 1 and _lib._causal is not None
    x = torch.as_tensor(utils.load_wavfile('mix.wav').astype(np.complex64)).to(model.device)[None]
    assert x.shape[1] > 8
    stream = model.open_stream(1)
    sep = torch.cat([stream.push(x), stream.flush()], dim=2)
    assert np.array_equal(_cbits(sep), _cbits(model.infer(x)))
    for i in (1, 2):
        sr, y = scipy.io.wavfile.read('mix_separated_%d.wav' % i)
        assert sr == 8000 and np.isfinite(y).all() and np.abs(y).max() > 0
        utils.save_wavfile('direct_%d.wav' % i, sep[0, i - 1].cpu().numpy())
        assert open('direct_%d.wav' % i, 'rb').read() == open('mix_separated_%d.wav' % i, 'rb').read()
    check_lstm_status()


# ------------------------------------------------------------------------------------ (f) the untouched path
def test_a_model_with_another_encoder_never_maps_the_library():
    '''a fresh process builds a `bilstm-orig` / `anchor` model, runs train_step, valid_step and infer, and ends with the
    library neither loaded nor mapped'''
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib\n"
        "from danet_amd.hparams import hparams\n"
        "from danet_amd.model import Model\n"
        "hparams.load(%r); hparams.digest()\n"
        "model = Model('other', device='cuda:0', seed=5).build()\n"
        "rng = np.random.RandomState(0)\n"
        "src = torch.as_tensor((rng.standard_normal((2, 2, 40, 33)) + 1j * rng.standard_normal((2, 2, 40, 33)))"
        ".astype(np.complex64)).cuda()\n"
        "tr = model.train_step(src); res = model.valid_step(src); out = model.infer(src.sum(1)); torch.cuda.synchronize()\n"
        "print('RAN:', tuple(out.shape) == (2, 2, 40, 33) and sorted(res) == ['SNR', 'loss'] and np.isfinite(float(tr['loss'])))\n"
        "print('STATE:', model.stream_block)\n"
        "print('UNMAPPED:', _lib._causal is None and 'libdanet_causal' not in open('/proc/self/maps').read())\n"
        "print('CORE:', 'libdanet_hip' in open('/proc/self/maps').read())\n"
    ) % (ROOT, dict(TINY, ENCODER_TYPE='bilstm-orig', INFER_ESTIMATOR_METHOD='anchor', ONLINE_INIT_FRAMES=None))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('RAN: True', 'STATE: None', 'UNMAPPED: True', 'CORE: True'):
        assert words in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
