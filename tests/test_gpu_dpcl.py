'''
GPU tests of the deep-clustering auxiliary loss (DPCL_WEIGHT, run with -m gpu): the three kernels of
libdanet_dpcl_hip.so against the float64 restatement tests/dpcl_ref.py over a table of shapes, every output and the
workspace between poisoned guard bands; bit-identical repeats, an utterance alone against the same utterance in a
batch, a silent utterance in a batch; then Model.train_step with the key null, 0.0 and 0.5 on every head path, the
untouched valid / infer paths, and the command line.

Bars.  A, Bm, c: 1e-5 of each tensor's maximum (the project's bar; the float32 restatement's error is printed beside
the kernel's).  L_b and the total: 1e-5 of ||A||^2 + 2 ||Bm||^2 + sum c^2, the size of the terms.  dembed: 1e-5 of
max_i 4 w_i (sum_f |A_ef v_if| + |Bm_e,y_i|) times |dloss * alpha / B|.  Parameter gradients of a step: 1e-5 of each
tensor's maximum against the null step's gradient plus what alpha * dV_ref leaves through the same encoder.
'''
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dpcl_ref as DR
from gpu_helpers import ROOT, rand_src

pytestmark = pytest.mark.gpu
POISON = -7.25e33
GUARD = 1024
BAR = 1e-5

# (N, E, C, B): every N, E, C and B of the envelope's edges at least three times, not the full product
CASES = [(1, 1, 1, 1), (1, 20, 2, 3), (1, 64, 4, 9), (2, 1, 2, 1), (2, 3, 3, 3), (2, 40, 4, 1), (63, 3, 2, 3),
         (63, 63, 1, 1), (63, 4, 4, 9), (64, 4, 2, 1), (64, 20, 3, 3), (64, 64, 2, 1), (65, 3, 2, 9), (65, 40, 3, 1),
         (65, 1, 4, 3), (255, 20, 2, 1), (255, 63, 3, 3), (255, 4, 1, 9), (256, 40, 2, 3), (256, 1, 3, 1),
         (256, 64, 4, 1), (257, 3, 1, 1), (257, 20, 4, 9), (257, 63, 2, 1), (516, 20, 2, 9), (516, 40, 3, 3),
         (516, 64, 4, 1), (516, 1, 1, 3), (4097, 20, 2, 3), (4097, 40, 3, 1), (4097, 63, 4, 1), (4097, 4, 2, 9),
         (4097, 3, 3, 1), (16512, 20, 2, 3), (16512, 40, 3, 1), (16512, 64, 4, 1), (16512, 1, 1, 1), (16512, 4, 2, 9),
         (16512, 63, 2, 1), (16512, 3, 4, 3)]


def _guarded(shape, dtype=torch.float32):
    '''(whole buffer, the view of `shape` in its middle): everything poisoned'''
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == POISON).all()) and bool((buf[-GUARD:] == POISON).all())


def _bits(t):
    a = t.detach().cpu().contiguous()
    if a.dim() == 0:
        a = a.reshape(1)
    return a.numpy().view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.element_size()]).copy()


def _inputs(N, E, C, B, seed=0):
    '''normal embeddings, uniform magnitudes, and (N permitting) rows with exact ties and exact zeros'''
    rng = np.random.RandomState(7919 * seed + 1000 * N + 10 * E + C + 100003 * B)
    V = rng.standard_normal((B, N, E)).astype(np.float32)
    S = rng.uniform(0.0, 2.0, (B, C, N)).astype(np.float32)
    if N >= 4:
        S[:, :, 1] = S[:, :1, 1]           # an exact tie of every source
        S[:, :, 2] = 0.0                   # an all-zero bin
        S[:, -1, 3] = S[:, max(C - 2, 0), 3]
    if N >= 300:
        S[:, :, 260:290] = 0.0             # a silent stretch across a tile boundary
    return V, S


class _Forward(object):
    '''stats + finalize of one case through ops, every output and the workspace guarded'''

    def __init__(self, V, S, alpha=0.5, main=1.25):
        from danet_amd import ops
        B, N, E = V.shape
        C = S.shape[1]
        self.dims = (B, N, E, C)
        self.embed, self.src_pwr = torch.from_numpy(V).cuda(), torch.from_numpy(S).cuda()
        nws = ops.dpcl_workspace_bytes(B, N, E, C)
        assert nws == DR.workspace_bytes(B, N, E, C)
        self.bufs = [_guarded((nws // 4,)), _guarded((B,), torch.float64), _guarded((1,)), _guarded((1,)),
                     _guarded((B, E, E + C)), _guarded((B, C + 1))]
        self.ws = self.bufs[0][1].view(torch.uint8)
        self.out = tuple(v for _, v in self.bufs[1:])
        self.main = None if main is None else torch.tensor(main, device='cuda')
        self.alpha = alpha
        self.run()

    def run(self):
        from danet_amd import ops
        B, N, E, C = self.dims
        ops.dpcl_stats(self.embed, self.src_pwr, ws=self.ws)
        ops.dpcl_finalize(self.ws, B, N, E, C, self.alpha, main=self.main, out=self.out)
        torch.cuda.synchronize()
        assert all(_guards_intact(buf) for buf, _ in self.bufs)
        return [_bits(v) for _, v in self.bufs]

    def poison(self):
        for _, v in self.bufs:
            v.fill_(POISON)


@pytest.fixture(scope='module')
def reference():
    '''the float64 restatement of every case, computed once and shared'''
    cache = {}

    def get(case):
        if case not in cache:
            N, E, C, B = case
            V, S = _inputs(N, E, C, B)
            cache[case] = (V, S, DR.batch(V, S, main=1.25, alpha=0.5))
        return cache[case]
    return get


# --------------------------------------------------------------------------- stats + finalize
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%d-E%d-C%d-B%d' % c)
def test_stats_and_finalize_against_the_restatement(case, reference):
    N, E, C, B = case
    V, S, ref = reference(case)
    f = _Forward(V, S)
    per_utt, dpcl, total, tables, cs = [t.cpu().numpy().astype(np.float64) for t in f.out]
    assert np.isfinite(tables).all() and np.isfinite(cs).all()
    worst = dict(A=0.0, Bm=0.0, c=0.0, A32=0.0, Bm32=0.0, c32=0.0, L=0.0)
    for b in range(B):
        st = ref['stats'][b]
        A32, Bm32, c32, _ = DR.stats_f32(V[b], S[b])
        for name, got, got32, want in (('A', tables[b][:, :E], A32, st['A']), ('Bm', tables[b][:, E:], Bm32, st['Bm']),
                                       ('c', cs[b][:C], c32, st['c'])):
            peak = np.abs(want).max()
            err = np.abs(got - want).max() / peak
            worst[name] = max(worst[name], err)
            worst[name + '32'] = max(worst[name + '32'], np.abs(got32 - want).max() / peak)
            assert err <= BAR, (b, name, err)
        assert abs(cs[b][C] - st['S']) <= BAR * st['S']
        errL = abs(per_utt[b] - ref['per_utt'][b]) / DR.term_size(st)
        worst['L'] = max(worst['L'], errL)
        assert errL <= BAR, (b, errL)
    size = np.mean([DR.term_size(st) for st in ref['stats']])
    err_d, err_t = abs(dpcl[0] - ref['dpcl']) / size, abs(total[0] - ref['total']) / (1.25 + 0.5 * size)
    print('N=%d E=%d C=%d B=%d  kernel A %.2e Bm %.2e c %.2e | float32 restatement A %.2e Bm %.2e c %.2e | L %.2e '
          'dpcl %.2e total %.2e' % (N, E, C, B, worst['A'], worst['Bm'], worst['c'], worst['A32'], worst['Bm32'],
                                    worst['c32'], worst['L'], err_d, err_t))
    assert err_d <= BAR and err_t <= BAR
    # main NULL means 0; alpha = 0 gives main back bit for bit
    f0 = _Forward(V, S, alpha=0.0, main=1.25)
    assert _bits(f0.out[2])[0] == np.float32(1.25).view(np.uint32) and np.array_equal(_bits(f0.out[1]), _bits(f.out[1]))
    fn = _Forward(V, S, alpha=0.5, main=None)
    assert abs(float(fn.out[2]) - 0.5 * ref['dpcl']) <= BAR * 0.5 * size


# --------------------------------------------------------------------------- backward
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%d-E%d-C%d-B%d' % c)
def test_backward_against_the_restatement(case, reference):
    from danet_amd import ops
    N, E, C, B = case
    V, S, ref = reference(case)
    alpha = 0.5
    f = _Forward(V, S, alpha=alpha)
    tables, cs = f.out[3].contiguous(), f.out[4].contiguous()
    bars = np.array([DR.grad_bar(V[b], ref['stats'][b]) for b in range(B)])
    which = CASES.index(case) % 3
    dlosses = [(None, 1.0), (torch.tensor(1.0, device='cuda'), 1.0), (torch.tensor(-0.37, device='cuda'), -0.37)]
    order = dlosses[which:] + dlosses[:which]
    worst = 0.0
    for dl, k in (order if N <= 516 else order[:1]):          # the large shapes take one of the three in turn
        buf, out = _guarded((B, N, E))
        ops.dpcl_bwd(f.embed, f.src_pwr, tables, cs, alpha / B, dloss=dl, out=out)
        torch.cuda.synchronize()
        assert _guards_intact(buf)
        got = out.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        for b in range(B):
            err = np.abs(got[b] - k * ref['dembed'][b]).max()
            bar = BAR * bars[b] * abs(k * alpha / B)
            worst = max(worst, err / (bars[b] * abs(k * alpha / B)))
            assert err <= bar, (b, k, err, bar)
    # end to end through the autograd Function, the incoming gradient a non-trivial device scalar
    emb = f.embed.clone().requires_grad_(True)
    main = torch.tensor(1.25, device='cuda', requires_grad=True)
    total, dpcl = ops.dpcl_loss(emb, f.src_pwr, main, alpha)
    assert total.dim() == 0 and dpcl.dim() == 0 and not dpcl.requires_grad and total.requires_grad
    (total * -0.37).backward()
    torch.cuda.synchronize()
    got = emb.grad.cpu().numpy().astype(np.float64)
    assert float(main.grad) == np.float32(-0.37)              # main passes through with the gradient unchanged
    assert np.array_equal(_bits(total), _bits(f.out[2])) and np.array_equal(_bits(dpcl), _bits(f.out[1]))
    for b in range(B):
        assert np.abs(got[b] + 0.37 * ref['dembed'][b]).max() <= BAR * bars[b] * 0.37 * alpha / B, b
    print('N=%d E=%d C=%d B=%d  dembed error %.2e of its bar\'s unit' % (N, E, C, B, worst))


def test_one_hot_embedding_has_zero_loss_and_a_gradient_inside_the_bar():
    from danet_amd import ops
    N, E, C, B = 516, 4, 3, 3
    _, S = _inputs(N, E, C, B)
    V = np.zeros((B, N, E), np.float32)
    for b in range(B):
        V[b, np.arange(N), DR.labels(S[b])] = 1.0
    ref = DR.batch(V, S, alpha=1.0)
    assert np.abs(ref['per_utt']).max() <= 1e-15 and np.abs(ref['dembed']).max() <= 1e-15
    f = _Forward(V, S, alpha=1.0, main=None)
    for b in range(B):
        assert abs(float(f.out[0][b])) <= BAR * DR.term_size(ref['stats'][b])
    buf, out = _guarded((B, N, E))
    ops.dpcl_bwd(f.embed, f.src_pwr, f.out[3], f.out[4], 1.0 / B, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    got = out.cpu().numpy().astype(np.float64)
    for b in range(B):
        bar = DR.grad_bar(V[b], ref['stats'][b])
        assert bar > 1e-4 and np.abs(got[b]).max() <= BAR * bar / B


# --------------------------------------------------------------------------- structural
# (B = 8 and 16: the XCD-aware workgroup mapping, which needs B to be a multiple of 8)
@pytest.mark.parametrize('case', [(516, 20, 2, 9), (4097, 40, 3, 9), (257, 64, 4, 9), (65, 3, 2, 9), (2049, 20, 2, 8),
                                  (300, 40, 3, 16)],
                         ids=lambda c: 'N%d-E%d-C%d-B%d' % c)
def test_repeats_and_an_utterance_alone_are_bit_identical(case):
    from danet_amd import ops
    N, E, C, B = case
    V, S = _inputs(N, E, C, B, seed=1)
    f = _Forward(V, S)
    first = f.run()
    f.poison()
    assert all(np.array_equal(a, b) for a, b in zip(first, f.run()))
    d1 = ops.dpcl_bwd(f.embed, f.src_pwr, f.out[3], f.out[4], 0.5 / B)
    d2 = ops.dpcl_bwd(f.embed, f.src_pwr, f.out[3], f.out[4], 0.5 / B)
    assert np.array_equal(_bits(d1), _bits(d2))
    per = DR.workspace_bytes(1, N, E, C)
    ref = DR.batch(V, S, main=1.25, alpha=0.5)
    for b in (0, B // 2, B - 1):
        assert abs(float(f.out[0][b]) - ref['per_utt'][b]) <= BAR * DR.term_size(ref['stats'][b]), b
        got = d1[b].cpu().numpy().astype(np.float64)
        assert np.abs(got - ref['dembed'][b]).max() <= BAR * DR.grad_bar(V[b], ref['stats'][b]) * 0.5 / B, b
        g = _Forward(V[b:b + 1], S[b:b + 1])
        assert np.array_equal(_bits(g.ws), _bits(f.ws)[b * per:(b + 1) * per]), b       # the partials
        assert _bits(g.out[0])[0] == _bits(f.out[0])[b]                                  # L_b
        assert np.array_equal(_bits(g.out[3])[0], _bits(f.out[3])[b]) and np.array_equal(_bits(g.out[4])[0],
                                                                                         _bits(f.out[4])[b])
        da = ops.dpcl_bwd(g.embed, g.src_pwr, g.out[3], g.out[4], 0.5 / B)
        assert np.array_equal(_bits(da)[0], _bits(d1)[b]), b


def test_a_misaligned_embedding_takes_the_slower_path_to_the_same_bits():
    from danet_amd import ops
    N, E, C, B = 516, 20, 2, 3
    V, S = _inputs(N, E, C, B, seed=2)
    f = _Forward(V, S)
    d = ops.dpcl_bwd(f.embed, f.src_pwr, f.out[3], f.out[4], 0.25)
    store = torch.zeros(B * N * E + 1, device='cuda')
    shifted = store[1:].view(B, N, E)
    shifted.copy_(f.embed)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    ws = ops.dpcl_stats(shifted, f.src_pwr)
    assert np.array_equal(_bits(ws), _bits(f.ws))
    d2 = ops.dpcl_bwd(shifted, f.src_pwr, f.out[3], f.out[4], 0.25)
    assert np.array_equal(_bits(d2), _bits(d))


def test_a_silent_utterance_in_a_batch_gives_zeros_and_no_nan():
    from danet_amd import ops
    N, E, C, B = 300, 20, 2, 3
    V, S = _inputs(N, E, C, B, seed=3)
    S[1] = 0.0
    ref = DR.batch(V, S, main=1.25, alpha=0.5)
    f = _Forward(V, S)
    per_utt, dpcl, total, tables, cs = [t.cpu().numpy() for t in f.out]
    assert per_utt[1] == 0.0 and not tables[1].any() and not cs[1].any()
    assert all(np.isfinite(t).all() for t in (per_utt, dpcl, total, tables, cs))
    assert abs(dpcl[0] - ref['dpcl']) <= BAR * np.mean([DR.term_size(st) for st in ref['stats']])
    d = ops.dpcl_bwd(f.embed, f.src_pwr, f.out[3], f.out[4], 0.5 / B).cpu().numpy()
    assert np.isfinite(d).all() and not d[1].any() and d[0].any() and d[2].any()
    # all silent: the dry forward of Model.build()
    f = _Forward(V, 0 * S)
    assert float(f.out[1]) == 0.0 and float(f.out[2]) == 1.25 and not f.out[3].any() and not f.out[0].any()
    d = ops.dpcl_bwd(f.embed, f.src_pwr, f.out[3], f.out[4], 0.5 / B)
    assert not d.any()


def test_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    V, S = _inputs(65, 4, 2, 2)
    f = _Forward(V, S)
    before = f.run()
    f.poison()
    small = f.ws[:-4]
    with pytest.raises(_lib.DanetHipError) as e:
        ops.dpcl_stats(f.embed, f.src_pwr, ws=small)
    assert 'workspace too small' in str(e.value)
    with pytest.raises(_lib.DanetHipError) as e:
        ops.dpcl_finalize(small, 2, 65, 4, 2, 0.5, out=f.out)
    assert 'workspace too small' in str(e.value)
    with pytest.raises(_lib.DanetHipError) as e:
        ops.dpcl_finalize(f.ws, 2, 65, 4, 2, -0.5, out=f.out)
    assert 'alpha must' in str(e.value)
    buf, out = _guarded((2, 65, 4))
    with pytest.raises(_lib.DanetHipError) as e:
        ops.dpcl_bwd(f.embed, f.src_pwr, f.out[3].contiguous(), f.out[4].contiguous(), float('nan'), out=out)
    assert 'scale must' in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all()) and all(bool((b == POISON).all()) for b, _ in f.bufs)
    assert all(np.array_equal(a, b) for a, b in zip(before, f.run()))


# --------------------------------------------------------------------------- model
BASE = dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=1, LSTM_HDIM=16,
            NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor', INFER_ESTIMATOR_METHOD='anchor',
            SEPARATOR_TYPE='dot-softmax-orig')


def _build(hp, **keys):
    from danet_amd.model import Model
    hp.reset()
    hp.load(dict(BASE, **keys))
    hp.digest()
    return Model('dpcl', device='cuda', seed=3).build()


def test_null_and_zero_weight_train_bit_equal_parameters(hp):
    src = torch.as_tensor(rand_src_of(hp)).cuda()
    runs = {}
    for tag, keys in (('null', {}), ('zero', dict(DPCL_WEIGHT=0.0))):
        model = _build(hp, **keys)
        outs = [model.train_step(src) for _ in range(3)]
        torch.cuda.synchronize()
        runs[tag] = (outs, _bits(model._flat))
    assert [list(o) for o in runs['null'][0]] == [['loss', 'SNR', 'LR']] * 3
    assert [list(o) for o in runs['zero'][0]] == [['loss', 'SNR', 'LR', 'DPCL']] * 3
    for a, b in zip(*[r[0] for r in runs.values()]):
        assert _bits(a['loss']) == _bits(b['loss']) and _bits(a['SNR']) == _bits(b['SNR'])
        assert np.isfinite(float(b['DPCL'])) and float(b['DPCL']) > 0
    assert np.array_equal(runs['null'][1], runs['zero'][1])


def rand_src_of(hp, T=8):
    hp.reset()
    hp.load(BASE)
    hp.digest()
    return rand_src(hp, T, seed=5)


@pytest.mark.parametrize('path', ['fused', 'unfused', 'si-sdr', 'noisy'])
def test_half_weight_adds_the_restatements_gradient_on_every_head_path(hp, path):
    from danet_amd import ops
    alpha = 0.5
    src_h = rand_src_of(hp)
    src = torch.as_tensor(src_h).cuda()
    keys = dict(TRAIN_LOSS='si-sdr') if path == 'si-sdr' else {}
    extra = {}
    if path == 'noisy':
        rng = np.random.RandomState(9)
        B, T, F = src_h.shape[0], src_h.shape[2], src_h.shape[3]
        noise = torch.as_tensor(((rng.randn(B, T, F) + 1j * rng.randn(B, T, F)) * 2).astype(np.complex64)).cuda()
        extra = dict(s_noise=noise, s_noise_gain=torch.as_tensor(rng.uniform(0.5, 1.5, B).astype(np.float32)).cuda())

    def step(**more):
        model = _build(hp, **dict(keys, **more))
        model.keep_grads = True
        model.fuse_heads = path != 'unfused'
        out = model.train_step(src, **extra)
        torch.cuda.synchronize()
        return model, out, {k: v.copy() for k, v in model.grad_dict().items()}

    _, out0, g0 = step()
    _, out1, g1 = step(DPCL_WEIGHT=alpha)
    # what alpha * dV_ref leaves through the same encoder, at the same (initial) parameters
    ref = _build(hp, **keys)
    ref.zero_grad()
    if path == 'noisy':
        o = ref.forward_noisy(src, extra['s_noise'], extra['s_noise_gain'], with_train=False)
    else:
        o = ref.forward(src, with_train=False)
    embed = o['embed']
    B, E = hp.BATCH_SIZE, hp.EMBED_SIZE
    V = embed.detach().cpu().numpy().reshape(B, -1, E)
    S = ops.frontend(src)['src_pwr'].cpu().numpy().reshape(B, hp.MAX_N_SIGNAL, -1)     # the CLEAN sources'
    r = DR.batch(V, S, alpha=alpha)
    embed.backward(torch.as_tensor(r['dembed'].astype(np.float32)).cuda().view_as(embed))
    ops.join_deferred()
    torch.cuda.synchronize()
    g2 = ref.grad_dict()
    assert abs(float(out1['DPCL']) - r['dpcl']) <= BAR * np.mean([DR.term_size(st) for st in r['stats']])
    want_loss = float(out0['loss']) + alpha * r['dpcl']
    assert abs(float(out1['loss']) - want_loss) <= 1e-5 * (abs(float(out0['loss'])) + alpha * r['dpcl'])
    assert _bits(out1['SNR']) == _bits(out0['SNR'])
    worst, moved = 0.0, 0
    for k in g0:
        want = g0[k].astype(np.float64) + g2[k].astype(np.float64)
        peak = np.abs(want).max()
        err = np.abs(g1[k] - want).max()
        if peak > 0:
            worst = max(worst, err / peak)
        moved += bool(np.abs(g2[k]).max() > 1e-3 * np.abs(g0[k]).max())
        assert err <= BAR * peak, (k, err, peak)
    print('%s: worst parameter-gradient error %.2e of the tensor\'s maximum; %d of %d tensors moved by the auxiliary '
          'loss' % (path, worst, moved, len(g0)))
    assert moved >= 2


def test_valid_infer_build_and_the_norm_clip_with_the_key_set(hp):
    src = torch.as_tensor(rand_src_of(hp)).cuda()
    mix = src.sum(dim=1).contiguous()
    res = {}
    for tag, keys in (('null', {}), ('on', dict(DPCL_WEIGHT=0.1))):
        model = _build(hp, **keys)                              # build(): the all-zero dry forward
        assert all(bool(torch.isfinite(v).all()) for v in model.vars.values())
        v = model.valid_step(src)
        res[tag] = (list(v), [_bits(v[k]) for k in v], _bits(model.infer(mix)), model.collectives_per_step())
    assert res['null'][0] == res['on'][0] == ['loss', 'SNR']
    assert all(np.array_equal(a, b) for a, b in zip(res['null'][1], res['on'][1]))
    assert np.array_equal(res['null'][2], res['on'][2]) and res['null'][3] == res['on'][3]
    with torch.no_grad():
        o = model.forward(src)
        assert 'dpcl' in o and np.isfinite(float(o['dpcl'])) and 'dpcl' not in model.debug_fetch(src)
    model = _build(hp, DPCL_WEIGHT=0.1, GRAD_CLIP_NORM=0.5)
    out = model.train_step(src)
    assert list(out) == ['loss', 'SNR', 'LR', 'DPCL', 'grad_norm', 'clip_coef']
    assert all(np.isfinite(float(out[k])) for k in ('loss', 'SNR', 'DPCL', 'grad_norm', 'clip_coef'))
    assert out['DPCL'].is_cuda and out['DPCL'].dim() == 0 and not out['DPCL'].requires_grad


# --------------------------------------------------------------------------- CLI
def test_command_line_prints_a_dpcl_column(tmp_path):
    base = dict(BASE, BATCH_SIZE=2, LSTM_HDIM=8, MAX_TRAIN_LEN=128)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)
    cfg = tmp_path / 'dpcl.json'
    cfg.write_text(json.dumps(dict(base, DPCL_WEIGHT=0.1)))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'dpcl', '-m', 'train', '-ds', 'toy', '-c',
                          str(cfg), '-ne', '1', '-bs', '2'], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('Epoch 1/1')][0]
    assert 'DPCL=' in line and line.index('LR=') < line.index('DPCL='), line
    value = float(line.split('DPCL=')[1].split()[0])
    assert np.isfinite(value) and 0.0 <= value <= 100.0
    valid = [l for l in out.stdout.splitlines() if l.startswith('Valid  1/1')][0]
    assert 'DPCL' not in valid
