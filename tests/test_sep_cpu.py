'''
CPU checks (no GPU) of tests/sep_ref.py, the references and case tables of tests/test_gpu_sep_envelope.py:

- the analytic float64 gradients equal float64 autograd through oracle/torch_ref.py (sep_dot, pit_mse_loss) to
  1e-10, for every (C, act, mode), with a forced permutation that is not the best one and with phasors that
  are not of unit length (restated in torch where torch_ref has no argument for them);
- the permutation order is itertools.permutations' for C in 1..4 and ties go to the first;
- the restated constants (pick_ep, chunk counts, the partials' size) equal danet_workspace_bytes;
- the tables reach every (EP, EF, CP) x act of the separators, x (act, mode) of the fused kernels, every
  CP x mode of the loss, every (EP, EF) x (act, mode) with partials, and every edge the tables were written for;
- both conditions of the bar hold for every row: the float32 restatement stays below 1e-6 of float64 for every
  compared output, and (outside the tie rows) the runner-up permutation's float64 loss exceeds the best by
  at least 1e-3 relative for every utterance.
'''
import itertools
import math

import numpy as np
import pytest
import torch

import sep_ref as sr
from oracle import torch_ref as R


# ------------------------------------------------------------------ gradients against autograd
def _small(C, act, mode, seed, phasor_len=1.0, B=3, N=11, E=5):
    rng = np.random.RandomState(seed)
    d = dict(embed=rng.randn(B, N, E) / np.sqrt(E), attr=rng.randn(B, C, E), mix_pwr=np.abs(rng.randn(B, N)) + 0.1,
             src=rng.randn(B, C, N) + 1j * rng.randn(B, C, N), dout=rng.randn(B, C, N))
    ang = rng.uniform(-np.pi, np.pi, (B, N))
    d['phasor'] = np.stack([np.cos(ang), np.sin(ang)], axis=-1) * phasor_len
    return d


def _t(a, grad=False):
    return torch.tensor(a, requires_grad=grad)


@pytest.mark.parametrize('C', [1, 2, 3, 4])
@pytest.mark.parametrize('act', [0, 1])
def test_separator_gradients_equal_autograd(C, act):
    d = _small(C, act, 0, 10 * C + act)
    B, N = d['mix_pwr'].shape
    embed, attr = _t(d['embed'], True), _t(d['attr'], True)
    out, masks = R.sep_dot(_t(d['mix_pwr']).reshape(B, 1, N), attr, embed, 'softmax' if act == 0 else 'sigmoid')
    out = out.reshape(B, C, N)
    (out * _t(d['dout'])).sum().backward()
    o, m = sr.sep_forward(act, d['mix_pwr'], d['attr'], d['embed'], np.float64)
    de, da = sr.sep_backward(act, d['mix_pwr'], d['attr'], d['embed'], d['dout'], np.float64)
    assert sr.relerr(o, out.detach().numpy()) < 1e-10
    assert sr.relerr(m, masks.reshape(B, N, C).detach().numpy()) < 1e-10
    assert sr.relerr(de, embed.grad.numpy()) < 1e-10
    assert sr.relerr(da, attr.grad.numpy()) < 1e-10


def _torch_chain(d, act, mode, C, perm_idx):
    '''float64 autograd of separator -> phase re-attach -> PIT-MSE; with perm_idx the permutation is forced
    (restated in torch: pit_mse_loss has no argument for it)'''
    B, N = d['mix_pwr'].shape
    embed, attr = _t(d['embed'], True), _t(d['attr'], True)
    p, _ = R.sep_dot(_t(d['mix_pwr']).reshape(B, 1, N), attr, embed, 'softmax' if act == 0 else 'sigmoid')
    src = _t(d['src']).reshape(B, C, 1, N)
    ph = torch.complex(_t(d['phasor'][..., 0]), _t(d['phasor'][..., 1])).reshape(B, 1, 1, N)
    x, y = (src, ph * p) if mode == 0 else (src.abs(), p)
    if perm_idx is None:
        loss, perms, idx = R.pit_mse_loss(x, y)
    else:
        diff = x[:, :, None] - y[:, None, :]
        sq = diff.real ** 2 + diff.imag ** 2 if diff.is_complex() else diff ** 2
        cross = sq.mean(dim=(3, 4))
        pm = torch.tensor(sr.perms_of(C))[torch.as_tensor(perm_idx, dtype=torch.long)]
        loss = cross[torch.arange(B)[:, None], torch.arange(C)[None, :], pm].sum(dim=1).mean()
        idx = torch.as_tensor(perm_idx)
    return loss, idx, p, embed, attr


@pytest.mark.parametrize('C', [1, 2, 3, 4])
@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('variant', ['best', 'forced', 'phasor0.5', 'phasor2'])
def test_fused_chain_equals_autograd(C, act, mode, variant):
    ln = {'phasor0.5': 0.5, 'phasor2': 2.0}.get(variant, 1.0)
    d = _small(C, act, mode, 100 * C + 10 * act + mode, phasor_len=ln)
    B, N = d['mix_pwr'].shape
    p64 = sr.sep_forward(act, d['mix_pwr'], d['attr'], d['embed'], np.float64)[0]
    L, S, sig = sr.pit_cross(mode, d['src'], p64, d['phasor'], np.float64)
    loss, snr, best, v = sr.pit_reduce(L, S, sig, N, sr.EPS, np.float64)
    used = (best + 1) % math.factorial(C) if variant == 'forced' else best
    dloss, ddev = 1.7, -0.6
    tl, tidx, tp, embed, attr = _torch_chain(d, act, mode, C, used if variant == 'forced' else None)
    if variant != 'forced':
        assert np.array_equal(tidx.numpy(), best)
        assert abs(float(tl.detach()) - loss) < 1e-10 * abs(loss)
        # SNR of the complex estimate under the chosen permutation (main.py:308-309)
        pm = torch.tensor(sr.perms_of(C))[tidx]
        ph = torch.complex(_t(d['phasor'][..., 0]), _t(d['phasor'][..., 1])).reshape(B, 1, N)
        est = (ph * tp.reshape(B, C, N).detach())
        est_for_truth = torch.gather(est, 1, pm[:, :, None].expand(B, C, N))
        tsnr = R.batch_snr(_t(d['src']), est_for_truth, sr.EPS).mean()
        assert abs(float(tsnr) - snr) < 1e-10 * max(abs(snr), 1)
    tp.retain_grad()
    (tl * dloss * ddev).backward()
    scale = sr.grad_scale(B, N, dloss, ddev)
    dsep = sr.pit_dsep(mode, d['src'], p64, d['phasor'], used, scale, np.float64)
    de, da = sr.sep_backward(act, d['mix_pwr'], d['attr'], d['embed'], dsep, np.float64)
    assert sr.relerr(dsep, tp.grad.reshape(B, C, N).numpy()) < 1e-10
    assert sr.relerr(de, embed.grad.numpy()) < 1e-10
    assert sr.relerr(da, attr.grad.numpy()) < 1e-10
    if variant == 'forced' and C > 1:
        # the forced permutation's gradient is not the best one's: the rows that feed it can tell them apart
        other = sr.pit_dsep(mode, d['src'], p64, d['phasor'], best, scale, np.float64)
        assert sr.relerr(other, dsep) > 1e-2


# ------------------------------------------------------------------ permutation order, tie rule
def test_permutation_order_and_first_on_ties():
    for C in (1, 2, 3, 4):
        assert sr.perms_of(C) == list(itertools.permutations(range(C)))
        # perm_losses walks them in that order: L[i][j] = 1 except a 0 on the pairs of permutation q
        for q, perm in enumerate(sr.perms_of(C)):
            L = np.ones((1, C, C))
            L[0, np.arange(C), list(perm)] = 0
            assert sr.perm_search(sr.perm_losses(L, 1))[0] == q
        v = sr.perm_losses(np.ones((2, C, C)), 7)
        assert (sr.perm_search(v) == 0).all()
    v = np.array([[3., 1., 2., 1., 1., 5.], [2., 2., 2., 2., 2., 1.]])
    assert list(sr.perm_search(v)) == [1, 5]


# ------------------------------------------------------------------ restated constants
def test_restated_sizes_agree_with_the_library():
    from danet_amd import _lib
    ns = sorted(set(sr.SIZE_N) | set(sr.LOSS_N) | {c.N for c in sr.ALL_ROWS} | {2 * sr.CHUNK_N, 2 * sr.LOSS_CHUNK})
    for E in range(1, 65):
        want = 4 if E <= 4 else 8 if E <= 8 else 20 if E <= 20 else 40 if E <= 40 else 64
        assert sr.pick_ep(E) == want
        for N in ns:
            for B, C in ((1, 1), (3, 2), (17, 3), (2, 4)):
                assert _lib.ws_bytes(_lib.WS_SEPARATE_BWD, B, C, N, E) == sr.ws_separate_bwd(B, C, N, E) \
                    == B * sr.cdiv(N, 2048) * C * want * 4
                assert _lib.ws_bytes(_lib.WS_SEPARATE_PIT, B, C, N, E) == sr.ws_separate_pit(B, C, N, E)
                assert _lib.ws_bytes(_lib.WS_SEPARATE_PIT_GRAD, B, C, N, E) == sr.ws_partials(B, C, N, E)
                if C == 2:
                    assert sr.ws_partials(B, C, N, E) == B * sr.cdiv(N, 2048) * 2 * 2 * want * 4
    for N in ns:
        for B in (1, 3, 17, 65535):
            assert _lib.ws_bytes(_lib.WS_SEPARATE_PIT_RECORDS, B, N) == sr.ws_records(B, N) == B * sr.cdiv(N, 2048) * 33 * 4
            for C in (1, 2, 3, 4):
                assert _lib.ws_bytes(_lib.WS_PIT_MSE, B, C, N) == sr.ws_pit_mse(B, C, N) == B * sr.cdiv(N, 4096) * 33 * 4
    for c in sr.ALL_ROWS:
        if c.kind != 'loss':
            assert _lib.ws_bytes(_lib.WS_SEPARATE_PIT, c.B, c.C, c.N, c.E) == sr.ws_separate_pit(c.B, c.C, c.N, c.E)
            assert _lib.ws_bytes(_lib.WS_SEPARATE_PIT_GRAD, c.B, c.C, c.N, c.E) == sr.ws_partials(c.B, c.C, c.N, c.E)


def test_size_query_and_refused_shapes():
    '''danet_workspace_bytes answers (size_t)-1 for a bad op, a bad dim count and a negative dim (the header);
    the shape refusals of table 5 belong to the entry points, which test_gpu_sep_envelope.py checks: the query
    covers B = 0 / N = 0 (0 bytes: nothing to launch), partials at C = 3 (0 = not offered) and E = 65 (0 bytes
    of per-E scratch: pick_ep has no instantiation)'''
    from danet_amd import _lib
    for op, dims in ((_lib.WS_SEPARATE_BWD, (2, 2, 5, 4)), (_lib.WS_SEPARATE_PIT, (2, 2, 5, 4)),
                     (_lib.WS_SEPARATE_PIT_GRAD, (2, 2, 5, 4)), (_lib.WS_SEPARATE_PIT_RECORDS, (2, 5)),
                     (_lib.WS_PIT_MSE, (2, 2, 5))):
        assert _lib.ws_bytes(op, *dims) > 0
        for i in range(len(dims)):
            bad = list(dims)
            bad[i] = -1
            with pytest.raises(_lib.DanetHipError):
                _lib.ws_bytes(op, *bad)
        with pytest.raises(_lib.DanetHipError):
            _lib.ws_bytes(op, *dims[:-1])
        for i in (0, 2 if len(dims) > 2 else 1):               # B = 0, N = 0
            zero = list(dims)
            zero[i] = 0
            assert _lib.ws_bytes(op, *zero) == 0
    assert _lib.ws_bytes(_lib.WS_SEPARATE_PIT_GRAD, 2, 3, 5, 4) == 0
    assert _lib.ws_bytes(_lib.WS_SEPARATE_BWD, 2, 2, 5, 65) == 0
    assert _lib.ws_bytes(_lib.WS_SEPARATE_PIT_GRAD, 2, 2, 5, 65) == 0


# ------------------------------------------------------------------ coverage of the tables
ALL_INST = {(ep, ef, cp) for ep in sr.EPS_LIST for ef in (False, True) for cp in (1, 2, 3, 4)}


def test_tables_reach_every_instantiation():
    sep = {c.inst + (c.act,) for c in sr.SEP_ROWS}
    assert sep >= {i + (a,) for i in ALL_INST for a in (0, 1)}
    fused = {c.inst + (c.act, c.mode) for c in sr.FUSED_ROWS if not c.partials}
    assert fused >= {i + (a, m) for i in ALL_INST for a in (0, 1) for m in (0, 1)}
    part = {c.inst[:2] + (c.act, c.mode) for c in sr.FUSED_ROWS if c.partials}
    assert part >= {(ep, ef, a, m) for ep in sr.EPS_LIST for ef in (False, True) for a in (0, 1) for m in (0, 1)}
    assert all(c.C == 2 for c in sr.FUSED_ROWS if c.partials)
    loss = {(c.C, c.mode) for c in sr.LOSS_ROWS}
    assert loss == {(C, m) for C in (1, 2, 3, 4) for m in (0, 1)}
    for rows in (sr.INST_SEP, sr.INST_FUSED, sr.INST_PARTIALS):
        assert all((c.B, c.N) == (2, 2049) for c in rows)
        for ep in sr.EPS_LIST:
            es = {c.E for c in rows if c.inst[0] == ep}
            assert ep in es and any(E % 2 for E in es)
            # the guarded 16-byte path of load_row / store_row: E % 4 == 0 below EP (EP = 4 and 8 have no such E)
            assert ep in (4, 8) or any(E % 4 == 0 and E < ep for E in es)
        assert {c.E for c in rows if c.vector_guarded} == {12, 24, 44}
    assert {c.E for c in sr.INST_SEP} == set(sr.E_LIST) == {1, 3, 4, 5, 8, 12, 17, 20, 24, 33, 40, 44, 63, 64}
    # E = 64 stays at N = 2049; the largest buffer is the 17 x 32769 x 20 embedding
    assert all(c.N == 2049 for c in sr.ALL_ROWS if c.E > 40)
    assert max(c.B * c.N * max(c.E, 2 * c.C) for c in sr.ALL_ROWS) == 17 * 32769 * 20


def test_tables_contain_every_edge():
    for rows, kind in ((sr.SIZE_SEP, 'sep'), (sr.SIZE_FUSED, 'fused')):
        for E, C in ((20, 2), (7, 3)):
            sel = [c for c in rows if (c.E, c.C) == (E, C)]
            assert {c.N for c in sel} >= {1, 255, 256, 257, 2047, 2048, 2049, 4097, 16385, 32769}
            multi = {c.B for c in sel if sr.n_chunks(c.N) > 1}
            assert multi >= {1, 7, 8, 16, 17, 24}
            assert any((c.B, c.N) == (17, 32769) for c in sel)
    assert sr.n_chunks(2049) == 2 and 2049 - sr.CHUNK_N == 1            # a chunk of exactly one bin
    assert sr.loss_chunks(4097) == 2 and 4097 - sr.LOSS_CHUNK == 1
    assert sr.n_chunks(32769) == 17 and sr.loss_chunks(65537) == 17    # the second round of ordered_chunk_sum
    assert sr.cdiv(16385, 256) > 64                                     # the second grid-stride trip (64 workgroups)
    assert {c.kind for c in sr.LIMIT} == {'sep', 'fused', 'loss'}
    assert all((c.B, c.N, c.C) == (65535, 3, 2) and c.E in (0, 4) for c in sr.LIMIT)
    loss = sr.LOSS
    for C in (2, 4):
        assert {c.N for c in loss if c.C == C} >= set(sr.LOSS_N) == {1, 4095, 4096, 4097, 16385, 65537}
        assert {c.B for c in loss if c.C == C and sr.loss_chunks(c.N) > 1} >= {1, 15, 16, 17, 33}
    # the second 16-utterance round of pit_final_kernel together with more than one chunk, fused and stand-alone
    assert any(c.B > 16 and sr.n_chunks(c.N) > 1 for c in sr.FUSED_ROWS)
    assert any(c.B > 16 and sr.loss_chunks(c.N) > 1 for c in sr.LOSS_ROWS)
    # every permutation is the best one of some utterance
    for c in sr.ALL_PERMS:
        best = sr.reference(c)[0]['perm_idx']
        assert set(best) == set(range(math.factorial(c.C))), c.describe()
        assert c.B > 16 or c.C == 3
    assert {(c.kind, c.C) for c in sr.ALL_PERMS} >= {('loss', 4), ('fused', 3), ('fused', 4)}
    # options and values
    assert {(c.kind, c.C) for c in sr.TIES} == {(k, C) for k in ('loss', 'fused') for C in (2, 3, 4)}
    assert {(c.kind, c.C) for c in sr.FORCED} >= {('fused', 2), ('fused', 3), ('fused', 4), ('loss', 3), ('loss', 4)}
    assert all((c.dloss, c.dloss_dev) == (1.7, -0.6) for c in sr.DLOSS) and {c.kind for c in sr.DLOSS} == {'fused', 'loss'}
    assert {(c.kind, c.phasor_len, c.mode) for c in sr.PHASOR} == {(k, ln, m) for k in ('fused', 'loss')
                                                                 for ln in (0.5, 2.0) for m in (0, 1)}
    assert {(c.kind, c.mode) for c in sr.ZERO} == {(k, m) for k in ('fused', 'loss') for m in (0, 1)}
    assert {(c.kind, c.act, c.C) for c in sr.SAT} >= {(k, 0, C) for k in ('sep', 'fused') for C in (2, 3, 4)} | \
        {('sep', 1, 2), ('fused', 1, 2)}
    # a non-involution among the forced / best permutations of the C >= 3 gradient rows
    for c in sr.FORCED + [x for x in sr.ALL_PERMS if x.kind == 'fused']:
        if c.C >= 3:
            used = sr.reference(c)[0]['used_perm']
            perms = sr.perms_of(c.C)
            assert any(tuple(perms[q][perms[q][i]] for i in range(c.C)) != tuple(range(c.C)) for q in used), c.describe()


def test_special_inputs_are_what_they_claim():
    for c in sr.PHASOR:
        ph = sr.inputs(c)['phasor'].astype(np.float64)
        assert np.allclose(np.hypot(ph[..., 0], ph[..., 1]), c.phasor_len, rtol=1e-6)
    for c in sr.ZERO:
        d = sr.inputs(c)
        zero = (d['src'] == 0).all(axis=1)
        assert zero.any() and (d['phasor'][zero] == np.array([1, 0], np.float32)).all()
    for c in sr.SAT:
        d = sr.inputs(c)
        lg = np.einsum('bne,bce->bnc', d['embed'].astype(np.float64), d['attr'].astype(np.float64))
        assert np.abs(lg).max() <= 101 and np.abs(lg).max() >= 99
        m32 = sr.sep_masks(c.act, d['attr'], d['embed'], np.float32)
        if c.act == 0:
            s = np.sort(lg, axis=-1)
            assert (np.diff(s, axis=-1) >= 30).all()
            assert (m32.max(axis=-1) == 1).all() and (np.sort(m32, axis=-1)[..., :-1] < 1e-12).all()
        else:
            assert (np.abs(lg) >= 99).all() and ((m32 == 1) | (m32 < 1e-40)).all()
    for c in sr.NEAR_TIES:
        d, (r64, r32) = sr.inputs(c), sr.reference(c)
        assert np.array_equal(d['attr'][:, c.tie[0]], d['attr'][:, c.tie[1]]) and c.C == 2 and c.partials
        assert (r64['v'][:, 0] == r64['v'][:, 1]).all() and not r64['perm_idx'].any()
        # the references under the other permutation: the same loss, the attractor gradients' rows swapped
        o64, o32 = sr.reference_under(c, np.ones(c.B, np.int32))
        assert o64['loss'] == r64['loss'] and np.array_equal(o64['dattr'][:, ::-1], r64['dattr'])
        assert sr.relerr(o32['dattr'], o64['dattr']) < sr.F32_BAR and sr.relerr(o32['dembed'], o64['dembed']) < sr.F32_BAR
    for c in sr.TIES:
        d = sr.inputs(c)
        j1, j2 = c.tie
        if c.kind == 'loss':
            assert np.array_equal(d['sep_pwr'][:, j1], d['sep_pwr'][:, j2])
        else:
            assert np.array_equal(d['attr'][:, j1], d['attr'][:, j2])
        r64, r32 = sr.reference(c)
        perms = sr.perms_of(c.C)
        for r in (r64, r32):
            for b in range(c.B):
                q = r['perm_idx'][b]
                swapped = tuple({j1: j2, j2: j1}.get(j, j) for j in perms[q])
                q2 = perms.index(swapped)
                assert r['v'][b, q] == r['v'][b, q2] and q < q2, (c.describe(), b)     # an exact tie, the first wins
                others = np.delete(r['v'][b], [q, q2])
                assert not len(others) or (others >= r['v'][b, q]).all()
        assert np.array_equal(r64['perm_idx'], r32['perm_idx'])


def test_identically_zero_outputs_are_the_one_speaker_softmax_gradients():
    '''an output whose float64 reference is all zero has no maximum to be relative to: only dembed / dattr of a
    softmax over one speaker are, and sep_ref holds them to the size of the terms that cancel (zero_scale)'''
    for c in sr.SEP_ROWS + sr.FUSED_ROWS:
        r64, r32 = sr.reference(c)
        zero = {k for k in sr.compared_outputs(c) if k not in ('loss', 'snr') and not np.any(r64[k])}
        if c.act == 0 and c.C == 1:
            assert zero == {'dembed', 'dattr'} and not np.any(r32['dembed']) and not np.any(r32['dattr'])
            assert all(r64['zero_scale'][k] > 1e-3 * c.scale for k in zero), c.describe()
        else:
            assert not zero and 'zero_scale' not in r64, c.describe()
    for c in sr.LOSS_ROWS:
        assert np.any(sr.reference(c)[0]['dsep'])


# ------------------------------------------------------------------ the two conditions of the bar, every row
@pytest.mark.parametrize('table', ['SEP_ROWS', 'FUSED_ROWS', 'LOSS_ROWS'])
def test_both_conditions_hold_for_every_row(table):
    worst = {}
    bad = []
    for c in getattr(sr, table):
        errs = sr.restatement_errors(c)
        assert set(errs) == set(sr.compared_outputs(c))
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
            if not e < sr.F32_BAR:
                bad.append((c.name, k, e))
        if c.kind != 'sep':
            r64, r32 = sr.reference(c)
            assert np.isfinite(r64['v']).all() and np.isfinite(r64['loss']) and np.isfinite(r64['snr'])
            if not c.tie:
                gap = sr.runner_up_gap(r64['v'])
                if not (gap >= sr.GAP).all():
                    bad.append((c.name, 'runner-up gap', float(gap.min())))
                assert np.array_equal(r64['perm_idx'], r32['perm_idx']), c.describe()
    print(table, ' '.join('%s=%.1e' % kv for kv in sorted(worst.items())))
    assert not bad, bad
