'''
GPU tests of the separator and PIT-loss heads (csrc/attractor.hip, csrc/loss.hip, csrc/pit_common.h) over
everything include/danet_hip.h promises for them, called through the C entry points (danet_separate_fwd,
danet_separate_bwd, danet_pit_mse_fwd, danet_pit_mse_bwd, danet_separate_pit_fwd_records,
danet_separate_pit_final, danet_separate_pit_bwd) so that a failure names one kernel: every (EP, EF, CP)
instantiation with both activations and both loss modes (E up to 64, C up to 4), the guarded 16-byte row
path, `dattr_partials` of BOTH permutations in the buffer itself, chunks of exactly one bin, the second
round of ordered_chunk_sum and of pit_final_kernel, B = 65535, all 24 permutations, a forced permutation
that is not the best one, NULL options, dloss and *dloss_dev, phasors off the unit circle, all-zero
frames, exact ties, saturated masks, run-to-run bit-identity, and every refusal.

Every output is compared with the float64 numpy reference of tests/sep_ref.py at TOL = 1e-5 of its maximum
(loss relative, SNR against max(|snr|, 1)); perm_idx must be exact.  The bar comes with two conditions that
tests/test_sep_cpu.py asserts for every row: the float32 restatement of the same case stays below 1e-6
against float64, and outside the tie rows the runner-up permutation loses by at least 1e-3 relative.
Outputs, `records` and the exact-size workspaces sit between sentinel guards and start out as NaN: a slot
that is read without having been written poisons the result.  Saturated rows: finite gradients, masks and
forward outputs at the bar (the gradients there are exp(-30) of the inputs' size).

The estimators (danet_attractor_*), including the two consumers of `dattr_partials`, are not under test here.

Measured on an MI355X (worst kernel error | the float32 restatement's worst | worst kernel / float32 ratio of a
single row, the restatement floored at 1e-8), all against the 1e-5 bar: separate_fwd 3.2e-7 | 2.3e-7 | 1.9;
separate_bwd 3.2e-7 | 3.8e-7 | 3.4; pit_mse_fwd 3.8e-7 | 4.6e-7 | 11.3; pit_mse_bwd 3.1e-7 | 4.0e-7 | 2.9;
sep_pit_fwd (records + final) 3.3e-7 | 4.2e-7 | 6.6; sep_pit_bwd 1.2e-6 | 8.7e-7 | 3.0 (dattr at E = 1, C = 4);
dattr_partials 2.6e-7 | 2.9e-7 | 4.4.  The heads are as accurate as plain float32 and no bar had to move;
test_zz_family_report prints the table on every run.  sep_pwr_out is NOT bit-equal to danet_separate_fwd's
output (the two kernels' dot products are contracted differently) and is held to the bar; dattr with
dembed = NULL came out bit-equal to the full backward's.  The file takes 9 s (626 cases), 4 s of them the
float64 and float32 references.

Found by these tests and fixed in csrc/ (each row failed before): of two exactly tied permutations
danet_separate_pit_bwd fed `records` took the second where danet_separate_pit_final reports the first
(tie-fused-C3: dattr 4.0e-1 of its maximum, now 1.9e-7; every fused row now also asserts that the records-fed
backward and one fed part 2's perm_idx give the same bits); danet_pit_mse_bwd launched with mode = 2 instead of
returning DANET_ERR_ARG.

Found and NOT changed: at C = 2 two bit-identical attractors do not give bit-identical estimates in most
instantiations (measured: E in {4, 7, 8, 12, 20, 33, 40} x act x mode x partials; only EP = 40 with partials
does).  The compiler contracts the two speakers' dot products differently (sep_pit_fwd_kernel<20, 2, true, true>:
speaker 1 twenty fused multiply-adds, twelve of speaker 0's terms unfused), the estimates come out an ulp apart
and an "exact tie" is decided by rounding -- either index is a correct float32 answer, 1e-7 relative in the loss.
Forcing one contraction makes them identical but moves the forward's rounding, and with it every later step of a
training run; the exact-tie row at C = 2 therefore sits on an instantiation that is symmetric (E = 40 with
partials), and test_near_ties holds the E = 20 one to what the header promises there (sep_ref.NEAR_TIES).
'''
import numpy as np
import pytest
import torch

import sep_ref as sr
from sep_ref import Launch, Report

pytestmark = pytest.mark.gpu


def _ids(rows):
    return [c.name for c in rows]


def _bits(a):
    return None if a is None else np.atleast_1d(np.ascontiguousarray(a)).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _report(case, family, refs=None, **outputs):
    rep = Report(case, family, refs)
    for name, got in outputs.items():
        rep.add(name, got)
    if rep.rows:
        rep.check()
    else:
        print('%-34s %-14s finite' % (case.name, family))


# ------------------------------------------------------------------ one row of each kind
def run_sep(case):
    L = Launch(case)
    out, masks = L.separate_fwd()
    de, da = L.separate_bwd()
    return dict(out=out, masks=masks, dembed=de, dattr=da)


def check_sep(case, got=None):
    got = got or run_sep(case)
    _report(case, 'separate_fwd', out=got['out'], masks=got['masks'])
    _report(case, 'separate_bwd', dembed=got['dembed'], dattr=got['dattr'])


def run_fused(case):
    '''forward part 1 (with sep_pwr_out, with partials where the row has them), part 2, and the backward: fed the
    forward's records, or in the forced rows a perm_idx that is deliberately not the best permutation'''
    c = case
    L = Launch(c)
    out, gp = L.pit_fwd_records(sep_pwr_out=True)
    loss, snr, perm = L.pit_final()
    forced = sr.reference(c)[0]['used_perm'] if c.forced else None
    de, da = L.pit_bwd(perm_idx=forced)
    if forced is None:
        # the records-fed backward derives the SAME index as part 2 reports (the header's promise), ties and near
        # ties included: fed that perm_idx instead, the same kernel gives the same bits
        de2, da2 = L.pit_bwd(perm_idx=perm)
        assert _same_bits(de, de2) and _same_bits(da, da2), \
            '%s: the records-fed backward ran under another permutation than perm_idx reports' % c.describe()
    got = dict(out=out, loss=loss, snr=snr, perm_idx=perm, dembed=de, dattr=da, records=L.records.numpy())
    if gp is not None:
        got['gp'] = gp
    return got


def check_fused(case, got=None):
    c = case
    got = got or run_fused(c)
    r64 = sr.reference(c)[0]
    assert np.array_equal(got['perm_idx'], r64['perm_idx']), \
        '%s: perm_idx differs for utterances %s' % (c.describe(), np.nonzero(got['perm_idx'] != r64['perm_idx'])[0][:16])
    _report(c, 'sep_pit_fwd', out=got['out'], loss=got['loss'], snr=got['snr'])
    _report(c, 'sep_pit_bwd', dembed=got['dembed'], dattr=got['dattr'])
    if 'gp' in got:
        _report(c, 'dattr_partials', partials=sr.sum_partials(got['gp'], c.E, c.dloss))


def run_loss(case):
    L = Launch(case)
    loss, snr, perm = L.pit_mse_fwd()
    ds = L.pit_mse_bwd(sr.reference(case)[0]['used_perm'])
    return dict(loss=loss, snr=snr, perm_idx=perm, dsep=ds)


def check_loss(case, got=None):
    c = case
    got = got or run_loss(c)
    r64 = sr.reference(c)[0]
    assert np.array_equal(got['perm_idx'], r64['perm_idx']), \
        '%s: perm_idx differs for utterances %s' % (c.describe(), np.nonzero(got['perm_idx'] != r64['perm_idx'])[0][:16])
    _report(c, 'pit_mse_fwd', loss=got['loss'], snr=got['snr'])
    _report(c, 'pit_mse_bwd', dsep=got['dsep'])


RUN = {'sep': (run_sep, check_sep), 'fused': (run_fused, check_fused), 'loss': (run_loss, check_loss)}


def check(case):
    RUN[case.kind][1](case)


# ------------------------------------------------------------------ 1. the instantiation matrix
@pytest.mark.parametrize('case', sr.INST_SEP, ids=_ids(sr.INST_SEP))
def test_separator_instantiations(case):
    check(case)


@pytest.mark.parametrize('case', sr.INST_FUSED, ids=_ids(sr.INST_FUSED))
def test_fused_instantiations(case):
    check(case)


@pytest.mark.parametrize('case', sr.INST_PARTIALS, ids=_ids(sr.INST_PARTIALS))
def test_fused_instantiations_with_partials(case):
    check(case)


# ------------------------------------------------------------------ 2. size edges, each run twice
@pytest.mark.parametrize('case', sr.REPEATED, ids=_ids(sr.REPEATED))
def test_size_edges_and_repeatability(case):
    run, chk = RUN[case.kind]
    first = run(case)
    chk(case, first)
    second = run(case)
    for k in first:
        assert _same_bits(np.asarray(first[k]), np.asarray(second[k])), '%s: %s differs between two runs' % (case, k)


@pytest.mark.parametrize('case', sr.LIMIT, ids=_ids(sr.LIMIT))
def test_batch_limit(case):
    check(case)


# ------------------------------------------------------------------ 3. the stand-alone loss, every permutation
@pytest.mark.parametrize('case', sr.LOSS, ids=_ids(sr.LOSS))
def test_standalone_loss(case):
    check(case)


@pytest.mark.parametrize('case', sr.ALL_PERMS, ids=_ids(sr.ALL_PERMS))
def test_every_permutation_is_found(case):
    check(case)


# ------------------------------------------------------------------ 4. options and values
_VALUES = sr.FORCED + sr.DLOSS + sr.PHASOR + sr.ZERO + sr.TIES + sr.SAT


@pytest.mark.parametrize('case', _VALUES, ids=_ids(_VALUES))
def test_values(case):
    check(case)


@pytest.mark.parametrize('case', sr.NEAR_TIES, ids=_ids(sr.NEAR_TIES))
def test_near_ties(case):
    '''identical attractors whose estimates the kernel leaves an ulp apart (sep_ref.NEAR_TIES): either index is a
    correct float32 answer; it must be a minimum to rounding, the backward must run under it (run_fused), and loss,
    SNR, gradients and partials are those of that permutation at the bar'''
    c = case
    got = run_fused(c)
    v, perm = sr.reference(c)[0]['v'], got['perm_idx']
    assert (v[np.arange(c.B), perm] <= v.min(axis=1) * (1 + 1e-6)).all(), (perm, v)
    print('%s: estimates of the two identical attractors %s' % (
        c.name, 'are bit-identical' if _same_bits(got['out'][:, 0], got['out'][:, 1]) else 'DIFFER'), 'perm_idx', perm)
    refs = sr.reference_under(c, perm)
    _report(c, 'sep_pit_fwd', refs, out=got['out'], loss=got['loss'], snr=got['snr'])
    _report(c, 'sep_pit_bwd', refs, dembed=got['dembed'], dattr=got['dattr'])
    _report(c, 'dattr_partials', refs, partials=sr.sum_partials(got['gp'], c.E, c.dloss))


def test_separator_options():
    c = sr.OPTION_SEP
    got = run_sep(c)
    check_sep(c, got)
    out_only, none = Launch(c).separate_fwd(masks=False)
    assert none is None and _same_bits(out_only, got['out'])


@pytest.mark.parametrize('case', sr.OPTION_FUSED, ids=_ids(sr.OPTION_FUSED))
def test_fused_options(case):
    c = case
    got = run_fused(c)
    check_fused(c, got)
    r64 = sr.reference(c)[0]
    # sep_pwr_out NULL: the same records; partials NULL (another instantiation): records at the bar via loss
    L = Launch(c)
    out, gp = L.pit_fwd_records(sep_pwr_out=False)
    assert out is None and _same_bits(L.records.numpy(), got['records'])
    if gp is not None:
        assert _same_bits(gp, got['gp'])
        L2 = Launch(c)
        L2.pit_fwd_records(sep_pwr_out=False, partials=False)
        loss2, snr2, perm2 = L2.pit_final()
        assert np.array_equal(perm2, r64['perm_idx'])
        _report(c, 'sep_pit_fwd', loss=loss2, snr=snr2)
    # sep_pwr_out against danet_separate_fwd's output of the same inputs
    sep_out, _ = Launch(c).separate_fwd(masks=False)
    print('%s: sep_pwr_out %s danet_separate_fwd bit for bit' % (c.name, 'equals' if _same_bits(sep_out, got['out'])
                                                                else 'DIFFERS from'))
    _report(c, 'separate_fwd', out=sep_out)
    # snr NULL: the same loss and permutation
    loss, snr, perm = L.pit_final(snr=False)
    assert snr is None and _same_bits(np.float32(loss), np.float32(got['loss'])) and np.array_equal(perm, got['perm_idx'])
    # fed perm_idx (the best one) instead of records: the same kernel under the same permutation
    de, da = L.pit_bwd(perm_idx=got['perm_idx'])
    assert _same_bits(de, got['dembed']) and _same_bits(da, got['dattr'])
    # dembed NULL: dattr alone (another code path of the kernel: at the bar)
    none, da = L.pit_bwd(dembed=False)
    assert none is None
    print('%s: dattr with dembed = NULL %s the full backward bit for bit' % (
        c.name, 'equals' if _same_bits(da, got['dattr']) else 'DIFFERS from'))
    _report(c, 'sep_pit_bwd', dattr=da)


def test_loss_options():
    c = sr.OPTION_LOSS
    got = run_loss(c)
    check_loss(c, got)
    loss, snr, perm = Launch(c).pit_mse_fwd(snr=False)
    assert snr is None and _same_bits(np.float32(loss), np.float32(got['loss'])) and np.array_equal(perm, got['perm_idx'])


# ------------------------------------------------------------------ 5. refusals
def _refusal_args(ep):
    '''valid arguments at the base shape: device inputs, every output (and the workspace) a guarded buffer'''
    a = dict(sr.BASE)
    B, C, N, E = a['B'], a['C'], a['N'], a['E']
    rng = np.random.RandomState(5)
    f = lambda *s: sr.dev(rng.rand(*s).astype(np.float32))
    a.update(dloss_dev=None, mix_pwr=f(B, N), attr=f(B, C, E), embed=f(B, N, E), dout=f(B, C, N), src=f(B, C, N, 2),
             phasor=f(B, N, 2), sep_pwr=f(B, C, N))
    outs = dict(out=B * C * N, masks=B * N * C, dembed=B * N * E, dattr=B * C * E, loss=1, snr=1, perm_idx=B,
                dsep=B * C * N, sep_pwr_out=B * C * N, records=sr.ws_records(B, N) // 4, dattr_partials=None,
                ws=sr.WS_OF[ep](a) // 4 if ep in sr.WS_OF else None)
    # what this entry point READS is a valid input (nothing is launched, but nothing here may depend on that)
    if ep in ('danet_pit_mse_bwd', 'danet_separate_pit_bwd'):
        a['perm_idx'] = torch.zeros(B, dtype=torch.int32, device='cuda')
        del outs['perm_idx']
    if ep in ('danet_separate_pit_final', 'danet_separate_pit_bwd'):
        a['records'] = torch.zeros(sr.ws_records(B, N) // 4, device='cuda')
        del outs['records']
    guards = {}
    for k, n in outs.items():
        if k in sr.SIGS[ep]:
            guards[k] = a[k] = None if n is None else sr.Guarded(n, torch.int32 if k == 'perm_idx' else None)
    if ep in sr.WS_OF:
        a['ws_bytes'] = sr.WS_OF[ep](a)
    return a, guards


_REFUSALS = sr.refusals()


@pytest.mark.parametrize('ep,change,want', _REFUSALS,
                         ids=['%s-%s' % (ep[6:], '-'.join('%s=%s' % kv for kv in ch.items())) for ep, ch, _ in _REFUSALS])
def test_refusals(ep, change, want):
    a, guards = _refusal_args(ep)
    for k, v in change.items():
        if k == 'ws_short':
            a['ws_bytes'] -= v
        elif v == 'given':
            guards[k] = a[k] = sr.Guarded(sr.ws_partials(2, 2, a['N'], a['E']) // 4)
        else:
            a[k] = v
    rc = sr.call(ep, a)
    torch.cuda.synchronize()
    assert rc == want, '%s(%s) returned %d, not %d' % (ep, change, rc, want)
    for k, g in guards.items():
        assert g is None or g.untouched(), '%s(%s) touched %s' % (ep, change, k)


# ------------------------------------------------------------------ measured values
def test_zz_family_report():
    print()
    print('family           worst kernel error | float32 restatement | worst kernel / float32 ratio (bar %g)' % sr.TOL)
    for fam, (k, f, r) in sorted(Report.families.items()):
        print('%-16s %.1e | %.1e | %.1f' % (fam, k, f, r))
    assert Report.families, 'run with the rest of the file'
