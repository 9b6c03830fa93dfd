'''
GPU tests of the BPTT step's pipeline (csrc/lstm.hip, lstm_bwd_rs_kernel): at U <= 16 the owners' saved
activations arrive through LDS from the waves that idle in the gate phase, fetched two steps ahead; the
cell value is carried from step to step; the terms of the gate derivatives that do not need dh are formed
at the step's top, the bias-gradient sums one step late with a flush after the loop.  (The A/B build in
which da leaves through the idle waves one step behind, out of a double-buffered tile, passes the same
cases.)

The shapes are the smallest at which that pipeline can go wrong: T = 1 .. 5 (shorter than, equal to and
just longer than the two-step fetch depth and the one-step store lag) with a one-row second cluster
(B = 17) and a ragged unit group at U = 16 (H = 20) and U = 8 (H = 36); U = 32 (no idle waves: in-wave
fetch and store, carried cell); the flagship instantiation <16,1> with 3 twins at T = 5; ndir = 1; no
twins where the default plan has some; padded lddy / ldw with NaN in the gaps; the three bias-gradient
forms at T = 3; cells that differ by orders of magnitude between the two steps of a T = 2 sequence;
bit-equality between placements.

da and db are compared with the float64 scan of tests/lstm_layer.py at its bar, 1e-5 of each output's
maximum, under its precondition that the float32 CPU restatement stays below 1e-6.  The BPTT is fed the
kernel's own forward state of the same case, as a train step does.
'''
import numpy as np
import pytest
import torch

import lstm_layer as ll
from lstm_layer import Case

pytestmark = pytest.mark.gpu

U8, U16, U32 = {'lstm_bwd_u': 8}, {'lstm_bwd_u': 16}, {'lstm_bwd_u': 32}
PAD = (8, 4, 12, 8)        # ldw, ldy, lddy, ldx beyond the row (multiples of 4 floats)

# (case, U, twins)
TIMES = ([(Case('u16-h20-T%d' % T, 17, T, 8, 20, 2, U16, pad=PAD if T in (2, 5) else (0, 0, 0, 0)), 16, False)
          for T in (1, 2, 3, 4, 5)] +
         [(Case('u8-h36-T%d' % T, 17, T, 8, 36, 2, U8, pad=PAD if T in (1, 4) else (0, 0, 0, 0)), 8, False)
          for T in (1, 2, 3, 4, 5)])
SHAPES = [
    (Case('u32-h40-T3', 17, 3, 8, 40, 2, U32), 32, False),
    (Case('u16-ndir1-T4', 17, 4, 8, 20, 1, U16), 16, False),
    (Case('u16-twins-padded-T3', 17, 3, 8, 260, 2, pad=PAD), 16, True),
    (Case('u16-no-twins-T4', 17, 4, 8, 260, 2, {'lstm_bwd_u': 16, 'lstm_bwd_s': 1}), 16, False),
]
FLAGSHIP = Case('cfg2-T5', 32, 5, 16, 300, 2)
# T = 2 with a wide spread of cell magnitudes: a step that took c_t for c_{t-1} (or kept the first step's
# c_t) is wrong by orders of magnitude in the forget-gate column and in tanh(c)
CARRY = Case('carry-T2', 17, 2, 8, 20, 2, U16, scale=20.0)
FORMS = Case('forms-T3', 17, 3, 8, 20, 2, U16)
PLACED = Case('placed-T4', 17, 4, 8, 260, 2)


@pytest.fixture(autouse=True, scope='module')
def _device_matches_the_plans():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == ll.CUS, 'the plans are computed for %d compute units, this device has %d' % (ll.CUS, n)
    yield


def _forward_and_bptt(case):
    out, _, _ = ll.check_forward(case)
    res, _, _ = ll.check_backward(case, out['gates'], out['cell'])
    return out, res


@pytest.mark.parametrize('case,U,twins', TIMES + SHAPES, ids=[c[0].name for c in TIMES + SHAPES])
def test_short_sequences(case, U, twins):
    plan = ll.bwd_plan(case.B, case.H, case.ndir, case.opts)
    assert (plan['U'], plan['S'] > 1) == (U, twins), plan
    assert plan['G'] == 2 and case.B % 16 == 1
    _forward_and_bptt(case)


def test_flagship_instantiation_short():
    c = FLAGSHIP
    plan = ll.bwd_plan(c.B, c.H, c.ndir, c.opts)
    assert (plan['U'], plan['NTW'], plan['S']) == (16, 1, 3), plan
    _forward_and_bptt(c)


def cell_spread(case):
    '''per direction the share of (row, unit) pairs whose two cell values differ by more than 100x'''
    cells = ll.reference(case)['cell']
    out = []
    for c in cells:
        a = c.abs().numpy()
        lo, hi = a.min(axis=0), a.max(axis=0)
        out.append(float((hi > 100 * lo).mean()))
    return out


def test_carried_cell_with_a_wide_spread():
    c = CARRY
    assert c.T == 2 and all(s > 0.1 for s in cell_spread(c)), cell_spread(c)
    _forward_and_bptt(c)


def test_bias_gradient_forms_short():
    '''db == NULL, deferred + reduce and beta = 1 at T = 3: the sums are flushed after the loop'''
    c = FORMS
    plan = ll.bwd_plan(c.B, c.H, c.ndir, c.opts)
    out, _, _ = ll.check_forward(c)
    base, _, _ = ll.check_backward(c, out['gates'], out['cell'])
    g = torch.Generator().manual_seed(5)
    db0 = [torch.randn(4 * c.H, generator=g) * float(np.abs(base['db'][d]).max()) for d in range(c.ndir)]
    ll.check_backward(c, out['gates'], out['cell'], beta=1.0, db0=db0, tag=' beta=1')
    b = ll.Bwd(c, out['gates'], out['cell'], db0=db0)
    before = [t.t.clone() for t in b.db]
    res = b.run(0.0, ll.DB_DEFERRED)
    assert all(torch.equal(t.t, t0) for t, t0 in zip(b.db, before)), 'the deferred launch touched db'
    b.reduce(0.0)
    res = b.collect()
    for d in range(c.ndir):
        assert np.array_equal(res['da'][d], base['da'][d])
        assert np.array_equal(res['db'][d], base['db'][d]), 'deferred db differs from the in-call sum'
    b = ll.Bwd(c, out['gates'], out['cell'], want_db=False)
    res = b.run()
    assert all(np.array_equal(x, y) for x, y in zip(res['da'], base['da']))
    assert all(t.untouched() for t in b.db)
    assert bool((b.ws.words_from(ll.slab_offset(plan)) == ll.SENT).all()), 'db == NULL wrote the slab'


def test_placement_is_bit_equal_short():
    res = []
    for opts in ({'lstm_xmap': 0}, {'lstm_xmap': 1}):
        c = Case('%s %s' % (PLACED.name, opts), PLACED.B, PLACED.T, PLACED.D, PLACED.H, PLACED.ndir, opts,
                 seed=PLACED.seed)
        plan = ll.bwd_plan(c.B, c.H, c.ndir, opts)
        assert plan['S'] > 1 and plan['U'] == 16, plan
        res.append(_forward_and_bptt(c)[1])
    for name in ('da', 'db'):
        for a, b in zip(res[0][name], res[1][name]):
            assert np.array_equal(a, b), 'BPTT %s differs between lstm_xmap 0 and 1' % name
