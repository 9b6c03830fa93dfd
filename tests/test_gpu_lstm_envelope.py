'''
GPU tests of the recurrent kernels (csrc/lstm.hip) across the whole envelope include/danet_hip.h
promises, called through the C entry points (danet_lstm_fwd, danet_lstm_fwd_fused, danet_lstm_bwd,
danet_lstm_bwd_db_reduce, danet_lstm_fwd_prefill, danet_lstm_train_prefill) so that a failure names a
recurrent kernel and not a GEMM: all fifteen lstm_bwd_rs_kernel<U, NTW> instantiations, the five
hoisted and four fused forward instantiations, the options that change the launch geometry
(lstm_bwd_u, lstm_bwd_s, lstm_xmap, lstm_bwd_twin_xcd, lstm_fwd_small, lstm_fwd_un, lstm_fwd_fused),
ragged batches and unit groups, leading dimensions larger than the rows, both status forms, every
prefill form, deferred and accumulated bias gradients, dirty workspaces, saturated gates, T from 1
to 1251, and the edges of the two envelope queries.

Every case is compared with the float64 scan of tests/lstm_layer.py at TOL = 1e-5 of each output's
maximum (y, gates, cell; da, db), per direction, and once more on the ragged last unit group and the
ragged last row cluster alone.  The bar comes with a condition: the float32 CPU restatement of the
same case must itself stay below 1e-6 against float64, so that the bar never sits within a factor of
ten of plain float32 rounding; a case that breaks the condition is a badly chosen input.  Outputs
and the exact-size workspace sit between sentinel guards, padded leading dimensions hold a NaN in
the gaps of the inputs, and every launch's status word must read 0 (tests/lstm_layer.py).  The BPTT
is fed the kernel's own saved gates and cells of the same case (what a train step does) and, once
per U, the float32-rounded reference gates and cells, so that a forward fault can neither mask nor
fake a backward one.  Which instantiation a case runs is not observable through the ABI: it rests
on the restated plans of tests/lstm_layer.py, which tests/test_lstm_envelope_cpu.py anchors to the
library's workspace sizes and envelope queries and checks against these tables.

Non-finite data are not fed on purpose: the forward's exchange reads the bit pattern 0xFFFFFFFF, a
NaN, as "not yet published", and nothing here sets lstm_fault_inject or lowers lstm_spin_limit.

Measured on an MI355X with the library of commit d4bda7f (worst kernel error | the float32
restatement's worst | worst kernel / float32 ratio of a single case), all against the 1e-5 bar:
MFMA forward 3.4e-7 | 5.1e-7 | 2.0; small forward 3.1e-7 | 4.4e-7 | 1.3; fused forward 3.7e-7 | 5.1e-7 |
1.8; BPTT U = 8 6.2e-7 | 7.5e-7 | 1.6; U = 16 3.9e-7 | 5.2e-7 | 1.1; U = 32 5.1e-7 | 4.9e-7 | 1.9.  The
recurrent kernels are as accurate as plain float32; test_zz_family_report prints the table on every
run.  The file takes 17 s, 15 s of them the float64 and float32 CPU scans of the T = 512 case.
'''
import numpy as np
import pytest
import torch

import lstm_layer as ll
from lstm_layer import Case

pytestmark = pytest.mark.gpu

TOL = ll.TOL

U8, U16, U32 = {'lstm_bwd_u': 8}, {'lstm_bwd_u': 16}, {'lstm_bwd_u': 32}
PAD = (8, 4, 12, 8)        # ldw, ldy, lddy, ldx beyond the row (multiples of 4 floats: 16-byte rows)


def _o(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


# ------------------------------------------------------------------ the BPTT matrix
# (case, U, NTW, S > 1, NI) -- the plan each case is expected to get (csrc/lstm.hip, make_rs_plan /
# choose_rs_plan; tests/test_lstm_envelope_cpu.py recomputes it).  Every case runs the hoisted forward
# first, so the wide ones (H >= 388) are also the forward cases whose weight pieces spill to LDS.
BPTT = [
    # U = 8 (fp32 MFMA)
    (Case('u8-ntw1-tiny', 15, 3, 8, 20, 2, pad=PAD), 8, 1, False, 1),
    (Case('u8-ntw1-twins', 1, 4, 12, 260, 1, status='null'), 8, 1, True, 3),
    (Case('u8-ntw2', 33, 3, 16, 172, 2, pad=PAD, status='null'), 8, 2, False, 2),
    (Case('u8-ntw2-twins-ni5', 1, 3, 16, 516, 1, U8), 8, 2, True, 5),
    (Case('u8-ntw3', 17, 6, 24, 340, 2), 8, 3, False, 3),
    (Case('u8-ntw3-twins', 1, 3, 16, 516, 1, _o(U8, {'lstm_bwd_s': 2}), pad=PAD), 8, 3, True, 5),
    (Case('u8-ntw4', 33, 3, 16, 388, 1, U8, status='null'), 8, 4, False, 4),
    (Case('u8-ntw5-ni5', 17, 3, 16, 516, 1, U8, pad=PAD), 8, 5, False, 5),
    # U = 16 (six-piece bf16 MFMA)
    (Case('u16-ntw1-pinned', 15, 3, 8, 20, 2, U16), 16, 1, False, 1),
    (Case('u16-ntw1-b200', 200, 3, 16, 76, 2, status='null'), 16, 1, False, 1),
    (Case('u16-ntw1-twins', 17, 4, 24, 260, 2, pad=PAD), 16, 1, True, 3),
    (Case('u16-ntw1-s5-ni5', 1, 3, 16, 516, 1), 16, 1, True, 5),
    (Case('u16-ntw2', 97, 3, 16, 148, 2), 16, 2, False, 2),
    (Case('u16-ntw2-wide-default', 17, 3, 16, 388, 2, pad=PAD, status='null'), 16, 2, True, 4),
    (Case('u16-ntw2-h608', 17, 3, 16, 608, 1), 16, 2, True, 5),
    (Case('u16-ntw3', 49, 3, 16, 324, 2), 16, 3, False, 3),
    (Case('u16-ntw3-twins-ni5', 33, 3, 16, 516, 1, pad=PAD), 16, 3, True, 5),
    (Case('u16-ntw4', 96, 3, 16, 388, 1, status='null'), 16, 4, False, 4),
    (Case('u16-ntw5-ni5', 17, 3, 16, 516, 2), 16, 5, False, 5),
    # U = 32 (six-piece bf16 MFMA, owner-side split)
    (Case('u32-ntw1-pinned', 15, 3, 8, 20, 2, U32, pad=PAD), 32, 1, False, 1),
    (Case('u32-ntw1-twins', 33, 3, 16, 340, 2, status='null'), 32, 1, True, 3),
    (Case('u32-ntw1-wide-partner', 17, 3, 16, 388, 2, U32, pad=PAD), 32, 1, True, 4),
    (Case('u32-ntw2', 193, 3, 16, 148, 2), 32, 2, False, 2),                       # BPTT only
    (Case('u32-ntw2-pinned', 193, 3, 16, 132, 2, U32), 32, 2, False, 2),
    (Case('u32-ntw2-twins-ni5', 17, 3, 16, 516, 2, U32, status='null'), 32, 2, True, 5),
    (Case('u32-ntw3', 97, 3, 16, 292, 2, pad=PAD), 32, 3, False, 3),               # BPTT only
    (Case('u32-ntw3-twins-ni5', 17, 3, 16, 516, 2, _o(U32, {'lstm_bwd_s': 2})), 32, 3, True, 5),
    (Case('u32-ntw4', 96, 3, 16, 388, 2), 32, 4, False, 4),                        # BPTT only
    (Case('u32-ntw4-pinned', 17, 3, 16, 388, 2, _o(U32, {'lstm_bwd_s': 1}), pad=PAD), 32, 4, False, 4),
    (Case('u32-ntw5-ni5', 128, 3, 16, 516, 1, status='null'), 32, 5, False, 5),    # BPTT only
]
# shapes inside the BPTT's envelope whose forward does not fit one workgroup per CU (danet_lstm_fwd answers
# DANET_ERR_UNSUPPORTED): the default plan reaches these instantiations only there, so the BPTT runs on the
# float32-rounded reference gates and cells; the pinned neighbours run behind the kernel's own forward
BPTT_ONLY = ('u32-ntw2', 'u32-ntw3', 'u32-ntw4', 'u32-ntw5-ni5')
# cases whose BPTT is fed the float32-rounded REFERENCE gates and cells as well (one per U)
REF_FED = ('u8-ntw3', 'u16-ntw1-twins', 'u32-ntw1-twins')

# ------------------------------------------------------------------ placement
# (case, ncl, padded twin grid has idle workgroups, twin order falls back) at S > 1.  Each case runs
# with the defaults (lstm_bwd_twin_xcd = 1), with lstm_bwd_twin_xcd = 0 (xmap 1) and with
# lstm_xmap = 0; placement changes who computes, not what: the results must be bit-equal.
PLACEMENT = [
    (Case('place-ncl1-padded', 1, 3, 16, 516, 1), 1, True, False),
    (Case('place-ncl2-padded', 1, 4, 12, 260, 2), 2, True, False),
    (Case('place-ncl4-padded', 17, 4, 24, 260, 2), 4, True, False),
    (Case('place-ncl8', 49, 3, 16, 260, 2), 8, False, False),
    (Case('place-ncl4-fallback', 17, 3, 16, 324, 2), 4, False, True),
]
PLACEMENT_OPTS = [{}, {'lstm_bwd_twin_xcd': 0}, {'lstm_xmap': 0}]

# ------------------------------------------------------------------ ring depth and time
TIMES = [Case('time-T%d' % T, 20, T, 16, 36, 2) for T in (1, 2, 3, 4, 5, 7)]
LONG = Case('time-T512-cfg2', 16, 512, 24, 300, 2)
LONG_B1 = Case('time-T1251-b1', 1, 1251, 24, 300, 2)          # forward only, the small kernel

# ------------------------------------------------------------------ hoisted forward instantiations
# (case, kernel); the BPTT matrix adds fwd<1,4,8> at H = 388 .. 608 (weight pieces in LDS)
FORWARD = [
    (Case('fwd-mt2-default', 81, 3, 16, 300, 2), 'fwd<2,4,8>'),
    (Case('fwd-mt2-forced', 64, 3, 16, 300, 2, {'lstm_fwd_un': 8}, pad=PAD), 'fwd<2,4,8>'),
    (Case('fwd-un12-default', 64, 3, 16, 300, 2), 'fwd<1,4,12>'),
    (Case('fwd-un12-forced', 17, 3, 16, 100, 2, {'lstm_fwd_un': 12}, pad=PAD, status='null'), 'fwd<1,4,12>'),
    (Case('fwd-un12-h608', 33, 3, 16, 608, 1, {'lstm_fwd_un': 12}), 'fwd<1,4,12>'),
    (Case('fwd-h608-b48', 48, 3, 16, 608, 1), 'fwd<1,4,8>'),
    (Case('fwd-b5-outside-small', 5, 4, 12, 36, 2), 'fwd<1,4,8>'),
    (Case('small1-h4', 1, 5, 8, 4, 2, pad=PAD), 'small<1>'),
    (Case('small1-h36', 1, 5, 8, 36, 1, status='null'), 'small<1>'),
    (Case('small1-h320', 1, 4, 16, 320, 2), 'small<1>'),
    (Case('small4-b2-h4', 2, 5, 8, 4, 1), 'small<4>'),
    (Case('small4-b3-h132', 3, 4, 8, 132, 2, pad=PAD), 'small<4>'),
    (Case('small4-b4-h320', 4, 4, 16, 320, 2, status='null'), 'small<4>'),
    (Case('small-h324-outside', 3, 3, 16, 324, 1), 'fwd<1,4,8>'),
    (Case('mfma-b1-h36', 1, 5, 8, 36, 1, {'lstm_fwd_small': 0}), 'fwd<1,4,8>'),
    (Case('mfma-b3-h132', 3, 4, 8, 132, 2, {'lstm_fwd_small': 0}, pad=PAD), 'fwd<1,4,8>'),
    (Case('mfma-b4-h320', 4, 4, 16, 320, 2, {'lstm_fwd_small': 0}), 'fwd<1,4,8>'),
]

# ------------------------------------------------------------------ fused forward instantiations
FX1 = {'lstm_fwd_fused': 1}     # B < 24 takes the fused kernel only when forced
# x of the wide-input cases (D >= 320) is scaled down: with x ~ 0.7 randn the float32 restatement's own
# x Wx sum over D terms misses 1e-6 (1.1e-6 .. 2.7e-6 measured on the CPU), i.e. the input, not the bar, is wrong
WIDE = 0.2
FUSED = [
    (Case('fx21-d8', 20, 3, 8, 36, 2, FX1), 'fx<2,1>'),
    (Case('fx21-d150', 17, 3, 150, 64, 2, FX1, pad=PAD, scale=0.5), 'fx<2,1>'),
    (Case('fx21-d160', 32, 3, 160, 300, 2, scale=0.5), 'fx<2,1>'),
    (Case('fx42-d161-h320', 20, 3, 161, 320, 1, FX1, status='null', scale=0.5), 'fx<4,2>'),
    (Case('fx42-d164', 15, 3, 164, 36, 2, FX1, scale=0.5), 'fx<4,2>'),
    (Case('fx42-d320', 17, 3, 320, 132, 2, FX1, pad=PAD, scale=WIDE), 'fx<4,2>'),
    (Case('fx83-d324', 33, 3, 324, 64, 1, scale=WIDE), 'fx<8,3>'),
    (Case('fx83-d600-cfg2', 32, 4, 600, 300, 2, status='null', scale=WIDE), 'fx<8,3>'),
    (Case('fx83-d608', 17, 3, 608, 36, 2, FX1, pad=PAD, scale=WIDE), 'fx<8,3>'),
    (Case('fx84-d612', 17, 3, 612, 64, 2, FX1, scale=WIDE), 'fx<8,4>'),
    (Case('fx84-d630', 5, 3, 630, 36, 1, FX1, pad=PAD, scale=WIDE), 'fx<8,4>'),
    (Case('fx84-d640-h320', 20, 3, 640, 320, 1, FX1, scale=WIDE), 'fx<8,4>'),
]

# ------------------------------------------------------------------ saturated gates
# biases put the pre-activations of half of the units at +-20, +-90 and +-200 (every level in every
# gate) next to ordinary units; forward (hoisted and fused) and the BPTT at every U
SATURATED = [Case('sat-u16', 17, 4, 16, 72, 2, _o(U16, FX1), sat=True),
             Case('sat-u8', 17, 4, 16, 72, 2, U8, sat=True, pad=PAD),
             Case('sat-u32', 17, 4, 16, 72, 2, U32, sat=True),
             Case('sat-small', 3, 4, 16, 72, 2, sat=True)]

FLAGS = Case('flags', 32, 5, 16, 64, 2, pad=PAD)
FLAGS_RAGGED = Case('flags-ragged', 33, 4, 16, 172, 2)         # 3 clusters, the last with one row

# last supported / first unsupported B on 256 CUs (danet_lstm_bwd_db_supported): (H, ndir, B)
BWD_EDGES = [(300, 2, 192), (300, 1, 400), (600, 2, 96), (600, 1, 208)]
# danet_lstm_fwd_fused_supported: ndir * ceil(B / 16) * ceil(H / 8) <= 256, H <= 320
FX_EDGES = [(300, 2, 48), (300, 1, 96), (320, 2, 48), (320, 1, 96)]

_family = {}


def _note(family, k, f):
    w = _family.setdefault(family, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], k), max(w[1], f), max(w[2], k / max(f, 1e-30))


def _fwd_family(kernel):
    return 'small forward' if kernel.startswith('small') else ('fused forward' if kernel.startswith('fx') else 'MFMA forward')


@pytest.fixture(autouse=True, scope='module')
def _device_matches_the_tables():
    '''the expectations in the tables are computed for 256 compute units (gfx950)'''
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == ll.CUS, 'the case tables assume %d compute units, this device has %d' % (ll.CUS, n)
    yield


def _reference_state(case):
    r = ll.reference(case)
    return dict(gates=[g.float().numpy() for g in r['gates']], cell=[c.float().numpy() for c in r['cell']])


def _forward_and_bptt(case):
    kernel = ll.fwd_plan(case.B, case.H, case.ndir, case.opts)['kernel']
    if kernel is None:
        # the BPTT's envelope is wider than the forward's (BPTT_ONLY): float32-rounded reference state
        assert case.name in BPTT_ONLY, case.describe()
        out = _reference_state(case)
    else:
        out, k, f = ll.check_forward(case)
        _note(_fwd_family(kernel), k, f)
    res, k, f = ll.check_backward(case, out['gates'], out['cell'])
    _note('BPTT U=%d' % ll.bwd_plan(case.B, case.H, case.ndir, case.opts)['U'], k, f)
    return out, res


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize('case,U,NTW,twins,NI', BPTT, ids=[c[0].name for c in BPTT])
def test_bptt_instantiation(case, U, NTW, twins, NI):
    plan = ll.bwd_plan(case.B, case.H, case.ndir, case.opts)
    assert (plan['U'], plan['NTW'], plan['S'] > 1, plan['NI']) == (U, NTW, twins, NI), plan
    out, _ = _forward_and_bptt(case)
    if case.name in REF_FED:
        st = _reference_state(case)
        _, k, f = ll.check_backward(case, st['gates'], st['cell'], tag=' ref-fed')
        _note('BPTT U=%d' % U, k, f)


@pytest.mark.parametrize('case,ncl,padded,fallback', PLACEMENT, ids=[c[0].name for c in PLACEMENT])
def test_placement_is_bit_equal(case, ncl, padded, fallback):
    res = []
    for opts in PLACEMENT_OPTS:
        c = Case('%s %s' % (case.name, opts or 'default'), case.B, case.T, case.D, case.H, case.ndir, opts,
                 seed=case.seed)
        plan = ll.bwd_plan(c.B, c.H, c.ndir, opts)
        assert plan['ncl'] == ncl and plan['S'] > 1
        if not opts:
            assert plan['xmap'] == (1 if fallback else 2) and plan['twin_fallback'] == fallback
            assert (plan.get('idle', 0) > 0) == padded
        else:
            assert plan['xmap'] == opts.get('lstm_xmap', 1)
        res.append(_forward_and_bptt(c))
    for out, bw in res[1:]:
        for name in ('y', 'gates', 'cell'):
            for a, b in zip(out[name], res[0][0][name]):
                assert np.array_equal(a, b), 'forward %s differs between placements' % name
        for name in ('da', 'db'):
            for a, b in zip(bw[name], res[0][1][name]):
                assert np.array_equal(a, b), 'BPTT %s differs between placements' % name


@pytest.mark.parametrize('case', TIMES, ids=[c.name for c in TIMES])
def test_ring_depth_and_short_sequences(case):
    _forward_and_bptt(case)


def test_long_sequence_cfg2_width():
    '''T = 512: the phase bit in the LSB of the exchanged partial dh over a long sequence'''
    _forward_and_bptt(LONG)


def test_long_sequence_single_row_forward():
    '''T = 1251, B = 1: the inference shape on the small kernel, forward only'''
    assert ll.fwd_plan(1, 300, 2)['kernel'] == 'small<1>'
    _, k, f = ll.check_forward(LONG_B1)
    _note('small forward', k, f)


@pytest.mark.parametrize('case,kernel', FORWARD, ids=[c[0].name for c in FORWARD])
def test_forward_instantiation(case, kernel):
    assert ll.fwd_plan(case.B, case.H, case.ndir, case.opts)['kernel'] == kernel
    _, k, f = ll.check_forward(case)
    _note(_fwd_family(kernel), k, f)


@pytest.mark.parametrize('case,kernel', FUSED, ids=[c[0].name for c in FUSED])
def test_fused_forward_instantiation(case, kernel):
    '''the fused and the hoisted forward of one case, each against float64 (not against each other)'''
    from danet_amd import _lib
    assert ll.fx_plan(case.B, case.H, case.ndir, case.D, case.opts)['kernel'] == kernel
    with ll.set_options(case.opts):
        assert _lib.load().danet_lstm_fwd_fused_supported(case.T, case.B, case.H, case.ndir, case.D) == 1
    _, k, f = ll.check_forward(case, fused=True)
    _note('fused forward', k, f)
    _, k, f = ll.check_forward(case)
    _note(_fwd_family(ll.fwd_plan(case.B, case.H, case.ndir, case.opts)['kernel']), k, f)


@pytest.mark.parametrize('case', SATURATED, ids=[c.name for c in SATURATED])
def test_saturated_gates(case):
    inp = ll.inputs(case)
    assert float(inp['gx'][0].abs().max()) > 150 and all(torch.isfinite(t).all() for t in inp['gx'])
    _forward_and_bptt(case)
    if case.opts.get('lstm_fwd_fused') == 1:
        _, k, f = ll.check_forward(case, fused=True)
        _note('fused forward', k, f)


def _same(a, b):
    return all(np.array_equal(x, y) for n in a for x, y in zip(a[n], b[n]))


def test_prefill_forms_are_bit_equal():
    '''in-call prefill, danet_lstm_fwd_prefill (n = 3 launches by one call) and
    danet_lstm_train_prefill: the same results, bit for bit, forward and BPTT'''
    c = FLAGS
    base, _, _ = ll.check_forward(c)
    base_b, _, _ = ll.check_backward(c, base['gates'], base['cell'])
    f0 = ll.Fwd(c)
    for f in [f0] + f0.prefill(n_extra=2):
        assert _same(f.run(ll.PREFILLED), base)
    for fused in (False, True):
        fw = [ll.Fwd(c, fused) for _ in range(3)]
        bw = [ll.Bwd(c, base['gates'], base['cell']) for _ in range(3)]
        ll.train_prefill(fw, bw)
        for f, b in zip(fw, bw):
            out = f.run(ll.PREFILLED)
            if not fused:
                assert _same(out, base)
            assert _same(b.run(0.0, ll.PREFILLED), base_b)
    ff = ll.Fwd(c, fused=True)
    ff.prefill()
    with_prefill = ff.run(ll.PREFILLED)
    in_call, k, f = ll.check_forward(c, fused=True)
    _note('fused forward', k, f)
    assert _same(with_prefill, in_call)


@pytest.mark.parametrize('case', [FLAGS, FLAGS_RAGGED], ids=['flags', 'flags-ragged'])
def test_bias_gradient_forms(case):
    '''deferred + reduce, beta = 1 and db == NULL against float64; db == NULL leaves the slab alone'''
    c = case
    out, _, _ = ll.check_forward(c)
    base, k, f = ll.check_backward(c, out['gates'], out['cell'])
    plan = ll.bwd_plan(c.B, c.H, c.ndir, c.opts)
    fam = 'BPTT U=%d' % plan['U']
    _note(fam, k, f)
    # beta = 1 onto a db of the gradient's own size
    g = torch.Generator().manual_seed(5)
    db0 = [torch.randn(4 * c.H, generator=g) * float(np.abs(base['db'][d]).max()) for d in range(c.ndir)]
    _, k, f = ll.check_backward(c, out['gates'], out['cell'], beta=1.0, db0=db0, tag=' beta=1')
    _note(fam, k, f)
    # deferred: db untouched by the launch, then finished by the reduce call (beta 0 and 1)
    for beta in (0.0, 1.0):
        b = ll.Bwd(c, out['gates'], out['cell'], db0=db0)
        before = [t.t.clone() for t in b.db]
        res = b.run(beta, ll.DB_DEFERRED)
        assert all(torch.equal(t.t, t0) for t, t0 in zip(b.db, before)), 'the deferred launch touched db'
        b.reduce(beta)
        res = b.collect()
        r64, r32 = ll.reference(c), ll.reference(c, f32=True)
        rep = ll.Report(c)
        for d in range(c.ndir):
            add = db0[d].double().numpy() * beta
            rep.add(plan, 'db[%d]' % d, res['db'][d], r64['db'][d].numpy() + add, r32['db'][d].numpy() + add)
            assert np.array_equal(res['da'][d], base['da'][d])
            if beta == 0.0:
                assert np.array_equal(res['db'][d], base['db'][d]), 'deferred db differs from the in-call sum'
        _note(fam, *rep.check(fam + ' deferred'))
    # db == NULL: da as before, db buffers and the slab region of the workspace untouched
    b = ll.Bwd(c, out['gates'], out['cell'], want_db=False)
    res = b.run()
    assert all(np.array_equal(x, y) for x, y in zip(res['da'], base['da']))
    assert all(t.untouched() for t in b.db)
    assert bool((b.ws.words_from(ll.slab_offset(plan)) == ll.SENT).all()), 'db == NULL wrote the slab'


@pytest.mark.parametrize('case', [FLAGS] + [c[0] for c in BPTT if c[0].name in ('u16-ntw1-twins', 'u32-ntw1-twins')], ids=['flags', 'u16-twins', 'u32-twins'])
def test_rerun_on_dirty_buffers_is_bit_equal(case):
    '''the kernels must not depend on what the previous launch left in workspace and outputs'''
    for fused in (False, True) if case is FLAGS else (False,):
        f = ll.Fwd(case, fused)
        first = f.run()
        assert _same(f.run(), first)
    b = ll.Bwd(case, first['gates'], first['cell'])
    one = b.run()
    assert _same(b.run(), one)
    # and a workspace a FORWARD launch used before
    b2 = ll.Bwd(case, first['gates'], first['cell'])
    b2.ws = f.ws
    assert _same(b2.run(), one)


def test_envelope_queries_at_their_edges():
    from danet_amd import _lib
    L = _lib.load()
    for H, ndir, B in BWD_EDGES:
        assert L.danet_lstm_bwd_db_supported(8, B, H, ndir) == 1, (H, ndir, B)
        assert L.danet_lstm_bwd_db_supported(8, B + 1, H, ndir) == 0, (H, ndir, B + 1)
    _lib.set_option('lstm_fwd_fused', 1)
    for H, ndir, B in FX_EDGES:
        assert L.danet_lstm_fwd_fused_supported(8, B, H, ndir, 64) == 1, (H, ndir, B)
        assert L.danet_lstm_fwd_fused_supported(8, B + 1, H, ndir, 64) == 0, (H, ndir, B + 1)


def test_unsupported_launch_touches_nothing():
    '''first unsupported B at H = 300, both directions: DANET_ERR_UNSUPPORTED, nothing launched'''
    from danet_amd import _lib
    c = Case('unsupported', 193, 2, 16, 300, 2, FX1)
    assert ll.bwd_plan(c.B, c.H, c.ndir) is None and not ll.fx_plan(c.B, c.H, c.ndir, c.D, c.opts)['ok']
    z = lambda *s: np.zeros(s, np.float32)
    b = ll.Bwd(c, [z(c.T, c.B, 4 * c.H)] * 2, [z(c.T, c.B, c.H)] * 2)
    assert b.launch() == ll.ERR_UNSUPPORTED
    f = ll.Fwd(c, fused=True)
    assert f.launch() == ll.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(t.untouched() for t in b.da + b.db + f.gates + f.cell + [f.ypad])
    for ws in (b.ws, f.ws):
        assert bool((ws.buf.view(torch.int32) == ll.SENT).all()), 'an unsupported launch wrote its workspace'
    with ll.set_options(c.opts):
        fw, bw = [ll.Fwd(c)], [ll.Bwd(c, [z(c.T, c.B, 4 * c.H)] * 2, [z(c.T, c.B, c.H)] * 2)]
        rc = _lib.load().danet_lstm_train_prefill(
            _lib.stream(), c.T, c.B, c.H, c.ndir, c.ldy, 1, ll._ptrs([fw[0].ypad.t]), ll._ptrs([fw[0].ws.buf]),
            ll._ptrs([bw[0].ws.buf]))
    assert rc == ll.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert fw[0].ypad.untouched() and bool((bw[0].ws.buf.view(torch.int32) == ll.SENT).all())


def test_zz_family_report():
    '''prints the worst errors per kernel family of this run (the module docstring's table)'''
    for fam in sorted(_family):
        k, f, r = _family[fam]
        print('%-14s kernel %.2e  float32 %.2e  worst ratio %.1f' % (fam, k, f, r))
        assert k < TOL
