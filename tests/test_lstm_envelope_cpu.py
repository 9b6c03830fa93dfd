'''
CPU checks (no GPU) of the case tables of tests/test_gpu_lstm_envelope.py.  Which template
instantiation of csrc/lstm.hip a shape runs cannot be asked of the library, so tests/lstm_layer.py
restates the launch plans: make_plan, make_rs_plan and choose_rs_plan (the "host side" section of
csrc/lstm.hip, from `struct LstmPlan` to `dn_ws_lstm`), the fused forward's envelope (fwd_fused_ok)
and the placement choice at the end of danet_lstm_bwd.  Here that restatement is anchored to what
the library does answer without a device (dn_num_cus() assumes 256 compute units then):
danet_workspace_bytes(DANET_WS_LSTM, ...), danet_lstm_bwd_db_supported and
danet_lstm_fwd_fused_supported over a grid of shapes that includes every table shape.  Then the
tables are checked against it: all fifteen lstm_bwd_rs_kernel<U, NTW>, the five hoisted and four
fused forward kernels, every placement row, the ragged / NI / S conditions.  A later edit of the
tables cannot silently drop coverage.  Cases that pin both lstm_bwd_u and lstm_bwd_s need only
NTW = ceil(ceil(NT / S) / 8); the default-choice cases rest on the restated choose_rs_plan.
'''
import numpy as np

import lstm_layer as ll
import test_gpu_lstm_envelope as env

ALL_BPTT = {(U, n) for U in (8, 16, 32) for n in (1, 2, 3, 4, 5)}
ALL_FWD = {'fwd<1,4,8>', 'fwd<2,4,8>', 'fwd<1,4,12>', 'small<1>', 'small<4>'}
ALL_FX = {'fx<2,1>', 'fx<4,2>', 'fx<8,3>', 'fx<8,4>'}
NI_REACHABLE = 5          # largest owner-iteration count inside H <= 608 (RS_NI_MAX = 6 is headroom)


def _all_cases():
    cases = [c[0] for c in env.BPTT] + [c[0] for c in env.PLACEMENT] + env.TIMES + [env.LONG, env.LONG_B1]
    cases += [c[0] for c in env.FORWARD] + [c[0] for c in env.FUSED] + env.SATURATED + [env.FLAGS, env.FLAGS_RAGGED]
    return cases


def _with_options(opts, fn):
    from danet_amd import _lib
    _lib.load()
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        return fn(_lib.load())
    finally:
        _lib.apply_env_options()


def test_restated_plans_agree_with_the_library():
    from danet_amd import _lib
    L = _lib.load()
    shapes = {(B, H, nd) for nd in (1, 2) for B in list(range(1, 36)) + [48, 49, 64, 81, 96, 97, 128, 129, 192, 193,
                                                                         200, 208, 209, 400, 401]
              for H in range(4, 613, 8)}
    shapes |= {(c.B, c.H, c.ndir) for c in _all_cases()}
    shapes |= {(B + e, H, nd) for H, nd, B in env.BWD_EDGES + env.FX_EDGES for e in (0, 1)}
    for B, H, nd in sorted(shapes):
        assert L.danet_lstm_bwd_db_supported(4, B, H, nd) == int(ll.choose_rs_plan(B, H, nd) is not None), (B, H, nd)
        assert _lib.ws_bytes(_lib.WS_LSTM, 4, B, H, nd) == ll.ws_lstm(4, B, H, nd), (B, H, nd)
        for D in (8, 640, 644):
            assert L.danet_lstm_fwd_fused_supported(4, B, H, nd, D) == int(ll.fx_plan(B, H, nd, D)['ok']), (B, H, nd, D)
    # under the pins the tables use
    for c in _all_cases():
        want = ll.bwd_plan(c.B, c.H, c.ndir, c.opts) is not None
        got = _with_options(c.opts, lambda L: L.danet_lstm_bwd_db_supported(c.T, c.B, c.H, c.ndir))
        assert got == int(want), c.describe()
        want = ll.fx_plan(c.B, c.H, c.ndir, c.D, c.opts)['ok']
        got = _with_options(c.opts, lambda L: L.danet_lstm_fwd_fused_supported(c.T, c.B, c.H, c.ndir, c.D))
        assert got == int(want), c.describe()
        assert _lib.ws_bytes(_lib.WS_LSTM, c.T, c.B, c.H, c.ndir) == ll.ws_lstm(c.T, c.B, c.H, c.ndir)


def test_bptt_matrix_runs_every_instantiation():
    seen, by_u = set(), {}
    for case, U, NTW, twins, NI in env.BPTT:
        p = ll.bwd_plan(case.B, case.H, case.ndir, case.opts)
        assert p is not None, case.describe()
        assert (p['U'], p['NTW'], p['S'] > 1, p['NI']) == (U, NTW, twins, NI), case.describe()
        if 'lstm_bwd_u' in case.opts and 'lstm_bwd_s' in case.opts:      # nothing rests on the chooser
            assert p['S'] == case.opts['lstm_bwd_s']
            assert NTW == ll.cdiv(ll.cdiv(p['NT'], p['S']), 8)
        seen.add((U, NTW))
        by_u.setdefault(U, []).append((case, p))
        fwd = ll.fwd_plan(case.B, case.H, case.ndir, case.opts)['kernel']
        assert (fwd is None) == (case.name in env.BPTT_ONLY), case.describe()
    assert seen == ALL_BPTT, ALL_BPTT - seen
    # thirteen are reached by the default plan, <8,4> and <8,5> only with lstm_bwd_u = 8
    default = {(U, n) for case, U, n, _, _ in env.BPTT if not case.opts}
    assert default == ALL_BPTT - {(8, 4), (8, 5)}, ALL_BPTT - default
    for U, rows in by_u.items():
        assert {p['S'] > 1 for _, p in rows} == {False, True}, U
        assert {1, NI_REACHABLE} <= {p['NI'] for _, p in rows}, U
        # ragged batch and a ragged last unit group whose last 16-tile is part padding, in one case
        assert any(c.B % 16 in (1, 15) and c.H % U and c.H % 16 for c, _ in rows), U
        assert {c.ndir for c, _ in rows} == {1, 2} or U == 32, U
        assert any(c.pad != (0, 0, 0, 0) for c, _ in rows) and any(c.status == 'null' for c, _ in rows), U
    assert {c.ndir for c, *_ in env.BPTT} == {1, 2}
    # NI never exceeds NI_REACHABLE inside the header's H <= 608
    assert max(ll.rs_plan(1, H, 1, U)['NI'] for U in (8, 16, 32) for H in range(4, 609, 4)) == NI_REACHABLE
    # the wide-layer default (H > 384 takes U = 16 first) and its U = 32 partner at the same shape
    wide = {c.name: c for c, *_ in env.BPTT}
    a, b = wide['u16-ntw2-wide-default'], wide['u32-ntw1-wide-partner']
    assert (a.B, a.H, a.ndir) == (b.B, b.H, b.ndir) and a.H > 384 and not a.opts and b.opts == {'lstm_bwd_u': 32}
    assert ll.rs_plan(a.B, a.H, a.ndir, 32)['ok']
    assert set(env.REF_FED) <= set(wide) and {ll.bwd_plan(wide[n].B, wide[n].H, wide[n].ndir)['U']
                                              for n in env.REF_FED} == {8, 16, 32}


def test_placement_rows():
    ncls, padded_seen, fallback_seen = set(), False, False
    for case, ncl, padded, fallback in env.PLACEMENT:
        p = ll.bwd_plan(case.B, case.H, case.ndir)
        assert p['ncl'] == ncl and p['S'] > 1, case.describe()
        assert p['twin_fallback'] == fallback and p['xmap'] == (1 if fallback else 2)
        assert (p.get('idle', 0) > 0) == padded
        if padded:
            assert p['P'] % (8 // ncl) != 0
        if fallback:
            assert 8 * ll.cdiv(p['P'], 8 // ncl) * p['S'] > ll.CUS >= ncl * p['P'] * p['S']
        for o in env.PLACEMENT_OPTS[1:]:
            q = ll.bwd_plan(case.B, case.H, case.ndir, o)
            assert q['xmap'] == o.get('lstm_xmap', 1) and (q['U'], q['S'], q['NTW']) == (p['U'], p['S'], p['NTW'])
        ncls.add(ncl)
        padded_seen |= padded
        fallback_seen |= fallback
    assert ncls == {1, 2, 4, 8} and padded_seen and fallback_seen
    assert [o.get('lstm_xmap', 1) for o in env.PLACEMENT_OPTS] == [1, 1, 0]
    assert env.PLACEMENT_OPTS[1] == {'lstm_bwd_twin_xcd': 0}


def test_forward_tables_run_every_instantiation():
    seen = set()
    for case, kernel in env.FORWARD:
        assert ll.fwd_plan(case.B, case.H, case.ndir, case.opts)['kernel'] == kernel, case.describe()
        seen.add(kernel)
    assert seen == ALL_FWD, ALL_FWD - seen
    F = {c.name: (c, k) for c, k in env.FORWARD}
    # <1,4,12> and <2,4,8> both chosen and forced by lstm_fwd_un
    for k, un in (('fwd<1,4,12>', 12), ('fwd<2,4,8>', 8)):
        rows = [c for c, kk in env.FORWARD if kk == k]
        assert any(not c.opts for c in rows) and any(c.opts.get('lstm_fwd_un') == un for c in rows), k
    small = [c for c, k in env.FORWARD if k.startswith('small')]
    assert {c.B for c in small} == {1, 2, 3, 4} and {4, 320} <= {c.H for c in small}
    mfma = [c for c, k in env.FORWARD if c.opts.get('lstm_fwd_small') == 0]
    assert {c.B for c in mfma} >= {1, 3, 4} and all(c.B <= 4 and c.H <= 320 for c in mfma)
    assert F['fwd-b5-outside-small'][0].B == 5 and F['small-h324-outside'][0].H == 324
    # H = 608 (the header's maximum) and the widths whose weight pieces spill to LDS (nbw > 3)
    every = [c for c in _all_cases() if ll.fwd_plan(c.B, c.H, c.ndir, c.opts)['kernel'] in ('fwd<1,4,8>', 'fwd<1,4,12>')]
    assert any(c.H == 608 for c in every)
    assert {ll.fwd_plan(c.B, c.H, c.ndir, c.opts)['nbw'] for c in every} >= {1, 2, 3, 4, 5}
    assert ll.fwd_plan(17, 384, 1)['nbw'] == 3 and ll.fwd_plan(17, 388, 1)['nbw'] == 4
    assert ll.fwd_plan(env.LONG_B1.B, env.LONG_B1.H, env.LONG_B1.ndir)['kernel'] == 'small<1>'
    # ragged unit groups and row clusters of the forward kernels' own geometry
    for k in ('fwd<1,4,8>', 'fwd<2,4,8>', 'fwd<1,4,12>'):
        plans = [(c, ll.fwd_plan(c.B, c.H, c.ndir, c.opts)) for c in _all_cases()]
        plans = [(c, p) for c, p in plans if p['kernel'] == k]
        assert any(c.H % p['UN'] for c, p in plans) and any(c.B % p['rows'] for c, p in plans), k


def test_fused_table_runs_every_instantiation():
    seen = {}
    for case, kernel in env.FUSED:
        assert ll.fx_plan(case.B, case.H, case.ndir, case.D, case.opts)['kernel'] == kernel, case.describe()
        assert ll.fwd_plan(case.B, case.H, case.ndir, case.opts)['kernel'], case.describe()
        seen.setdefault(kernel, []).append(case)
    assert set(seen) == ALL_FX, ALL_FX - set(seen)
    Ds = {c.D for c, _ in env.FUSED}
    assert {160, 161, 320, 324, 608, 612, 640} <= Ds                 # both sides of every switch, and the maximum
    assert any(D % 4 for D in Ds) and all(any(c.D % 16 for c in cs) for cs in seen.values())
    assert any(c.H == 320 for c, _ in env.FUSED)
    assert any(c.B < 24 and c.opts.get('lstm_fwd_fused') == 1 for c, _ in env.FUSED)
    assert any(c.B >= 24 and not c.opts for c, _ in env.FUSED)
    assert any(c.pad[3] for c, _ in env.FUSED if c.D % 4)            # ldx beyond the zero-filled last group


def test_time_table_and_saturated_inputs():
    assert [c.T for c in env.TIMES] == [1, 2, 3, 4, 5, 7] and all(c.ndir == 2 for c in env.TIMES)
    assert (env.LONG.T, env.LONG.H, env.LONG.ndir) == (512, 300, 2)
    assert (env.LONG_B1.T, env.LONG_B1.B) == (1251, 1)
    assert {ll.bwd_plan(c.B, c.H, c.ndir, c.opts)['U'] for c in env.SATURATED if c.B > 4} == {8, 16, 32}
    for c in env.SATURATED:
        inp = ll.inputs(c)
        for d in range(c.ndir):
            gx = inp['gx'][d].numpy().reshape(-1, 4, c.H)
            assert np.isfinite(gx).all()
            for gate in range(4):
                col = gx[:, gate, :]
                for level in (20, 90, 200):
                    assert ((col > level - 8) & (col < level + 8)).any(), (c.name, gate, level)
                    assert ((col < -level + 8) & (col > -level - 8)).any(), (c.name, gate, -level)
            assert (np.abs(gx).max(axis=0) < 8).sum() >= c.H           # ordinary units next to them


def test_envelope_edges_are_the_library_answers():
    '''the sentence in include/danet_hip.h: on 256 CUs the largest B is 192 / 400 at H = 300 and 96 / 208
    at H = 600 for ndir = 2 / 1'''
    from danet_amd import _lib
    L = _lib.load()
    assert env.BWD_EDGES == [(300, 2, 192), (300, 1, 400), (600, 2, 96), (600, 1, 208)]
    for H, ndir, B in env.BWD_EDGES:
        assert L.danet_lstm_bwd_db_supported(8, B, H, ndir) == 1 and L.danet_lstm_bwd_db_supported(8, B + 1, H, ndir) == 0
        assert max(b for b in range(1, 512) if ll.choose_rs_plan(b, H, ndir)) == B
    assert _with_options({'lstm_fwd_fused': 1}, lambda L: [
        (L.danet_lstm_fwd_fused_supported(8, B, H, nd, 64), L.danet_lstm_fwd_fused_supported(8, B + 1, H, nd, 64))
        for H, nd, B in env.FX_EDGES]) == [(1, 0)] * len(env.FX_EDGES)
    for H, nd, B in env.FX_EDGES:
        o = {'lstm_fwd_fused': 1}
        assert ll.fx_plan(B, H, nd, 64, o)['ok'] and not ll.fx_plan(B + 1, H, nd, 64, o)['ok']


def test_sentinel_is_nan_poison_and_not_the_kernels_flag():
    assert np.isnan(np.array(ll.SENT, np.int32).view(np.float32))
    assert ll.SENT != 0xFFFFFFFF and ll.GUARD % 4 == 0
