'''
Layer harness of the GPU tests of the recurrent kernels (csrc/lstm.hip), shared by
tests/test_gpu_lstm_envelope.py and tests/test_lstm_envelope_cpu.py.  Test infrastructure only.

Three parts:

* the launch plans of csrc/lstm.hip restated in Python (make_plan, make_rs_plan, choose_rs_plan,
  dn_ws_lstm, the fused forward's envelope and the BPTT's placement choice), so that a case can say
  which template instantiation it runs and which rows / units are the ragged ones.  Nothing of this
  is observable through the ABI except the workspace size and the two envelope queries;
  tests/test_lstm_envelope_cpu.py anchors the restatement to those.
* the float64 reference: oracle/torch_ref.lstm_scan restated with the hoisted pre-activation
  gx = x Wx + b as a leaf, so that it yields y, the saved post-activation gates (g | i | f | o column
  blocks), the cells and, by autograd, da = dL/dgx and db = sum_{t,b} da for a random dy.  The same
  function on float32 tensors is the "float32 restatement" whose own error against float64 must stay
  below F32_BAR: the bar TOL then never sits within a factor of ten of what plain float32 rounding
  does to that input.  All inputs are float32-representable, so kernel, restatement and reference
  start from the same numbers.
* guarded launches of the C entry points through _lib (danet_lstm_fwd, danet_lstm_fwd_fused,
  danet_lstm_bwd, danet_lstm_bwd_db_reduce and the two prefill calls): every output and the
  exact-size workspace sit between sentinel guards that must survive bit for bit, padded leading
  dimensions hold a NaN in the gaps of the inputs, every launch's status word is read back.
'''
import ctypes
import functools

import numpy as np
import torch

from gpu_helpers import relerr

TOL = 1e-5             # every output of every case, relative to the tensor's (or the slice's) maximum
F32_BAR = 1e-6         # the float32 CPU restatement of the same case against float64
SENT = 0x7FC5A5A5      # a quiet NaN with a payload (never the kernels' own 0xFFFFFFFF "not yet published")
GUARD = 64             # guard floats before and after every buffer (keeps the 16-byte alignment)
WS_TAIL = 64           # guard floats behind the exact-size workspace
UNPUBLISHED = -1       # 0xFFFFFFFF as int32
CUS = 256              # gfx950; dn_num_cus() answers the same without a device
PREFILLED, DB_DEFERRED = 1, 2
ERR_UNSUPPORTED = -3


def cdiv(a, b):
    return -(-a // b)


def align_up(a, b):
    return cdiv(a, b) * b


# ------------------------------------------------------------------ the launch plans, restated
def rs_plan(B, H, ndir, U, es=0, cus=CUS):
    '''make_rs_plan (csrc/lstm.hip): reduce-scatter BPTT geometry for U units per producer group;
    es = option lstm_bwd_s'''
    G, P = cdiv(B, 16), cdiv(H, U)
    NT = cdiv(P * U, 16)
    NI = cdiv(P, 512 // (4 * U))
    ncl = ndir * G
    smax = min(cus // (ncl * P), NT)
    S = smax
    for sv in range(1, smax + 1):
        if cdiv(NT, sv) <= 8:
            S = sv
            break
    if 1 <= es <= smax:
        S = es
    NTW = cdiv(cdiv(NT, S), 8) if S > 0 else 99
    ring = 3 * ncl * P * NT * 1024
    ok = H % 4 == 0 and smax >= 1 and NTW <= 5 and NI <= 6 and ring < 0xFFFFFFF0
    return dict(ok=ok, U=U, G=G, P=P, S=S, NT=NT, NTW=NTW, NI=NI, ncl=ncl, smax=smax, ring=ring)


def choose_rs_plan(B, H, ndir, pin=0, es=0, cus=CUS):
    '''choose_rs_plan (csrc/lstm.hip): pin = option lstm_bwd_u.  None outside the envelope.'''
    if not pin and H > 384:
        r = rs_plan(B, H, ndir, 16, es, cus)
        if r['ok']:
            return r
    best, best_cost = None, 1 << 30
    for U in (8, 16, 32):
        if pin and pin != U:
            continue
        r = rs_plan(B, H, ndir, U, es, cus)
        if not r['ok']:
            continue
        cost = cdiv(cdiv(r['NT'], r['S']), 4) * U
        if cost < best_cost:
            best, best_cost = r, cost
    return best


def bwd_plan(B, H, ndir, opts=None, cus=CUS):
    '''the plan danet_lstm_bwd launches under the option values `opts`: choose_rs_plan + the
    placement choice (xmap 0 / 1, or 2 = the twin-co-located order with its padded grid)'''
    o = opts or {}
    r = choose_rs_plan(B, H, ndir, o.get('lstm_bwd_u', 0), o.get('lstm_bwd_s', 0), cus)
    if r is None:
        return None
    r = dict(r)
    xm = o.get('lstm_xmap', -1)
    xm = xm if xm >= 0 else 1
    xm = 1 if xm == 2 else xm
    grid = r['ncl'] * r['P'] * r['S']
    r['twin_fallback'] = False
    if o.get('lstm_bwd_twin_xcd', 1) == 1 and xm == 1 and r['ncl'] <= 8 and 8 % r['ncl'] == 0 and r['S'] > 1:
        npar = 8 // r['ncl']
        g2 = 8 * cdiv(r['P'], npar) * r['S']
        if g2 <= cus:
            xm, grid = 2, g2
            r['idle'] = g2 - r['ncl'] * r['P'] * r['S']
            r['npar'] = npar
        else:
            r['twin_fallback'] = True
    r['xmap'], r['grid'] = xm, grid
    return r


def fwd_plan(B, H, ndir, opts=None, cus=CUS):
    '''which forward kernel danet_lstm_fwd launches (make_plan + the small-batch branch)'''
    o = opts or {}
    UN, P = 8, cdiv(H, 8)
    MT = 2 if ndir * cdiv(B, 16) * P > cus else 1
    if B > 4:
        want = o.get('lstm_fwd_un', 0)
        fits12 = ndir * cdiv(B, 16) * cdiv(H, 12) <= cus
        if (want == 12 or (want != 8 and MT == 2)) and fits12:
            UN, P, MT = 12, cdiv(H, 12), 1
    G = cdiv(B, 16 * MT)
    nbw = (cdiv(cdiv(H, 16), 4) + 1) // 2          # k-blocks per wave; those behind the third live in LDS
    r = dict(UN=UN, P=P, MT=MT, G=G, nbw=nbw, grid=ndir * G * P, rows=16 * MT)
    if H % 4 or H > 608:
        r['kernel'] = None
    elif B <= 4 and H <= 320 and o.get('lstm_fwd_small', 1) != 0:
        r['kernel'] = 'small<%d>' % (1 if B == 1 else 4)
        r.update(grid=ndir * P, rows=4, G=1)
    elif r['grid'] > cus:
        r['kernel'] = None
    else:
        r['kernel'] = 'fwd<%d,4,%d>' % (MT, UN)
    return r


def fx_plan(B, H, ndir, D, opts=None, cus=CUS):
    '''fwd_fused_ok + the <window, early> choice of danet_lstm_fwd_fused'''
    o = opts or {}
    P, G = cdiv(H, 8), cdiv(B, 16)
    e = o.get('lstm_fwd_fused', -1)
    inside = H % 4 == 0 and H <= 320 and 0 < D <= 640 and ndir * G * P <= cus
    ok = inside and e != 0 and (e == 1 or B >= 24)
    k = '2,1' if D <= 160 else ('4,2' if D <= 320 else ('8,3' if D <= 608 else '8,4'))
    return dict(ok=ok, UN=8, P=P, G=G, MT=1, rows=16, grid=ndir * G * P, kernel='fx<%s>' % k if ok else None)


def ws_lstm(T, B, H, ndir, cus=CUS):
    '''dn_ws_lstm: status block + the largest ring over U + the per-cluster bias-gradient slab'''
    ring = max([0] + [r['ring'] for r in (rs_plan(B, H, ndir, U, 0, cus) for U in (8, 16, 32)) if r['ok']])
    return align_up(256 + ring, 256) + align_up(ndir * cdiv(B, 16) * 4 * H * 4, 256)


def slab_offset(plan):
    '''byte offset of the bias-gradient slab behind the ring of the plan that runs'''
    return align_up(256 + plan['ring'], 256)


# ------------------------------------------------------------------ cases and their data
class Case(object):
    '''one (B, T, D, H, ndir) with its option values, leading-dimension paddings and input recipe.
    pad = (ldw, ldy, lddy, ldx) extra floats; sat: saturating bias offsets in chosen units;
    status: 'own' (caller-owned device word) or 'null' (workspace word 0).'''

    def __init__(self, name, B, T, D, H, ndir, opts=None, pad=(0, 0, 0, 0), sat=False, status='own',
                 seed=None, scale=1.0):
        self.name, self.B, self.T, self.D, self.H, self.ndir = name, B, T, D, H, ndir
        self.opts = dict(opts or {})
        self.pad, self.sat, self.status, self.scale = tuple(pad), sat, status, scale
        self.seed = seed if seed is not None else (B * 1009 + T * 101 + D * 13 + H * 7 + ndir) % (1 << 31)

    def __repr__(self):
        return self.name

    def key(self):
        return (self.B, self.T, self.D, self.H, self.ndir, self.sat, self.seed, self.scale)

    @property
    def ldw(self):
        return 4 * self.H + self.pad[0]

    @property
    def ldy(self):
        return self.ndir * self.H + self.pad[1]

    @property
    def lddy(self):
        return self.ndir * self.H + self.pad[2]

    @property
    def ldx(self):
        return align_up(self.D, 4) + self.pad[3]

    def describe(self):
        return ('%s: B=%d T=%d D=%d H=%d ndir=%d opts=%s pad=%s\n  forward %s\n  fused   %s\n  BPTT    %s' % (
            self.name, self.B, self.T, self.D, self.H, self.ndir, self.opts, self.pad,
            fwd_plan(self.B, self.H, self.ndir, self.opts), fx_plan(self.B, self.H, self.ndir, self.D, self.opts),
            bwd_plan(self.B, self.H, self.ndir, self.opts)))


SAT_LEVELS = (20.0, -20.0, 90.0, -90.0, 200.0, -200.0)


def _sat_bias(H, rng):
    '''bias offsets that put the pre-activations of chosen units at about +-20, +-90 and +-200, each
    level in each of the four gates, next to ordinary units (at most half of the units are touched)'''
    off = np.zeros(4 * H)
    units = rng.permutation(H)[:max(1, H // 2)]
    for j, u in enumerate(units):
        gate, level = j % 4, SAT_LEVELS[(j // 4) % len(SAT_LEVELS)]
        off[gate * H + u] = level
    return off


@functools.lru_cache(maxsize=None)
def _inputs(key):
    B, T, D, H, ndir, sat, seed, scale = key
    from oracle import danet_oracle as O
    rng = np.random.RandomState(seed)
    r = 1.5 / np.sqrt(H)
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32))
    d = dict(x=f32(rng.randn(T, B, D) * 0.7 * scale), dy=f32(rng.randn(T, B, ndir * H)), W=[], b=[], gx=[])
    for _ in range(ndir):
        d['W'].append(f32(rng.uniform(-r, r, size=(D + H, 4 * H))))
        b = O.lstm_bias_init(H) + rng.randn(4 * H) * 0.1
        if sat:
            b = b + _sat_bias(H, rng)
        d['b'].append(f32(b))
    for k in range(ndir):    # the hoisted gx the kernel gets: float64 x Wx + b rounded to float32
        gx = d['x'].double().reshape(T * B, D) @ d['W'][k][:D].double() + d['b'][k].double()
        d['gx'].append(gx.float().reshape(T, B, 4 * H))
    return d


def inputs(case):
    '''float32 CPU tensors of a case: x [T][B][D], dy [T][B][ndir*H], per direction W [D+H][4H],
    b [4H] and the hoisted gx [T][B][4H]'''
    return _inputs(case.key())


def _scan(gx, Wh, H, reverse):
    '''oracle/torch_ref.lstm_scan from the hoisted pre-activation on, time-major, returning what the
    kernels save as well: y [T][B][H], gates [T][B][4H] (g | i | f | o, g linear), cells [T][B][H]'''
    T, B = gx.shape[:2]
    c = gx.new_zeros(B, H)
    h = gx.new_zeros(B, H)
    ys, gs, cs = [None] * T, [None] * T, [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        a = gx[t] + h @ Wh
        g = a[:, :H]
        i = torch.sigmoid(a[:, H:2 * H])
        f = torch.sigmoid(a[:, 2 * H:3 * H])
        o = torch.sigmoid(a[:, 3 * H:])
        c = i * g + f * c
        h = o * torch.tanh(c)
        ys[t], gs[t], cs[t] = h, torch.cat([g, i, f, o], -1), c
    return torch.stack(ys), torch.stack(gs), torch.stack(cs)


def _reference(key, fused, dtype, backward):
    B, T, D, H, ndir, sat, seed, scale = key
    inp = _inputs(key)
    n0 = torch.get_num_threads()
    torch.set_num_threads(min(16, n0))
    try:
        out = dict(y=[], gates=[], cell=[], da=[], db=[])
        leaves = []
        for d in range(ndir):
            W = inp['W'][d].to(dtype)
            if fused:
                gx = inp['x'].to(dtype).reshape(T * B, D) @ W[:D] + inp['b'][d].to(dtype)
                gx = gx.reshape(T, B, 4 * H).detach()
            else:
                gx = inp['gx'][d].to(dtype).clone()
            gx.requires_grad_(backward)
            y, g, c = _scan(gx, W[D:], H, reverse=(d == 1))
            leaves.append(gx)
            out['y'].append(y)
            out['gates'].append(g.detach())
            out['cell'].append(c.detach())
        if backward:
            y = torch.cat(out['y'], -1)
            (y * inp['dy'].to(dtype)).sum().backward()
            for gx in leaves:
                out['da'].append(gx.grad)
                out['db'].append(gx.grad.sum(dim=(0, 1)))
        out['y'] = [y.detach() for y in out['y']]
        return out
    finally:
        torch.set_num_threads(n0)


@functools.lru_cache(maxsize=None)
def _reference_cached(key, fused, f32, backward):
    return _reference(key, fused, torch.float32 if f32 else torch.float64, backward)


def reference(case, fused=False, f32=False, backward=True):
    '''dict of per-direction lists y [T][B][H], gates [T][B][4H], cell [T][B][H], da [T][B][4H],
    db [4H]; float64, or the float32 restatement'''
    return _reference_cached(case.key(), bool(fused), bool(f32), bool(backward))


# ------------------------------------------------------------------ the error measure
def _slices(case, plan, K):
    '''index sets of a [T][B][K][H] output: all of it, and the last unit group / last row cluster
    alone where the plan leaves them ragged'''
    s = [('all', (slice(None),) * 4)]
    if plan is None:
        return s
    UN, rows = plan.get('UN', plan.get('U')), plan.get('rows', 16)
    if case.H % UN:
        s.append(('last-units', (slice(None), slice(None), slice(None), slice((cdiv(case.H, UN) - 1) * UN, None))))
    if case.B % rows:
        s.append(('last-rows', (slice(None), slice((cdiv(case.B, rows) - 1) * rows, None))))
    return s


def errors(case, plan, name, got, ref64, ref32):
    '''[(label, kernel error, float32 restatement's error)] of one output of one direction, per slice.
    The arrays are [T][B][K*H] (db: [K*H]); a slice whose float64 reference is all zero is skipped.'''
    H = case.H
    shape = (-1, case.B, got.shape[-1] // H, H) if got.ndim == 3 else (1, 1, got.shape[-1] // H, H)
    g, r64, r32 = (np.asarray(a, np.float64).reshape(shape) for a in (got, ref64, ref32))
    out = []
    for label, idx in _slices(case, plan, shape[2]):
        if label == 'last-rows' and shape[1] == 1:
            continue
        if not np.abs(r64[idx]).max() > 0:
            continue
        out.append(('%s %s' % (name, label), relerr(g[idx], r64[idx]), relerr(r32[idx], r64[idx])))
    return out


class Report(object):
    '''collects (label, kernel error, float32 error) rows, prints them and asserts the two bars'''

    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, plan, name, got, ref64, ref32):
        assert np.isfinite(np.asarray(got)).all(), '%s: non-finite %s\n%s' % (self.case, name, self.case.describe())
        self.rows += errors(self.case, plan, name, got, ref64, ref32)

    def worst(self):
        return max(r[1] for r in self.rows), max(r[2] for r in self.rows)

    def check(self, family):
        k, f = self.worst()
        print('%-28s %-10s kernel %.2e  float32 %.2e  ratio %.1f' % (self.case.name, family, k, f, k / max(f, 1e-30)))
        bad32 = [r for r in self.rows if not r[2] < F32_BAR]
        assert not bad32, 'badly chosen input, float32 alone misses %g: %s\n%s' % (F32_BAR, bad32, self.case.describe())
        bad = [r for r in self.rows if not r[1] < TOL]
        assert not bad, '%s\n%s' % (bad, self.case.describe())
        return k, f


# ------------------------------------------------------------------ guarded buffers
def _sent(n):
    return torch.full((n,), SENT, dtype=torch.int32, device='cuda').view(torch.float32)


class Guarded(object):
    '''n floats between GUARD sentinel floats on either side, all pre-filled with the sentinel'''

    def __init__(self, n):
        self.n = n
        self.buf = _sent(n + 2 * GUARD)
        self.t = self.buf[GUARD:GUARD + n]

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENT).all())


def padded(t2d, ld, finite_to=None):
    '''a [rows][ld] device buffer holding t2d in its first columns and a NaN in the gap; columns up
    to finite_to (the header's rule for x: the last 4-float group of a row) hold zero instead'''
    rows, cols = t2d.shape
    buf = _sent(rows * ld).view(rows, ld)
    buf[:, :cols] = t2d.cuda()
    if finite_to is not None and finite_to > cols:
        buf[:, cols:finite_to] = 0
    return buf


class Workspace(object):
    '''exactly danet_workspace_bytes(DANET_WS_LSTM, ...) bytes followed by a sentinel tail'''

    def __init__(self, case):
        from danet_amd import _lib
        self.nbytes = _lib.ws_bytes(_lib.WS_LSTM, case.T, case.B, case.H, case.ndir)
        assert self.nbytes % 4 == 0
        self.buf = _sent(self.nbytes // 4 + WS_TAIL)

    def tail_intact(self):
        return bool((self.buf.view(torch.int32)[self.nbytes // 4:] == SENT).all())

    def word0(self):
        return int(self.buf.view(torch.int32)[0])

    def words_from(self, byte_off):
        return self.buf.view(torch.int32)[byte_off // 4:self.nbytes // 4]


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class set_options(object):
    '''the case's option values for the duration of a launch (the suite's autouse fixture restores
    the defaults after every test as well)'''

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        from danet_amd import _lib
        for k, v in self.opts.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        from danet_amd import _lib
        _lib.apply_env_options()
        return False


# ------------------------------------------------------------------ the launches
class Fwd(object):
    '''buffers of one forward launch of a case (hoisted: danet_lstm_fwd on gx; fused:
    danet_lstm_fwd_fused on x, W, b); run() launches, checks status, guards and the ypad rules and
    returns CPU arrays y, gates, cell per direction'''

    def __init__(self, case, fused=False):
        c = self.case = case
        self.fused = fused
        inp = inputs(case)
        T, B, H, D, nd = c.T, c.B, c.H, c.D, c.ndir
        self.W = [padded(inp['W'][d], c.ldw) for d in range(nd)]
        self.bias = [inp['b'][d].cuda() for d in range(nd)]
        if fused:
            self.x = padded(inp['x'].reshape(T * B, D), c.ldx, finite_to=align_up(D, 4))
        else:
            self.gx = [inp['gx'][d].reshape(T * B, 4 * H).cuda() for d in range(nd)]
        self.ypad = Guarded((T + 2) * B * c.ldy)
        self.gates = [Guarded(T * B * 4 * H) for _ in range(nd)]
        self.cell = [Guarded(T * B * H) for _ in range(nd)]
        self.ws = Workspace(case)
        self.status = torch.zeros(1, dtype=torch.int32, device='cuda')
        self._in = [t.view(torch.int32).clone() for t in self._input_tensors()]

    def _input_tensors(self):
        return self.W + self.bias + ([self.x] if self.fused else self.gx)

    def launch(self, flags=0):
        from danet_amd import _lib
        c, p, L = self.case, _lib.ptr, _lib.load()
        st = p(self.status) if c.status == 'own' else None
        g, ce = [t.t for t in self.gates], [t.t for t in self.cell]
        with set_options(c.opts):
            if self.fused:
                rc = L.danet_lstm_fwd_fused(
                    _lib.stream(), c.T, c.B, c.H, c.ndir, p(self.x), c.ldx, c.D, p(self.W[0]), p(self.W[-1]),
                    c.ldw, p(self.bias[0]), p(self.bias[-1]), p(self.ypad.t), c.ldy, p(g[0]), p(g[-1]),
                    p(ce[0]), p(ce[-1]), p(self.ws.buf), self.ws.nbytes, st, flags)
            else:
                Wh = [W[c.D:] for W in self.W]
                rc = L.danet_lstm_fwd(
                    _lib.stream(), c.T, c.B, c.H, c.ndir, p(self.gx[0]), p(self.gx[-1]), p(Wh[0]), p(Wh[-1]),
                    c.ldw, p(self.ypad.t), c.ldy, p(g[0]), p(g[-1]), p(ce[0]), p(ce[-1]),
                    p(self.ws.buf), self.ws.nbytes, st, flags)
        return rc

    def prefill(self, n_extra=0):
        '''danet_lstm_fwd_prefill for this launch (and n_extra more of the same shape, returned)'''
        from danet_amd import _lib
        c = self.case
        others = [Fwd(c, self.fused) for _ in range(n_extra)]
        every = [self] + others
        _lib.check(_lib.load().danet_lstm_fwd_prefill(
            _lib.stream(), c.T, c.B, c.ldy, len(every), _ptrs([f.ypad.t for f in every]),
            _ptrs([f.ws.buf for f in every])))
        return others

    def collect(self):
        '''synchronise, check everything a forward launch promises, return its outputs'''
        c = self.case
        T, B, H, nd = c.T, c.B, c.H, c.ndir
        torch.cuda.synchronize()
        where = '\n' + c.describe()
        assert int(self.status) == 0, 'status word %#x%s' % (int(self.status), where)
        if c.status == 'null':
            assert self.ws.word0() == 0, 'workspace word 0 = %#x%s' % (self.ws.word0(), where)
        assert self.ws.tail_intact(), 'wrote behind the workspace' + where
        assert self.ypad.intact(), 'wrote outside ypad' + where
        for d in range(nd):
            assert self.gates[d].intact(), 'wrote outside gates[%d]%s' % (d, where)
            assert self.cell[d].intact(), 'wrote outside cell[%d]%s' % (d, where)
        for t, t0 in zip(self._input_tensors(), self._in):
            assert torch.equal(t.view(torch.int32), t0), 'an input changed' + where
        yp = self.ypad.t.view(T + 2, B, c.ldy)
        assert not bool(yp[0, :, :nd * H].any()) and not bool(yp[T + 1, :, :nd * H].any()), 'pad blocks not zero' + where
        assert not bool((yp[1:T + 1, :, :nd * H].view(torch.int32) == UNPUBLISHED).any()), 'unpublished state left' + where
        y = yp[1:T + 1].cpu().numpy()
        return dict(y=[y[:, :, d * H:(d + 1) * H] for d in range(nd)],
                    gates=[g.t.view(T, B, 4 * H).cpu().numpy() for g in self.gates],
                    cell=[g.t.view(T, B, H).cpu().numpy() for g in self.cell])

    def run(self, flags=0):
        rc = self.launch(flags)
        from danet_amd import _lib
        assert rc == 0, '%s%s' % (_lib.load().danet_last_error(), '\n' + self.case.describe())
        return self.collect()


class Bwd(object):
    '''buffers of one danet_lstm_bwd launch of a case on the given saved gates and cells (CPU arrays
    [T][B][4H] / [T][B][H] per direction)'''

    def __init__(self, case, gates, cells, db0=None, want_db=True):
        c = self.case = case
        inp = inputs(case)
        T, B, H, nd = c.T, c.B, c.H, c.ndir
        self.Wh = [padded(inp['W'][d][c.D:], c.ldw) for d in range(nd)]
        self.dy = padded(inp['dy'].reshape(T * B, nd * H), c.lddy)
        self.gates_in = [torch.as_tensor(np.ascontiguousarray(g)).cuda() for g in gates]
        self.cell_in = [torch.as_tensor(np.ascontiguousarray(g)).cuda() for g in cells]
        self.da = [Guarded(T * B * 4 * H) for _ in range(nd)]
        self.db = [Guarded(4 * H) for _ in range(nd)]
        self.want_db = want_db
        if db0 is not None:
            for d in range(nd):
                self.db[d].t.copy_(db0[d].cuda())
        self.ws = Workspace(case)
        self.status = torch.zeros(1, dtype=torch.int32, device='cuda')
        self._in = [t.view(torch.int32).clone() for t in self._input_tensors()]

    def _input_tensors(self):
        return self.Wh + [self.dy] + self.gates_in + self.cell_in

    def launch(self, beta=0.0, flags=0):
        from danet_amd import _lib
        c, p, L = self.case, _lib.ptr, _lib.load()
        st = p(self.status) if c.status == 'own' else None
        da = [t.t for t in self.da]
        db = [t.t for t in self.db] if self.want_db else [None, None]
        with set_options(c.opts):
            return L.danet_lstm_bwd(
                _lib.stream(), c.T, c.B, c.H, c.ndir, p(self.dy), c.lddy, p(self.Wh[0]), p(self.Wh[-1]), c.ldw,
                p(self.gates_in[0]), p(self.gates_in[-1]), p(self.cell_in[0]), p(self.cell_in[-1]),
                p(da[0]), p(da[-1]), p(db[0]), p(db[-1]), beta, p(self.ws.buf), self.ws.nbytes, st, flags)

    def reduce(self, beta=0.0):
        from danet_amd import _lib
        c, p = self.case, _lib.ptr
        with set_options(c.opts):
            _lib.check(_lib.load().danet_lstm_bwd_db_reduce(
                _lib.stream(), c.T, c.B, c.H, c.ndir, p(self.db[0].t), p(self.db[-1].t), beta,
                p(self.ws.buf), self.ws.nbytes))

    def collect(self):
        c = self.case
        T, B, H, nd = c.T, c.B, c.H, c.ndir
        torch.cuda.synchronize()
        where = '\n' + c.describe()
        assert int(self.status) == 0, 'status word %#x%s' % (int(self.status), where)
        if c.status == 'null':
            assert self.ws.word0() == 0, 'workspace word 0 = %#x%s' % (self.ws.word0(), where)
        assert self.ws.tail_intact(), 'wrote behind the workspace' + where
        for d in range(nd):
            assert self.da[d].intact(), 'wrote outside da[%d]%s' % (d, where)
            assert self.db[d].intact(), 'wrote outside db[%d]%s' % (d, where)
        for t, t0 in zip(self._input_tensors(), self._in):
            assert torch.equal(t.view(torch.int32), t0), 'an input changed' + where
        return dict(da=[g.t.view(T, B, 4 * H).cpu().numpy() for g in self.da],
                    db=[g.t.cpu().numpy() for g in self.db])

    def run(self, beta=0.0, flags=0):
        rc = self.launch(beta, flags)
        from danet_amd import _lib
        assert rc == 0, '%s%s' % (_lib.load().danet_last_error(), '\n' + self.case.describe())
        return self.collect()


def train_prefill(fwds, bwds):
    '''danet_lstm_train_prefill: the forward launches' buffers and the BPTT launches' rings in one call'''
    from danet_amd import _lib
    c = fwds[0].case
    with set_options(c.opts):
        _lib.check(_lib.load().danet_lstm_train_prefill(
            _lib.stream(), c.T, c.B, c.H, c.ndir, c.ldy, len(fwds), _ptrs([f.ypad.t for f in fwds]),
            _ptrs([f.ws.buf for f in fwds]), _ptrs([b.ws.buf for b in bwds])))


# ------------------------------------------------------------------ whole cases
def check_forward(case, fused=False, flags=0, fwd=None):
    '''one forward launch against float64: y, gates and cell of every direction, per slice.
    Returns (outputs, worst kernel error, worst float32 error).'''
    plan = (fx_plan if fused else fwd_plan)(case.B, case.H, case.ndir, *((case.D,) if fused else ()), case.opts)
    assert plan['kernel'], 'outside the forward envelope\n' + case.describe()
    out = (fwd or Fwd(case, fused)).run(flags)
    r64 = reference(case, fused, backward=False)
    r32 = reference(case, fused, f32=True, backward=False)
    rep = Report(case)
    for d in range(case.ndir):
        for name in ('y', 'gates', 'cell'):
            rep.add(plan, '%s[%d]' % (name, d), out[name][d], r64[name][d].numpy(), r32[name][d].numpy())
    k, f = rep.check(plan['kernel'])
    return out, k, f


def check_backward(case, gates, cells, beta=0.0, flags=0, db0=None, tag=''):
    '''one BPTT launch on the given saved gates and cells against the float64 da and db'''
    plan = bwd_plan(case.B, case.H, case.ndir, case.opts)
    assert plan, 'outside the BPTT envelope\n' + case.describe()
    out = Bwd(case, gates, cells, db0=db0).run(beta, flags)
    r64, r32 = reference(case), reference(case, f32=True)
    rep = Report(case)
    for d in range(case.ndir):
        rep.add(plan, 'da[%d]' % d, out['da'][d], r64['da'][d].numpy(), r32['da'][d].numpy())
        ref_db, ref_db32 = r64['db'][d].numpy(), r32['db'][d].numpy()
        if db0 is not None:
            ref_db, ref_db32 = ref_db + db0[d].double().numpy(), ref_db32 + db0[d].numpy()
        rep.add(plan, 'db[%d]' % d, out['db'][d], ref_db, ref_db32)
    k, f = rep.check('bptt<%d,%d>%s' % (plan['U'], plan['NTW'], tag))
    return out, k, f
