'''
Plain numpy references, case tables and guarded launches of the separator and PIT-loss heads
(csrc/attractor.hip: separate_fwd_kernel, separate_bwd_kernel, sep_pit_fwd_kernel, sep_pit_bwd_kernel,
sum_chunks_kernel; csrc/loss.hip: pit_cross_kernel, pit_bwd_kernel; csrc/pit_common.h: pit_final_kernel,
ordered_chunk_sum, nth_perm), shared by tests/test_sep_cpu.py (no GPU) and tests/test_gpu_sep_envelope.py.

References.  Every function takes a dtype: run in float64 it is the reference, run in float32 it is the
restatement that says how far plain float32 arithmetic lands from float64 on the same inputs (the
condition of the bar: a case whose restatement misses F32_BAR is a badly chosen input).  Sums over the
N time-frequency bins run along the contiguous axis (numpy's pairwise summation there), as the kernels'
thread -> wave -> workgroup -> chunk trees do.  The gradients are written out analytically;
tests/test_sep_cpu.py anchors them to float64 autograd through oracle/torch_ref.py.

Restated constants of the sources: pick_ep, CHUNK_N, LOSS_CHUNK, REC and the layout of `dattr_partials`
([B][nch][C!][C][EP]); tests/test_sep_cpu.py anchors them to danet_workspace_bytes.

Which template instantiation a shape runs is not observable through the ABI; every table row carries the
(EP, EF, CP) it is expected to reach (Case.inst) and tests/test_sep_cpu.py checks the tables' coverage.

Layouts (include/danet_hip.h): embed [B][N][E], attr [B][C][E], mix_pwr [B][N], src complex64 [B][C][N],
phasor [B][N][2], out / sep_pwr / dsep_pwr [B][C][N], masks [B][N][C].
'''
import functools
import itertools
import math
import zlib

import numpy as np

TOL = 1e-5             # the bar: error of an output relative to its maximum magnitude, against float64
F32_BAR = 1e-6         # the condition: the float32 restatement of the same case against float64
GAP = 1e-3             # the condition on perm_idx: runner-up loss / best loss - 1 in float64
EPS = 1e-7             # batch_snr's eps (app/ops.py:191-222)

CHUNK_N = 2048         # csrc/attractor.hip
LOSS_CHUNK = 4096      # csrc/loss.hip
REC = 33               # csrc/pit_common.h
MAXC = 4
EPS_LIST = (4, 8, 20, 40, 64)
GUARD = 64             # sentinel floats on either side of a guarded buffer (keeps 16-byte alignment)
SENT = 0x7FC5A5A5      # a quiet NaN with a payload: an unwritten slot that is read poisons the result

OK, ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3, -4


def pick_ep(E):
    for ep in EPS_LIST:
        if E <= ep:
            return ep
    return 0


def cdiv(a, b):
    return -(-a // b)


def n_chunks(N):
    return cdiv(N, CHUNK_N)


def loss_chunks(N):
    return cdiv(N, LOSS_CHUNK)


def ws_separate_bwd(B, C, N, E):
    return B * n_chunks(N) * C * pick_ep(E) * 4


def ws_separate_pit(B, C, N, E):
    return max(B * n_chunks(N) * REC * 4, ws_separate_bwd(B, C, N, E))


def ws_records(B, N):
    return B * n_chunks(N) * REC * 4


def ws_pit_mse(B, C, N):
    return B * loss_chunks(N) * REC * 4


def ws_partials(B, C, N, E):
    '''bytes of dattr_partials [B][nch][C!][C][EP]; offered for C == 2 only'''
    return B * n_chunks(N) * math.factorial(C) * C * pick_ep(E) * 4 if C == 2 else 0


def perms_of(C):
    return list(itertools.permutations(range(C)))


# ------------------------------------------------------------------ references
def _cdt(dt):
    return np.complex128 if dt == np.float64 else np.complex64


def sep_masks(act, attr, embed, dt):
    '''masks [B][N][C]: softmax over C (act 0, max-subtracted) or sigmoid (act 1) of embed . attr^T'''
    # (einsum's own loops: identical attractor rows give bit-identical logits, which the tie rows need)
    lg = np.einsum('bne,bce->bnc', embed.astype(dt), attr.astype(dt))
    if act == 0:
        e = np.exp(lg - lg.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)
    e = np.exp(-np.abs(lg))
    return np.where(lg >= 0, 1 / (1 + e), e / (1 + e)).astype(dt)


def sep_forward(act, mix_pwr, attr, embed, dt):
    '''(out [B][C][N] = mix_pwr * mask, masks [B][N][C])'''
    m = sep_masks(act, attr, embed, dt)
    return np.ascontiguousarray((mix_pwr.astype(dt)[..., None] * m).transpose(0, 2, 1)), m


def _sum_bins(dl, x):
    '''sum_n dl[b][n][c] * x[b][n][e] -> [B][C][E], N along the contiguous axis of the summed product'''
    B, N, C = dl.shape
    if N <= 64:
        return np.einsum('bnc,bne->bce', dl, x)
    out = np.empty((B, C, x.shape[-1]), dl.dtype)
    for b in range(B):
        dt_, xt = np.ascontiguousarray(dl[b].T), np.ascontiguousarray(x[b].T)     # [C][N], [E][N]
        out[b] = (dt_[:, None, :] * xt[None, :, :]).sum(axis=-1)
    return out


def sep_backward(act, mix_pwr, attr, embed, dout, dt, masks=None):
    '''(dembed [B][N][E], dattr [B][C][E]) of sep_forward for the upstream gradient dout [B][C][N]'''
    m = sep_masks(act, attr, embed, dt) if masks is None else masks
    dm = dout.astype(dt).transpose(0, 2, 1) * mix_pwr.astype(dt)[..., None]          # dL/dmask
    if act == 0:
        dl = m * (dm - (m * dm).sum(axis=-1, keepdims=True))
    else:
        dl = dm * m * (1 - m)
    dembed = np.einsum('bnc,bce->bne', dl, attr.astype(dt))
    return dembed, _sum_bins(dl, embed.astype(dt))


def pit_cross(mode, src, p, phasor, dt):
    '''(L [B][C][C], S [B][C][C], sig [B]): L[i][j] = sum_n of the loss's error between truth i and estimate j
    (mode 0: |s_i - phasor p_j|^2, mode 1: (|s_i| - p_j)^2), S the complex one (for the SNR), sig = sum |s|^2'''
    s = src.astype(_cdt(dt))
    sr, si = np.ascontiguousarray(s.real), np.ascontiguousarray(s.imag)
    p = p.astype(dt)
    ph = phasor.astype(dt)
    er, ei = ph[:, None, :, 0] * p, ph[:, None, :, 1] * p
    dr = sr[:, :, None, :] - er[:, None, :, :]
    di = si[:, :, None, :] - ei[:, None, :, :]
    S = (dr * dr + di * di).sum(axis=-1)
    if mode == 1:
        d = np.hypot(sr, si)[:, :, None, :] - p[:, None, :, :]
        L = (d * d).sum(axis=-1)
    else:
        L = S
    sig = (sr * sr + si * si).sum(axis=-1).sum(axis=-1)
    return L, S, sig


def perm_losses(L, N):
    '''v [B][C!]: sum_i L[i][perm[i]] / N in itertools.permutations order, added in the order of i'''
    B, C = L.shape[:2]
    inv_n = L.dtype.type(1) / L.dtype.type(N)
    cols = []
    for perm in perms_of(C):
        v = np.zeros(B, L.dtype)
        for i in range(C):
            v = v + L[:, i, perm[i]] * inv_n
        cols.append(v)
    return np.stack(cols, axis=1)


def perm_search(v):
    '''index of the smallest loss, the first one on ties'''
    return np.argmin(v, axis=1).astype(np.int32)


def pit_reduce(L, S, sig, N, eps, dt, perm_idx=None):
    '''(loss, snr, perm_idx, v): the batch means of pit_final_kernel'''
    B, C = L.shape[:2]
    v = perm_losses(L, N)
    idx = perm_search(v) if perm_idx is None else perm_idx
    best_s = perm_losses(S, N)[np.arange(B), idx]
    loss = v[np.arange(B), idx].mean(dtype=dt)
    k = dt(10 / math.log(10))
    snr_b = k * (np.log(sig / dt(N) / dt(C) + dt(eps)) - np.log(best_s / dt(C) + dt(eps)))
    return dt(loss), dt(snr_b.mean(dtype=dt)), idx, v


def pit_dsep(mode, src, p, phasor, perm_idx, scale, dt):
    '''dsep_pwr [B][C][N] = scale * g, scale = dloss * dloss_dev * 2 / (B N) and g_j = p_j |ph|^2 - Re(conj(ph) t_j)
    (mode 0) or p_j - |t_j| (mode 1), t_j the truth that perms[perm_idx[b]] pairs with estimate j'''
    B, C, N = p.shape
    s = src.astype(_cdt(dt))
    inv = np.empty((B, C), np.int64)
    pm = np.array(perms_of(C))[perm_idx]                 # [B][C]: truth i is paired with estimate pm[i]
    inv[np.arange(B)[:, None], pm] = np.arange(C)[None, :]
    t = np.take_along_axis(s, inv[:, :, None], axis=1)   # t[b][j] = s[b][inv[j]]
    p = p.astype(dt)
    ph = phasor.astype(dt)
    if mode == 1:
        g = p - np.hypot(t.real, t.imag)
    else:
        px, py = ph[:, None, :, 0], ph[:, None, :, 1]
        g = p * (px * px + py * py) - (px * t.real + py * t.imag)
    return dt(scale) * g


def grad_scale(B, N, dloss=1.0, dloss_dev=None):
    return dloss * (1.0 if dloss_dev is None else dloss_dev) * 2.0 / (float(B) * float(N))


# ------------------------------------------------------------------ cases
class Case(object):
    '''one row of a table.  kind: 'sep' (danet_separate_fwd / _bwd), 'fused' (danet_separate_pit_*),
    'loss' (danet_pit_mse_*).'''

    def __init__(self, kind, name, B, C, N, E=0, act=0, mode=0, partials=False, want='random', phasor_len=1.0,
                 zero_frame=False, tie=None, sat=False, dloss=1.0, dloss_dev=None, forced=False, salt=0):
        assert kind in ('sep', 'fused', 'loss')
        self.kind, self.name, self.B, self.C, self.N, self.E = kind, name, B, C, N, E
        self.act, self.mode, self.partials, self.want = act, mode, partials, want
        self.phasor_len, self.zero_frame, self.tie, self.sat = phasor_len, zero_frame, tie, sat
        self.dloss, self.dloss_dev, self.forced = dloss, dloss_dev, forced
        self.salt = salt          # another draw of the inputs: a row that broke a condition of the bar is replaced

    def __repr__(self):
        return self.name

    @property
    def inst(self):
        '''(EP, EF, CP) of the attractor.hip kernels this row reaches'''
        return (pick_ep(self.E), self.E == pick_ep(self.E), self.C)

    @property
    def vector_guarded(self):
        '''the guarded 16-byte path of load_row / store_row: E % 4 == 0 below EP'''
        return self.E % 4 == 0 and self.E < pick_ep(self.E)

    @property
    def grads_compared(self):
        '''saturated rows: the gradients are exp(-30) of the inputs' size and carry the logits' float32 rounding
        as a relative error; the issue asks for finite results and for the masks there'''
        return not self.sat

    @property
    def scale(self):
        return grad_scale(self.B, self.N, self.dloss, self.dloss_dev)

    def describe(self):
        return ('%s: kind=%s B=%d C=%d N=%d E=%d act=%d mode=%d inst=%s partials=%s want=%s phasor_len=%g zero_frame=%s '
                'tie=%s sat=%s dloss=%g dloss_dev=%s forced=%s' % (
                    self.name, self.kind, self.B, self.C, self.N, self.E, self.act, self.mode, self.inst, self.partials,
                    self.want, self.phasor_len, self.zero_frame, self.tie, self.sat, self.dloss, self.dloss_dev,
                    self.forced))


def _sat_embedding(rng, B, C, N, E, act):
    '''logits near +-100 whose pairwise gaps are at least 30 (softmax masks exactly 0 / 1 in float32), or
    sigmoid logits +-100: attr[c] = 10 e_c, embed[n] = sum_c level[n][c] / 10 e_c'''
    assert E >= C
    levels = np.array([100.0, -100.0, 62.0, -64.0][:C]) if act == 0 else np.array([100.0, -100.0, 100.0, -100.0][:C])
    lv = np.stack([rng.permutation(levels) for _ in range(B * N)]).reshape(B, N, C) + rng.uniform(-1, 1, (B, N, C))
    embed = np.zeros((B, N, E))
    embed[:, :, :C] = lv / 10
    attr = np.zeros((B, C, E))
    attr[:, np.arange(C), np.arange(C)] = 10
    return embed.astype(np.float32), attr.astype(np.float32)


def _make_src(rng, p, ang, mix, want):
    '''truth whose magnitudes follow the estimates under the permutation want[b]: truth i <- estimate want[b][i]'''
    B, C, N = p.shape
    pw = np.take_along_axis(p, want[:, :, None], axis=1)
    mag = pw * rng.uniform(0.6, 1.4, (B, C, N)) + 0.2 * mix[:, None, :] * rng.uniform(0, 1, (B, C, N))
    a = ang[:, None, :] + 0.4 * rng.randn(B, C, N)
    return (mag * np.exp(1j * a)).astype(np.complex64)


def _build(case):
    c = case
    rng = np.random.RandomState((zlib.crc32(c.name.encode()) + c.salt) & 0x7FFFFFFF)
    B, C, N, E = c.B, c.C, c.N, c.E
    d = {}
    ang = rng.uniform(-np.pi, np.pi, (B, N))
    mix = ((np.abs(rng.randn(B, N)) + 0.1) * 2).astype(np.float32)
    d['mix_pwr'] = mix
    if c.kind != 'loss':
        if c.sat:
            embed, attr = _sat_embedding(rng, B, C, N, E, c.act)
        else:
            embed = (rng.randn(B, N, E) / np.sqrt(E)).astype(np.float32)
            attr = rng.randn(B, C, E).astype(np.float32)
        if c.tie:
            attr[:, c.tie[1]] = attr[:, c.tie[0]]
        d['embed'], d['attr'] = embed, attr
        p = sep_forward(c.act, mix, attr, embed, np.float64)[0]
    else:
        p = ((np.abs(rng.randn(B, C, N)) + 0.1) * 0.5 * mix[:, None, :]).astype(np.float32)
        if c.tie:
            p[:, c.tie[1]] = p[:, c.tie[0]]
        d['sep_pwr'] = p
    if c.kind == 'sep':
        d['dout'] = rng.randn(B, C, N).astype(np.float32)
        return d
    nperm = math.factorial(C)
    which = np.arange(B) % nperm if c.want == 'cycle' else rng.randint(0, nperm, B)
    want = np.array(perms_of(C))[which]
    src = _make_src(rng, p.astype(np.float64), ang, mix.astype(np.float64), want)
    if c.zero_frame:
        lo, hi = min(3, N - 1), min(N, 12)
        ang[:, lo:hi] = 0
    phasor = (np.stack([np.cos(ang), np.sin(ang)], axis=-1) * c.phasor_len).astype(np.float32)
    for _ in range(50):
        if c.zero_frame:
            src[:, :, lo:hi] = 0
        if C == 1 or c.tie:
            break
        v = perm_losses(pit_cross(c.mode, src, p, phasor, np.float64)[0], N)
        bad = np.nonzero(runner_up_gap(v) < 3 * GAP)[0]
        if not len(bad):
            break
        # a near tie between two permutations (a badly chosen input): draw that utterance's truth again
        src[bad] = _make_src(rng, p[bad].astype(np.float64), ang[bad], mix[bad].astype(np.float64), want[bad])
    d['src'], d['phasor'], d['want'] = src, phasor, which.astype(np.int32)
    return d


def runner_up_gap(v):
    '''second smallest / smallest - 1 of each row of v [B][C!] (inf for one permutation)'''
    if v.shape[1] == 1:
        return np.full(v.shape[0], np.inf)
    s = np.sort(v, axis=1)
    return s[:, 1] / s[:, 0] - 1


@functools.lru_cache(maxsize=2)
def _inputs(name):
    return _build(BY_NAME[name])


def inputs(case):
    '''float32 / complex64 host arrays of the case (treat as read-only)'''
    return _inputs(case.name)


def _zero_scale(r, d, dout):
    '''softmax over ONE speaker: the mask is 1 and dembed, dattr are 0 = dm - 1 * dm, exactly so in float64 and in
    the restatement.  A kernel may leave the rounding residue of the two terms (a fused multiply-add keeps dout *
    mix_pwr unrounded on one side), so these outputs are held to TOL of the size of the terms that cancel,
    max |dm| max |attr| and max_e sum_n |dm x|, instead of to their own maximum, which is 0'''
    dm = np.abs(dout.astype(np.float64) * d['mix_pwr'][:, None, :])[:, 0, :]                   # [B][N]
    r['zero_scale'] = {'dembed': float(dm.max() * np.abs(d['attr']).max()),
                       'dattr': float((dm[:, :, None] * np.abs(d['embed'])).sum(axis=1).max())}
    r['zero_scale']['partials'] = r['zero_scale']['dattr']


def _reference(case, dt, perm_idx):
    c, d = case, inputs(case)
    r = {}
    if c.kind == 'sep':
        r['out'], r['masks'] = sep_forward(c.act, d['mix_pwr'], d['attr'], d['embed'], dt)
        r['dembed'], r['dattr'] = sep_backward(c.act, d['mix_pwr'], d['attr'], d['embed'], d['dout'], dt, r['masks'])
        if c.act == 0 and c.C == 1:
            _zero_scale(r, d, d['dout'])
        return r
    if c.kind == 'fused':
        p, m = sep_forward(c.act, d['mix_pwr'], d['attr'], d['embed'], dt)
        r['out'], r['masks'] = p, m
    else:
        p = d['sep_pwr']
    L, S, sig = pit_cross(c.mode, d['src'], p, d['phasor'], dt)
    r['loss'], r['snr'], r['perm_idx'], r['v'] = pit_reduce(L, S, sig, c.N, EPS, dt)
    best = r['perm_idx'] if perm_idx is None else perm_idx
    nperm = math.factorial(c.C)
    used = (best + 1) % nperm if c.forced else best       # forced: deliberately NOT the best permutation
    r['used_perm'] = used.astype(np.int32)
    dsep = pit_dsep(c.mode, d['src'], p, d['phasor'], used, c.scale, dt)
    if c.kind == 'loss':
        r['dsep'] = dsep
        return r
    r['dembed'], r['dattr'] = sep_backward(c.act, d['mix_pwr'], d['attr'], d['embed'], dsep, dt, m)
    if c.act == 0 and c.C == 1:
        _zero_scale(r, d, dsep)
    if c.partials:
        # every permutation's attractor gradient at scale dloss * 2 / (B N): [B][C!][C][E]
        per = []
        for q in range(nperm):
            ds = pit_dsep(c.mode, d['src'], p, d['phasor'], np.full(c.B, q), grad_scale(c.B, c.N, c.dloss), dt)
            per.append(sep_backward(c.act, d['mix_pwr'], d['attr'], d['embed'], ds, dt, m)[1])
        r['partials'] = np.stack(per, axis=1)
    return r


@functools.lru_cache(maxsize=2)
def _reference_cached(name):
    case = BY_NAME[name]
    r64 = _reference(case, np.float64, None)
    # the restatement's gradients are those of the SAME permutation (like for like)
    r32 = _reference(case, np.float32, r64.get('perm_idx'))
    return r64, r32


def reference_under(case, perm_idx):
    '''(float64 reference, float32 restatement) whose loss, SNR and gradients are those of the given permutations
    instead of the best ones (the near-tie rows)'''
    d, out = inputs(case), []
    for dt in (np.float64, np.float32):
        r = _reference(case, dt, perm_idx)
        L, S, sig = pit_cross(case.mode, d['src'], r['out'], d['phasor'], dt)
        r['loss'], r['snr'] = pit_reduce(L, S, sig, case.N, EPS, dt, perm_idx)[:2]
        out.append(r)
    return tuple(out)


def reference(case):
    '''(float64 reference, float32 restatement): dicts of the outputs of the case's kind'''
    return _reference_cached(case.name)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def snr_err(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1.0)


def compared_outputs(case):
    '''names of the outputs of a row that are held to the bar (and to the restatement's condition)'''
    c = case
    if c.kind == 'sep':
        names = ['out', 'masks']
        grads = ['dembed', 'dattr']
    elif c.kind == 'fused':
        names = ['out', 'loss', 'snr']
        grads = ['dembed', 'dattr'] + (['partials'] if c.partials else [])
    else:
        names = ['loss', 'snr']
        grads = ['dsep']
    return names + (grads if c.grads_compared else [])


def error_of(name, got, r64):
    '''error of the output `name` against the float64 reference r64 (a dict of reference()): relative to the
    output's maximum; the SNR against max(|snr|, 1); an output that is identically zero against its zero_scale'''
    ref = r64[name]
    if name == 'snr':
        return snr_err(got, ref)
    if name in r64.get('zero_scale', ()) and not np.any(ref):
        return float(np.abs(np.asarray(got, np.float64)).max() / r64['zero_scale'][name])
    return relerr(got, ref)


def restatement_errors(case):
    '''{output: error of the float32 restatement against float64}'''
    r64, r32 = reference(case)
    return {k: error_of(k, r32[k], r64) for k in compared_outputs(case)}


# ------------------------------------------------------------------ the tables
# every EP: E == EP, an odd E and, where one exists, an E % 4 == 0 below EP
E_LIST = (1, 3, 4) + (5, 8) + (12, 17, 20) + (24, 33, 40) + (44, 63, 64)
ACT = ('sm', 'sg')
MODE = ('cx', 'mag')

# 1. the instantiation matrix, B = 2, N = 2049 (two chunks, the second of exactly one bin)
INST_SEP = [Case('sep', 'inst-sep-E%d-C%d-%s' % (E, C, ACT[a]), 2, C, 2049, E, act=a)
            for E in E_LIST for C in (1, 2, 3, 4) for a in (0, 1)]
# draws replaced because they broke a condition (tests/test_sep_cpu.py): E = 1 leaves B * C = 2 .. 8 attractor
# gradients, each a sum of mixed sign that may cancel, and attractors that may nearly coincide (a near tie)
SALT = {'inst-fused-E1-C1-sg-mag': 4, 'inst-fused-E1-C2-sm-mag': 4, 'inst-fused-E1-C4-sg-cx': 5}


def _fused_name(E, C, a, m):
    return 'inst-fused-E%d-C%d-%s-%s' % (E, C, ACT[a], MODE[m])


INST_FUSED = [Case('fused', _fused_name(E, C, a, m), 2, C, 2049, E, act=a, mode=m, salt=SALT.get(_fused_name(E, C, a, m), 0))
              for E in E_LIST for C in (1, 2, 3, 4) for a in (0, 1) for m in (0, 1)]
INST_PARTIALS = [Case('fused', 'inst-part-E%d-%s-%s' % (E, ACT[a], MODE[m]), 2, 2, 2049, E, act=a, mode=m,
                      partials=True, dloss=1.7)
                 for E in E_LIST for a in (0, 1) for m in (0, 1)]

# 2. size edges at (E, C) = (20, 2) [softmax, complex, with partials] and (7, 3) [sigmoid, magnitude]
SIZE_N = (1, 255, 256, 257, 2047, 2048, 2049, 4097, 16385, 32769)
SIZE_B = (1, 7, 8, 16, 17, 24)
_SZ = [(3, N) for N in SIZE_N] + [(B, 2049) for B in SIZE_B] + [(17, 32769)]


def _size_rows(kind):
    rows = []
    for B, N in _SZ:
        tag = 'B%d-N%d' % (B, N)
        if kind == 'sep':
            rows.append(Case('sep', 'size-sep-E20-C2-' + tag, B, 2, N, 20, act=0))
            rows.append(Case('sep', 'size-sep-E7-C3-' + tag, B, 3, N, 7, act=1))
        else:
            rows.append(Case('fused', 'size-fused-E20-C2-' + tag, B, 2, N, 20, act=0, mode=0, partials=True))
            rows.append(Case('fused', 'size-fused-E7-C3-' + tag, B, 3, N, 7, act=1, mode=1))
    return rows


SIZE_SEP = _size_rows('sep')
SIZE_FUSED = _size_rows('fused')
# B = 65535, the stated limit, for every forward and backward entry point
LIMIT = [Case('sep', 'limit-sep-B65535', 65535, 2, 3, 4, act=0),
         Case('fused', 'limit-fused-B65535', 65535, 2, 3, 4, act=0, mode=0, partials=True),
         Case('loss', 'limit-loss-B65535', 65535, 2, 3, mode=0)]

# 3. the stand-alone loss
LOSS_N = (1, 4095, 4096, 4097, 16385, 65537)
LOSS_B = (1, 15, 16, 17, 33)
LOSS = [Case('loss', 'loss-C%d-%s' % (C, MODE[m]), 3, C, 4097, mode=m) for C in (1, 2, 3, 4) for m in (0, 1)]
LOSS += [Case('loss', 'loss-C2-cx-N%d' % N, 2, 2, N, mode=0) for N in LOSS_N]
LOSS += [Case('loss', 'loss-C4-mag-N%d' % N, 2, 4, N, mode=1) for N in LOSS_N]
LOSS += [Case('loss', 'loss-C2-mag-B%d' % B, B, 2, 4097, mode=1) for B in LOSS_B]
LOSS += [Case('loss', 'loss-C4-cx-B%d' % B, B, 4, 4097, mode=0) for B in LOSS_B]
# each of the C! permutations is the best one of some utterance (two rounds of pit_final_kernel at C = 4)
ALL_PERMS = [Case('loss', 'perms24-loss-C4-cx', 26, 4, 257, mode=0, want='cycle'),
             Case('loss', 'perms24-loss-C4-mag', 26, 4, 257, mode=1, want='cycle'),
             Case('fused', 'perms6-fused-C3', 7, 3, 2049, 7, act=0, mode=0, want='cycle'),
             Case('fused', 'perms24-fused-C4', 26, 4, 2049, 5, act=1, mode=1, want='cycle')]

# 4. options and values
FORCED = [Case('fused', 'forced-fused-C2', 3, 2, 2049, 20, act=0, mode=0, forced=True),
          Case('fused', 'forced-fused-C3', 7, 3, 2049, 7, act=1, mode=1, forced=True, want='cycle'),
          Case('fused', 'forced-fused-C4', 5, 4, 300, 12, act=0, mode=0, forced=True),
          Case('loss', 'forced-loss-C3', 7, 3, 4097, mode=0, forced=True, want='cycle'),
          Case('loss', 'forced-loss-C4', 5, 4, 300, mode=1, forced=True)]
DLOSS = [Case('fused', 'dloss-fused-C2', 3, 2, 2049, 20, act=0, mode=0, dloss=1.7, dloss_dev=-0.6, partials=True),
         Case('fused', 'dloss-fused-C3', 3, 3, 300, 8, act=1, mode=1, dloss=1.7, dloss_dev=-0.6),
         Case('loss', 'dloss-loss-C3', 3, 3, 300, mode=0, dloss=1.7, dloss_dev=-0.6)]
PHASOR = [Case(k, 'phasor%g-%s-%s' % (ln, k, MODE[m]), 3, 2 if k == 'fused' else 3, 2049, 20 if k == 'fused' else 0,
               act=0, mode=m, phasor_len=ln, partials=(k == 'fused'))
          for k in ('fused', 'loss') for ln in (0.5, 2.0) for m in (0, 1)]
ZERO = [Case('fused', 'zero-fused-%s' % MODE[m], 3, 2, 300, 20, act=0, mode=m, zero_frame=True, partials=True)
        for m in (0, 1)]
ZERO += [Case('loss', 'zero-loss-%s' % MODE[m], 3, 3, 300, mode=m, zero_frame=True) for m in (0, 1)]
TIES = [Case('loss', 'tie-loss-C2', 5, 2, 4097, mode=0, tie=(0, 1)),
        Case('loss', 'tie-loss-C3', 19, 3, 4097, mode=1, tie=(0, 2), want='cycle'),
        Case('loss', 'tie-loss-C4', 26, 4, 300, mode=0, tie=(1, 3), want='cycle'),
        # (sigmoid: with two identical softmax rows the embedding gradient vanishes by symmetry.  E = 40 with
        # partials: at C = 2 most instantiations do NOT turn identical attractors into identical estimates, see NEAR_TIES)
        Case('fused', 'tie-fused-C2', 5, 2, 2049, 40, act=1, mode=0, tie=(0, 1), partials=True),
        Case('fused', 'tie-fused-C3', 19, 3, 2049, 7, act=1, mode=1, tie=(1, 2), want='cycle'),
        Case('fused', 'tie-fused-C4', 26, 4, 300, 8, act=0, mode=0, tie=(0, 3), want='cycle')]
# Identical attractor rows where the kernel's two estimates are NOT bit-identical: the compiler contracts the two
# speakers' dot products differently (sep_pit_fwd_kernel<20, 2, true, true>: speaker 1 a chain of 20 fused
# multiply-adds, 12 of speaker 0's terms unfused; measured: every C = 2 instantiation tried below EP = 40), so the
# estimates are an ulp apart, the two permutations' losses differ by 1e-7 relative and either index is a correct
# float32 answer.  What the header still promises there: danet_separate_pit_final and the records-fed backward
# arrive at the SAME index, the index is a minimum to float32 rounding, and loss / SNR / gradients are those of
# that permutation at the bar.  (Not changed in the kernel: any change of the forward's rounding changes every
# later step of a training run.)
NEAR_TIES = [Case('fused', 'neartie-fused-C2-E20', 5, 2, 2049, 20, act=1, mode=0, tie=(0, 1), partials=True)]
SAT = [Case('sep', 'sat-sep-softmax-C%d' % C, 2, C, 300, 20, act=0, sat=True) for C in (2, 3, 4)]
SAT += [Case('sep', 'sat-sep-sigmoid-C2', 2, 2, 300, 20, act=1, sat=True)]
SAT += [Case('fused', 'sat-fused-softmax-C%d-%s' % (C, MODE[m]), 2, C, 300, 20, act=0, mode=m, sat=True,
             partials=(C == 2)) for C in (2, 3, 4) for m in (0, 1)]
SAT += [Case('fused', 'sat-fused-sigmoid-C2', 2, 2, 300, 20, act=1, mode=0, sat=True)]
# the option rows (masks / sep_pwr_out / snr / dembed NULL or given, records or perm_idx) run on these
OPTION_SEP = Case('sep', 'opt-sep', 3, 3, 2049, 12, act=0)
OPTION_FUSED = [Case('fused', 'opt-fused-E12-C3', 3, 3, 2049, 12, act=0, mode=0),
                Case('fused', 'opt-fused-E20-C2', 3, 2, 2049, 20, act=1, mode=1, partials=True)]
OPTION_LOSS = Case('loss', 'opt-loss', 3, 3, 4097, mode=0)

SEP_ROWS = INST_SEP + SIZE_SEP + [c for c in LIMIT + SAT if c.kind == 'sep'] + [OPTION_SEP]
FUSED_ROWS = (INST_FUSED + INST_PARTIALS + SIZE_FUSED +
              [c for c in LIMIT + ALL_PERMS + FORCED + DLOSS + PHASOR + ZERO + TIES + NEAR_TIES + SAT if c.kind == 'fused'] +
              OPTION_FUSED)
LOSS_ROWS = LOSS + [c for c in LIMIT + ALL_PERMS + FORCED + DLOSS + PHASOR + ZERO + TIES if c.kind == 'loss'] + [OPTION_LOSS]
ALL_ROWS = SEP_ROWS + FUSED_ROWS + LOSS_ROWS
REPEATED = SIZE_SEP + SIZE_FUSED          # every row of table 2 runs twice and must be bit-identical
BY_NAME = {c.name: c for c in ALL_ROWS}
assert len(BY_NAME) == len(ALL_ROWS)

# 5. refusals: (entry point, changed arguments, expected return code); every one is returned before any launch
BASE = dict(act=0, mode=0, B=2, C=2, N=5, E=4, eps=EPS, dloss=1.0)
SIGS = {
    'danet_separate_fwd': ('act', 'B', 'C', 'N', 'E', 'mix_pwr', 'attr', 'embed', 'out', 'masks'),
    'danet_separate_bwd': ('act', 'B', 'C', 'N', 'E', 'mix_pwr', 'attr', 'embed', 'dout', 'dembed', 'dattr', 'ws',
                           'ws_bytes'),
    'danet_pit_mse_fwd': ('mode', 'B', 'C', 'N', 'src', 'sep_pwr', 'phasor', 'eps', 'loss', 'snr', 'perm_idx', 'ws',
                          'ws_bytes'),
    'danet_pit_mse_bwd': ('mode', 'B', 'C', 'N', 'src', 'sep_pwr', 'phasor', 'perm_idx', 'dloss', 'dloss_dev', 'dsep'),
    'danet_separate_pit_fwd_records': ('act', 'mode', 'B', 'C', 'N', 'E', 'mix_pwr', 'attr', 'embed', 'src', 'phasor',
                                       'sep_pwr_out', 'records', 'dattr_partials'),
    'danet_separate_pit_final': ('B', 'C', 'N', 'eps', 'records', 'loss', 'snr', 'perm_idx'),
    'danet_separate_pit_bwd': ('act', 'mode', 'B', 'C', 'N', 'E', 'mix_pwr', 'attr', 'embed', 'src', 'phasor',
                               'perm_idx', 'records', 'dloss', 'dloss_dev', 'dembed', 'dattr', 'ws', 'ws_bytes'),
}
REQUIRED = {      # the pointers that must not be NULL (perm_idx / records of the fused backward: one of the two)
    'danet_separate_fwd': ('mix_pwr', 'attr', 'embed', 'out'),
    'danet_separate_bwd': ('mix_pwr', 'attr', 'embed', 'dout', 'dembed', 'dattr'),
    'danet_pit_mse_fwd': ('src', 'sep_pwr', 'phasor', 'loss', 'perm_idx'),
    'danet_pit_mse_bwd': ('src', 'sep_pwr', 'phasor', 'perm_idx', 'dsep'),
    'danet_separate_pit_fwd_records': ('mix_pwr', 'attr', 'embed', 'src', 'phasor', 'records'),
    'danet_separate_pit_final': ('records', 'loss', 'perm_idx'),
    'danet_separate_pit_bwd': ('mix_pwr', 'attr', 'embed', 'src', 'phasor', 'dattr'),
}
WS_OF = {'danet_separate_bwd': lambda a: ws_separate_bwd(a['B'], a['C'], a['N'], a['E']),
         'danet_separate_pit_bwd': lambda a: ws_separate_pit(a['B'], a['C'], a['N'], a['E']),
         'danet_pit_mse_fwd': lambda a: ws_pit_mse(a['B'], a['C'], a['N'])}
SEPARATORS = ('danet_separate_fwd', 'danet_separate_bwd', 'danet_separate_pit_fwd_records', 'danet_separate_pit_bwd')


def refusals():
    rows = []
    for ep, sig in SIGS.items():
        if 'E' in sig:
            rows.append((ep, {'E': 65}, ERR_UNSUPPORTED))
            rows.append((ep, {'E': 0}, ERR_ARG))
        rows.append((ep, {'C': 5}, ERR_ARG))
        rows.append((ep, {'B': 0}, ERR_ARG))
        rows.append((ep, {'N': 0}, ERR_ARG))
        if 'act' in sig:
            rows.append((ep, {'act': 2}, ERR_ARG))
        if 'mode' in sig:
            rows.append((ep, {'mode': 2}, ERR_ARG))
        for name in REQUIRED[ep]:
            rows.append((ep, {name: None}, ERR_ARG))
        if ep in SEPARATORS:
            rows.append((ep, {'B': 65536}, ERR_UNSUPPORTED))
        elif ep.startswith('danet_pit_mse'):
            rows.append((ep, {'B': 65536}, ERR_ARG))
        if ep in WS_OF:
            rows.append((ep, {'ws_short': 1}, ERR_WORKSPACE))
            rows.append((ep, {'ws': None}, ERR_WORKSPACE))
    rows.append(('danet_separate_pit_bwd', {'perm_idx': None, 'records': None}, ERR_ARG))
    rows.append(('danet_separate_pit_fwd_records', {'C': 3, 'dattr_partials': 'given'}, ERR_UNSUPPORTED))
    return rows


# ------------------------------------------------------------------ guarded device buffers, launches
def _torch():
    import torch
    return torch


class Guarded(object):
    '''n elements (4 bytes each) between GUARD sentinel words on either side, all pre-filled with the sentinel, a
    NaN: the guards must survive bit for bit, and a slot that is read without having been written poisons the result'''

    def __init__(self, n, dtype=None):
        torch = _torch()
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(dtype or torch.float32)

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def written(self):
        '''no element still holds the sentinel'''
        return not bool((self.buf[GUARD:GUARD + self.n] == SENT).any())

    def numpy(self, shape=None):
        a = self.t.cpu().numpy()
        return a.reshape(shape) if shape is not None else a


def dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    if np.iscomplexobj(a):
        a = a.view(np.float32)
    return torch.from_numpy(a).cuda()


def _arg(v):
    if isinstance(v, Guarded):
        return v.t.data_ptr()
    if v is None or isinstance(v, (int, float)):
        return v
    return v.data_ptr()


def call(ep, args):
    '''the entry point `ep` on the current stream with the named arguments of SIGS[ep]; returns its code'''
    from danet_amd import _lib
    L = _lib.load()
    return getattr(L, ep)(_lib.stream(), *[_arg(args[k]) for k in SIGS[ep]])


class Launch(object):
    '''the device inputs of a row and its guarded outputs; every run_* allocates its outputs anew, at exactly
    their size, checks the return code and, after the synchronisation, every guard'''

    def __init__(self, case):
        c = self.case = case
        d = inputs(case)
        self.a = dict(act=c.act, mode=c.mode, B=c.B, C=c.C, N=c.N, E=c.E, eps=EPS, dloss=c.dloss, dloss_dev=None)
        for k in ('mix_pwr', 'attr', 'embed', 'dout', 'src', 'phasor', 'sep_pwr'):
            if k in d:
                self.a[k] = dev(d[k])
        if c.dloss_dev is not None:
            self.a['dloss_dev'] = dev(np.array([c.dloss_dev], np.float32))
        self.guards = []

    def g(self, n, dtype=None):
        buf = Guarded(n, dtype)
        self.guards.append(buf)
        return buf

    def run(self, ep, **kw):
        torch = _torch()
        args = dict(self.a)
        args.update(kw)
        rc = call(ep, args)
        torch.cuda.synchronize()
        assert rc == OK, '%s returned %d: %s' % (ep, rc, self.case.describe())
        for buf in self.guards:
            assert buf.intact(), '%s wrote outside a buffer: %s' % (ep, self.case.describe())
        return args

    # -- danet_separate_fwd / _bwd
    def separate_fwd(self, masks=True):
        c = self.case
        out, mk = self.g(c.B * c.C * c.N), self.g(c.B * c.N * c.C) if masks else None
        self.run('danet_separate_fwd', out=out, masks=mk)
        assert out.written() and (mk is None or mk.written())
        return out.numpy((c.B, c.C, c.N)), None if mk is None else mk.numpy((c.B, c.N, c.C))

    def separate_bwd(self):
        c = self.case
        nb = ws_separate_bwd(c.B, c.C, c.N, c.E)
        de, da, ws = self.g(c.B * c.N * c.E), self.g(c.B * c.C * c.E), self.g(nb // 4)
        self.run('danet_separate_bwd', dembed=de, dattr=da, ws=ws, ws_bytes=nb)
        assert de.written() and da.written()
        return de.numpy((c.B, c.N, c.E)), da.numpy((c.B, c.C, c.E))

    # -- danet_pit_mse_fwd / _bwd
    def pit_mse_fwd(self, snr=True):
        torch, c = _torch(), self.case
        nb = ws_pit_mse(c.B, c.C, c.N)
        loss, sn, pi, ws = self.g(1), self.g(1) if snr else None, self.g(c.B, torch.int32), self.g(nb // 4)
        self.run('danet_pit_mse_fwd', loss=loss, snr=sn, perm_idx=pi, ws=ws, ws_bytes=nb)
        assert ws.written()
        return float(loss.numpy()[0]), None if sn is None else float(sn.numpy()[0]), pi.numpy()

    def pit_mse_bwd(self, perm_idx):
        c = self.case
        ds = self.g(c.B * c.C * c.N)
        self.run('danet_pit_mse_bwd', perm_idx=dev(np.asarray(perm_idx, np.int32)), dsep=ds)
        assert ds.written()
        return ds.numpy((c.B, c.C, c.N))

    # -- danet_separate_pit_fwd_records / _final / _bwd
    def pit_fwd_records(self, sep_pwr_out=False, partials=None):
        c = self.case
        partials = c.partials if partials is None else partials
        nch, EP = n_chunks(c.N), pick_ep(c.E)
        self.records = self.g(ws_records(c.B, c.N) // 4)
        out = self.g(c.B * c.C * c.N) if sep_pwr_out else None
        gp = self.g(ws_partials(c.B, c.C, c.N, c.E) // 4) if partials else None
        self.run('danet_separate_pit_fwd_records', sep_pwr_out=out, records=self.records, dattr_partials=gp)
        assert self.records.written() and (out is None or out.written()) and (gp is None or gp.written())
        return (None if out is None else out.numpy((c.B, c.C, c.N)),
                None if gp is None else gp.numpy((c.B, nch, math.factorial(c.C), c.C, EP)))

    def pit_final(self, snr=True):
        torch, c = _torch(), self.case
        loss, sn, pi = self.g(1), self.g(1) if snr else None, self.g(c.B, torch.int32)
        self.run('danet_separate_pit_final', records=self.records, loss=loss, snr=sn, perm_idx=pi)
        return float(loss.numpy()[0]), None if sn is None else float(sn.numpy()[0]), pi.numpy()

    def pit_bwd(self, perm_idx=None, dembed=True):
        '''perm_idx None: the backward is fed the forward's records and derives the permutation itself'''
        c = self.case
        nb = ws_separate_pit(c.B, c.C, c.N, c.E)
        de, da, ws = self.g(c.B * c.N * c.E) if dembed else None, self.g(c.B * c.C * c.E), self.g(nb // 4)
        kw = dict(perm_idx=None, records=self.records) if perm_idx is None else \
            dict(perm_idx=dev(np.asarray(perm_idx, np.int32)), records=None)
        self.run('danet_separate_pit_bwd', dembed=de, dattr=da, ws=ws, ws_bytes=nb, **kw)
        assert (de is None or de.written()) and da.written()
        return None if de is None else de.numpy((c.B, c.N, c.E)), da.numpy((c.B, c.C, c.E))


def sum_partials(gp, E, dloss):
    '''[B][nch][C!][C][EP] -> each permutation's summed partials times dloss [B][C!][C][E] (float64 sums: the
    consumers' chunk sum is not under test here); the pad columns e >= E must be exact zeros'''
    assert not np.any(gp[..., E:]), 'non-zero pad column in dattr_partials'
    return gp[..., :E].astype(np.float64).sum(axis=1) * dloss


class Report(object):
    '''collects (output, kernel error, restatement error) of one row, prints them and asserts both bars'''
    families = {}

    def __init__(self, case, family, refs=None):
        self.case, self.family, self.rows = case, family, []
        self.r64, self.r32 = refs or reference(case)

    def add(self, name, got, ref_name=None):
        ref_name = ref_name or name
        assert np.isfinite(np.asarray(got, np.float64)).all(), 'non-finite %s: %s' % (name, self.case.describe())
        if ref_name not in compared_outputs(self.case):
            return                                              # (saturated rows: the gradients must be finite)
        self.rows.append((name, error_of(ref_name, got, self.r64), error_of(ref_name, self.r32[ref_name], self.r64)))

    def check(self):
        k, f = max(r[1] for r in self.rows), max(r[2] for r in self.rows)
        print('%-34s %-14s kernel %.2e  float32 %.2e  ratio %.1f  %s' % (
            self.case.name, self.family, k, f, k / max(f, 1e-8),
            ' '.join('%s=%.1e' % r[:2] for r in self.rows)))
        fam = Report.families.setdefault(self.family, [0.0, 0.0, 0.0])
        fam[0], fam[1], fam[2] = max(fam[0], k), max(fam[1], f), max(fam[2], k / max(f, 1e-8))
        bad32 = [r for r in self.rows if not r[2] < F32_BAR]
        assert not bad32, 'badly chosen input, float32 alone misses %g: %s\n%s' % (F32_BAR, bad32, self.case.describe())
        bad = [r for r in self.rows if not r[1] < TOL]
        assert not bad, '%s\n%s' % (bad, self.case.describe())
