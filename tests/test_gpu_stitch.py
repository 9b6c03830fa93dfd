'''
GPU tests (run with -m gpu) of chunked inference (INFER_CHUNK_LEN): the three kernels of libdanet_stitch_hip.so through
ops against the float64 restatement tests/stitch_ref.py over a table of shapes, every output and the workspace between
poisoned guard bands, bit-identical repeats; known answers (swapped channels undone bit for bit, an all-zero overlap, an
exact tie, garbage permutation tables, argument errors before any launch); then Model.infer_chunks / infer_long / infer
and the command line at the shape of smoke().

Bars.  Affinity: |S - math.fsum| <= 1e-12 * sum |a b| (a float64 tree over at most 2^25 terms errs by about
25 * 2^-53 of that sum).  Assignment: the restatement's best total beats the runner-up by more than 1e-9 relative in
every pair of every case (asserted first), then perm must be equal.  Merge outside the fades: bit for bit
np.float32(m) * np.float32(ph).  Inside: 4 * 2^-24 * (|a| + |b|) per real component (one rounding each for b - a, the
multiply-add and the phasor product).
'''
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stitch_ref as SR
from gpu_helpers import ROOT, check_lstm_status, small_model

pytestmark = pytest.mark.gpu

POISON = -7.25e33
IPOISON = -1234567
GUARD = 1024
EPS = 2.0 ** -24
CS, FS = (1, 2, 3, 4), (1, 33, 129, 257)
LVS = ((2, 1), (4, 1), (4, 2), (8, 3), (128, 32), (128, 64))
NS = (2, 3, 7, 40)


def _table():
    '''(C, F, L, V, T): every (L, V) with every n of NS and every last hop of {1, 2, H - 1, H} that exists, C and F
    dealt round so that all 16 (C, F) pairs occur every 16 cases'''
    cases = []
    for L, V in LVS:
        H = L - V
        for n in NS:
            for hop in sorted(set(h for h in (1, 2, H - 1, H) if 1 <= h <= H)):
                k = len(cases)
                T = (n - 2) * H + hop + L
                assert SR.chunks(T, L, V) == n and SR.plan(T, L, V)[-1] - SR.plan(T, L, V)[-2] == hop
                cases.append((CS[k % 4], FS[(k // 4) % 4], L, V, T))
    assert set((c[0], c[1]) for c in cases) == set((C, F) for C in CS for F in FS)
    return cases


CASES = _table()


def _guarded(shape, dtype=torch.float32, poison=POISON):
    '''(whole buffer, the view of `shape` in its middle): everything poisoned'''
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, poison=POISON):
    return bool((buf[:GUARD] == poison).all()) and bool((buf[-GUARD:] == poison).all())


def _bits(t):
    a = torch.view_as_real(t) if t.is_complex() else t
    a = a.detach().cpu().contiguous()
    return a.numpy().view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.element_size()]).copy()


def speakers(C, T, F, seed):
    '''C magnitude tracks with distinct levels, spectral envelopes and frame patterns, float32 [C, T, F]'''
    rng = np.random.RandomState(seed)
    f = np.arange(F)[None, None, :]
    t = np.arange(T)[None, :, None]
    c = np.arange(C)[:, None, None]
    env = (1.0 + 0.5 * c) * (1.0 + 4.0 * (f % C == c) + 2.0 * ((t + c) % (C + 1) == 0))
    return (env * rng.uniform(0.5, 1.5, (C, T, F))).astype(np.float32)


def inputs(C, F, L, V, T, seed=0, jitter=0.2):
    '''(mags [n, C, L, F], phasor [n, L, F, 2], swaps): the chunks of `speakers`, every chunk with its own channel
    order and its own multiplicative jitter (so the two sources of a fade differ); unit phasors'''
    rng = np.random.RandomState(1000003 * seed + 7919 * T + 101 * F + 13 * L + C)
    chunks = SR.cut(speakers(C, T, F, seed + T), T, L, V)                       # [n, C, L, F]
    n = len(chunks)
    swaps = [list(range(C))] + [list(rng.permutation(C)) for _ in range(n - 1)]
    mags = np.stack([ch[sw] for ch, sw in zip(chunks, swaps)])
    if jitter:
        mags = mags * rng.uniform(1.0 - jitter, 1.0 + jitter, mags.shape)
    th = rng.uniform(-np.pi, np.pi, (T, F))
    ph = SR.cut(np.stack([np.cos(th), np.sin(th)], axis=-1).astype(np.float32).transpose(2, 0, 1), T, L, V)
    return mags.astype(np.float32), np.ascontiguousarray(ph.transpose(0, 2, 3, 1)), swaps


class Run(object):
    '''the three stages of one case through ops, every output and the workspace guarded'''

    def __init__(self, mags, phasor, T, V, perm=None):
        from danet_amd import ops
        n, C, L, F = mags.shape
        self.mags, self.phasor = torch.from_numpy(mags).cuda(), torch.from_numpy(phasor).cuda()
        nws = ops.stitch_workspace_bytes(T, L, V, C, F)
        assert nws == SR.workspace_bytes(T, L, V, C, F)
        self.ws_buf, self.ws = _guarded((nws // 8,), torch.float64)
        self.S_buf, self.S = _guarded((n - 1, C, C), torch.float64)
        self.perm_buf, self.perm = _guarded((n, C), torch.int32, IPOISON)
        self.out_buf, out = _guarded((C, T, F, 2))
        self.out = torch.view_as_complex(out)
        ws8 = self.ws.view(torch.uint8)
        assert ops.stitch_affinity(self.mags, T, V, ws=ws8) is ws8
        ops.stitch_assign(ws8, T, L, V, C, F, out=(self.S, self.perm))
        if perm is not None:
            self.perm.copy_(torch.from_numpy(np.asarray(perm, np.int32)).cuda())
        assert ops.stitch_merge(self.mags, self.phasor, self.perm, T, V, out=self.out) is self.out
        torch.cuda.synchronize()

    def intact(self):
        return (_guards_intact(self.ws_buf) and _guards_intact(self.S_buf) and _guards_intact(self.out_buf)
                and _guards_intact(self.perm_buf, IPOISON))

    def written(self):
        return not any(bool((t == p).any()) for t, p in ((self.ws, POISON), (self.S, POISON), (self.perm, IPOISON),
                                                         (torch.view_as_real(self.out), POISON)))

    def bits(self):
        return [_bits(t) for t in (self.ws, self.S, self.perm, self.out)]


def check_merge(out, mags, phasor, perm, T, V):
    '''out complex64 [C, T, F] (numpy) against the restatement with the table `perm`: bit for bit outside the fades,
    inside them within 4 * 2^-24 * (|a| + |b|) per real component; -> the worst fade error over its bar'''
    mag, a, b, faded = SR.merge_mag(mags, perm, T, V)
    ph = SR.owner_phasor(phasor, T, V)
    worst = 0.0
    for k, part in ((0, out.real), (1, out.imag)):
        p32 = ph[None, :, :, k]
        assert np.array_equal(part[:, ~faded], (a * p32)[:, ~faded])          # float32 x float32, one rounding
        err = np.abs(part.astype(np.float64) - mag * p32.astype(np.float64))[:, faded]
        bar = (4 * EPS * (np.abs(a).astype(np.float64) + np.abs(b)))[:, faded]
        assert (err <= bar).all(), float((err / np.maximum(bar, 1e-300)).max())
        if faded.any():
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
    return worst


# ------------------------------------------------------------------------------------- kernels
def test_the_table_covers_the_grid_and_the_restatement_meets_the_margin_in_every_case():
    '''no device work: the assignment margin is shown from the restatement alone, for every pair of every case'''
    assert len(CASES) == sum(4 * len(set(h for h in (1, 2, L - V - 1, L - V) if 1 <= h <= L - V)) for L, V in LVS)
    assert set(c[2:4] for c in CASES) == set(LVS) and set(SR.chunks(T, L, V) for _, _, L, V, T in CASES) == set(NS)
    worst = float('inf')
    for C, F, L, V, T in CASES:
        mags, _ph, _ = inputs(C, F, L, V, T)
        worst = min(worst, min(SR.margin(S) for S in SR.affinity(mags, T, V)))
    print('smallest margin of the table: %.3e' % worst)
    assert worst > 1e-9


@pytest.mark.parametrize('C,F,L,V,T', CASES)
def test_three_stages_against_the_restatement(C, F, L, V, T):
    mags, phasor, _swaps = inputs(C, F, L, V, T)
    n = len(mags)
    r = Run(mags, phasor, T, V)
    assert r.intact() and r.written()
    # affinity: the tiles summed in order are S, and S is math.fsum to 1e-12 of the sum of magnitudes
    exact, absum = SR.affinity_exact(mags, T, V)
    part = r.ws.cpu().numpy().reshape(n - 1, -1, C, C)
    S = r.S.cpu().numpy()
    tiles = np.zeros_like(S)
    for k in range(part.shape[1]):
        tiles = tiles + part[:, k]
    assert np.array_equal(tiles, S)
    err = float((np.abs(S - exact) / np.maximum(absum, 1e-300)).max())
    # assignment: the margin from the restatement alone, then equal tables
    ref = SR.affinity(mags, T, V)
    margin = min(SR.margin(Si) for Si in ref)
    assert margin > 1e-9, margin
    want = SR.chain(ref)
    perm = r.perm.cpu().numpy()
    worst = check_merge(r.out.cpu().numpy(), mags, phasor, want, T, V)
    print('C=%d F=%d L=%d V=%d T=%d n=%d  S err %.2e of sum|ab| (bar 1e-12)  margin %.2e  fade err %.2f of its bar'
          % (C, F, L, V, T, n, err, margin, worst))
    assert (np.abs(S - exact) <= 1e-12 * absum).all()
    assert np.array_equal(perm, want)
    # repeats are bit-identical
    again = Run(mags, phasor, T, V)
    assert all(np.array_equal(x, y) for x, y in zip(r.bits(), again.bits())) and again.intact()


@pytest.mark.parametrize('C,F,L,V,T', [(2, 129, 128, 32, 300), (3, 33, 8, 3, 41), (4, 257, 4, 1, 30), (4, 1, 8, 4, 23),
                                       (1, 33, 4, 2, 9), (2, 1, 128, 64, 400)])
def test_swapped_channels_are_undone_and_the_merge_is_the_truth_bit_for_bit(C, F, L, V, T):
    truth = speakers(C, T, F, seed=T)
    mags, phasor, swaps = inputs(C, F, L, V, T, jitter=0)
    assert min(SR.margin(S) for S in SR.affinity(mags, T, V)) > 1e-9
    r = Run(mags, phasor, T, V)
    perm = r.perm.cpu().numpy()
    for i, sw in enumerate(swaps):
        assert [sw[k] for k in perm[i]] == list(range(C)), i          # output channel c is speaker c in every chunk
    ph = SR.owner_phasor(phasor, T, V)
    out = r.out.cpu().numpy()
    assert np.array_equal(out.real, truth * ph[None, :, :, 0]) and np.array_equal(out.imag, truth * ph[None, :, :, 1])
    assert r.intact()


def test_an_all_zero_overlap_gives_the_identity_and_an_exact_tie_the_first_permutation():
    C, F, L, V, T = 3, 33, 8, 3, 18
    mags, phasor, _ = inputs(C, F, L, V, T)
    starts = SR.plan(T, L, V)
    mags[1, :, :starts[0] + L - starts[1]] = 0.0                      # chunk 1's side of pair 0's overlap
    r = Run(mags, phasor, T, V)
    assert not r.S[0].any() and r.perm[1].tolist() == [0, 1, 2]
    assert np.array_equal(r.perm.cpu().numpy(), SR.chain(SR.affinity(mags, T, V)))
    # every entry of S equal: a tie of all permutations
    mags = np.full((2, 4, 4, 5), 3.0, np.float32)
    r = Run(mags, np.ones((2, 4, 5, 2), np.float32), 6, 2)
    S = r.S.cpu().numpy()
    assert (S == S[0, 0, 0]).all() and S[0, 0, 0] == 9.0 * 2 * 5 and r.perm.tolist() == [[0, 1, 2, 3]] * 2
    # S = [[0, 2, 2], [2, 0, 2], [2, 2, 0]]: (1, 2, 0) and (2, 0, 1) tie at 6; the first of them wins
    mags = np.zeros((2, 3, 2, 3), np.float32)
    mags[0, :, 1, :] = 2.0 * np.eye(3)
    mags[1, :, 0, :] = 1.0 - np.eye(3)
    r = Run(mags, np.ones((2, 2, 3, 2), np.float32), 3, 1)
    assert r.S[0].tolist() == [[0, 2, 2], [2, 0, 2], [2, 2, 0]] and r.perm.tolist() == [[0, 1, 2], [1, 2, 0]]
    assert r.intact()


def test_garbage_permutation_tables_are_clamped_and_nothing_outside_out_is_written():
    C, F, L, V, T = 3, 129, 8, 3, 41
    mags, phasor, _ = inputs(C, F, L, V, T)
    n = len(mags)
    rng = np.random.RandomState(3)
    garbage = rng.choice(np.array([-1, -2 ** 31, 2 ** 31 - 1, 3, 4, 1 << 20, -(1 << 20), 0, 1, 2], np.int64), (n, C))
    r = Run(mags, phasor, T, V, perm=garbage)
    assert r.intact() and r.written()
    check_merge(r.out.cpu().numpy(), mags, phasor, np.clip(garbage, 0, C - 1), T, V)


def test_misaligned_buffers_take_the_narrow_paths_to_the_same_bits():
    from danet_amd import ops
    C, F, L, V, T = 2, 129, 128, 32, 300                              # L * F and H * F multiples of 4: the wide path
    mags, phasor, _ = inputs(C, F, L, V, T)
    r = Run(mags, phasor, T, V)
    buf = torch.zeros(mags.size + 1, device='cuda')
    off = buf[1:].view(mags.shape)                                    # 4 bytes off a 16-byte boundary
    off.copy_(r.mags)
    assert off.data_ptr() % 16 == 4
    ws = ops.stitch_affinity(off, T, V)
    assert np.array_equal(_bits(ws.view(torch.float64)), _bits(r.ws))
    obuf, out = _guarded((C * T * F + 1, 2))
    out = torch.view_as_complex(out[1:]).view(C, T, F)                # 8 bytes off a 16-byte boundary
    assert out.data_ptr() % 16 == 8
    ops.stitch_merge(r.mags, r.phasor, r.perm, T, V, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(r.out)) and _guards_intact(obuf) and bool((obuf[GUARD:GUARD + 2] == POISON).all())


def test_argument_errors_are_raised_before_any_launch():
    from danet_amd import _lib
    lib = _lib.load_stitch()
    C, F, L, V, T = 2, 33, 8, 3, 41
    mags, phasor, _ = inputs(C, F, L, V, T)
    r = Run(mags, phasor, T, V)
    n = len(mags)
    need = SR.workspace_bytes(T, L, V, C, F)
    _b1, ws = _guarded((need // 8,), torch.float64)
    _b2, S = _guarded((n - 1, C, C), torch.float64)
    _b3, perm = _guarded((n, C), torch.int32, IPOISON)
    _b4, out = _guarded((C, T, F, 2))
    st = _lib.stream()
    fade = torch.ones(V, device='cuda')
    p = _lib.ptr
    calls = [
        (lib.danet_stitch_affinity, (st, T, L, V, C, F, p(r.mags), p(ws), need - 8), 'workspace too small'),
        (lib.danet_stitch_affinity, (st, T, L, V, 5, F, p(r.mags), p(ws), need), 'need 1 <= C'),
        (lib.danet_stitch_affinity, (st, L, L, V, C, F, p(r.mags), p(ws), need), 'need T > L'),
        (lib.danet_stitch_affinity, (st, T, L, V, C, F, None, p(ws), need), 'null'),
        (lib.danet_stitch_assign, (st, T, L, V, C, F, p(r.ws), need, p(S) + 4, p(perm)), 'misaligned'),
        (lib.danet_stitch_assign, (st, T, L, V, C, F, p(r.ws), need - 1, p(S), p(perm)), 'workspace too small'),
        (lib.danet_stitch_assign, (st, T, L, L, C, F, p(r.ws), need, p(S), p(perm)), 'need T >= 1'),
        (lib.danet_stitch_merge, (st, T, L, V, C, F, p(r.mags), p(r.phasor), None, p(r.perm), p(out)), 'null'),
        (lib.danet_stitch_merge, (st, T, L, V, C, F, p(r.mags), p(r.phasor), p(fade), p(r.perm), p(out) + 4), 'misaligned'),
        (lib.danet_stitch_merge, (st, T, L, V, C, 0, p(r.mags), p(r.phasor), p(fade), p(r.perm), p(out)), 'need 1 <= C'),
    ]
    for fn, args, msg in calls:
        assert fn(*args) == -1, msg
        assert msg in lib.danet_stitch_last_error().decode(), (msg, lib.danet_stitch_last_error())
        with pytest.raises(_lib.DanetHipError):
            _lib.stitch_check(-1)
    torch.cuda.synchronize()
    for t, poison in ((ws, POISON), (S, POISON), (perm, IPOISON), (out, POISON)):
        assert bool((t == poison).all())                              # nothing was launched


# --------------------------------------------------------------------------------------- model
MODEL = dict(BATCH_SIZE=1, LSTM_HDIM=8, INFER_CHUNK_LEN=16, INFER_CHUNK_OVERLAP=4, INFER_CHUNK_BATCH=3)


def _mixture(hp, T, seed=0):
    rng = np.random.RandomState(seed)
    F = hp.FEATURE_SIZE
    return torch.from_numpy(((rng.randn(1, T, F) + 1j * rng.randn(1, T, F)) * 4).astype(np.complex64)).cuda()


def test_infer_long_is_the_restatement_applied_to_infer_chunks(hp):
    from danet_amd import ops
    model = small_model(hp, **MODEL)
    assert model.infer_chunk == (16, 4, 3)
    T, (L, V, _G) = 50, model.infer_chunk
    x = _mixture(hp, T)
    starts = ops.stitch_plan(T, L, V)
    assert starts == SR.plan(T, L, V) and len(starts) == 4              # groups of 3 and 1
    out = model.infer(x)
    assert tuple(out.shape) == (1, hp.MAX_N_SIGNAL, T, hp.FEATURE_SIZE) and out.dtype == torch.complex64
    assert np.array_equal(_bits(out), _bits(model.infer_long(x)))
    chunks = torch.stack([x[0, s:s + L] for s in starts])
    mags, phasor = model.infer_chunks(chunks)
    assert hp.BATCH_SIZE == 1
    assert np.array_equal(_bits(ops.stitch(mags, phasor, T, V)), _bits(out[0]))
    # the front end is pointwise: every chunk that covers a frame holds the same phasor bits for it
    whole = ops.frontend(x[:, None].contiguous())['phasor'][0]
    for i, s in enumerate(starts):
        assert np.array_equal(_bits(phasor[i]), _bits(whole[s:s + L])), i
    m, ph = mags.cpu().numpy(), phasor.cpu().numpy()
    S, perm = ops.stitch_assign(ops.stitch_affinity(mags, T, V), T, L, V, m.shape[1], m.shape[3])
    exact, absum = SR.affinity_exact(m, T, V)
    assert (np.abs(S.cpu().numpy() - exact) <= 1e-12 * absum).all()
    ref = SR.affinity(m, T, V)
    assert min(SR.margin(Si) for Si in ref) > 1e-9
    want = SR.chain(ref)
    assert np.array_equal(perm.cpu().numpy(), want)
    check_merge(out[0].cpu().numpy(), m, ph, want, T, V)
    check_lstm_status()


def test_mask_sum_of_the_softmax_separator_survives_the_cross_fade(hp):
    '''sum_c out[c] against the mixture: the chunked route may deviate twice as far as key-null infer does on one
    chunk (the cross-fade adds two roundings)'''
    model = small_model(hp, **MODEL)
    T, L = 50, 16
    x = _mixture(hp, T, seed=1)
    scale = float(x.abs().max())
    long_dev = float((model.infer(x)[0].sum(0) - x[0]).abs().max()) / scale
    model.infer_chunk = None                                            # the key-null route of the same model
    one_dev = float((model.infer(x[:, :L])[0].sum(0) - x[0, :L]).abs().max()) / scale
    print('mask-sum deviation: chunked %.3e, key-null infer on one chunk %.3e' % (long_dev, one_dev))
    assert long_dev <= 2 * one_dev
    check_lstm_status()


def test_a_batch_of_two_with_the_key_set_raises_the_named_error(hp):
    model = small_model(hp, **MODEL)
    x = _mixture(hp, 50)
    with pytest.raises(ValueError) as e:
        model.infer(torch.cat([x, x]))
    assert 'INFER_CHUNK_LEN' in str(e.value)


def test_short_input_and_key_null_are_todays_infer_and_never_map_the_library():
    '''a fresh process: key null -> infer is the literal front-end / encoder / estimator / separator / re-attach chain
    bit for bit; key set and T <= L -> the same bits as key null; libdanet_stitch is never mapped'''
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops\n"
        "from danet_amd.hparams import hparams as hp\n"
        "from gpu_helpers import small_model\n"
        "bits = lambda t: torch.view_as_real(t).cpu().numpy().view(np.uint32)\n"
        "rng = np.random.RandomState(0)\n"
        "null = small_model(hp, BATCH_SIZE=1, LSTM_HDIM=8)\n"
        "F = hp.FEATURE_SIZE\n"
        "x = torch.from_numpy(((rng.randn(1, 50, F) + 1j * rng.randn(1, 50, F)) * 4).astype(np.complex64)).cuda()\n"
        "a = null.infer(x)\n"
        "with torch.no_grad():\n"
        "    fe = ops.frontend(x[:, None].contiguous())\n"
        "    emb = null.encoder(fe['mix_log'])\n"
        "    attr = null.valid_estimator(emb, s_mix_pwr=fe['mix_pwr'])\n"
        "    b = ops.reattach_phase(null.separator(fe['mix_pwr'], attr, emb.reshape(1, -1, hp.EMBED_SIZE)), fe['phasor'])\n"
        "print('NULL:', null.infer_chunk is None and np.array_equal(bits(a), bits(b)))\n"
        "short = null.infer(x[:, :16])\n"
        "hp.reset()\n"
        "keyed = small_model(hp, BATCH_SIZE=1, LSTM_HDIM=8, INFER_CHUNK_LEN=16, INFER_CHUNK_OVERLAP=4)\n"
        "print('SHORT:', keyed.infer_chunk == (16, 4, 16) and np.array_equal(bits(keyed.infer(x[:, :16])), bits(short))\n"
        "      and np.array_equal(bits(keyed.infer(x[:, :12])), bits(null.infer(x[:, :12]))))\n"
        "torch.cuda.synchronize()\n"
        "print('STATUS:', ops.lstm_status_ok())\n"
        "print('UNMAPPED:', _lib._stitch is None and 'libdanet_stitch' not in open('/proc/self/maps').read()\n"
        "      and 'libdanet_hip' in open('/proc/self/maps').read())\n"
    ) % (ROOT, os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('NULL: True', 'SHORT: True', 'STATUS: True', 'UNMAPPED: True'):
        assert words in out.stdout, out.stdout + out.stderr


def test_demo_mode_separates_a_four_second_wav_in_chunks(hp, tmp_path, monkeypatch):
    import scipy.io.wavfile
    from danet_amd import cli, datasets, utils
    monkeypatch.chdir(tmp_path)
    cfg = dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
               NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
               INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig', DATASET_TYPE='synth',
               INFER_CHUNK_LEN=512, INFER_CHUNK_OVERLAP=128, INFER_CHUNK_BATCH=4)
    (tmp_path / 'cfg.json').write_text(json.dumps(cfg))
    wave = (datasets.speech_shaped_wave(np.random.RandomState(2), 32000, 8000)).astype(np.int16)
    scipy.io.wavfile.write('mix.wav', 8000, wave)
    out = io.StringIO()
    model = cli.main(['-n', 'chunked', '-m', 'demo', '-if', 'mix.wav', '-c', 'cfg.json'], out=out)
    assert model.infer_chunk == (512, 128, 4) and hp.BATCH_SIZE == 1
    feat = utils.load_wavfile('mix.wav')
    T = feat.shape[0]
    assert T == 1 + -(-32000 // 16) and SR.chunks(T, 512, 128) == 5
    sep = model.infer(torch.as_tensor(feat.astype(np.complex64)).to(model.device)[None])[0].cpu().numpy()
    model.check_status()
    for i in (1, 2):
        sr, y = scipy.io.wavfile.read('mix_separated_%d.wav' % i)
        assert sr == 8000 and len(y) == T * 16 and np.isfinite(y).all() and np.abs(y).max() > 0
        utils.save_wavfile('direct_%d.wav' % i, sep[i - 1])
        assert open('direct_%d.wav' % i, 'rb').read() == open('mix_separated_%d.wav' % i, 'rb').read()
    check_lstm_status()
