'''
GPU tests of the reverberation of the wavdir dataset (run with -m gpu): danet_reverb_apply against the float64
restatement tests/reverb_ref.py on every written sample, its exactness and bounds guarantees, the dataset end to
end on both routes, and the command line.

BAR of the kernel, per output sample: |y - y64| <= 1.01 * K * 2^-24 * conv(|h|, |x|)[n] + 2^-126, the standard
bound of a K-term float32 dot product in any order, with or without fused multiply-adds, over identical float32
inputs (gamma_K = K u / (1 - K u) <= 1.01 K u for K <= 8192, u = 2^-24).  It is derived, not measured; the
sequential float32 numpy sum is held to it on the CPU (tests/test_reverb_cpu.py).
'''
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import mix_ref as M
import prep_ref as P
import reverb_ref as RR
import speed_ref as SR
from gpu_helpers import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 2, 3, 5, 255, 256, 257, 1023, 1025, 4099]
POISON = 0x7fc00abc          # a NaN no computation produces
RATE = 16000


def _bank(K):
    '''the rule's bank with K taps: R chosen so that 4 * ceil(R * RATE / 4) = K'''
    b = RR.bank((K - 2) / float(RATE), RATE)
    assert b.shape == (32, K)
    return b


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _desc(rows):
    from danet_amd import ops
    d = np.zeros(len(rows), ops.REVERB_DESC_DTYPE)
    for u, r in enumerate(rows):
        d[u] = (r['so'], r['L'], r['do'], r.get('ob', 0), r.get('oc', r['L']), r['row'], 0)
    return d


def _launch(pool, rows, bank, out):
    '''one launch through the Python layer (host-validated descriptors)'''
    from danet_amd import ops
    ops.reverb_apply(pool, _desc(rows), bank, bank.shape[1], out)
    torch.cuda.synchronize()


def _poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int32, device='cuda').view(torch.float32)


def _layout(specs, seed):
    '''rows (L, row) laid out in one pool at source offsets of every residue mod 4 and destination spans of every
    residue mod 4, apart by bands of 5 .. 7 floats -> (rows, pool, out_len)'''
    rng = np.random.RandomState(seed)
    rows, so, do = [], 0, 9
    for u, (L, row) in enumerate(specs):
        so += (u % 4 - so) % 4 + 4 * int(rng.randint(0, 3))
        do += ((u // 4 + u) % 4 - do) % 4
        rows.append(dict(L=L, row=row, so=so, do=do))
        so += L
        do += L + 5 + u % 3
    pool = np.clip(rng.standard_normal(so + 11) * 4000, -32768, 32767).astype(np.int16).astype(np.float32)
    return rows, pool, do + 9


def _refs(rows, pool, bank):
    return [RR.apply(pool[r['so']:r['so'] + r['L']], bank[r['row']]) for r in rows]


def _check_rows(out_bits, rows, refs, K):
    '''every written sample of every row against float64 -> worst error / bar'''
    worst = 0.0
    for r, (y64, S) in zip(rows, refs):
        ob, oc = r.get('ob', 0), r.get('oc', r['L'])
        y = out_bits[r['do'] + ob:r['do'] + ob + oc].view(np.float32).astype(np.float64)
        if oc:
            ratio = float((np.abs(y - y64[ob:ob + oc]) / RR.bound(S[ob:ob + oc], K)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (r, ratio)
    return worst


def _bands_untouched(out_bits, rows):
    written = np.zeros(len(out_bits), bool)
    for r in rows:
        lo = r['do'] + r.get('ob', 0)
        hi = lo + r.get('oc', r['L'])
        assert not written[lo:hi].any()
        written[lo:hi] = True
    assert (out_bits[~written] == POISON).all()
    assert not (out_bits[written] == POISON).any()                # every float of every span is written


# ------------------------------------------------------------------------------- kernel vs float64
@pytest.mark.parametrize('K', [4, 8, 36, 260, 4000])
def test_every_length_at_every_offset_residue_against_float64(K):
    bank = _bank(K)
    specs = [(L, (3 * i + 7 * q) % 32) for i, L in enumerate(LENGTHS) for q in range(4)]
    specs += [(L, 0) for L in (5, 257, 4099)]                      # the dry row
    rows, pool, n_out = _layout(specs, seed=K)
    assert {r['so'] % 4 for r in rows} == {r['do'] % 4 for r in rows} == {0, 1, 2, 3}
    refs = _refs(rows, pool, bank)
    a, b = _poisoned(n_out), _poisoned(n_out)
    _launch(cu(pool), rows, cu(bank), a)
    _launch(cu(pool), rows, cu(bank), b)
    got = _bits(a)
    worst = _check_rows(got, rows, refs, K)
    print('K %d, %d rows: worst error / bar %.3f' % (K, len(rows), worst))
    _bands_untouched(got, rows)
    assert np.array_equal(got, _bits(b))                           # two launches: identical bits
    for r in rows:                                                 # row 0: the input as values
        if r['row'] == 0:
            assert np.array_equal(got[r['do']:r['do'] + r['L']].view(np.float32), pool[r['so']:r['so'] + r['L']])


def test_8192_taps_in_a_seven_row_launch():
    K = 8192
    bank = _bank(K)
    rows, pool, n_out = _layout([(5, 31), (4099, 17), (5, 0), (4099, 31), (1, 9), (257, 1), (1025, 30)], seed=5)
    refs = _refs(rows, pool, bank)
    out = _poisoned(n_out)
    _launch(cu(pool), rows, cu(bank), out)
    print('K 8192: worst error / bar %.3f' % _check_rows(_bits(out), rows, refs, K))
    _bands_untouched(_bits(out), rows)


@pytest.fixture(scope='module')
def many():
    '''130 rows at K = 260 with mixed bank rows in ONE launch into a poisoned buffer, and their float64 reference'''
    K = 260
    rng = np.random.RandomState(1)
    bank = _bank(K)
    specs = [(L, int(rng.randint(0, 32))) for L in LENGTHS * 4]
    specs += [(int(rng.randint(1, 3000)), int(rng.randint(0, 32))) for _ in range(130 - len(specs))]
    rows, pool, n_out = _layout(specs, seed=2)
    out = _poisoned(n_out)
    dev = dict(pool=cu(pool), bank=cu(bank))
    _launch(dev['pool'], rows, dev['bank'], out)
    return dict(K=K, bank=bank, rows=rows, pool=pool, n_out=n_out, refs=_refs(rows, pool, bank), a=_bits(out), dev=dev)


def test_130_rows_in_one_launch_against_float64(many):
    worst = _check_rows(many['a'], many['rows'], many['refs'], many['K'])
    print('130 rows, %d samples: worst error / bar %.3f' % (sum(r['L'] for r in many['rows']), worst))
    _bands_untouched(many['a'], many['rows'])


@pytest.mark.parametrize('n_utt', [1, 7])
def test_rows_alone_and_by_sevens_equal_the_130_row_launch(many, n_utt):
    '''a row's values do not depend on n_utt or on its neighbours'''
    rows = many['rows']
    out = _poisoned(many['n_out'])
    for k in range(0, len(rows), n_utt):
        _launch(many['dev']['pool'], rows[k:k + n_utt], many['dev']['bank'], out)
    assert np.array_equal(_bits(out), many['a'])


def test_a_span_launch_is_the_slice_of_the_whole_launch(many):
    '''out_begin in {0, 1, 3, L - 1} x out_count in {0, 1, L} (cut to the utterance), over all 130 rows: the bits of
    the whole-utterance launch inside the span, poison outside it'''
    n = 0
    for b_kind in range(4):
        for c_kind in range(3):
            rows = []
            for r in many['rows']:
                L = r['L']
                ob = min([0, 1, 3, L - 1][b_kind], L - 1)
                oc = min([0, 1, L][c_kind], L - ob)
                rows.append(dict(r, ob=ob, oc=oc))
            out = _poisoned(many['n_out'])
            _launch(many['dev']['pool'], rows, many['dev']['bank'], out)
            got = _bits(out)
            _bands_untouched(got, rows)
            for r in rows:
                lo, hi = r['do'] + r['ob'], r['do'] + r['ob'] + r['oc']
                assert np.array_equal(got[lo:hi], many['a'][lo:hi]), r
                n += r['oc']
    assert n > 0
    # a span across tile boundaries of a long row, at K = 4000
    bank = _bank(4000)
    rng = np.random.RandomState(8)
    x = (rng.standard_normal(4099) * 3000).astype(np.int16).astype(np.float32)
    whole, part = _poisoned(4200), _poisoned(4200)
    _launch(cu(x), [dict(so=0, L=4099, do=50, row=29)], cu(bank), whole)
    _launch(cu(x), [dict(so=0, L=4099, do=50, row=29, ob=1000, oc=2100)], cu(bank), part)
    a, b = _bits(whole), _bits(part)
    assert np.array_equal(a[1050:3150], b[1050:3150]) and (b[:1050] == POISON).all() and (b[3150:] == POISON).all()


def test_host_visible_errors_launch_nothing(many):
    from danet_amd import _lib, ops
    pool, bank, out = many['dev']['pool'], many['dev']['bank'], _poisoned(4096)
    r = dict(so=0, L=100, do=0, row=3)
    for bad, msg in ((dict(r, row=32), 'row = 32'), (dict(r, so=len(many['pool']) - 50), 'outside the pool'),
                     (dict(r, do=4000), 'inside the buffer'), (dict(r, ob=50, oc=51), 'outside its')):
        with pytest.raises(ValueError, match=msg):
            ops.reverb_apply(pool, _desc([bad]), bank, 260, out)
    d = cu(_desc([r]).view(np.uint8), torch.uint8)
    lib = _lib.load_reverb()
    args = [_lib.stream(), 1, pool.data_ptr(), pool.numel(), d.data_ptr(), bank.data_ptr(), 260, out.data_ptr(),
            out.numel()]
    for at, value in ((1, 0), (5, bank.data_ptr() + 4), (6, 262), (6, 0), (6, 8196), (4, d.data_ptr() + 4)):
        bad = list(args)
        bad[at] = value
        assert lib.danet_reverb_apply(*bad) == -1, (at, value)
    torch.cuda.synchronize()
    assert (_bits(out) == POISON).all()


def test_what_only_the_device_sees_is_clamped():
    '''descriptor rows straight into device memory, unvalidated: the pool lies between two bands of 1e30 (a sample
    read from outside would wreck the sum), the destination between two poisoned bands; the output is the
    restatement of the clamped row'''
    from danet_amd import ops
    rng = np.random.RandomState(7)
    K = 260
    bank = _bank(K)
    n_src, n_dst, guard = 5003, 9000, 1021
    big = np.full(guard + n_src + guard, 1e30, np.float32)
    big[guard:guard + n_src] = np.clip(rng.standard_normal(n_src) * 3000, -32768, 32767).astype(np.int16)
    src_all, dst_all = cu(big), _poisoned(guard + n_dst + guard)
    pool, dst = src_all[guard:guard + n_src], dst_all[guard:guard + n_dst]
    host = big[guard:guard + n_src]
    i64 = np.iinfo(np.int64)
    #        src_offset   src_length dst_offset  out_begin out_count row
    cases = [(n_src - 100, 1000,      100,        0,        250,      3),        # the source leaves the pool
             (-50,         200,       400,        0,        200,      5),        # ... in front
             (-50,         50,        650,        0,        50,       5),        # ... entirely: zeros
             (10,          -5,        720,        0,        40,       5),        # negative length: nothing
             (n_src + 7,   300,       800,        0,        300,      31),       # behind the pool: zeros
             (i64.min,     100,       1150,       0,        100,      31),
             (i64.max,     100,       1300,       0,        100,      31),
             (100,         2000,      -30,        0,        100,      7),        # the destination leaves the buffer
             (100,         2000,      n_dst - 60, 0,        500,      7),
             (100,         2000,      n_dst + 5,  0,        500,      7),
             (100,         2000,      i64.min,    0,        i64.max,  7),
             (100,         300,       1500,       -20,      100,      9),        # the span leaves the utterance
             (100,         300,       1700,       250,      500,      9),
             (100,         300,       2100,       400,      50,       9),
             (100,         300,       2100,       i64.min,  i64.max,  9),
             (100,         300,       2100,       10,       -7,       9),
             (100,         300,       2100,       i64.max,  i64.max,  9),
             (3000,        1500,      2500,       0,        1500,     -4),       # row out of range
             (3000,        1500,      4100,       0,        1500,     99999),
             (0,           2600,      5700,       0,        i64.max,  30)]
    d = np.zeros(len(cases), ops.REVERB_DESC_DTYPE)
    for u, c in enumerate(cases):
        d[u] = c + (0,)
    dev = cu(d.view(np.uint8), torch.uint8)
    ops.reverb_apply(pool, dev, cu(bank), K, dst)                 # a device table is the caller's word: no host check
    torch.cuda.synchronize()
    got = _bits(dst_all)
    assert (got[:guard] == POISON).all() and (got[guard + n_dst:] == POISON).all()
    body = got[guard:guard + n_dst]
    written = np.zeros(n_dst, bool)
    n_checked = 0
    for c in cases:
        x, lo, hi, row = RR.clamp_row(host, n_dst, *c)
        if hi <= lo:
            continue
        y64, S = RR.apply(x, bank[row])
        y = body[c[2] + lo:c[2] + hi].view(np.float32).astype(np.float64)
        assert np.isfinite(y).all() and np.abs(y).max() < 1e6, c
        assert (np.abs(y - y64[lo:hi]) <= RR.bound(S[lo:hi], K)).all(), c
        assert not written[c[2] + lo:c[2] + hi].any()
        written[c[2] + lo:c[2] + hi] = True
        n_checked += 1
    assert n_checked == 13
    assert (body[~written] == POISON).all()


# ------------------------------------------------------------------------- dataset end to end
def _config(hp, root, **kw):
    base = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(root), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
                BATCH_SIZE=4, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=48)
    base.update(kw)
    hp.reset()
    hp.load(base)
    hp.digest()


def _window(n):
    import scipy.signal.windows
    return np.sqrt(scipy.signal.windows.hann(n)).astype(np.float32)


def _dataset(hp, root, **kw):
    from danet_amd import datasets
    _config(hp, root, **kw)
    ds = datasets.WavDirData()
    ds.install_and_load()
    return ds


def _device_epochs(ds, subset, bs, n_epochs, crop_len, shuffle=True):
    return [b.cpu().numpy().copy() for _ in range(n_epochs)
            for b in ds.epoch_device(subset, bs, shuffle=shuffle, device='cuda', crop_len=crop_len)]


def _host_epochs(ds, subset, bs, n_epochs, crop_len, shuffle=True):
    from danet_amd import feed
    return [np.ascontiguousarray(feed.to_batch_host(pt, crop_len)) for _ in range(n_epochs)
            for pt in ds.epoch(subset, bs, shuffle=shuffle)]


def _restated_epochs(ds, bs, n_epochs, crop_len, R, P_range, gains_of):
    '''the train batches by their definition: the draws of tests/speed_ref.py and tests/reverb_ref.py,
    (ops.speed_resample,) ops.reverb_apply of WHOLE utterances over the restated descriptors into a scratch laid out
    as the dataset documents it, ops.stft_batch of that scratch, times the restated gains'''
    from danet_amd import ops
    lengths, offsets = ds.lengths['train'], ds.offsets['train']
    pool, window = cu(ds.pool_host['train']), cu(_window(256))
    bank = RR.bank(R, 8000)
    K = bank.shape[1]
    bank = cu(bank)
    if P_range is None:
        stride = (int(lengths.max()) + 3) // 4 * 4
    else:
        tab = cu(SR.table(P_range))
        stride = (SR.out_len(int(lengths.max()), 512 - int(np.floor(512 * P_range))) + 3) // 4 * 4
        speed_rng = SR.stream(0, 'train')
    rng = RR.stream(0, 'train')
    out, rows_seen = [], []
    for _ in range(n_epochs):
        for idx in P.index_plan(len(lengths), bs, True):
            src, so, L = pool, offsets[idx], lengths[idx]
            spots = np.arange(bs, dtype=np.int64) * stride
            if P_range is not None:
                p, L = SR.draw(lengths[idx], speed_rng, P_range, 256)
                src = torch.zeros(bs * stride, dtype=torch.float32, device='cuda')
                ops.speed_resample(pool, ops.speed_desc(so, lengths[idx], spots, L, p, pool.numel(), src.numel()), tab, src)
                so = spots
            frames = [P.num_frames(int(l), 256, 64) for l in L]
            T_max, pads = P.draw_pads(frames)
            beg, cnt = P.draw_crop(T_max, crop_len)
            rows = RR.draw(bs, rng)
            wet = torch.zeros(bs * stride, dtype=torch.float32, device='cuda')
            ops.reverb_apply(src, ops.reverb_desc(so, L, spots, np.zeros(bs, np.int64), L, rows, src.numel(),
                                                  wet.numel()), bank, K, wet)
            desc = ops.prep_desc(spots, L, pads, T_max, wet.numel(), 256, 64)
            X = ops.stft_batch(wet, desc, T_max, window, 256, 64, t_begin=beg, t_count=cnt).cpu().numpy()
            g = gains_of(idx)
            if g is not None:
                X = (g[:, None, None, None] * X.view(np.float32).reshape(X.shape + (2,))).view(np.complex64)[..., 0]
            out.append(X)
            rows_seen.append(rows)
            # the span the device route asks for is the restated one
            for u in range(bs):
                f, c = ds.reverb_span([L[u]], [pads[u]], beg, cnt, 256, 64)
                assert (int(f[0]), int(c[0])) == RR.span(int(L[u]), pads[u], beg, cnt, 256, 64)
    return out, rows_seen


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('reverb') / 'tree'
    SR.write_tree(root, seed=4, n_per_subset=14)
    return root


@pytest.mark.parametrize('speed', [False, True])
@pytest.mark.parametrize('mix', [False, True])
def test_dataset_equals_the_restated_reverberation_on_both_routes(hp, tree, mix, speed):
    R = 0.05
    keys = dict(REVERB_RT60_MAX=R)
    if mix:
        keys.update(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0)
    if speed:
        keys.update(SPEED_PERTURB_RANGE=0.1)
    ds = _dataset(hp, tree, **keys)
    bs, C = hp.BATCH_SIZE * hp.MAX_N_SIGNAL, hp.MAX_N_SIGNAL
    random.seed(21)
    np.random.seed(22)
    dev = _device_epochs(ds, 'train', bs, 2, hp.MAX_TRAIN_LEN)
    assert ds._ring['cuda:0']['row'] == 24 + (40 if speed else 0) + 48 + (4 if mix else 0)
    ring = ds._reverb_scratch[('train', 'cuda:0')]
    assert len(ring['bufs']) == ds.DESC_DEPTH and ring['stride'] % 4 == 0
    assert ring['stride'] == (ds.speed_stride('train') if speed else (int(ds.lengths['train'].max()) + 3) // 4 * 4)
    assert (('train', 'cuda:0') in ds._speed_scratch) == speed
    # the device route asked for spans only: somewhere the NaN of the allocation is still there
    assert any(bool(torch.isnan(b).any()) for b in ring['bufs'])

    mix_rng = M.stream(0, 'train')
    random.seed(21)
    np.random.seed(22)
    want, rows_seen = _restated_epochs(ds, bs, 2, hp.MAX_TRAIN_LEN, R, 0.1 if speed else None,
                                       (lambda idx: M.gains(ds.power['train'][idx], mix_rng, C, 5.0, 3.0)) if mix
                                       else (lambda idx: None))
    assert len(dev) == len(want) == 4
    for a, b in zip(dev, want):
        assert a.shape[:2] == (hp.BATCH_SIZE, C) and np.isfinite(a.view(np.float32)).all()
        assert np.array_equal(P.bits(a).reshape(-1), P.bits(b).reshape(-1))
    assert len({int(k) for rows in rows_seen for k in rows}) > 8

    # epoch() gives the same batches: a fresh dataset, so that its streams start where the first one's did
    ds2 = _dataset(hp, tree, **keys)
    random.seed(21)
    np.random.seed(22)
    host = _host_epochs(ds2, 'train', bs, 2, hp.MAX_TRAIN_LEN)
    assert len(host) == len(dev)
    for a, b in zip(dev, host):
        assert a.shape == b.shape and np.array_equal(P.bits(a), P.bits(b))


def test_key_null_gives_the_batches_of_before_and_range_zero_the_same_values(hp, tree):
    bs = 8
    got = {}
    for key in ('absent', None, 0):
        keys = {} if key == 'absent' else dict(REVERB_RT60_MAX=key)
        ds = _dataset(hp, tree, **keys)
        random.seed(21)
        np.random.seed(22)
        got[key] = _device_epochs(ds, 'train', bs, 2, 48)
        if key != 0:
            assert ds._reverb_scratch == {} and ds._reverb_bank == {} and ds._reverb_rng == {}
            assert ds._ring['cuda:0']['row'] == 24
    for a, b, c in zip(got['absent'], got[None], got[0]):
        assert np.abs(a).max() > 0 and np.array_equal(P.bits(a), P.bits(b))
        assert np.array_equal(a, c)                                # R = 0: every row dry, the input as values


def test_valid_and_test_are_the_batches_of_key_null_and_launch_nothing(hp, tree):
    got = {}
    for key in (None, 0.05):
        ds = _dataset(hp, tree, REVERB_RT60_MAX=key)
        for subset in ('valid', 'test'):
            random.seed(4)
            got[key, subset] = _device_epochs(ds, subset, 8, 1, None, shuffle=False)
            random.seed(4)
            got[key, subset, 'host'] = _host_epochs(ds, subset, 8, 1, None, shuffle=False)
        assert ds._reverb_scratch == {} and ds._reverb_bank == {} and ds._reverb_rng == {}
    for subset in ('valid', 'test'):
        assert len(got[None, subset]) == 2
        for a, b, c in zip(got[None, subset], got[0.05, subset], got[0.05, subset, 'host']):
            assert np.array_equal(P.bits(a), P.bits(b)) and np.array_equal(P.bits(a), P.bits(c))
    cfg = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(tree), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
               BATCH_SIZE=4, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=48)
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, datasets\n"
        "from danet_amd.hparams import hparams\n"
        "cfg = json.loads(%r)\n"
        "cfg['REVERB_RT60_MAX'] = json.loads(sys.argv[1])\n"
        "hparams.load(cfg); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.install_and_load()\n"
        "subsets = ('valid', 'test') if cfg['REVERB_RT60_MAX'] is not None else ('train', 'valid', 'test')\n"
        "n = sum(1 for s in subsets for b in ds.epoch_device(s, 8, False, 'cuda', None))\n"
        "n += sum(1 for s in subsets for b in ds.epoch(s, 8))\n"
        "maps = open('/proc/self/maps').read()\n"
        "print('BATCHES:', n, 'UNMAPPED:', _lib._reverb is None and 'libdanet_reverb_hip' not in maps and "
        "'libdanet_prep_hip' in maps)\n"
    ) % (ROOT, json.dumps(cfg))
    for key, n in (('0.05', 8), ('null', 12)):                     # set: valid / test only; null: train too
        out = subprocess.run([sys.executable, '-c', code, key], capture_output=True, text=True, timeout=600)
        assert 'BATCHES: %d UNMAPPED: True' % n in out.stdout, out.stdout + out.stderr[-3000:]


# ----------------------------------------------------------------------------------------- CLI
def test_command_line_trains_with_the_key_set(tmp_path):
    SR.write_tree(tmp_path / 'tree', seed=8, n_per_subset=16, seconds=(0.2, 0.5))
    cfg = tmp_path / 'cfg.json'
    cfg.write_text(json.dumps(dict(
        BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
        NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor', INFER_ESTIMATOR_METHOD='anchor',
        SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64, DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'),
        REVERB_RT60_MAX=0.2)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'rv', '-m', 'train', '-ds', 'wavdir',
                          '-c', str(cfg), '-ne', '1', '-bs', '4'], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'wavdir train: 16 files' in out.stdout and 'Epoch 1/1' in out.stdout
    assert np.isfinite(float(out.stdout.split('Epoch 1/1 loss=')[1].split()[0]))
