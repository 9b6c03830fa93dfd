'''
GPU tests of the active speech level of the wavdir dataset (MIX_LEVEL_MEASURE = "active"): danet_level_activity
against the float64 restatement tests/level_ref.py -- counts EXACTLY equal, after the restatement itself has shown
that no q[n] of any case comes within 1e-9 relative of a threshold (include/danet_level_hip.h: the kernel's q lies
within 2^-34 of the exact recurrence) -- its robustness, and the dataset end to end on generated WAVs.
'''
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import level_ref as LR
import mix_ref as M
import noise_ref as NR
import prep_ref as P
from gpu_helpers import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024           # asserted against ops.LEVEL_TILE below: the lengths are built around it
N_ROWS = 130
# (sampling rate the input is drawn at, g, I): the rule at 8 kHz; at 48 kHz -- g nearest the bound, a hangover
# of more than nine tiles; no hangover; a hangover of 5 samples
CASES = {
    'fs8000': (8000, LR.params(8000)[0], 1600),
    'fs48000': (48000, LR.params(48000)[0], 9600),
    'hang0': (8000, LR.params(8000)[0], 0),
    'hang5': (8000, LR.params(8000)[0], 5),
}
SEEDS = {'fs8000': 1, 'fs48000': 2, 'hang0': 3, 'hang5': 4}      # picked on the CPU: the margin below holds
_cache = {}


def _lengths(I):
    return [1, 2, 255, 256, 257, I, I + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 3, 70001]


def _case(name):
    '''the pool, the tables and the restated counts of one (g, I) case, computed once: row r has the length
    _lengths(I)[r % 12] and sits at an offset congruent to r modulo 4'''
    if name not in _cache:
        fs, g, I = CASES[name]
        rng = np.random.RandomState(SEEDS[name])
        lens = np.asarray([_lengths(I)[r % 12] for r in range(N_ROWS)], dtype=np.int64)
        offs, at = [], 0
        for r, L in enumerate(lens):
            at += (r - at) % 4
            offs.append(at)
            at += int(L)
        pool = rng.randn(at + 5).astype(np.float32) * 1e6       # what lies between the rows is loud
        thr, cnt, margin = np.ones((N_ROWS, 16)), np.zeros((N_ROWS, 16), np.int64), np.inf
        for r, (o, L) in enumerate(zip(offs, lens)):
            if L == 0:
                continue
            x = LR.gated_noise(rng, int(L), fs, rms=float(10.0 ** rng.uniform(1, 4)))
            pool[o:o + L] = x
            thr[r] = LR.thresholds(LR.sum_squares(x) / L)
            q = LR.envelope(x, g)
            cnt[r] = LR.counts(q, thr[r], I)
            margin = min(margin, LR.min_margin(q, thr[r]))
        _cache[name] = dict(pool=pool, offs=np.asarray(offs, np.int64), lens=lens, thr=thr, cnt=cnt, margin=margin,
                            g=g, I=I)
    return _cache[name]


def _run(case, rows):
    from danet_amd import ops
    c = _case(case)
    got = ops.level_activity(cu(c['pool']), c['offs'][rows], c['lens'][rows], c['thr'][rows], c['g'], c['I'])
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(c['lens'][rows]), 16) and got.is_cuda
    return got.cpu().numpy()


# ---------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize('case', sorted(CASES))
def test_counts_equal_the_restatement_exactly(case):
    from danet_amd import ops
    assert ops.LEVEL_TILE == TILE and ops.LEVEL_THRESHOLDS == 16
    c = _case(case)
    # the condition of exactness, from the restatement alone: no q[n] within 1e-9 relative of any threshold
    print('%s: smallest |q / c_j - 1| = %.3g' % (case, c['margin']))
    assert c['margin'] >= 1e-9, c['margin']
    assert sorted(set(int(o) % 4 for o in c['offs'])) == [0, 1, 2, 3]
    if c['I'] > 2 * TILE:
        assert c['I'] > 2 * ops.LEVEL_TILE                      # a hangover longer than two tiles
    all_rows = np.arange(N_ROWS)
    got = _run(case, all_rows)
    bad = np.nonzero((got != c['cnt']).any(axis=1))[0]
    assert not len(bad), (case, bad[:5], c['lens'][bad[:5]], got[bad[:1]], c['cnt'][bad[:1]])
    seven = np.arange(5, 12)
    assert sorted(set(int(o) % 4 for o in c['offs'][seven])) == [0, 1, 2, 3]
    assert np.array_equal(_run(case, seven), c['cnt'][seven])
    for r in (5, 8, 10, 11):                                    # launches of ONE row, one per offset residue
        assert np.array_equal(_run(case, np.asarray([r])), c['cnt'][[r]]), (case, r)
    # the grid is at work: thresholds that everything, something and nothing reaches
    long_rows = c['cnt'][c['lens'] == 70001]
    assert (long_rows[:, 0] > 60000).all() and (long_rows[:, 15] == 0).all()
    assert all(len(set(row.tolist())) >= 8 for row in long_rows)


def test_repeated_calls_agree_bit_for_bit_and_rows_do_not_depend_on_their_company():
    rows = np.arange(N_ROWS)
    a, b = _run('fs8000', rows), _run('fs8000', rows)
    assert np.array_equal(a, b)
    some = np.asarray([11, 3, 23, 10, 11])
    assert np.array_equal(_run('fs8000', some), a[some])


def test_guarded_counts_and_workspace_are_left_alone():
    from danet_amd import _lib
    lib = _lib.load_level()
    c = _case('fs8000')
    rows = np.arange(12)
    n, guard, poison = len(rows), 64, 0x7ff8dead0000beef
    max_len = 70001 + 5000                                      # rows shorter than max_len: tiles no row has
    tiles = -(-max_len // TILE)
    need = lib.danet_level_workspace_bytes(n, max_len)
    assert need == n * tiles * 208
    pool = cu(c['pool'])
    out_all = torch.full((guard + n * 16 + guard,), poison, dtype=torch.int64, device='cuda')
    ws_all = torch.full((guard + need // 8 + guard,), poison, dtype=torch.int64, device='cuda')
    assert ws_all.data_ptr() % 16 == 0
    o, l, t = cu(c['offs'][rows], torch.int64), cu(c['lens'][rows], torch.int64), cu(c['thr'][rows], torch.float64)

    def call(ws_bytes):
        return lib.danet_level_activity(_lib.stream(), n, pool.data_ptr(), pool.numel(), o.data_ptr(), l.data_ptr(),
                                        max_len, c['g'], c['I'], t.data_ptr(), out_all.data_ptr() + 8 * guard,
                                        ws_all.data_ptr() + 8 * guard, ws_bytes)
    assert call(need - 1) == -1 and b'workspace too small' in lib.danet_level_last_error()
    torch.cuda.synchronize()
    assert bool((out_all == poison).all()) and bool((ws_all == poison).all())      # refused: nothing launched
    assert call(need) == 0, lib.danet_level_last_error()
    torch.cuda.synchronize()
    out_h, ws_h = out_all.cpu().numpy(), ws_all.cpu().numpy()
    for arr, m in ((out_h, n * 16), (ws_h, need // 8)):
        assert (arr[:guard] == poison).all() and (arr[guard + m:] == poison).all()
    assert np.array_equal(out_h[guard:guard + n * 16].reshape(n, 16), c['cnt'][rows])
    # the tiles a row does not have are never written: states first, 16 bytes a tile, the records behind them
    state = ws_h[guard:guard + n * tiles * 2].reshape(n, tiles, 2)
    rec = ws_h[guard + n * tiles * 2:guard + need // 8].reshape(n, tiles, 24)
    for u, L in enumerate(c['lens'][rows]):
        used = -(-int(L) // TILE)
        assert not (state[u, :used] == poison).any() and (state[u, used:] == poison).all(), u
        assert not (rec[u, :used] == poison).any() and (rec[u, used:] == poison).all(), u


def test_rows_are_clamped_to_what_the_device_can_see():
    '''rows that leave the pool are cut to it: the pool sits between two bands of 1e30, a sample read from outside
    would lift the envelope over every threshold'''
    from danet_amd import ops
    rng = np.random.RandomState(7)
    n, guard, fs, max_len = 90003, 1021, 8000, 70000
    g, _k, I = LR.params(fs)
    big = np.full(guard + n + guard, 1e30, np.float32)
    big[guard:guard + n] = LR.gated_noise(rng, n, fs, rms=500.0)
    dev = cu(big)
    pool, host = dev[guard:guard + n], big[guard:guard + n]
    i64 = np.iinfo(np.int64)
    rows = [(n - 100, 1000, n - 100, 100),        # (offset, length) as given -> (offset, length) it is cut to
            (-50, 2000, 0, 1950),
            (-50, 50, 0, 0),
            (10, -5, 0, 0),
            (n + 7, 300, 0, 0),
            (0, n + 5, 0, max_len),               # longer than max_len: cut to max_len
            (3, 70001, 3, max_len),
            (i64.min, i64.max, 0, 0),
            (i64.max, i64.max, 0, 0),
            (-3, i64.max, 0, max_len),
            (1000, 66000, 1000, 66000)]
    thr, want, margin = np.ones((len(rows), 16)), np.zeros((len(rows), 16), np.int64), np.inf
    for u, (_o, _l, o, L) in enumerate(rows):
        if L:
            x = host[o:o + L]
            thr[u] = LR.thresholds(LR.sum_squares(x) / L)
            q = LR.envelope(x, g)
            want[u], margin = LR.counts(q, thr[u], I), min(margin, LR.min_margin(q, thr[u]))
    assert margin >= 1e-9, margin
    offs = torch.tensor([r[0] for r in rows], dtype=torch.int64, device='cuda')
    lens = torch.tensor([r[1] for r in rows], dtype=torch.int64, device='cuda')
    got = ops.level_activity(pool, offs, lens, cu(thr, torch.float64), g, I, max_len=max_len).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    with pytest.raises(ValueError, match='max_len'):
        ops.level_activity(pool, offs, lens, cu(thr, torch.float64), g, I)


def test_every_host_visible_argument_error_launches_nothing(monkeypatch):
    from danet_amd import _lib, ops
    pool = cu(np.ones(5000, np.float32))
    thr = np.ones((2, 16))
    ok = dict(offsets=[0, 100], lengths=[100, 4000], thresholds=thr, g=0.99, hang=1600)
    assert tuple(ops.level_activity(pool, **ok).shape) == (2, 16)

    def boom():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load_level', boom)
    monkeypatch.setattr(_lib, 'stream', boom)
    bad = [dict(g=0.0), dict(g=1.0), dict(g=-0.1), dict(g=1.5), dict(g=float('nan')), dict(hang=-1),
           dict(hang=(1 << 40) + 1), dict(offsets=[], lengths=[]), dict(offsets=[0], lengths=[1, 2]),
           dict(offsets=[0, 4990], lengths=[100, 20]), dict(offsets=[-1, 0]), dict(lengths=[100, -4]),
           dict(thresholds=np.ones((2, 15))), dict(thresholds=np.ones((3, 16))), dict(thresholds=np.ones(32)),
           dict(thresholds=cu(np.ones((2, 16)), torch.float32)), dict(max_len=(1 << 31) + 1), dict(max_len=-1)]
    for kw in bad:
        with pytest.raises(ValueError, match='level_activity'):
            ops.level_activity(pool, **dict(ok, **kw))
    with pytest.raises(ValueError, match='max_len'):
        ops.level_activity(pool, cu([0, 100], torch.int64), cu([100, 4000], torch.int64), thr, 0.99, 1600)


# ------------------------------------------------------------------------- dataset end to end
def _window(n):
    import scipy.signal.windows
    return np.sqrt(scipy.signal.windows.hann(n)).astype(np.float32)


def _write_tree(root, n=8, seed=3):
    '''two speakers in alternation, stored 30 dB apart: the quiet one talks throughout, the loud one pauses for
    60 % of every file'''
    import scipy.io.wavfile
    rng = np.random.RandomState(seed)
    for subset in ('train', 'test'):
        os.makedirs(os.path.join(str(root), subset), exist_ok=True)
        for i in range(n):
            L = int(rng.uniform(1.5, 2.2) * 8000)
            w = LR.gated_noise(rng, L, 8000, rms=60.0 if i % 2 == 0 else 60.0 * 10 ** 1.5,
                               duty=1.0 if i % 2 == 0 else 0.4)
            scipy.io.wavfile.write(os.path.join(str(root), subset, 'utt%03d.wav' % i), 8000,
                                   np.clip(np.rint(w), -32768, 32767).astype(np.int16))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('level') / 'tree'
    _write_tree(root)
    return root


def _config(hp, root, **kw):
    base = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(root), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
                BATCH_SIZE=2, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=48)
    base.update(kw)
    hp.reset()
    hp.load(base)
    hp.digest()


def _dataset(hp, root, **kw):
    from danet_amd import datasets
    _config(hp, root, **kw)
    ds = datasets.WavDirData()
    ds.install_and_load()
    return ds


def _restated_table(ds, subset):
    return np.asarray([LR.active_power(ds.pool_host[subset][o:o + n], 8000)
                       for o, n in zip(ds.offsets[subset], ds.lengths[subset])])


def _expected_epochs(ds, subset, bs, shuffle, crop_len, n_epochs, gains_of):
    '''the batches by their definition: ops.stft_batch of the plan (tests/prep_ref.py draws it), times the
    float32 gains `gains_of(idx)` gives (None: unscaled)'''
    from danet_amd import ops
    pool, window = cu(ds.pool_host[subset]), cu(_window(256))
    out = []
    for _ in range(n_epochs):
        for idx in P.index_plan(len(ds.lengths[subset]), bs, shuffle):
            T_max, pads = P.draw_pads([int(ds.frames[subset][i]) for i in idx])
            beg, cnt = P.draw_crop(T_max, crop_len)
            desc = ops.prep_desc(ds.offsets[subset][idx], ds.lengths[subset][idx], pads, T_max, pool.numel(), 256, 64)
            X = ops.stft_batch(pool, desc, T_max, window, 256, 64, t_begin=beg, t_count=cnt).cpu().numpy()
            g = gains_of(idx)
            if g is not None:
                assert g.dtype == np.float32
                X = (g[:, None, None, None] * X.view(np.float32).reshape(X.shape + (2,))).view(np.complex64)[..., 0]
            out.append(X)
    return out


def _seed():
    random.seed(21)
    np.random.seed(22)


def test_dataset_with_the_key_equals_the_plan_times_the_restated_gains(hp, tree):
    from danet_amd import feed
    ds = _dataset(hp, tree, MIX_SNR_RANGE=0.0, MIX_LEVEL_MEASURE='active')
    bs, C = hp.BATCH_SIZE * hp.MAX_N_SIGNAL, hp.MAX_N_SIGNAL
    _seed()
    dev = [b.cpu().numpy().copy() for _ in range(2)
           for b in ds.epoch_device('train', bs, shuffle=True, device='cuda', crop_len=hp.MAX_TRAIN_LEN)]
    assert 'libdanet_level_hip' in open('/proc/self/maps').read()
    ds.power_table('test', ds.upload_pool('test', ds._device('cuda')))
    table = {s: _restated_table(ds, s) for s in ('train', 'test')}
    for subset in ('train', 'test'):
        got = ds.power[subset]
        assert got.dtype == np.float64 and got.shape == (8,)
        assert np.all(np.abs(got - table[subset]) <= 1e-12 * table[subset]), (subset, got, table[subset])
        mean = np.asarray([M.mean_power(ds.pool_host[subset][o:o + n])
                           for o, n in zip(ds.offsets[subset], ds.lengths[subset])])
        ratio_db = 10.0 * np.log10(got / mean)
        assert np.all(ratio_db[0::2] < 0.1) and np.all(ratio_db[1::2] > 2.0), ratio_db      # only pauses count
        assert mean[1::2].min() / mean[0::2].max() > 100.0                                  # stored far apart

    rng = M.stream(0, 'train')
    _seed()
    want = _expected_epochs(ds, 'train', bs, True, hp.MAX_TRAIN_LEN, 2,
                            lambda idx: M.gains(table['train'][idx], rng, C, 0.0, None))
    assert len(dev) == len(want) == 2 * 2
    for a, b in zip(dev, want):
        assert a.shape == (hp.BATCH_SIZE, C) + b.shape[1:] and a.dtype == np.complex64
        assert np.array_equal(P.bits(a).reshape(-1), P.bits(b).reshape(-1))
    assert all(np.abs(x).max() > 0 for x in dev)

    # epoch(): a fresh dataset, so that its train stream starts where the first one's did
    ds2 = _dataset(hp, tree, MIX_SNR_RANGE=0.0, MIX_LEVEL_MEASURE='active')
    _seed()
    host = [np.ascontiguousarray(feed.to_batch_host(pt, hp.MAX_TRAIN_LEN)) for _ in range(2)
            for pt in ds2.epoch('train', bs, shuffle=True)]
    assert np.array_equal(ds2.power['train'].view(np.uint64), ds.power['train'].view(np.uint64))
    assert len(host) == len(dev)
    for a, b in zip(dev, host):
        assert a.shape == b.shape and np.array_equal(P.bits(a), P.bits(b))

    # the two sources of every mixture: equal restated active level after gain, the mean powers dBs apart
    groups = 0
    for idx, _T, _pads, _beg, _cnt, gains in ds.plan_epoch('train', bs, shuffle=False):
        g = gains.astype(np.float64).reshape(-1, C)
        level = 10.0 * np.log10(g * g * table['train'][idx].reshape(-1, C))
        assert np.all(np.abs(level[:, 0] - level[:, 1]) <= 1e-6), level
        groups += len(level)
    assert groups == 4

    # evaluation sweeps: the same mixtures every sweep, on both routes (valid is test's folder: test's table)
    for subset in ('valid', 'test'):
        sweeps = []
        for _ in range(2):
            random.seed(4)
            sweeps.append([b.cpu().numpy().copy() for b in ds.epoch_device(subset, bs, device='cuda')])
        rng = M.stream(0, subset)
        random.seed(4)
        want = _expected_epochs(ds, subset, bs, False, None, 1,
                                lambda idx: M.gains(table['test'][idx], rng, C, 0.0, None))
        random.seed(4)
        vh = [np.ascontiguousarray(feed.to_batch_host(pt, None)) for pt in ds.epoch(subset, bs)]
        assert len(sweeps[0]) == len(sweeps[1]) == len(want) == len(vh) == 2
        for a, b, c, d in zip(sweeps[0], sweeps[1], want, vh):
            assert np.array_equal(P.bits(a), P.bits(b)) and np.array_equal(P.bits(a).reshape(-1), P.bits(c).reshape(-1))
            assert np.array_equal(P.bits(a), P.bits(d))
    assert sorted(ds.power) == ['test', 'train']                    # the aliased valid shares test's table


def test_key_null_maps_no_library_and_yields_what_it_always_did(hp, tree, tmp_path):
    cfg = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(tree), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
               BATCH_SIZE=2, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=48, MIX_SNR_RANGE=3.0, MIX_LEVEL_MEASURE=None)
    code = (
        "import sys, json, random; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, datasets, feed\n"
        "from danet_amd.hparams import hparams\n"
        "hparams.load(json.loads(%r)); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.install_and_load()\n"
        "random.seed(31); np.random.seed(32)\n"
        "dev = [b.cpu().numpy().copy() for b in ds.epoch_device('train', 4, True, 'cuda', 48)]\n"
        "maps = open('/proc/self/maps').read()\n"
        "print('UNMAPPED:', _lib._level is None and 'libdanet_level' not in maps and 'libdanet_mix_hip' in maps)\n"
        "np.savez(%r, *dev)\n"
    ) % (ROOT, json.dumps(cfg), str(tmp_path / 'dev.npz'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert 'UNMAPPED: True' in out.stdout, out.stdout + out.stderr[-3000:]
    dev = np.load(str(tmp_path / 'dev.npz'))
    # a configuration from before the key existed: not in hparams at all
    ds = _dataset(hp, tree, MIX_SNR_RANGE=3.0)
    del hp.__dict__['MIX_LEVEL_MEASURE']
    ds = type(ds)()
    ds.install_and_load()
    assert not hasattr(hp, 'MIX_LEVEL_MEASURE') and ds.level_key is None
    random.seed(31)
    np.random.seed(32)
    unset = [b.cpu().numpy().copy() for b in ds.epoch_device('train', 4, True, 'cuda', 48)]
    mean = np.asarray([M.mean_power(ds.pool_host['train'][o:o + n])
                       for o, n in zip(ds.offsets['train'], ds.lengths['train'])])
    assert np.all(np.abs(ds.power['train'] - mean) <= 1e-12 * mean)
    rng = M.stream(0, 'train')
    random.seed(31)
    np.random.seed(32)
    want = _expected_epochs(ds, 'train', 4, True, 48, 1, lambda idx: M.gains(ds.power['train'][idx], rng, 2, 3.0, None))
    assert len(want) == len(unset) == len(dev.files) == 2
    for k, (w, u) in enumerate(zip(want, unset)):
        a = dev['arr_%d' % k]
        assert np.array_equal(P.bits(a), P.bits(u)) and np.array_equal(P.bits(a).reshape(-1), P.bits(w).reshape(-1))


def test_noise_gain_follows_the_active_powers(hp, tree, tmp_path):
    from danet_amd import feed
    folder = str(tmp_path / 'noise')
    NR.write_noise(folder, [700, 1500, 30000, 9000, 40000])
    keys = dict(MIX_SNR_RANGE=4.0, MIX_LEVEL_MEASURE='active')
    noise = dict(NOISE_DIR=folder, NOISE_SNR_MIN=-5.0, NOISE_SNR_MAX=15.0)
    bs, C, crop = 4, 2, 48
    ds = _dataset(hp, tree, **dict(keys, **noise))
    _seed()
    dev = [feed.NoisyBatch(b.src.clone(), b.noise.clone(), b.gain.clone())
           for _ in range(2) for b in ds.epoch_device('train', bs, shuffle=True, device='cuda', crop_len=crop)]
    assert len(dev) == 4
    table = _restated_table(ds, 'train')
    assert np.all(np.abs(ds.power['train'] - table) <= 1e-12 * table)
    ref_pw = np.asarray([M.mean_power(ds.noise_pool_host[o:o + n]) for o, n in zip(ds.noise_offsets, ds.noise_lengths)])
    assert np.abs(ds.noise_power - ref_pw).max() <= 1e-12 * ref_pw.max()        # P_n stays the mean power
    # the plan of the run without the noise keys, fed the restated ACTIVE table, then tests/noise_ref.py
    ds_plan = _dataset(hp, tree, **keys)
    ds_plan.power = {'train': table}
    _seed()
    items = [it for _ in range(2) for it in ds_plan.plan_epoch_reverb('train', bs, True, crop, crop=True)]
    rng = NR.stream(0, 'train')
    mean = np.asarray([M.mean_power(ds.pool_host['train'][o:o + n])
                       for o, n in zip(ds.offsets['train'], ds.lengths['train'])])
    moved = 0
    for a, (idx, T_max, _pads, _beg, _cnt, gains) in zip(dev, [it[:6] for it in items]):
        state = rng.get_state()
        ref = NR.plan(table[idx], gains, rng, C, ds.noise_offsets, ds.noise_lengths, ref_pw, T_max, -5.0, 15.0, 256, 64)
        assert np.array_equal(a.gain.cpu().numpy().view(np.uint32), ref['gains'].view(np.uint32))
        other = np.random.RandomState(0)
        other.set_state(state)
        by_mean = NR.plan(mean[idx], gains, other, C, ds.noise_offsets, ds.noise_lengths, ref_pw, T_max, -5.0, 15.0,
                          256, 64)
        moved += int(not np.array_equal(by_mean['gains'], ref['gains']))
    assert moved == len(dev)                  # the mean-power table would have given other noise gains


# ----------------------------------------------------------------------------------------- CLI
def test_command_line_trains_with_the_key_set(tmp_path):
    _write_tree(tmp_path / 'tree', n=8, seed=9)
    cfg = tmp_path / 'cfg.json'
    cfg.write_text(json.dumps(dict(
        BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
        NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor', INFER_ESTIMATOR_METHOD='anchor',
        SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64, DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'),
        MIX_SNR_RANGE=5.0, MIX_LEVEL_MEASURE='active')))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'lv', '-m', 'train', '-ds', 'wavdir',
                          '-c', str(cfg), '-ne', '1', '-bs', '2'], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    txt = out.stdout
    assert 'wavdir train: 8 files' in txt and 'Epoch 1/1' in txt and 'Valid  1/1' in txt      # two steps of 2 x 2
    assert np.isfinite(float(txt.split('Epoch 1/1 loss=')[1].split()[0]))
    assert np.isfinite(float(txt.split('Valid  1/1 loss=')[1].split()[0]))
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps(dict(json.loads(cfg.read_text()), MIX_LEVEL_MEASURE='mean')))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-m', 'train', '-ds', 'wavdir', '-c', str(bad),
                          '-ne', '1'], cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and 'MIX_LEVEL_MEASURE' in out.stderr
