'''
GPU tests of the speed perturbation of the wavdir dataset (run with -m gpu): danet_speed_resample against the
float64 restatement tests/speed_ref.py, its exactness and bounds guarantees, the dataset end to end on both
routes, and the command line.

BAR of the kernel, per output sample: |y - y64| <= 33 * 2^-24 * S_n + 2^-126 with S_n = sum_j |tab * x|, the
standard bound of a 32-term float32 dot product in any order, with or without fused multiply-adds, over
identical float32 inputs (31 additions and 32 products, each within 2^-24 relative: gamma_32 < 33 * 2^-24).  It
is derived, not measured; the sequential float32 numpy sum is held to it first, on the CPU.
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
import speed_ref as SR
from gpu_helpers import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 2, 31, 32, 33, 255, 256, 257, 4097, 65539]
SPEEDS = [384, 487, 511, 512, 513, 541, 640]
POISON = 0x7fc00abc          # a NaN no computation produces


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _desc(rows):
    from danet_amd import ops
    d = np.zeros(len(rows), ops.SPEED_DESC_DTYPE)
    for u, r in enumerate(rows):
        d[u] = (r['so'], r['L'], r['do'], r['n'], r['p'], 0)
    return d


def _launch(pool, rows, tab, out):
    '''one launch through the Python layer (host-validated descriptors)'''
    from danet_amd import ops
    ops.speed_resample(pool, _desc(rows), tab, out)
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def bank():
    '''130 utterances in one pool -- every (L, p) of the case table, then 60 of drawn length and speed -- at
    int16 scale, source offsets at every residue mod 4, destination spans apart by bands of 5 .. 7 floats; the
    float64 reference of every row, computed once'''
    rng = np.random.RandomState(1)
    tab = SR.table(0.1)
    rows = [dict(L=L, p=p) for L in LENGTHS for p in SPEEDS]
    rows += [dict(L=int(rng.randint(1, 3000)), p=int(rng.randint(384, 641))) for _ in range(130 - len(rows))]
    so, do = 0, 9
    for u, r in enumerate(rows):
        so += (u % 4 - so) % 4 + 4 * int(rng.randint(0, 3))
        r.update(so=so, do=do, n=SR.out_len(r['L'], r['p']))
        so += r['L']
        do += r['n'] + 5 + u % 3
    assert sorted(set(r['so'] % 4 for r in rows)) == [0, 1, 2, 3]
    assert all(set(r['so'] % 4 for r in rows if r['L'] == L) == {0, 1, 2, 3} for L in LENGTHS)
    pool = np.clip(rng.standard_normal(so + 11) * 4000, -32768, 32767).astype(np.int16).astype(np.float32)
    refs = []
    for r in rows:
        x = pool[r['so']:r['so'] + r['L']]
        y64, S = SR.resample(x, r['p'], tab)
        assert len(y64) == r['n']
        y32 = SR.resample_f32(x, r['p'], tab)                     # the bar holds for the plain float32 sum: CPU first
        assert (np.abs(y32.astype(np.float64) - y64) <= SR.bound(S)).all(), r
        refs.append((y64, S))
    return dict(rows=rows, pool=pool, tab=tab, refs=refs, out_len=do + 9)


def _poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int32, device='cuda').view(torch.float32)


def _check_rows(out_bits, bank, which):
    '''every output sample of the rows `which` against float64; -> worst error / bar'''
    worst = 0.0
    for u in which:
        r, (y64, S) = bank['rows'][u], bank['refs'][u]
        y = out_bits[r['do']:r['do'] + r['n']].view(np.float32).astype(np.float64)
        ratio = float((np.abs(y - y64) / SR.bound(S)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (u, r, ratio)
    return worst


def _bands_untouched(out_bits, rows):
    written = np.zeros(len(out_bits), bool)
    for r in rows:
        assert not written[r['do']:r['do'] + r['n']].any()
        written[r['do']:r['do'] + r['n']] = True
    assert (out_bits[~written] == POISON).all()
    assert not (out_bits[written] == POISON).any()                # every float of every span is written


# ------------------------------------------------------------------------------- kernel vs float64
@pytest.fixture(scope='module')
def launched(bank):
    '''all 130 rows in ONE launch into a poisoned buffer, twice'''
    pool, tab = cu(bank['pool']), cu(bank['tab'])
    a, b = _poisoned(bank['out_len']), _poisoned(bank['out_len'])
    _launch(pool, bank['rows'], tab, a)
    _launch(pool, bank['rows'], tab, b)
    return dict(pool=pool, tab=tab, a=_bits(a), b=_bits(b))


def test_130_rows_in_one_launch_against_float64(bank, launched):
    worst = _check_rows(launched['a'], bank, range(130))
    print('130 rows, %d samples: worst error / bar %.3f' % (sum(r['n'] for r in bank['rows']), worst))
    _bands_untouched(launched['a'], bank['rows'])
    assert np.array_equal(launched['a'], launched['b'])           # two launches: identical bits


@pytest.mark.parametrize('n_utt', [1, 7])
def test_rows_alone_and_by_sevens_equal_the_130_row_launch(bank, launched, n_utt):
    '''every row launched alone (130 launches) / in groups of seven into one poisoned buffer: the same bits as among
    129 others, the bands still poison; every sample against float64 again'''
    rows = bank['rows']
    out = _poisoned(bank['out_len'])
    for k in range(0, len(rows), n_utt):
        _launch(launched['pool'], rows[k:k + n_utt], launched['tab'], out)
    got = _bits(out)
    assert np.array_equal(got, launched['a'])
    _bands_untouched(got, rows)
    _check_rows(got, bank, range(130))


def test_identity_at_p_equal_q_with_the_p_zero_table(bank):
    rows = [dict(r, p=512, n=r['L']) for r in bank['rows']]
    do = 3
    for r in rows:
        r['do'] = do
        do += r['n'] + 2
    pool, tab, out = cu(bank['pool']), cu(SR.table(0.0)), _poisoned(do + 3)
    _launch(pool, rows, tab, out)
    got = _bits(out)
    src = bank['pool'].view(np.uint32)
    for r in rows:
        assert np.array_equal(got[r['do']:r['do'] + r['n']], src[r['so']:r['so'] + r['L']]), r
    _bands_untouched(got, rows)


def test_host_visible_errors_launch_nothing(bank):
    from danet_amd import _lib, ops
    pool, tab, out = cu(bank['pool']), cu(bank['tab']), _poisoned(4096)
    r = dict(so=0, L=100, do=0, n=100, p=512)
    for bad, msg in ((dict(r, p=383), 'p = 383'), (dict(r, so=len(bank['pool']) - 50), 'outside the pool'),
                     (dict(r, do=4000), 'inside the buffer')):
        with pytest.raises(ValueError, match=msg):
            ops.speed_resample(pool, _desc([bad]), tab, out)
    d = cu(_desc([r]).view(np.uint8), torch.uint8)
    lib = _lib.load_speed()
    assert lib.danet_speed_resample(_lib.stream(), 0, pool.data_ptr(), pool.numel(), d.data_ptr(), tab.data_ptr(),
                                    out.data_ptr(), out.numel()) == -1
    assert lib.danet_speed_resample(_lib.stream(), 1, pool.data_ptr(), pool.numel(), d.data_ptr(), tab.data_ptr() + 4,
                                    out.data_ptr(), out.numel()) == -1
    torch.cuda.synchronize()
    assert (_bits(out) == POISON).all()


def test_what_only_the_device_sees_is_clamped():
    '''descriptor rows straight into device memory, unvalidated: the pool lies between two bands of 1e30 (a sample
    read from outside would wreck the sum), the destination between two poisoned bands'''
    from danet_amd import ops
    rng = np.random.RandomState(7)
    n_src, n_dst, guard = 5003, 6000, 1021
    big = np.full(guard + n_src + guard, 1e30, np.float32)
    big[guard:guard + n_src] = np.clip(rng.standard_normal(n_src) * 3000, -32768, 32767).astype(np.int16)
    src_all, dst_all = cu(big), _poisoned(guard + n_dst + guard)
    pool, dst = src_all[guard:guard + n_src], dst_all[guard:guard + n_dst]
    host = big[guard:guard + n_src]
    tab = SR.table(0.1)
    i64 = np.iinfo(np.int64)
    #       src_offset  src_length  dst_offset dst_length  p      the samples x the kernel may see      written n, p used
    cases = [(n_src - 100, 1000,     100,       250,       512,   host[n_src - 100:],                   (0, 250), 512),
             (-50,         200,      400,       150,       600,   np.r_[np.zeros(50, np.float32), host[:150]], (0, 150), 600),
             (-50,         50,       600,       40,        512,   np.zeros(0, np.float32),              (0, 40), 512),
             (10,          -5,       700,       40,        512,   np.zeros(0, np.float32),              (0, 40), 512),
             (n_src + 7,   300,      800,       40,        512,   np.zeros(0, np.float32),              (0, 40), 512),
             (i64.min,     i64.max,  900,       40,        512,   np.zeros(0, np.float32),              (0, 40), 512),
             (i64.max,     i64.max,  1000,      40,        512,   np.zeros(0, np.float32),              (0, 40), 512),
             (100,         2000,     -30,       100,       450,   host[100:2100],                       (30, 100), 450),
             (100,         2000,     n_dst - 60, 500,      450,   host[100:2100],                       (0, 60), 450),
             (100,         2000,     n_dst + 5, 500,       450,   host[100:2100],                       (0, 0), 450),
             (100,         2000,     i64.min,   i64.max,   450,   host[100:2100],                       (0, 0), 450),
             (100,         2000,     1200,      -7,        450,   host[100:2100],                       (0, 0), 450),
             (3000,        1500,     1300,      1100,      100,   host[3000:4500],                      (0, 1100), 384),
             (3000,        1500,     2500,      1100,      99999, host[3000:4500],                      (0, 1100), 640),
             (0,           n_src,    3700,      2100,      512,   host,                                 (0, 2100), 512)]
    d = np.zeros(len(cases), ops.SPEED_DESC_DTYPE)
    for u, c in enumerate(cases):
        d[u] = c[:5] + (0,)
    dev = cu(d.view(np.uint8), torch.uint8)
    ops.speed_resample(pool, dev, cu(tab), dst)                  # a device table is the caller's word: no host check
    torch.cuda.synchronize()
    got = _bits(dst_all)
    assert (got[:guard] == POISON).all() and (got[guard + n_dst:] == POISON).all()
    body = got[guard:guard + n_dst]
    written = np.zeros(n_dst, bool)
    for (so, sl, do, dl, p, x, (n_lo, n_hi), p_used) in cases:
        if n_hi <= n_lo:
            continue
        y64, S = SR.resample(x, p_used, tab, n_out=n_hi)
        y = body[do + n_lo:do + n_hi].view(np.float32).astype(np.float64)
        assert np.isfinite(y).all() and np.abs(y).max() < 1e6, (so, sl, do, dl)
        assert (np.abs(y - y64[n_lo:]) <= SR.bound(S[n_lo:])).all(), (so, sl, do, dl, p)
        written[do + n_lo:do + n_hi] = True
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


def _restated_epochs(ds, bs, n_epochs, crop_len, P_range, gains_of):
    '''the train batches by their definition: the draw of tests/speed_ref.py, ops.speed_resample of the restated
    descriptors into a scratch laid out as the dataset documents it, ops.stft_batch of that scratch, times the
    restated gains -> (batches, frame counts per batch)'''
    from danet_amd import ops
    lengths, offsets = ds.lengths['train'], ds.offsets['train']
    pool, window, tab = cu(ds.pool_host['train']), cu(_window(256)), cu(SR.table(P_range))
    stride = (SR.out_len(int(lengths.max()), 512 - int(np.floor(512 * P_range))) + 3) // 4 * 4
    rng = SR.stream(0, 'train')
    out, frames_seen = [], []
    for _ in range(n_epochs):
        for idx in P.index_plan(len(lengths), bs, True):
            p, Lp = SR.draw(lengths[idx], rng, P_range, 256)
            frames = [P.num_frames(int(l), 256, 64) for l in Lp]
            T_max, pads = P.draw_pads(frames)
            beg, cnt = P.draw_crop(T_max, crop_len)
            spots = np.arange(bs, dtype=np.int64) * stride
            scratch = torch.zeros(bs * stride, dtype=torch.float32, device='cuda')
            ops.speed_resample(pool, ops.speed_desc(offsets[idx], lengths[idx], spots, Lp, p, pool.numel(),
                                                    scratch.numel()), tab, scratch)
            desc = ops.prep_desc(spots, Lp, pads, T_max, scratch.numel(), 256, 64)
            X = ops.stft_batch(scratch, desc, T_max, window, 256, 64, t_begin=beg, t_count=cnt).cpu().numpy()
            g = gains_of(idx)
            if g is not None:
                X = (g[:, None, None, None] * X.view(np.float32).reshape(X.shape + (2,))).view(np.complex64)[..., 0]
            out.append(X)
            frames_seen.append((frames, pads, T_max, beg, cnt, p))
    return out, frames_seen


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('speed') / 'tree'
    SR.write_tree(root, seed=4, n_per_subset=14)
    return root


def test_range_zero_gives_the_batches_of_key_null_on_both_routes(hp, tree):
    bs = 8
    got = {}
    for key in (None, 0):
        ds = _dataset(hp, tree, SPEED_PERTURB_RANGE=key)
        random.seed(21)
        np.random.seed(22)
        dev = _device_epochs(ds, 'train', bs, 2, 48)
        ds = _dataset(hp, tree, SPEED_PERTURB_RANGE=key)
        random.seed(21)
        np.random.seed(22)
        got[key] = (dev, _host_epochs(ds, 'train', bs, 2, 48))
    from danet_amd import _lib
    assert _lib._speed is not None                                # range 0 is ON: it launched
    assert len(got[None][0]) == len(got[0][0]) == 4
    for a, b, c, d in zip(got[None][0], got[0][0], got[None][1], got[0][1]):
        assert np.abs(a).max() > 0
        assert np.array_equal(P.bits(a), P.bits(b)) and np.array_equal(P.bits(c), P.bits(d))
        assert np.array_equal(P.bits(a), P.bits(c))


@pytest.mark.parametrize('mix', [False, True])
def test_dataset_equals_the_restated_resampling_on_both_routes(hp, tree, mix):
    keys = dict(SPEED_PERTURB_RANGE=0.1)
    if mix:
        keys.update(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0)
    ds = _dataset(hp, tree, **keys)
    bs, C = hp.BATCH_SIZE * hp.MAX_N_SIGNAL, hp.MAX_N_SIGNAL
    random.seed(21)
    np.random.seed(22)
    dev = _device_epochs(ds, 'train', bs, 2, hp.MAX_TRAIN_LEN)
    assert ds._ring['cuda:0']['row'] == 24 + 40 + (4 if mix else 0)
    assert len(ds._speed_scratch[('train', 'cuda:0')]['bufs']) == ds.DESC_DEPTH

    mix_rng = M.stream(0, 'train')
    random.seed(21)
    np.random.seed(22)
    want, seen = _restated_epochs(ds, bs, 2, hp.MAX_TRAIN_LEN, 0.1,
                                  (lambda idx: M.gains(ds.power['train'][idx], mix_rng, C, 5.0, 3.0)) if mix
                                  else (lambda idx: None))
    assert len(dev) == len(want) == 4
    for a, b, (frames, pads, T_max, beg, cnt, p) in zip(dev, want, seen):
        assert a.shape == (hp.BATCH_SIZE, C, cnt, 129) and b.shape == (bs, cnt, 129)
        assert np.array_equal(P.bits(a).reshape(-1), P.bits(b).reshape(-1))
        # the frame counts are those of L': outside [pad, pad + frames) of the uncropped axis every frame is zero,
        # and the last frame of a non-silent utterance inside the crop is not
        flat = np.abs(a.reshape(bs, cnt, 129)).max(axis=2)
        for u in range(bs):
            t = np.arange(beg, beg + cnt)
            outside = (t < pads[u]) | (t >= pads[u] + frames[u])
            assert (flat[u][outside] == 0).all()
            last = pads[u] + frames[u] - 2                         # the last frame holding samples of every length
            if beg <= last < beg + cnt:
                assert flat[u][last - beg] > 0
    assert any(int(q) != 512 for s in seen for q in s[5])

    # epoch() gives the same batches: a fresh dataset, so that its streams start where the first one's did
    ds2 = _dataset(hp, tree, **keys)
    random.seed(21)
    np.random.seed(22)
    host = _host_epochs(ds2, 'train', bs, 2, hp.MAX_TRAIN_LEN)
    assert len(host) == len(dev)
    for a, b in zip(dev, host):
        assert a.shape == b.shape and np.array_equal(P.bits(a), P.bits(b))


def test_valid_and_test_are_the_batches_of_key_null_and_launch_nothing(hp, tree, tmp_path):
    got = {}
    for key in (None, 0.1):
        ds = _dataset(hp, tree, SPEED_PERTURB_RANGE=key)
        for subset in ('valid', 'test'):
            random.seed(4)
            got[key, subset] = _device_epochs(ds, subset, 8, 1, None, shuffle=False)
            random.seed(4)
            got[key, subset, 'host'] = _host_epochs(ds, subset, 8, 1, None, shuffle=False)
        assert ds._speed_scratch == {} and ds._speed_table == {} and ds._speed_rng == {}
    for subset in ('valid', 'test'):
        assert len(got[None, subset]) == 2
        for a, b, c in zip(got[None, subset], got[0.1, subset], got[0.1, subset, 'host']):
            assert np.array_equal(P.bits(a), P.bits(b)) and np.array_equal(P.bits(a), P.bits(c))
    cfg = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(tree), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
               BATCH_SIZE=4, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=48, SPEED_PERTURB_RANGE=0.1)
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, datasets\n"
        "from danet_amd.hparams import hparams\n"
        "hparams.load(json.loads(%r)); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.install_and_load()\n"
        "n = sum(1 for s in ('valid', 'test') for b in ds.epoch_device(s, 8, False, 'cuda', None))\n"
        "n += sum(1 for s in ('valid', 'test') for b in ds.epoch(s, 8))\n"
        "maps = open('/proc/self/maps').read()\n"
        "print('BATCHES:', n, 'UNMAPPED:', _lib._speed is None and 'libdanet_speed_hip' not in maps and "
        "'libdanet_prep_hip' in maps)\n"
    ) % (ROOT, json.dumps(cfg))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert 'BATCHES: 8 UNMAPPED: True' in out.stdout, out.stdout + out.stderr[-3000:]


# ----------------------------------------------------------------------------------------- CLI
def test_command_line_trains_with_the_key_set(tmp_path):
    SR.write_tree(tmp_path / 'tree', seed=8, n_per_subset=16, seconds=(0.2, 0.5))
    cfg = tmp_path / 'cfg.json'
    cfg.write_text(json.dumps(dict(
        BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
        NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor', INFER_ESTIMATOR_METHOD='anchor',
        SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64, DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'),
        SPEED_PERTURB_RANGE=0.1)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-n', 'sp', '-m', 'train', '-ds', 'wavdir',
                          '-c', str(cfg), '-ne', '1', '-bs', '4'], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'wavdir train: 16 files' in out.stdout and 'Epoch 1/1' in out.stdout
    assert np.isfinite(float(out.stdout.split('Epoch 1/1 loss=')[1].split()[0]))
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps(dict(json.loads(cfg.read_text()), SPEED_PERTURB_RANGE=0.3)))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-m', 'train', '-ds', 'wavdir', '-c', str(bad),
                          '-ne', '1'], cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and 'SPEED_PERTURB_RANGE' in out.stderr
