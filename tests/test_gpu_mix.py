'''
GPU tests of the mixture level control of the wavdir dataset (run with -m gpu): danet_mix_power against
math.fsum of the float64 squares, danet_mix_scale_c64 bit for bit against numpy's float32 product, the
dataset end to end against tests/mix_ref.py, and the command line.

BAR of the power: relative error <= 1e-9.  Every term is non-negative and exact in float64, and no term
passes through more than 2^22 additions (include/danet_mix_hip.h), so the sum's relative error is at most
2^22 * 2^-53 = 4.7e-10.
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
from gpu_helpers import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-9
N = 256


def _check_power(got, pool, offs, lens, what):
    got = np.asarray(got)
    worst = 0.0
    for u, (o, n) in enumerate(zip(offs, lens)):
        want = M.sum_squares(pool[o:o + n])
        err = abs(got[u] - want) / want if want else abs(got[u])
        worst = max(worst, err)
        print('%s row %d (offset %d, %d samples): relative error %.3g' % (what, u, o, n, err))
        assert err <= BAR, (what, u, o, n, err)
    return worst


# ------------------------------------------------------------------------------------------ power
@pytest.mark.parametrize('residue', [0, 1, 2, 3])
def test_power_against_fsum_at_every_offset_residue(residue):
    from danet_amd import ops
    rng = np.random.RandomState(residue)
    lens = [N, N + 1, 4095, 65536, (1 << 20) + 3, 5 * 10 ** 6]
    offs, off = [], residue
    for n in lens:
        offs.append(off)
        off += n
        off += (residue - off) % 4 + 4 * int(rng.randint(0, 5))      # every row starts at the same residue mod 4
    assert all(o % 4 == residue for o in offs)
    pool = (rng.standard_normal(off).astype(np.float32) * np.float32(3000.0))
    pool[offs[3] + 100:offs[3] + 5000] = 0.0                          # a stretch of silence
    dev = cu(pool)
    assert dev.data_ptr() % 16 == 0
    got = ops.mix_power(dev, offs, lens)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (len(lens),)
    again = ops.mix_power(dev, offs, lens)
    a, b = got.cpu().numpy(), again.cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))       # two calls: bit for bit
    _check_power(a, pool, offs, lens, 'residue %d' % residue)


@pytest.mark.parametrize('n_utt', [1, 2, 1000])
def test_power_row_counts(n_utt):
    from danet_amd import ops
    rng = np.random.RandomState(40 + n_utt)
    if n_utt == 1:
        lens, offs, total = [300001], [7], 300010
    elif n_utt == 2:
        lens, offs, total = [N, (1 << 20) + 3], [(1 << 20) + 9, 2], (1 << 20) + 9 + N
    else:
        total = 1 << 21
        lens = [int(v) for v in rng.randint(N, 4096, size=n_utt)]
        lens[5], lens[500] = 200000, 65537                            # two rows of several slices among the short ones
        offs = [int(rng.randint(0, total - n + 1)) for n in lens]     # any order, overlapping
    pool = (rng.standard_normal(total).astype(np.float32) * np.float32(1000.0))
    dev = cu(pool)
    a = ops.mix_power(dev, offs, lens).cpu().numpy()
    b = ops.mix_power(dev, offs, lens).cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    _check_power(a, pool, offs, lens, 'n_utt %d' % n_utt)
    with pytest.raises(ValueError, match='outside the pool'):
        ops.mix_power(dev, [total - 10], [11])
    with pytest.raises(ValueError, match='outside the pool'):
        ops.mix_power(dev, [-1], [11])


def test_power_clamps_what_only_the_device_can_see():
    '''rows that leave the pool are cut to it: the pool sits between two bands of 1e30, any sample read from
    outside would wreck the sum'''
    from danet_amd import ops
    rng = np.random.RandomState(7)
    n, guard = 200003, 1021
    big = np.full(guard + n + guard, 1e30, np.float32)
    big[guard:guard + n] = rng.standard_normal(n).astype(np.float32) * 500
    dev = cu(big)
    pool = dev[guard:guard + n]
    host = big[guard:guard + n]
    i64 = np.iinfo(np.int64)
    rows = [(n - 100, 1000, n - 100, 100),        # (offset, length) as given -> (offset, length) it is cut to
            (-50, 200, 0, 150),
            (-50, 50, 0, 0),
            (10, -5, 0, 0),
            (n + 7, 300, 0, 0),
            (0, n + 5, 0, 70000),                 # longer than max_len: cut to max_len
            (3, 70001, 3, 70000),
            (i64.min, i64.max, 0, 0),
            (i64.max, i64.max, 0, 0),
            (-3, i64.max, 0, 70000),
            (1000, 66000, 1000, 66000)]
    offs = torch.tensor([r[0] for r in rows], dtype=torch.int64, device='cuda')
    lens = torch.tensor([r[1] for r in rows], dtype=torch.int64, device='cuda')
    got = ops.mix_power(pool, offs, lens, max_len=70000).cpu().numpy()
    assert np.isfinite(got).all() and got.max() < 1e20
    _check_power(got, host, [r[2] for r in rows], [r[3] for r in rows], 'clamped')
    with pytest.raises(ValueError, match='max_len'):
        ops.mix_power(pool, offs, lens)


def test_power_guarded_output_and_workspace_are_left_alone():
    from danet_amd import _lib
    lib = _lib.load_mix()
    rng = np.random.RandomState(9)
    lens = [N, 300000, 70000, 65536, 5]
    offs = [3, 1000, 400000, 500001, 0]
    pool_h = rng.standard_normal(600000).astype(np.float32) * 100
    pool, n, guard = cu(pool_h), len(lens), 64
    max_len = max(lens)
    need = lib.danet_mix_workspace_bytes(n, max_len)
    assert need == n * 5 * 8                                           # 5 slices of 65536 per row
    poison = 0x7ff8dead0000beef
    out_all = torch.full((guard + n + guard,), poison, dtype=torch.int64, device='cuda')
    ws_all = torch.full((guard + need // 8 + guard,), poison, dtype=torch.int64, device='cuda')
    o, l = cu(offs, torch.int64), cu(lens, torch.int64)
    rc = lib.danet_mix_power(_lib.stream(), n, pool.data_ptr(), pool.numel(), o.data_ptr(), l.data_ptr(), max_len,
                             out_all.data_ptr() + 8 * guard, ws_all.data_ptr() + 8 * guard, need)
    assert rc == 0, lib.danet_mix_last_error()
    torch.cuda.synchronize()
    out_h, ws_h = out_all.cpu().numpy(), ws_all.cpu().numpy()
    for arr, m in ((out_h, n), (ws_h, need // 8)):
        assert (arr[:guard] == poison).all() and (arr[guard + m:] == poison).all()
    assert not (out_h[guard:guard + n] == poison).any()
    _check_power(out_h[guard:guard + n].view(np.float64), pool_h, offs, lens, 'guarded')
    # the slices a row does not have are never written
    ws_rows = ws_h[guard:guard + n * 5].reshape(n, 5)
    for u, length in enumerate(lens):
        used = -(-length // 65536)
        assert not (ws_rows[u, :used] == poison).any() and (ws_rows[u, used:] == poison).all(), u
    # a too small workspace is refused before any launch
    assert lib.danet_mix_power(_lib.stream(), n, pool.data_ptr(), pool.numel(), o.data_ptr(), l.data_ptr(), max_len,
                               out_all.data_ptr() + 8 * guard, ws_all.data_ptr() + 8 * guard, need - 8) == -1


# ------------------------------------------------------------------------------------------ scale
def _scale_case(n_utt, t_count, F, pitched, ones=False):
    from danet_amd import ops
    guard, poison = 64, 0x7fc00abc
    ld = F + 3 if pitched else F
    gen = torch.Generator(device='cuda')
    gen.manual_seed(n_utt * 100003 + t_count * 101 + F)
    words = torch.full((2 * (guard + n_utt * t_count * ld + guard),), poison, dtype=torch.int32, device='cuda')
    flat = torch.view_as_complex(words.view(torch.float32).view(-1, 2))
    view = flat[guard:guard + n_utt * t_count * ld].view(n_utt, t_count, ld)[:, :, :F]
    x = torch.randn(n_utt, t_count, F, 2, device='cuda', generator=gen) * 3000.0
    x[0, 0, :8] = torch.tensor([[0.0, -0.0], [1e-40, -1e-41], [float('inf'), -float('inf')], [1.0, -1.0],
                                [3.4e38, 1.2e-38], [0.0, 5.0], [-0.0, 0.0], [2.0 ** -126, 2.0 ** -149]],
                               device='cuda')[:min(8, F)]
    x[-1, -1, -1] = torch.tensor([0.0, -0.0], device='cuda')
    view.copy_(torch.view_as_complex(x))
    before = P.bits(flat.cpu().numpy()).copy()
    if ones:
        g = np.ones(n_utt, np.float32)
    else:
        g = (10.0 ** np.random.RandomState(F + n_utt).uniform(-2, 2, size=n_utt)).astype(np.float32)
        g[0] = np.float32(0.3)
    got = ops.mix_scale_(view, cu(g))
    assert got.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    after = P.bits(flat.cpu().numpy())
    assert np.array_equal(after[:2 * guard], before[:2 * guard]) and np.array_equal(after[-2 * guard:], before[-2 * guard:])
    body_a = after[2 * guard:-2 * guard].reshape(n_utt, t_count, ld, 2)
    body_b = before[2 * guard:-2 * guard].reshape(n_utt, t_count, ld, 2)
    assert np.array_equal(body_a[:, :, F:], body_b[:, :, F:])          # the pitch gaps: bit-unchanged
    with np.errstate(over='ignore', invalid='ignore'):
        want = g[:, None, None, None] * body_b[:, :, :F].view(np.float32)     # np.float32(g) * x, one rounding
    assert want.dtype == np.float32
    assert np.array_equal(body_a[:, :, :F], want.view(np.uint32)), (n_utt, t_count, F, pitched)
    if ones:
        assert np.array_equal(body_a, body_b)                          # g = 1 leaves every bit
    else:
        zeros = (body_b[:, :, :F] & 0x7fffffff) == 0
        assert np.array_equal(body_a[:, :, :F][zeros], body_b[:, :, :F][zeros])      # zeros stay the zeros they were


@pytest.mark.parametrize('F', [33, 129, 2049])
@pytest.mark.parametrize('t_count', [1, 128])
@pytest.mark.parametrize('n_utt', [1, 7, 130])
def test_scale_bit_for_bit(n_utt, t_count, F):
    _scale_case(n_utt, t_count, F, pitched=False)
    _scale_case(n_utt, t_count, F, pitched=True)


@pytest.mark.parametrize('F', [33, 129])
@pytest.mark.parametrize('n_utt,t_count', [(1, 1), (7, 128), (130, 5)])
def test_scale_by_one_leaves_every_bit(n_utt, t_count, F):
    _scale_case(n_utt, t_count, F, pitched=False, ones=True)
    _scale_case(n_utt, t_count, F, pitched=True, ones=True)


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


def test_dataset_with_the_keys_set_equals_the_plan_times_the_restated_gains(hp, tmp_path):
    from danet_amd import datasets, feed
    M.write_tree(tmp_path / 'tree', seed=4, n_per_subset=14, subsets=('train', 'test'))
    R, L = 5.0, 3.0
    _config(hp, tmp_path / 'tree', MIX_SNR_RANGE=R, MIX_LEVEL_RANGE=L)
    ds = datasets.WavDirData()
    ds.install_and_load()
    bs, C = hp.BATCH_SIZE * hp.MAX_N_SIGNAL, hp.MAX_N_SIGNAL

    random.seed(21)
    np.random.seed(22)
    dev = [b.cpu().numpy().copy() for _ in range(2)
           for b in ds.epoch_device('train', bs, shuffle=True, device='cuda', crop_len=hp.MAX_TRAIN_LEN)]
    # the dataset's own power table against float64: stored scales run over 40 dB, one file is silent
    for subset in ('train', 'test'):
        if subset == 'test':
            ds.power_table('test', ds.upload_pool('test', ds._device('cuda')))
        table = ds.power[subset]
        assert table.dtype == np.float64 and table.shape == (14,)
        for u, (o, n) in enumerate(zip(ds.offsets[subset], ds.lengths[subset])):
            want = M.mean_power(ds.pool_host[subset][o:o + n])
            assert abs(table[u] - want) <= BAR * want, (subset, u, table[u], want)
        assert table[3] == 0.0 and table.max() / table[table > 0].min() > 1e3

    rng = M.stream(0, 'train')
    random.seed(21)
    np.random.seed(22)
    want = _expected_epochs(ds, 'train', bs, True, hp.MAX_TRAIN_LEN, 2,
                            lambda idx: M.gains(ds.power['train'][idx], rng, C, R, L))
    assert len(dev) == len(want) == 2 * 2
    for a, b in zip(dev, want):
        assert a.shape == (hp.BATCH_SIZE, C) + b.shape[1:] and a.dtype == np.complex64
        assert np.array_equal(P.bits(a).reshape(-1), P.bits(b).reshape(-1))
    assert any(np.abs(x).max() > 0 for x in dev)

    # epoch() gives the same batches: a fresh dataset, so that its train stream starts where the first one's did
    ds2 = datasets.WavDirData()
    ds2.install_and_load()
    random.seed(21)
    np.random.seed(22)
    host = [np.ascontiguousarray(feed.to_batch_host(pt, hp.MAX_TRAIN_LEN)) for _ in range(2)
            for pt in ds2.epoch('train', bs, shuffle=True)]
    assert np.array_equal(ds2.power['train'].view(np.uint64), ds.power['train'].view(np.uint64))
    assert len(host) == len(dev)
    for a, b in zip(dev, host):
        assert a.shape == b.shape and np.array_equal(P.bits(a), P.bits(b))

    # evaluation sweeps: no crop, the same mixtures every sweep (valid is test's folder here, its own stream)
    for subset in ('valid', 'test'):
        random.seed(4)
        v1 = [b.cpu().numpy().copy() for b in ds.epoch_device(subset, bs, device='cuda')]
        random.seed(4)
        v2 = [b.cpu().numpy().copy() for b in ds.epoch_device(subset, bs, device='cuda')]
        rng = M.stream(0, subset)
        random.seed(4)
        want = _expected_epochs(ds, subset, bs, False, None, 1,
                                lambda idx: M.gains(ds.power['test'][idx], rng, C, R, L))
        random.seed(4)
        vh = [np.ascontiguousarray(feed.to_batch_host(pt, None)) for pt in ds.epoch(subset, bs)]
        assert len(v1) == len(v2) == len(want) == len(vh) == 2
        for a, b, c, d in zip(v1, v2, want, vh):
            assert np.array_equal(P.bits(a), P.bits(b)) and np.array_equal(P.bits(a).reshape(-1), P.bits(c).reshape(-1))
            assert np.array_equal(P.bits(a), P.bits(d))


def test_r_zero_gives_every_source_of_a_group_the_same_power(hp, tmp_path):
    from danet_amd import datasets
    M.write_tree(tmp_path / 'tree', seed=5, n_per_subset=14, subsets=('train', 'test'))
    _config(hp, tmp_path / 'tree', MIX_SNR_RANGE=0.0)
    ds = datasets.WavDirData()
    ds.install_and_load()
    bs, C = hp.BATCH_SIZE * hp.MAX_N_SIGNAL, hp.MAX_N_SIGNAL
    ds.power_table('train', ds.upload_pool('train', ds._device('cuda')))
    groups = 0
    for idx, _T, _pads, _beg, _cnt, gains in ds.plan_epoch('train', bs, shuffle=False):
        Pw = ds.power['train'][idx].reshape(-1, C)
        g = gains.astype(np.float64).reshape(-1, C)
        for p, gg in zip(Pw, g):
            live = p > 0
            assert np.array_equal(gg[~live], np.ones((~live).sum()))
            if live.sum() > 1:
                lev = gg[live] ** 2 * p[live]
                assert np.abs(lev / lev[0] - 1).max() <= 1e-6, (p, gg)
                groups += 1
    assert groups >= 6


def test_keys_null_maps_no_library_and_yields_what_it_always_did(hp, tmp_path):
    from danet_amd import datasets
    M.write_tree(tmp_path / 'tree', seed=6, n_per_subset=10, subsets=('train', 'test'))
    cfg = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
               BATCH_SIZE=4, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=48, MIX_SNR_RANGE=None, MIX_LEVEL_RANGE=None)
    code = (
        "import sys, json, random; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, datasets, feed\n"
        "from danet_amd.hparams import hparams\n"
        "hparams.load(json.loads(%r)); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.install_and_load()\n"
        "random.seed(31); np.random.seed(32)\n"
        "dev = [b.cpu().numpy().copy() for b in ds.epoch_device('train', 8, True, 'cuda', 48)]\n"
        "random.seed(31); np.random.seed(32)\n"
        "host = [np.ascontiguousarray(feed.to_batch_host(pt, 48)) for pt in ds.epoch('train', 8, True)]\n"
        "maps = open('/proc/self/maps').read()\n"
        "print('UNMAPPED:', _lib._mix is None and 'libdanet_mix_hip' not in maps and 'libdanet_prep_hip' in maps)\n"
        "print('NOTHING:', ds.power == {} and ds._mix_rng == {} and ds._ring['cuda:0']['row'] == 24)\n"
        "np.savez(%r, *dev); np.savez(%r, *host)\n"
    ) % (ROOT, json.dumps(cfg), str(tmp_path / 'dev.npz'), str(tmp_path / 'host.npz'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert 'UNMAPPED: True' in out.stdout and 'NOTHING: True' in out.stdout, out.stdout + out.stderr[-3000:]
    _config(hp, tmp_path / 'tree')                                      # the keys not in the configuration at all
    ds = datasets.WavDirData()
    ds.install_and_load()
    random.seed(31)
    np.random.seed(32)
    want = _expected_epochs(ds, 'train', 8, True, 48, 1, lambda idx: None)
    random.seed(31)
    np.random.seed(32)
    unset = [b.cpu().numpy().copy() for b in ds.epoch_device('train', 8, True, 'cuda', 48)]
    dev, host = np.load(str(tmp_path / 'dev.npz')), np.load(str(tmp_path / 'host.npz'))
    assert len(want) == len(unset) == len(dev.files) == len(host.files) == 2
    for k, (w, u) in enumerate(zip(want, unset)):
        a, b = dev['arr_%d' % k], host['arr_%d' % k]
        assert np.array_equal(P.bits(a).reshape(-1), P.bits(w).reshape(-1))
        assert np.array_equal(P.bits(a), P.bits(b)) and np.array_equal(P.bits(a), P.bits(u))


def test_a_batch_size_that_is_no_multiple_of_the_sources_is_refused(hp, tmp_path):
    from danet_amd import datasets
    M.write_tree(tmp_path / 'tree', seed=7, n_per_subset=6, subsets=('train', 'test'))
    _config(hp, tmp_path / 'tree', MIX_LEVEL_RANGE=2.0)
    ds = datasets.WavDirData()
    ds.install_and_load()
    with pytest.raises(ValueError, match='multiple of MAX_N_SIGNAL'):
        next(iter(ds.epoch('train', 3)))


# ----------------------------------------------------------------------------------------- CLI
def test_command_line_trains_with_both_keys_set(tmp_path):
    M.write_tree(tmp_path / 'tree', seed=8, n_per_subset=16, subsets=('train', 'test'), seconds=(0.2, 0.5))
    cfg = tmp_path / 'cfg.json'
    cfg.write_text(json.dumps(dict(
        BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
        NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor', INFER_ESTIMATOR_METHOD='anchor',
        SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64, DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'tree'),
        MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)

    def main(*args):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py')] + list(args), cwd=str(tmp_path),
                             capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        return out.stdout

    txt = main('-n', 'mx', '-m', 'train', '-ds', 'wavdir', '-c', str(cfg), '-ne', '1', '-bs', '4')
    assert 'wavdir train: 16 files' in txt and 'Epoch 1/1' in txt and 'Valid  1/1' in txt
    assert np.isfinite(float(txt.split('Epoch 1/1 loss=')[1].split()[0]))
    assert np.isfinite(float(txt.split('Valid  1/1 loss=')[1].split()[0]))
    txt = main('-n', 'mx2', '-m', 'train', '-ds', 'wavdir', '-c', str(cfg), '-ne', '1', '-bs', '4', '--sync-feed',
               '--no-valid-on-epoch')
    assert np.isfinite(float(txt.split('Epoch 1/1 loss=')[1].split()[0]))
    # a bad value stops the run and names the key
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps(dict(json.loads(cfg.read_text()), MIX_SNR_RANGE=-3)))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '-m', 'train', '-ds', 'wavdir', '-c', str(bad),
                          '-ne', '1'], cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and 'MIX_SNR_RANGE' in out.stderr
