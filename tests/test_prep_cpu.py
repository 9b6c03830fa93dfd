'''
CPU tests (no GPU) of the wavdir dataset's boundary: the extension library libdanet_prep_hip.so against
its header (exports, prototypes, no environment read, lazy load, host-visible argument errors, the
frame count), the untouched other libraries, the registry / DATASET_DIR, WAV discovery and decoding,
and the batching plan with its `random` draw order.
'''
import ctypes
import os
import random
import re
import subprocess
import sys
from math import ceil

import numpy as np
import pytest

import prep_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_prep_hip.h')


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


# ------------------------------------------------------------------------------------------ ABI
def test_extension_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_prep()
    syms = _header_symbols('danet_prep_hip.h', 'danet_prep_')
    assert syms == ['danet_prep_abi_version', 'danet_prep_last_error', 'danet_prep_num_frames',
                    'danet_prep_stft_batch', 'danet_prep_stft_plan', 'danet_prep_workspace_bytes']
    assert set(_lib.PREP_PROTOTYPES) == set(syms)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.PREP_LIB_PATH], capture_output=True, text=True,
                         check=True)
    exported = sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())
    assert exported == syms, set(exported) ^ set(syms)
    assert lib.danet_prep_abi_version() == 1 == _lib.PREP_ABI_VERSION


def test_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'const void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64,
             'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'const float*': ctypes.c_void_p,
             'float*': ctypes.c_void_p, 'const danet_prep_utt_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.PREP_PROTOTYPES.items():
        m = re.search(r'([a-z_ ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        want = [w for w in want if w is not None]
        assert args == want, (name, args, want)
    # the descriptor row: 24 bytes, the fields the header names, in its order
    from danet_amd import ops
    assert ops.PREP_DESC_DTYPE.itemsize == 24
    body = re.search(r'typedef struct danet_prep_utt \{(.*?)\} danet_prep_utt_t;', txt, flags=re.S).group(1)
    fields = re.findall(r'(int64_t|int32_t)\s+([a-z_]+);', body)
    assert [f for _, f in fields] == list(ops.PREP_DESC_DTYPE.names)
    assert [dict(int64_t=8, int32_t=4)[t] for t, _ in fields] == \
        [ops.PREP_DESC_DTYPE[n].itemsize for n in ops.PREP_DESC_DTYPE.names]


def test_library_does_not_read_the_environment():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.PREP_LIB_PATH], capture_output=True, text=True, check=True)
    assert 'getenv' not in out.stdout
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'prep')
    srcs = [f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp'))]
    assert srcs
    for f in srcs:
        src = open(os.path.join(d, f)).read()
        assert 'getenv' not in src and 'environ' not in src, f
        code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
        assert 'asm' not in code and 'atomic' not in code, f                   # plain HIP C++


def test_other_libraries_are_untouched():
    from danet_amd import _lib
    assert _lib.PREP_PROTOTYPES and os.path.exists(_lib.PREP_LIB_PATH)      # the new symbols live in a library of their own
    for path in (_lib.LIB_PATH, _lib.CONV_LIB_PATH, _lib.DROPOUT_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
        assert 'danet_prep_' not in out.stdout, path
    for table in (_lib.PROTOTYPES, _lib.CONV_PROTOTYPES, _lib.DROPOUT_PROTOTYPES):
        assert not any(k.startswith('danet_prep_') for k in table)
    assert _lib.load().danet_abi_version() == 7
    assert _lib.load_conv().danet_conv_abi_version() == 1
    assert _lib.load_dropout().danet_dropout_abi_version() == 1


def test_lazy_load_and_missing_library_is_a_loud_error(tmp_path):
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, cli\n"
        "from danet_amd.hparams import hparams\n"
        "hparams.digest()\n"
        "ds = hparams.get_dataset()(); ds.install_and_load()\n"
        "next(iter(ds.epoch('train', 4)))\n"
        "maps = open('/proc/self/maps').read()\n"
        "print('TOY:', hparams.DATASET_TYPE, 'LAZY:', _lib._prep is None and 'libdanet_prep_hip' not in maps)\n"
        "_lib.PREP_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_prep()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_prep_hip.so' in str(e))\n"
    ) % (ROOT, str(tmp_path / 'nope.so'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'TOY: toy LAZY: True' in out.stdout and 'LOUD: True' in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------- frame count
@pytest.mark.parametrize('N,S', [(256, 64), (512, 128), (256, 48), (256, 100), (64, 24), (512, 511)])
def test_num_frames_agrees_with_the_core_library(N, S):
    from danet_amd import _lib
    core, prep = _lib.load(), _lib.load_prep()
    for Ls in range(N, N + 4 * S + 1):
        T = prep.danet_prep_num_frames(Ls, N, S)
        assert T == core.danet_stft_num_frames(Ls, N, S) == P.num_frames(Ls, N, S), (Ls, T)
        if N % S == 0:
            assert T == 1 + -(-Ls // S)
    for Ls in (N - 1, 1, 0, -5):
        assert prep.danet_prep_num_frames(Ls, N, S) == -1
        assert b'num_frames' in prep.danet_prep_last_error()
    assert prep.danet_prep_num_frames(N, N, 0) == -1 and prep.danet_prep_num_frames(2 * N, N, N + 1) == -1


def test_num_frames_python_side():
    from danet_amd import datasets, ops
    for N, S in ((256, 64), (512, 128), (256, 48)):
        for Ls in range(N, N + 3 * S):
            assert datasets._stft_frames(Ls, N, S) == ops.prep_num_frames(Ls, N, S) == P.num_frames(Ls, N, S)
    with pytest.raises(ValueError):
        ops.prep_num_frames(255, 256, 64)


# ------------------------------------------------------------------- host-visible argument errors
def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_prep()
    ok = dict(stream=None, n_utt=4, pool=1024, pool_len=100000, desc=2048, T_out=40, t_begin=0, t_count=40,
              N=256, S=64, window=4096, plan=8192, out=16384, ld_out=129)
    cases = [(dict(N=100), b'power of two'), (dict(N=32), b'power of two'), (dict(N=8192), b'power of two'),
             (dict(S=0), b'stride'), (dict(S=257), b'stride'), (dict(n_utt=0), b'n_utt'),
             (dict(pool=None), b'null'), (dict(desc=None), b'null'), (dict(window=None), b'null'),
             (dict(plan=None), b'null'), (dict(out=None), b'null'), (dict(pool_len=-1), b'pool_len'),
             (dict(T_out=0), b't_begin'), (dict(t_begin=-1), b't_begin'), (dict(t_count=0), b't_begin'),
             (dict(t_begin=1), b't_begin + t_count <= T_out'), (dict(t_begin=30, t_count=11), b'T_out'),
             (dict(ld_out=128), b'ld_out'), (dict(pool=1026), b'misaligned'), (dict(desc=2052), b'misaligned'),
             (dict(out=16388), b'misaligned'), (dict(plan=8200), b'misaligned'),
             (dict(n_utt=1 << 30, T_out=1 << 20, t_count=1 << 20), b'2^31')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_prep_stft_batch(*a.values()) == -1, kw
        assert msg in lib.danet_prep_last_error(), (kw, lib.danet_prep_last_error())
    assert lib.danet_prep_workspace_bytes(256) >= 256 * 4 + 4
    assert lib.danet_prep_workspace_bytes(100) == ctypes.c_size_t(-1).value
    for kw, msg in [(dict(N=96), b'power of two'), (dict(window=None), b'null'), (dict(ws=None), b'null'),
                    (dict(ws=8200), b'aligned'), (dict(nbytes=16), b'too small')]:
        a = dict(dict(stream=None, N=256, window=4096, ws=8192, nbytes=4096), **kw)
        assert lib.danet_prep_stft_plan(*a.values()) == -1, kw
        assert msg in lib.danet_prep_last_error(), (kw, lib.danet_prep_last_error())
    with pytest.raises(_lib.DanetHipError, match='stride'):
        _lib.prep_check(lib.danet_prep_stft_batch(*dict(ok, S=0).values()))


def test_descriptor_validation_happens_in_python_before_any_launch():
    from danet_amd import ops
    d = ops.prep_desc([0, 300], [300, 256], [2, 0], 8, 556, 256, 64)
    assert d.dtype == ops.PREP_DESC_DTYPE and d['offset'].tolist() == [0, 300] and d['pad_left'].tolist() == [2, 0]
    assert d['reserved'].tolist() == [0, 0]
    with pytest.raises(ValueError, match='exceeds T_out'):
        ops.prep_desc([0], [300], [3], 8, 556, 256, 64)          # 3 + 6 frames > 8
    with pytest.raises(ValueError, match='exceeds T_out'):
        ops.prep_desc([0], [300], [-1], 8, 556, 256, 64)
    with pytest.raises(ValueError, match='outside the pool'):
        ops.prep_desc([300], [300], [0], 8, 556, 256, 64)
    with pytest.raises(ValueError, match='longer than input'):
        ops.prep_desc([0], [255], [0], 8, 556, 256, 64)


# -------------------------------------------------------------------------- registry and config
def test_registry_and_dataset_dir(hp):
    from danet_amd import datasets
    H = sys.modules['danet_amd.hparams']
    assert H.DEFAULTS['DATASET_DIR'] is None and hp.DATASET_DIR is None
    assert re.fullmatch(hp.pattern, 'DATASET_DIR')
    hp.load(dict(DATASET_TYPE='wavdir'))
    hp.digest()
    assert hp.get_dataset() is datasets.WavDirData
    ds = hp.get_dataset()()
    with pytest.raises(ValueError, match='DATASET_DIR'):
        ds.install_and_load()
    assert not ds.is_loaded
    with pytest.raises(RuntimeError):
        next(iter(ds.epoch('train', 4)))
    hp.load(dict(DATASET_DIR='/some/where'))
    assert hp.DATASET_DIR == '/some/where'


# --------------------------------------------------------------------------------------- loading
def _write(path, rate, data):
    import scipy.io.wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scipy.io.wavfile.write(path, rate, data)


def _small_tree(root, with_valid=True):
    rng = np.random.RandomState(1)
    spec = {}
    for subset in ('train', 'valid', 'test') if with_valid else ('train', 'test'):
        spec[subset] = []
        for name, rate, n in (('b/z.wav', 8000, 700), ('a/y.wav', 11025, 1000), ('a/x.WAV', 8000, 256),
                              ('c.wav', 11025, 353)):
            data = (rng.randn(n) * 3000).astype(np.int16)
            _write(os.path.join(root, subset, name), rate, data)
            spec[subset].append((os.path.join(root, subset, name), rate, data))
    _write(os.path.join(root, 'train', 'a', 'short.wav'), 8000, (rng.randn(255) * 100).astype(np.int16))
    _write(os.path.join(root, 'train', 'a', 'short2.wav'), 11025, (rng.randn(351) * 100).astype(np.int16))
    open(os.path.join(root, 'train', 'notes.txt'), 'w').write('not audio')
    return spec


def test_loading_discovery_resampling_and_skips(hp, tmp_path, capsys):
    import scipy.signal
    from danet_amd import datasets
    root = str(tmp_path / 'data')
    spec = _small_tree(root)
    hp.load(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000))
    hp.digest()
    ds = datasets.WavDirData()
    ds.load_host()
    printed = capsys.readouterr().out
    assert printed.count('wavdir train:') == 1 and '2 shorter than FFT_SIZE skipped' in printed
    assert ds.skipped == dict(train=2, valid=0, test=0)
    for subset in ('train', 'valid', 'test'):
        want = sorted(p for p, _, _ in spec[subset])
        assert ds.files[subset] == want                          # sorted path order, short files gone
        by_path = {p: (r, d) for p, r, d in spec[subset]}
        off = 0
        for i, p in enumerate(ds.files[subset]):
            rate, data = by_path[p]
            n = len(data) if rate == 8000 else int(ceil(len(data) * 8000 / rate))
            assert ds.lengths[subset][i] == n and ds.offsets[subset][i] == off
            w = ds.pool_host[subset][off:off + n]
            ref = data if rate == 8000 else scipy.signal.resample(data, n)
            assert w.dtype == np.float32 and np.array_equal(w, np.asarray(ref, dtype=np.float32))   # stored scale
            assert ds.frames[subset][i] == P.num_frames(n, 256, 64)
            off += n
        assert len(ds.pool_host[subset]) == off
    # 353 samples at 11025 Hz -> ceil(353 * 8000 / 11025) = 257 >= FFT_SIZE: kept; 351 -> 255: skipped
    assert any(p.endswith('c.wav') for p in ds.files['train'])
    assert np.abs(ds.pool_host['train']).max() > 1000             # int16 scale, not normalised


def test_stereo_file_raises_and_names_the_file(hp, tmp_path):
    from danet_amd import datasets
    root = str(tmp_path / 'data')
    _small_tree(root)
    bad = os.path.join(root, 'test', 'a', 'stereo.wav')
    _write(bad, 8000, np.zeros((400, 2), np.int16))
    hp.load(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64))
    hp.digest()
    with pytest.raises(ValueError, match='stereo.wav'):
        datasets.WavDirData().load_host()


def test_valid_falls_back_to_test_and_missing_folders(hp, tmp_path):
    from danet_amd import datasets
    root = str(tmp_path / 'data')
    _small_tree(root, with_valid=False)
    hp.load(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64))
    hp.digest()
    ds = datasets.WavDirData()
    ds.load_host()
    assert ds.files['valid'] == ds.files['test'] and ds.pool_host['valid'] is ds.pool_host['test']
    for missing in ('test', 'train'):
        os.rename(os.path.join(root, missing), os.path.join(root, missing + '_gone'))
        with pytest.raises(IOError, match=missing):
            datasets.WavDirData().load_host()
        os.rename(os.path.join(root, missing + '_gone'), os.path.join(root, missing))
    # a subset with nothing usable in it is an error
    os.makedirs(os.path.join(root, 'valid'))
    _write(os.path.join(root, 'valid', 's.wav'), 8000, np.zeros(100, np.int16))
    with pytest.raises(IOError, match='no usable'):
        datasets.WavDirData().load_host()


# --------------------------------------------------------------------------------- batching plan
def _loaded(hp, tmp_path, n=11):
    from danet_amd import datasets
    root = str(tmp_path / 'plan')
    rng = np.random.RandomState(2)
    for subset in ('train', 'test'):
        for i in range(n):
            _write(os.path.join(root, subset, 'u%02d.wav' % i), 8000,
                   (rng.randn(300 + 97 * ((i * 5) % n)) * 2000).astype(np.int16))
    hp.load(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64, BATCH_SIZE=2,
                 MAX_N_SIGNAL=2, MAX_TRAIN_LEN=8))
    hp.digest()
    ds = datasets.WavDirData()
    ds.load_host(out=open(os.devnull, 'w'))
    return ds


def test_index_plan_is_the_reference_formula(hp, tmp_path):
    ds = _loaded(hp, tmp_path)
    plan = ds.plan_indices('train', 4, shuffle=False)
    assert plan.shape == (3, 4)
    assert plan.reshape(-1).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0]        # wrap-around of the last batch
    assert np.array_equal(plan, P.index_plan(11, 4, False))
    np.random.seed(7)
    a = ds.plan_indices('train', 4, shuffle=True)
    s1 = np.random.get_state()[1].copy()
    np.random.seed(7)
    b = P.index_plan(11, 4, True)
    assert np.array_equal(a, b) and np.array_equal(s1, np.random.get_state()[1])
    assert sorted(a.reshape(-1).tolist()) == sorted(list(range(11)) + [0])


def test_draw_order_equals_random_zeropad_plus_the_crop(hp, tmp_path):
    from danet_amd import utils
    ds = _loaded(hp, tmp_path)
    F = hp.FEATURE_SIZE
    plan = ds.plan_indices('train', 4, shuffle=False)
    for crop in (False, True):
        random.seed(11)
        got = [ds.plan_batch('train', idx, hp.MAX_TRAIN_LEN, crop=crop) for idx in plan]
        state = random.getstate()
        random.seed(11)
        for idx, (T_max, pads, beg, cnt) in zip(plan, got):
            frames = [int(ds.frames['train'][i]) for i in idx]
            assert T_max == max(frames)
            for t, p in zip(frames, pads):                      # the literal reference path
                X = utils.random_zeropad(np.ones((t, F), np.complex64), T_max - t, axis=-2)
                assert X.shape == (T_max, F)
                assert X[:, 0].real.tolist() == [0.] * p + [1.] * t + [0.] * (T_max - t - p)
            if crop:
                assert T_max > hp.MAX_TRAIN_LEN
                assert beg == random.randint(0, T_max - hp.MAX_TRAIN_LEN - 1) and cnt == hp.MAX_TRAIN_LEN
            else:
                assert (beg, cnt) == (0, T_max)
        assert random.getstate() == state
        # and the helper's independent restatement draws the same
        random.seed(11)
        for idx, (T_max, pads, beg, cnt) in zip(plan, got):
            assert P.draw_pads([int(ds.frames['train'][i]) for i in idx]) == (T_max, pads)
            if crop:
                assert P.draw_crop(T_max, hp.MAX_TRAIN_LEN) == (beg, cnt)
    # a batch of equal lengths draws nothing
    random.seed(3)
    s0 = random.getstate()
    ds.plan_batch('train', np.array([1, 1, 1, 1]))
    assert random.getstate() == s0


def test_epoch_and_epoch_device_advance_random_like_the_reference_path(hp, tmp_path, monkeypatch):
    '''the generators themselves (device half stubbed out): after each batch of epoch() python's `random` is where
    utils.random_zeropad would have left it, after each batch of epoch_device() where random_zeropad plus the
    crop draw of feed.to_batch_host would have; np.random is where the reference's shuffle leaves it'''
    import torch
    from danet_amd import ops, utils
    ds = _loaded(hp, tmp_path)
    ds.is_loaded = True
    F, bs, crop_len = hp.FEATURE_SIZE, hp.BATCH_SIZE * hp.MAX_N_SIGNAL, hp.MAX_TRAIN_LEN
    launches = []

    class Spectra(object):
        def __init__(self, n, t):
            self.shape = (n, t, F)

        def cpu(self):
            return torch.zeros(self.shape, dtype=torch.complex64)

    def fake_stft_batch(pool, desc, T_out, window, N, S, t_begin=0, t_count=None, out=None):
        launches.append((np.array(desc['pad_left']), T_out, t_begin, t_count))
        return Spectra(len(desc), t_count)

    def fake_emit(device, pool, window, ring, subset, idx, T_max, pads, beg, cnt):
        launches.append((np.array(pads), T_max, beg, cnt))
        return torch.zeros(len(idx), cnt, F, dtype=torch.complex64)

    monkeypatch.setattr(ops, 'stft_batch', fake_stft_batch)
    monkeypatch.setattr(ds, '_device', lambda device=None: 'stub')
    monkeypatch.setattr(ds, 'upload_pool', lambda subset, device: torch.zeros(len(ds.pool_host[subset])))
    monkeypatch.setattr(ds, '_window_on', lambda device: None)
    monkeypatch.setattr(ds, '_take_ring', lambda device, n: None)
    monkeypatch.setattr(ds, '_emit', fake_emit)

    def reference_states(crop):
        '''the literal path: shuffle, then per batch random_zeropad per utterance (+ the crop draw)'''
        np.random.seed(5)
        random.seed(6)
        states = []
        for idx in P.index_plan(11, bs, True):
            frames = [int(ds.frames['train'][i]) for i in idx]
            T_max = max(frames)
            for t in frames:
                utils.random_zeropad(np.zeros((t, 1)), T_max - t, axis=-2)
            if crop and T_max > crop_len:
                random.randint(0, T_max - crop_len - 1)
            states.append(random.getstate())
        return states, np.random.get_state()[1].copy()

    for crop in (False, True):
        want, want_np = reference_states(crop)
        np.random.seed(5)
        random.seed(6)
        del launches[:]
        it = ds.epoch_device('train', bs, True, 'stub', crop_len) if crop else ds.epoch('train', bs, True)
        got = []
        for batch in it:
            got.append(random.getstate())
            if crop:
                assert tuple(batch.shape) == (hp.BATCH_SIZE, hp.MAX_N_SIGNAL, launches[-1][3], F)
            else:
                assert batch[0].shape == (bs, launches[-1][1], F) and batch[0].dtype == np.complex64
        assert got == want and len(got) == 3 == len(launches)
        assert np.array_equal(np.random.get_state()[1], want_np)
        for pads, T_max, beg, cnt in launches:
            assert (beg, cnt) == (0, T_max) if not crop else cnt == min(crop_len, T_max)


def test_cli_route_selection(hp):
    '''open_feed: a dataset without epoch_device, a plain iterator and sync_feed all take BatchFeed'''
    from danet_amd import datasets, feed
    hp.digest()
    toy = datasets.WhiteNoiseData()
    toy.install_and_load()
    src = feed.EpochSource(toy, 'train', hp.BATCH_SIZE * hp.MAX_N_SIGNAL)
    assert src.device_batches('cpu') is None
    assert isinstance(feed.open_feed(src, 'cpu', 64, False), feed.BatchFeed)
    assert isinstance(feed.open_feed(iter([]), 'cpu', 64, False), feed.BatchFeed)

    class Fast(datasets.WhiteNoiseData):
        def epoch_device(self, subset, batch_size, shuffle=False, device=None, crop_len=None):
            return iter([(subset, batch_size, shuffle, str(device), crop_len)])
    fast = feed.EpochSource(Fast(), 'valid', 6, shuffle=True)
    assert list(feed.open_feed(fast, 'cpu', 64, False)) == [('valid', 6, True, 'cpu', 64)]
    assert feed.open_feed(fast, 'cpu', 64, True).mode == 'sync'
