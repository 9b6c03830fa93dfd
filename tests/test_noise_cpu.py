'''
CPU tests (no GPU) of the additive noise of the wavdir dataset (NOISE_DIR, NOISE_SNR_MIN, NOISE_SNR_MAX): the
extension library libdanet_noise_hip.so against its header (exports, prototypes, ABI, lazy load, host-visible argument
errors), the untouched other eight libraries, the open EXTENSIONS registry, the three configuration keys, the plan --
draw order, segments, gains, streams, what is left alone -- against the restatement tests/noise_ref.py, and the host
feed's NoisyBatch.
'''
import ctypes
import importlib
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mix_ref as M
import noise_ref as NR
import reverb_ref as RR
import speed_ref as SR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_noise_hip.h')
NOISE_SYMBOLS = ['danet_noise_abi_version', 'danet_noise_frontend_fwd', 'danet_noise_last_error']
KEYS = ('NOISE_DIR', 'NOISE_SNR_MIN', 'NOISE_SNR_MAX')


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_noise_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_noise()
    syms = _header_symbols('danet_noise_hip.h', 'danet_noise_')
    assert syms == NOISE_SYMBOLS
    assert sorted(_lib.NOISE_PROTOTYPES) == syms
    assert _exports(_lib.NOISE_LIB_PATH) == syms
    assert lib.danet_noise_abi_version() == 1 == _lib.NOISE_ABI_VERSION == _lib.NOISE.abi
    txt = open(HEADER).read()
    assert '#define DANET_NOISE_ABI_VERSION 1' in txt and '#define DANET_NOISE_MAX_C 8' in txt
    rule = txt.split('#ifndef')[0]
    for words in ('rng.randint(0, n_noise, size=B)', 'rng.random_sample(B)', 'rng.uniform(lo, hi, size=B)',
                  'subset index, 3', 'Lfull = (T_max - 1) * S', '10^(-snr / 20)'):
        assert words in rule, words
    assert _lib.NOISE.prototypes is _lib.NOISE_PROTOTYPES and _lib.NOISE.prefix == 'danet_noise_'


def test_noise_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int,
             'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.NOISE_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert len(_lib.NOISE_PROTOTYPES['danet_noise_frontend_fwd'][1]) == 12


def test_noise_is_appended_to_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.NOISE in _lib.EXTENSIONS and build.NOISE in build.EXTENSIONS
    assert isinstance(_lib.NOISE, _lib.Library) and isinstance(build.NOISE, build.Library)
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert _lib.NOISE not in older and build.NOISE not in build.LIBRARIES + build.LATER_LIBRARIES
    assert [lib.name for lib in _lib.EXTENSIONS] == [os.path.basename(spec.src_dir) for spec in build.EXTENSIONS]
    assert _lib.EXTENSIONS.index(_lib.NOISE) > _lib.EXTENSIONS.index(_lib.METRIC)       # appended
    assert build.NOISE_LIB == build.NOISE.out == _lib.NOISE_LIB_PATH
    assert os.path.basename(build.NOISE_LIB) == _lib.NOISE.so == 'libdanet_noise_hip.so'
    assert os.path.isfile(os.path.join(build.NOISE.src_dir, 'exports.map'))
    assert callable(build.build_noise) and callable(_lib.load_noise) and callable(_lib.noise_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        build.build(verbose=False)
        assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7 and rest == []
        del seven[:]
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES)
    assert build.METRIC in rest and build.NOISE in rest and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 9
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_eight_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + (_lib.METRIC,)
    assert [spec.name for spec in older] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed', 'reverb', 'metric']
    assert [spec.abi for spec in older] == [7, 1, 1, 1, 1, 1, 1, 1]
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_noise_') for s in exported), spec.so


def test_noise_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.NOISE_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree'):
        assert word not in out.stdout, word
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'noise')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['noise.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'noise.hip')).read(), flags=re.S)
    code += csrc_scan.shared_code(code)              # and the shared headers it includes, same words
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new '):
        assert word not in code, word
    assert 'fp contract(off)' in code                  # fl(g * n) is rounded before it is added


def test_import_and_a_run_with_the_keys_null_never_touch_the_library(tmp_path):
    root = str(tmp_path / 'lazy')
    _tree(root)
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "print('UNMAPPED:', _lib._noise is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "def boom():\n"
        "    raise AssertionError('load_noise called')\n"
        "real = _lib.load_noise; _lib.load_noise = boom\n"
        "hparams.load(json.loads(%r)); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.load_host(); ds.is_loaded = True\n"
        "plan = list(ds.plan_epoch_noise('train', 4, True, 8, crop=True))\n"
        "print('PLANNED:', len(plan), all(len(p) == 9 and p[8] is None for p in plan), ds.noise_on,\n"
        "      ds.noise_stream('train') is None, ds._noise_rng == {} and ds._noise_pool_dev == {})\n"
        "print('STILL:', _lib._noise is None and 'libdanet_noise' not in open('/proc/self/maps').read())\n"
        "_lib.load_noise = real; _lib.NOISE_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_noise()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_noise_hip.so' in str(e) and %r in str(e)\n"
        "          and 'NOISE_DIR' in str(e))\n"
        "print('NONE:', _lib._noise is None)\n"
    ) % (ROOT, json.dumps(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64, NOISE_DIR=None,
                               NOISE_SNR_MIN=None, NOISE_SNR_MAX=None)), nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'PLANNED: 3 True False True True', 'STILL: True', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_noise()
    ok = dict(stream=None, B=2, C=2, N=100, src=1024, noise=2048, gain=4096, mix_pwr=8192, mix_log=16384,
              phasor=32768, src_pwr=65536, mix=131072)
    cases = [(dict(B=0), b'B must'), (dict(B=-1), b'B must'), (dict(C=0), b'C must'), (dict(C=9), b'C must'),
             (dict(N=0), b'N must'), (dict(N=-5), b'N must'), (dict(N=1 << 40), b'N must'),
             (dict(B=1 << 30, C=8, N=(1 << 40) - 1), b'B * C * N'),
             (dict(src=None), b'null'), (dict(noise=None), b'null'), (dict(mix_pwr=None), b'null'),
             (dict(mix_log=None), b'null'), (dict(phasor=None), b'null'), (dict(src_pwr=None), b'null'),
             (dict(src=1028), b'misaligned'), (dict(noise=2052), b'misaligned'), (dict(phasor=32772), b'misaligned'),
             (dict(mix=131076), b'misaligned'), (dict(gain=4098), b'misaligned'), (dict(mix_pwr=8193), b'misaligned'),
             (dict(mix_log=16386), b'misaligned'), (dict(src_pwr=65537), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_noise_frontend_fwd(*a.values()) == -1, kw
        assert msg in lib.danet_noise_last_error(), (kw, lib.danet_noise_last_error())
    assert _lib.noise_check(0) is None
    assert lib.danet_noise_frontend_fwd(None, 1, 1, 1, None, None, None, None, None, None, None, None) == -1
    text = lib.danet_noise_last_error().decode()
    assert 'null' in text
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.noise_check(-1)
    assert str(e.value) == 'libdanet_noise_hip error -1: %s' % text


# ----------------------------------------------------------------------------------- configuration
def _write(path, data, rate=8000):
    import scipy.io.wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scipy.io.wavfile.write(path, rate, data)


def _tree(root, n=12):
    rng = np.random.RandomState(2)
    for subset in ('train', 'test'):
        for i in range(n):
            _write(os.path.join(root, subset, 'u%02d.wav' % i),
                   (rng.randn(300 + 97 * ((i * 5) % n)) * 20 * 3 ** (i % 6)).astype(np.int16))


# noise lengths at 8 kHz: below FFT_SIZE (skipped), exactly FFT_SIZE, short, long, one silent
NOISE_LENGTHS = (200, 256, 700, 5000, 1300, 9000, 3000)
SILENT = (4,)


def _noise_dir(tmp_path):
    d = str(tmp_path / 'noise')
    if not os.path.isdir(d):
        NR.write_noise(d, NOISE_LENGTHS, silent=SILENT)
    return d


def _loaded(hp, tmp_path, noise=True, **keys):
    '''a loaded dataset whose power tables come from the host restatement (no device)'''
    from danet_amd import datasets
    root = str(tmp_path / 'noisy')
    if not os.path.isdir(root):
        _tree(root)
    if noise:
        keys = dict(dict(NOISE_DIR=_noise_dir(tmp_path), NOISE_SNR_MIN=-5.0, NOISE_SNR_MAX=20.0), **keys)
    hp.load(dict(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64, BATCH_SIZE=2,
                      MAX_N_SIGNAL=2, MAX_TRAIN_LEN=8), **keys))
    hp.digest()
    ds = datasets.WavDirData()
    ds.load_host(out=open(os.devnull, 'w'))
    ds.is_loaded = True
    for subset in ('train', 'test'):
        ds.power[subset] = np.asarray([M.mean_power(ds.pool_host[subset][o:o + n])
                                       for o, n in zip(ds.offsets[subset], ds.lengths[subset])])
    if ds.noise_on:
        ds.noise_power = np.asarray([M.mean_power(ds.noise_pool_host[o:o + n])
                                     for o, n in zip(ds.noise_offsets, ds.noise_lengths)])
    return ds


def test_keys_default_to_null_and_off(hp):
    from danet_amd import datasets
    H = sys.modules['danet_amd.hparams']
    for key in KEYS:
        assert key in H.DEFAULTS and H.DEFAULTS[key] is None and getattr(hp, key) is None
        assert re.fullmatch(hp.pattern, key) and key in H.__doc__ and key in datasets.WavDirData.__doc__
    ds = datasets.WavDirData()
    assert datasets.WavDirData.noise_keys() == (None, None) and not ds.noise_on
    assert ds.noise_stream('train') is None


BAD = [
    (dict(NOISE_DIR=5, NOISE_SNR_MIN=0, NOISE_SNR_MAX=10), 'NOISE_DIR'),
    (dict(NOISE_DIR=True, NOISE_SNR_MIN=0, NOISE_SNR_MAX=10), 'NOISE_DIR'),
    (dict(NOISE_DIR='x', NOISE_SNR_MAX=10), 'NOISE_SNR_MIN'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=0), 'NOISE_SNR_MAX'),
    (dict(NOISE_DIR='x'), 'NOISE_SNR_M'),
    (dict(NOISE_SNR_MIN=0), 'NOISE_DIR'),
    (dict(NOISE_SNR_MAX=10), 'NOISE_DIR'),
    (dict(NOISE_SNR_MIN=0, NOISE_SNR_MAX=10), 'NOISE_DIR'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=True, NOISE_SNR_MAX=10), 'NOISE_SNR_MIN'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=0, NOISE_SNR_MAX=False), 'NOISE_SNR_MAX'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN='low', NOISE_SNR_MAX=10), 'NOISE_SNR_MIN'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=0, NOISE_SNR_MAX='high'), 'NOISE_SNR_MAX'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=-30.5, NOISE_SNR_MAX=10), 'NOISE_SNR_MIN'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=0, NOISE_SNR_MAX=60.5), 'NOISE_SNR_MAX'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=float('nan'), NOISE_SNR_MAX=10), 'NOISE_SNR_MIN'),
    (dict(NOISE_DIR='x', NOISE_SNR_MIN=12, NOISE_SNR_MAX=10), 'NOISE_SNR_MIN'),
]


@pytest.mark.parametrize('keys,named', BAD)
def test_bad_values_raise_and_name_the_key(hp, tmp_path, keys, named):
    from danet_amd import datasets
    root = str(tmp_path / 'noisy')
    _tree(root, n=2)
    hp.load(dict(dict(DATASET_TYPE='wavdir', DATASET_DIR=root), **keys))
    hp.digest()
    ds = datasets.WavDirData()
    with pytest.raises(ValueError, match=named):
        ds.install_and_load()
    assert not ds.is_loaded


def test_the_edges_of_the_range_are_accepted(hp):
    from danet_amd import datasets
    hp.load(dict(NOISE_DIR='x', NOISE_SNR_MIN=-30, NOISE_SNR_MAX=60))
    assert datasets.WavDirData.noise_keys() == ('x', (-30.0, 60.0))
    hp.load(dict(NOISE_DIR='x', NOISE_SNR_MIN=7, NOISE_SNR_MAX=7))
    assert datasets.WavDirData.noise_keys() == ('x', (7.0, 7.0))


def test_a_batch_size_that_is_no_multiple_of_the_sources_names_the_key(hp, tmp_path):
    ds = _loaded(hp, tmp_path)
    with pytest.raises(ValueError, match='NOISE_DIR') as e:
        next(iter(ds.plan_epoch_noise('train', 3)))
    assert 'MAX_N_SIGNAL' in str(e.value)
    assert len(list(ds.plan_epoch_noise('valid', 3))) == 4          # valid / test carry no noise: any batch size


def test_every_other_dataset_ignores_the_keys(hp):
    hp.load(dict(NOISE_DIR=7, NOISE_SNR_MIN='loud', NOISE_SNR_MAX=True))
    hp.digest()
    ds = hp.get_dataset()()
    ds.install_and_load()
    assert hp.DATASET_TYPE == 'toy' and next(iter(ds.epoch('train', 4)))[0].shape[0] == 4


def test_noise_files_are_loaded_like_the_datasets_own(hp, tmp_path, capsys):
    from danet_amd import datasets
    ds = _loaded(hp, tmp_path)
    want = sorted(fn for fn in datasets.WavDirData.discover(hp.NOISE_DIR) if 'noise00' not in fn)
    assert ds.noise_files == want and ds.noise_skipped == 1 and len(want) == len(NOISE_LENGTHS) - 1
    by_name = {os.path.basename(fn): int(n) for fn, n in zip(ds.noise_files, ds.noise_lengths)}
    assert by_name == {'noise%02d.wav' % i: L for i, L in enumerate(NOISE_LENGTHS) if i}      # resampled to SMPRATE
    assert ds.noise_pool_host.dtype == np.float32 and len(ds.noise_pool_host) == sum(NOISE_LENGTHS[1:])
    assert np.array_equal(ds.noise_offsets, np.concatenate([[0], np.cumsum(ds.noise_lengths)[:-1]]))
    for fn, o, n in zip(ds.noise_files, ds.noise_offsets, ds.noise_lengths):
        assert np.array_equal(ds.noise_pool_host[o:o + n], datasets.WavDirData.read_wave(fn))      # stored scale
    assert np.abs(ds.noise_pool_host).max() > 1000
    hp.reset()
    ds = None
    hp.load(dict(DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'noisy'), NOISE_DIR=_noise_dir(tmp_path),
                 NOISE_SNR_MIN=0, NOISE_SNR_MAX=5))
    hp.digest()
    capsys.readouterr()
    datasets.WavDirData().load_host()
    assert 'wavdir noise: 6 files, 1 shorter than FFT_SIZE skipped' in capsys.readouterr().out


def test_no_usable_noise_file_and_a_stereo_noise_file(hp, tmp_path):
    from danet_amd import datasets
    root = str(tmp_path / 'noisy')
    _tree(root, n=2)
    empty = str(tmp_path / 'short_only')
    _write(os.path.join(empty, 'a.wav'), np.zeros(100, np.int16))
    keys = dict(DATASET_TYPE='wavdir', DATASET_DIR=root, NOISE_SNR_MIN=0, NOISE_SNR_MAX=5)
    for folder in (empty, str(tmp_path / 'missing')):
        hp.load(dict(keys, NOISE_DIR=folder))
        hp.digest()
        with pytest.raises(IOError, match='NOISE_DIR'):
            datasets.WavDirData().install_and_load()
    stereo = str(tmp_path / 'stereo')
    _write(os.path.join(stereo, 'two.wav'), np.zeros((400, 2), np.int16))
    hp.load(dict(keys, NOISE_DIR=stereo))
    with pytest.raises(ValueError, match='two.wav'):
        datasets.WavDirData().install_and_load()


# ------------------------------------------------------------------------------------------ the plan
def _tables(lengths, powers):
    lengths = np.asarray(lengths, np.int64)
    return np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) + 17, lengths, np.asarray(powers, np.float64)


def _same(got, ref):
    assert np.array_equal(got.files, ref['files']) and np.array_equal(got.snr, ref['snr'])
    assert np.array_equal(got.offsets, ref['offsets']) and np.array_equal(got.lengths, ref['lengths'])
    assert np.array_equal(got.pads, ref['pads'])
    assert got.offsets.dtype == got.lengths.dtype == got.pads.dtype == np.int64
    assert got.gains.dtype == np.float32 and np.array_equal(got.gains.view(np.uint32), ref['gains'].view(np.uint32))
    assert np.array_equal(got.gains64, ref['gains64'])


@pytest.mark.parametrize('N,S', [(256, 64), (512, 128), (256, 48)])
def test_full_length_has_exactly_t_max_frames(N, S):
    from danet_amd import datasets
    for L in (N, N + 1, N + S - 1, N + S, 5 * N + 7, 12345):
        T_max = datasets._stft_frames(L, N, S)
        assert T_max == NR.num_frames(L, N, S)
        Lfull = NR.full_length(T_max, S)
        assert datasets._stft_frames(Lfull, N, S) == T_max == NR.num_frames(Lfull, N, S) and Lfull >= N
        assert datasets._stft_frames(Lfull + 1, N, S) == T_max + 1


def test_draw_order_and_counts():
    from danet_amd import datasets
    off, lens, pw = _tables([3000, 400, 9000], [4.0, 9.0, 2.5])
    rng = NR.RecordingRandomState(7)
    random.seed(1)
    np.random.seed(2)
    s0, n0 = random.getstate(), np.random.get_state()[1].copy()
    got = datasets.WavDirData.plan_noise(np.arange(1, 13, dtype=np.float64), None, rng, 3, off, lens, pw, 20, -5, 10,
                                         256, 64)
    assert rng.calls == [('randint', 4), ('random_sample', 4), ('uniform', 4)]
    assert random.getstate() == s0 and np.array_equal(np.random.get_state()[1], n0)
    _same(got, NR.plan(np.arange(1, 13, dtype=np.float64), None, np.random.RandomState(7), 3, off, lens, pw, 20, -5,
                       10, 256, 64))
    assert len(got.gains) == 4 and -5 <= got.snr.min() and got.snr.max() <= 10


@pytest.mark.parametrize('N,S', [(256, 64), (256, 48)])
@pytest.mark.parametrize('u', [0.0, 0.37, 1.0 - 2.0 ** -53])
def test_both_segment_cases_and_their_edges(N, S, u):
    from danet_amd import datasets
    T_max = 30
    Lfull = NR.full_length(T_max, S)
    lens = [Lfull, Lfull - 1, N, Lfull + 1, 4 * Lfull, N + S + 3]
    off, lens, pw = _tables(lens, [1.0] * len(lens))
    seen = set()
    for seed in range(12):
        got = datasets.WavDirData.plan_noise(np.ones(8), None, NR.RecordingRandomState(seed, u), 2, off, lens, pw, T_max,
                                             0, 0, N, S)
        _same(got, NR.plan(np.ones(8), None, NR.RecordingRandomState(seed, u), 2, off, lens, pw, T_max, 0, 0, N, S))
        for b, f in enumerate(got.files):
            seen.add(int(f))
            Ln, o = int(lens[f]), int(off[f])
            if Ln >= Lfull:                   # a cut: exactly Lfull samples inside the file, no pad
                assert got.lengths[b] == Lfull and got.pads[b] == 0
                assert o <= got.offsets[b] and got.offsets[b] + Lfull <= o + Ln
                assert got.offsets[b] - o == (0 if u == 0 else (Ln - Lfull if u > 0.9 else int(u * (Ln - Lfull + 1))))
            else:                             # the whole file, inside the T_max frames
                T_n = NR.num_frames(Ln, N, S)
                assert (got.offsets[b], got.lengths[b]) == (o, Ln)
                assert 0 <= got.pads[b] and got.pads[b] + T_n <= T_max
                assert got.pads[b] == (0 if u == 0 else (T_max - T_n if u > 0.9 else int(u * (T_max - T_n + 1))))
    assert seen == set(range(len(lens)))


def test_gains_bit_for_bit_zero_for_silence_and_the_realised_snr():
    from danet_amd import datasets
    off, lens, pw = _tables([3000, 400, 9000, 800], [4.0e5, 9.0, 0.0, 2.5e7])
    rng0 = np.random.RandomState(3)
    powers = 10.0 ** rng0.uniform(0, 7, size=16)
    powers[4:6] = 0.0                                         # one silent mixture
    mix_gains = (10.0 ** rng0.uniform(-1, 1, size=16)).astype(np.float32)
    zero_file = zero_mix = checked = 0
    for seed in range(10):
        for gains in (None, mix_gains):
            got = datasets.WavDirData.plan_noise(powers, gains, np.random.RandomState(seed), 2, off, lens, pw, 25, -30,
                                                 60, 256, 64)
            _same(got, NR.plan(powers, gains, np.random.RandomState(seed), 2, off, lens, pw, 25, -30, 60, 256, 64))
            for b in range(8):
                rows = powers[2 * b:2 * b + 2]
                g_rows = None if gains is None else gains[2 * b:2 * b + 2]
                if pw[got.files[b]] == 0.0 or not rows.any():
                    assert got.gains[b] == 0.0 and got.gains64[b] == 0.0
                    zero_file += pw[got.files[b]] == 0.0
                    zero_mix += not rows.any()
                    continue
                real = NR.realised_snr(rows, g_rows, pw[got.files[b]], float(got.gains64[b]))
                assert abs(real - got.snr[b]) <= 1e-9, (real, got.snr[b])
                assert got.gains[b] == np.float32(got.gains64[b]) and got.gains[b] > 0
                checked += 1
    assert zero_file and zero_mix and checked > 80


# ------------------------------------------------------------------------------------------ streams
def _plan(ds, subset, shuffle=False):
    return [tuple(None if f is None else (f.copy() if isinstance(f, np.ndarray) else f) for f in item)
            for item in ds.plan_epoch_noise(subset, 4, shuffle, 8, crop=True)]


def test_keys_set_leave_every_other_stream_alone_and_the_train_stream_runs_on(hp, tmp_path):
    others = dict(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0, SPEED_PERTURB_RANGE=0.1, REVERB_RT60_MAX=0.3)

    def run(noise):
        hp.reset()
        ds = _loaded(hp, tmp_path, noise=noise, **others)
        random.seed(11)
        np.random.seed(12)
        plan = _plan(ds, 'train', shuffle=True) + _plan(ds, 'train', shuffle=True)
        return plan, random.getstate(), np.random.get_state()[1].copy(), ds
    off, r0, n0, _ = run(False)
    on, r1, n1, ds = run(True)
    assert r0 == r1 and np.array_equal(n0, n1)                     # `random` and np.random: as without the keys
    assert len(off) == len(on) == 6
    rng = NR.stream(0, 'train')                                    # ONE stream, on across both epochs
    srng, rrng = SR.stream(0, 'train'), RR.stream(0, 'train')
    for a, b in zip(off, on):
        assert len(a) == len(b) == 9 and a[8] is None
        assert np.array_equal(a[0], b[0]) and a[1:5] == b[1:5]
        assert np.array_equal(a[5], b[5])                          # the mix draws
        assert np.array_equal(a[6][0], b[6][0]) and np.array_equal(a[6][1], b[6][1])       # the speed draws
        assert np.array_equal(a[7], b[7])                          # the reverb draws
        assert np.array_equal(b[6][0], SR.draw(ds.lengths['train'][b[0]], srng, 0.1, 256)[0])
        assert np.array_equal(b[7], RR.draw(4, rrng))
        # P_c: the STORED files' powers; g_c: the float32 mix gains of the batch
        _same(b[8], NR.plan(ds.power['train'][b[0]], b[5], rng, 2, ds.noise_offsets, ds.noise_lengths, ds.noise_power,
                            b[1], -5.0, 20.0, 256, 64))
        assert len(b[8].gains) == 2
    assert not all(np.array_equal(x[8].files, y[8].files) and np.array_equal(x[8].snr, y[8].snr)
                   for x, y in zip(on[:3], on[3:]))
    # the eight-field and shorter generators keep their shapes
    random.seed(11)
    np.random.seed(12)
    assert all(len(item) == 8 for item in ds.plan_epoch_reverb('train', 4, True, 8, crop=True))
    assert all(len(item) == 7 for item in ds.plan_epoch_speed('train', 4, True, 8, crop=True))
    assert all(len(item) == 6 for item in ds.plan_epoch('train', 4, True, 8, crop=True))


def test_gains_are_one_with_the_mix_keys_null(hp, tmp_path):
    ds = _loaded(hp, tmp_path)
    rng = NR.stream(0, 'train')
    for b in _plan(ds, 'train'):
        assert b[5] is None
        _same(b[8], NR.plan(ds.power['train'][b[0]], None, rng, 2, ds.noise_offsets, ds.noise_lengths, ds.noise_power,
                            b[1], -5.0, 20.0, 256, 64))


def test_valid_and_test_carry_no_noise_and_ranks_differ(hp, tmp_path, monkeypatch):
    from danet_amd import dist
    ds0 = _loaded(hp, tmp_path)
    hp.reset()
    ds = _loaded(hp, tmp_path, noise=False)
    for subset in ('valid', 'test'):
        assert ds0.noise_stream(subset) is None
        random.seed(4)
        without = _plan(ds, subset)
        random.seed(4)
        with_keys = _plan(ds0, subset)
        assert all(item[8] is None for item in with_keys)
        for a, b in zip(without, with_keys):
            assert np.array_equal(a[0], b[0]) and a[1:5] == b[1:5]
    assert ds0._noise_rng == {}
    hp.reset()
    ds0 = _loaded(hp, tmp_path)
    a = _plan(ds0, 'train')
    monkeypatch.setattr(dist, 'rank', lambda: 1)
    ds1 = _loaded(hp, tmp_path)
    b = _plan(ds1, 'train')
    assert not all(np.array_equal(x[8].snr, y[8].snr) for x, y in zip(a, b))
    rng = NR.stream(1, 'train')
    for x in b:
        assert np.array_equal(x[8].snr, NR.plan(ds1.power['train'][x[0]], None, rng, 2, ds1.noise_offsets,
                                                ds1.noise_lengths, ds1.noise_power, x[1], -5.0, 20.0, 256, 64)['snr'])


def test_the_generators_with_the_device_half_stubbed(hp, tmp_path, monkeypatch):
    '''epoch() yields (spectra, noise), epoch_device() a NoisyBatch, and both leave python's `random` and np.random
    where the run without the keys leaves them; `valid` yields what it always did'''
    import torch
    from danet_amd import feed, ops
    F = 129

    def run(noise, route):
        hp.reset()
        ds = _loaded(hp, tmp_path, noise=noise)
        launches = []

        class Spectra(object):
            def __init__(self, n, t):
                self.shape = (n, t, F)

            def cpu(self):
                return torch.zeros(self.shape, dtype=torch.complex64)

        def fake_stft_batch(pool, desc, T_out, window, N, S, t_begin=0, t_count=None, out=None):
            launches.append((len(desc), T_out, t_begin, t_count))
            return Spectra(len(desc), t_count)

        def fake_emit(device, pool, window, ring, subset, idx, T_max, pads, beg, cnt, noise=None):
            out = torch.zeros(len(idx), cnt, F, dtype=torch.complex64)
            if noise is None:
                return out
            return out, torch.zeros(len(noise.gains), cnt, F, dtype=torch.complex64), torch.as_tensor(noise.gains)

        monkeypatch.setattr(ops, 'stft_batch', fake_stft_batch)
        monkeypatch.setattr(ops, 'mix_scale_', lambda batch, gains: batch)
        monkeypatch.setattr(ds, '_device', lambda device=None: 'cpu')
        monkeypatch.setattr(ds, 'upload_pool', lambda subset, device: torch.zeros(len(ds.pool_host[subset])))
        monkeypatch.setattr(ds, 'upload_noise', lambda device: torch.zeros(len(ds.noise_pool_host)))
        monkeypatch.setattr(ds, 'power_table', lambda subset, pool: None)
        monkeypatch.setattr(ds, '_window_on', lambda device: None)
        monkeypatch.setattr(ds, '_take_ring', lambda device, n: None)
        monkeypatch.setattr(ds, '_emit', fake_emit)
        random.seed(6)
        np.random.seed(5)
        if route == 'device':
            got = list(ds.epoch_device('train', 4, True, 'stub', 8)) + list(ds.epoch_device('valid', 4, False, 'stub'))
        else:
            got = list(ds.epoch('train', 4, True)) + list(ds.epoch('valid', 4, False))
        return got, random.getstate(), np.random.get_state()[1].copy(), launches

    for route in ('device', 'host'):
        off, r0, n0, l0 = run(False, route)
        on, r1, n1, l1 = run(True, route)
        assert r0 == r1 and np.array_equal(n0, n1) and len(off) == len(on) == 6
        for k, (a, b) in enumerate(zip(off, on)):
            if route == 'device':
                assert torch.is_tensor(a) and a.dim() == 4
                if k < 3:
                    assert isinstance(b, feed.NoisyBatch) and tuple(b.src.shape) == tuple(a.shape)
                    assert tuple(b.noise.shape) == (2,) + tuple(a.shape[2:]) and tuple(b.gain.shape) == (2,)
                else:
                    assert torch.is_tensor(b) and tuple(b.shape) == tuple(a.shape)
            else:
                assert len(a) == 1 and len(b) == (2 if k < 3 else 1) and b[0].shape == a[0].shape
                if k < 3:
                    assert b[1].shape == (2,) + a[0].shape[1:] and b[1].dtype == np.complex64
        if route == 'host':                   # one more STFT launch per TRAIN batch, over all T_max frames
            assert len(l1) == len(l0) + 3
            assert [x for x in l1 if x[0] == 2] == [(2, x[1], 0, x[1]) for x in l0[:3]]


# ------------------------------------------------------------------------------------------ the feed
@pytest.mark.parametrize('mode', ['sync', 'ahead'])
def test_batchfeed_carries_the_noise_through_the_same_crop(hp, mode, monkeypatch):
    import torch
    from danet_amd import feed
    hp.load(dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=8))
    hp.digest()
    F, T, crop = hp.FEATURE_SIZE, 11, 4
    rng = np.random.RandomState(0)
    pts = []
    for _ in range(3):
        src = (rng.randn(4, T, F) + 1j * rng.randn(4, T, F)).astype(np.complex64)
        noise = (rng.randn(2, T, F) + 1j * rng.randn(2, T, F)).astype(np.complex64)
        pts.append((src, noise))
    pts.append((pts[0][0],))                                       # a plain data point still comes out as a tensor
    draws = []
    real = feed.randint

    def counting(a, b):
        draws.append(real(a, b))
        return draws[-1]
    monkeypatch.setattr(feed, 'randint', counting)
    random.seed(9)
    got = []
    for item in feed.BatchFeed(iter(pts), 'cpu', crop, mode=mode):
        got.append(feed.NoisyBatch(*[None if t is None else t.clone() for t in item])
                   if isinstance(item, feed.NoisyBatch) else item.clone())
    assert len(got) == 4 and len(draws) == 4                       # exactly ONE draw per batch
    random.seed(9)
    for k, (pt, item) in enumerate(zip(pts, got)):
        beg = random.randint(0, T - crop - 1)
        assert beg == draws[k]
        want = pt[0].reshape(2, 2, T, F)[:, :, beg:beg + crop]
        if k == 3:
            assert torch.is_tensor(item) and np.array_equal(item.numpy(), want)
            continue
        assert isinstance(item, feed.NoisyBatch) and item.gain is None and item._fields == ('src', 'noise', 'gain')
        assert item.src.dtype == item.noise.dtype == torch.complex64
        assert item.src.is_contiguous() and item.noise.is_contiguous()
        assert np.array_equal(item.src.numpy(), want)
        assert np.array_equal(item.noise.numpy(), pt[1][:, beg:beg + crop])       # the SAME offset


def test_train_epoch_unpacks_a_noisy_batch():
    import io
    import torch
    from danet_amd import cli, feed
    calls = []

    class FakeModel(object):
        device = 'cpu'

        def train_step(self, src, sync_metrics=True, s_noise=None, s_noise_gain=None):
            calls.append((src, s_noise, s_noise_gain))
            return dict(loss=1.0)

        def reset_state(self):
            pass

    a, n, g = torch.zeros(1), torch.ones(1), torch.full((1,), 2.0)
    real = feed.open_feed
    try:
        feed.open_feed = lambda batches, device, crop_len, sync_feed: iter(batches)
        rep, k = cli.train_epoch(FakeModel(), [a, feed.NoisyBatch(a, n, g), feed.NoisyBatch(a, n, None)], io.StringIO())
    finally:
        feed.open_feed = real
    assert k == 3 and rep['loss'] == 1.0
    assert calls[0] == (a, None, None) and calls[1] == (a, n, g) and calls[2] == (a, n, None)
