'''
CPU tests (no GPU) of noisy evaluation (NOISE_EVAL_DIR, NOISE_EVAL_SNR_MIN, NOISE_EVAL_SNR_MAX): the extension library
libdanet_neval_hip.so against its header (exports, prototypes, ABI, lazy load, host-visible argument errors), the
untouched older libraries, the open EXTENSIONS registry and build_all, the three configuration keys, the evaluation
plan -- draw order, segments, gains, the stream that starts anew with every sweep, what is left alone -- against the
restatement tests/noise_ref.py, and known answers of the restatement tests/neval_ref.py.
'''
import ctypes
import importlib
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import metric_ref as MR
import mix_ref as M
import neval_ref as NV
import noise_ref as NR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_neval_hip.h')
NEVAL_SYMBOLS = ['danet_neval_abi_version', 'danet_neval_gram', 'danet_neval_last_error', 'danet_neval_si_sdr',
                 'danet_neval_synth', 'danet_neval_workspace_bytes']
KEYS = ('NOISE_EVAL_DIR', 'NOISE_EVAL_SNR_MIN', 'NOISE_EVAL_SNR_MAX')


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


def _sqrt_hann(N):
    import scipy.signal
    return np.sqrt(scipy.signal.windows.hann(N)).astype(np.float32)


# ------------------------------------------------------------------------------------------ ABI
def test_neval_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_neval()
    syms = _header_symbols('danet_neval_hip.h', 'danet_neval_')
    assert syms == NEVAL_SYMBOLS
    assert sorted(_lib.NEVAL_PROTOTYPES) == syms
    assert _exports(_lib.NEVAL_LIB_PATH) == syms
    assert lib.danet_neval_abi_version() == 1 == _lib.NEVAL_ABI_VERSION == _lib.NEVAL.abi
    txt = open(HEADER).read()
    assert '#define DANET_NEVAL_ABI_VERSION 1' in txt and '#define DANET_NEVAL_MAX_C 4' in txt
    rule = txt.split('#ifndef')[0]
    for words in ('<m, m>   = (cc + 2 cn) + nn', 'rounded ON ITS OWN', '10 log10(cc / nn)', '(0, 0, 0)'):
        assert words in rule, words
    assert _lib.NEVAL.prototypes is _lib.NEVAL_PROTOTYPES and _lib.NEVAL.prefix == 'danet_neval_'


def test_neval_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'const float*': ctypes.c_void_p,
             'float*': ctypes.c_void_p, 'const double*': ctypes.c_void_p, 'double*': ctypes.c_void_p,
             'int32_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.NEVAL_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert len(_lib.NEVAL_PROTOTYPES['danet_neval_synth'][1]) == 12


def test_neval_is_appended_to_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.NEVAL in _lib.EXTENSIONS and build.NEVAL in build.EXTENSIONS
    assert isinstance(_lib.NEVAL, _lib.Library) and isinstance(build.NEVAL, build.Library)
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert _lib.NEVAL not in older and build.NEVAL not in build.LIBRARIES + build.LATER_LIBRARIES
    assert [lib.name for lib in _lib.EXTENSIONS] == [os.path.basename(spec.src_dir) for spec in build.EXTENSIONS]
    assert _lib.EXTENSIONS.index(_lib.NEVAL) > _lib.EXTENSIONS.index(_lib.DPCL)          # appended
    assert build.NEVAL_LIB == build.NEVAL.out == _lib.NEVAL_LIB_PATH
    assert os.path.basename(build.NEVAL_LIB) == _lib.NEVAL.so == 'libdanet_neval_hip.so'
    assert os.path.isfile(os.path.join(build.NEVAL.src_dir, 'exports.map'))
    assert callable(build.build_neval) and callable(_lib.load_neval) and callable(_lib.neval_check)
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
    for spec in (build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL):
        assert spec in rest
    assert not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 14
    assert all(os.path.isfile(out) for out in outs)


def test_every_older_library_is_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + tuple(s for s in _lib.EXTENSIONS if s is not _lib.NEVAL)
    assert [spec.name for spec in older] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed', 'reverb', 'metric', 'noise',
                                             'level', 'wavloss', 'gclip', 'dpcl']
    assert [spec.abi for spec in older] == [7] + [1] * 12
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_neval_') for s in exported), spec.so


def test_neval_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.NEVAL_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree'):
        assert word not in out.stdout, word
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'neval')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['neval.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'neval.hip')).read(), flags=re.S)
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic'):
        assert word not in code, word
    assert 'fp contract(off)' in code                  # fl(g * z) is rounded before the split step adds it
    shared = csrc_scan.shared_code(code)               # wave_metric.h, ext_core.h
    assert '#include "wave_metric.h"' in code and '#include "ext_core.h"' in code
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic'):
        assert word not in shared, word


def test_import_maps_nothing_and_a_missing_file_is_a_loud_error(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, datasets, feed, cli\n"
        "print('UNMAPPED:', _lib._neval is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "_lib.NEVAL_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_neval()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_neval_hip.so' in str(e) and %r in str(e)\n"
        "          and 'NOISE_EVAL_DIR' in str(e))\n"
        "print('NONE:', _lib._neval is None)\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'UNMAPPED: True' in out.stdout and 'LOUD: True' in out.stdout and 'NONE: True' in out.stdout, \
        out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_neval()
    ok = dict(stream=None, B=2, C=2, T=9, N=256, S=64, ref=1024, est=2048, noise=16384, gain=32768, window=4096,
              wav=8192)
    cases = [(dict(T=1), b'T must be >= 2'), (dict(T=0), b'T must'), (dict(N=192), b'power of two'),
             (dict(N=32, S=8), b'power of two'), (dict(N=2048, S=512), b'power of two'), (dict(S=129), b'S must'),
             (dict(S=31), b'S must'), (dict(S=0), b'S must'), (dict(B=0), b'B and C'), (dict(C=0), b'B and C'),
             (dict(ref=None), b'null'), (dict(est=None), b'null'), (dict(noise=None), b'null'),
             (dict(window=None), b'null'), (dict(wav=None), b'null'),
             (dict(ref=1028), b'misaligned'), (dict(est=2052), b'misaligned'), (dict(noise=16388), b'misaligned'),
             (dict(gain=32770), b'misaligned'), (dict(window=4098), b'misaligned'), (dict(wav=8193), b'misaligned'),
             (dict(T=1 << 30, S=64), b'2^31')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_neval_synth(*a.values()) == -1, kw
        assert msg in lib.danet_neval_last_error(), (kw, lib.danet_neval_last_error())
    ok = dict(stream=None, B=2, M=5, Ls=100, wav=1024, G=2048)
    for kw, msg in [(dict(B=0), b'B must'), (dict(M=0), b'M must'), (dict(M=10), b'M must'), (dict(Ls=0), b'Ls must'),
                    (dict(Ls=1 << 31), b'Ls must'), (dict(wav=None), b'null'), (dict(G=None), b'null'),
                    (dict(wav=1026), b'misaligned'), (dict(G=2052), b'misaligned')]:
        a = dict(ok, **kw)
        assert lib.danet_neval_gram(*a.values()) == -1, kw
        assert msg in lib.danet_neval_last_error(), (kw, lib.danet_neval_last_error())
    ok = dict(stream=None, B=2, C=2, G=1024, per_utt=2048, perm_idx=4096, mean3=8192)
    for kw, msg in [(dict(B=0), b'B must'), (dict(C=0), b'C must'), (dict(C=5), b'C must'), (dict(G=None), b'null'),
                    (dict(per_utt=None), b'null'), (dict(perm_idx=None), b'null'), (dict(mean3=None), b'null'),
                    (dict(G=1028), b'misaligned'), (dict(per_utt=2052), b'misaligned'),
                    (dict(mean3=8196), b'misaligned'), (dict(perm_idx=4098), b'misaligned')]:
        a = dict(ok, **kw)
        assert lib.danet_neval_si_sdr(*a.values()) == -1, kw
        assert msg in lib.danet_neval_last_error(), (kw, lib.danet_neval_last_error())
    # the layout the header gives: five parts, each rounded up to a multiple of 256 bytes
    r = lambda n: (n + 255) & ~255
    for B, C, T, N, S in ((32, 2, 128, 256, 64), (1, 1, 2, 64, 32), (3, 4, 130, 1024, 128)):
        Ls, Mr = (T - 1) * S, 2 * C + 1
        want = r(B * Mr * Ls * 4) + r(B * Mr * Mr * 8) + r(B * 24) + r(24) + r(B * 4)
        assert lib.danet_neval_workspace_bytes(B, C, T, N, S) == want
    bad = ctypes.c_size_t(-1).value
    for args in ((1, 5, 9, 256, 64), (1, 1, 1, 256, 64), (1, 1, 9, 100, 25), (1, 1, 9, 256, 192), (0, 1, 9, 256, 64)):
        assert lib.danet_neval_workspace_bytes(*args) == bad, args
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.neval_check(-1)
    assert str(e.value).startswith('libdanet_neval_hip error -1: ')
    assert _lib.neval_check(0) is None


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
EVAL_LENGTHS = (4000, 300, 150, 8000, 1100)
SILENT = (4,)


def _noise_dir(tmp_path, name='noise', lengths=NOISE_LENGTHS, seed=5, silent=SILENT):
    d = str(tmp_path / name)
    if not os.path.isdir(d):
        NR.write_noise(d, lengths, seed=seed, silent=silent)
    return d


def _eval_keys(tmp_path):
    return dict(NOISE_EVAL_DIR=_noise_dir(tmp_path, 'held_out', EVAL_LENGTHS, seed=9, silent=()),
                NOISE_EVAL_SNR_MIN=0.0, NOISE_EVAL_SNR_MAX=15.0)


def _train_keys(tmp_path):
    return dict(NOISE_DIR=_noise_dir(tmp_path), NOISE_SNR_MIN=-5.0, NOISE_SNR_MAX=20.0)


def _loaded(hp, tmp_path, **keys):
    '''a loaded dataset whose power tables come from the host restatement (no device)'''
    from danet_amd import datasets
    root = str(tmp_path / 'noisy')
    if not os.path.isdir(root):
        _tree(root)
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
    if ds.noise_eval_on:
        ds.noise_eval_power = np.asarray([M.mean_power(ds.noise_eval_pool_host[o:o + n])
                                          for o, n in zip(ds.noise_eval_offsets, ds.noise_eval_lengths)])
    return ds


def test_keys_default_to_null_and_off(hp):
    from danet_amd import datasets
    H = sys.modules['danet_amd.hparams']
    for key in KEYS:
        assert key in H.DEFAULTS and H.DEFAULTS[key] is None and getattr(hp, key) is None
        assert re.fullmatch(hp.pattern, key) and key in H.__doc__ and key in datasets.WavDirData.__doc__
    ds = datasets.WavDirData()
    assert datasets.WavDirData.noise_eval_keys() == (None, None) and not ds.noise_eval_on
    assert all(ds.noise_eval_stream(s) is None for s in ('train', 'valid', 'test'))
    assert not any(ds.noisy(s) for s in ('train', 'valid', 'test'))


BAD = [
    (dict(NOISE_EVAL_DIR=5, NOISE_EVAL_SNR_MIN=0, NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_DIR'),
    (dict(NOISE_EVAL_DIR=True, NOISE_EVAL_SNR_MIN=0, NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_DIR'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_SNR_MIN'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=0), 'NOISE_EVAL_SNR_MAX'),
    (dict(NOISE_EVAL_DIR='x'), 'NOISE_EVAL_SNR_M'),
    (dict(NOISE_EVAL_SNR_MIN=0), 'NOISE_EVAL_DIR'),
    (dict(NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_DIR'),
    (dict(NOISE_EVAL_SNR_MIN=0, NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_DIR'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=True, NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_SNR_MIN'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=0, NOISE_EVAL_SNR_MAX=False), 'NOISE_EVAL_SNR_MAX'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN='low', NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_SNR_MIN'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=0, NOISE_EVAL_SNR_MAX='high'), 'NOISE_EVAL_SNR_MAX'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=-30.5, NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_SNR_MIN'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=0, NOISE_EVAL_SNR_MAX=60.5), 'NOISE_EVAL_SNR_MAX'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=float('nan'), NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_SNR_MIN'),
    (dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=12, NOISE_EVAL_SNR_MAX=10), 'NOISE_EVAL_SNR_MIN'),
]


@pytest.mark.parametrize('keys,named', BAD)
def test_bad_values_raise_and_name_the_key(hp, tmp_path, keys, named):
    from danet_amd import datasets
    root = str(tmp_path / 'noisy')
    _tree(root, n=2)
    hp.load(dict(dict(DATASET_TYPE='wavdir', DATASET_DIR=root), **keys))
    hp.digest()
    ds = datasets.WavDirData()
    with pytest.raises(ValueError, match=r'hparams\.' + named) as e:
        ds.install_and_load()
    assert not ds.is_loaded
    # the message speaks of the eval family alone: no train key is named
    assert not re.search(r'NOISE_(DIR|SNR_MIN|SNR_MAX)\b', str(e.value).replace('NOISE_EVAL_', ''))


def test_the_edges_of_the_range_and_the_independence_of_the_two_families(hp, tmp_path):
    from danet_amd import datasets
    hp.load(dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=-30, NOISE_EVAL_SNR_MAX=60))
    assert datasets.WavDirData.noise_eval_keys() == ('x', (-30.0, 60.0))
    assert datasets.WavDirData.noise_keys() == (None, None)
    hp.load(dict(NOISE_EVAL_DIR='x', NOISE_EVAL_SNR_MIN=7, NOISE_EVAL_SNR_MAX=7))
    assert datasets.WavDirData.noise_eval_keys() == ('x', (7.0, 7.0))
    hp.reset()
    hp.load(dict(NOISE_DIR='y', NOISE_SNR_MIN=1, NOISE_SNR_MAX=2))
    assert datasets.WavDirData.noise_eval_keys() == (None, None)
    assert datasets.WavDirData.noise_keys() == ('y', (1.0, 2.0))
    hp.reset()
    # the two folders may be the same path: two pools all the same
    d = _noise_dir(tmp_path)
    ds = _loaded(hp, tmp_path, NOISE_DIR=d, NOISE_SNR_MIN=0, NOISE_SNR_MAX=5, NOISE_EVAL_DIR=d, NOISE_EVAL_SNR_MIN=10,
                 NOISE_EVAL_SNR_MAX=10)
    assert ds.noise_files == ds.noise_eval_files and ds.noise_snr == (0.0, 5.0) and ds.noise_eval_snr == (10.0, 10.0)
    assert ds.noise_pool_host is not ds.noise_eval_pool_host
    assert np.array_equal(ds.noise_pool_host, ds.noise_eval_pool_host)


def test_a_batch_size_that_is_no_multiple_of_the_sources_names_the_key(hp, tmp_path):
    ds = _loaded(hp, tmp_path, **_eval_keys(tmp_path))
    for subset in ('valid', 'test'):
        with pytest.raises(ValueError, match='NOISE_EVAL_DIR') as e:
            next(iter(ds.plan_epoch_noise(subset, 3)))
        assert 'MAX_N_SIGNAL' in str(e.value)
    assert len(list(ds.plan_epoch_noise('train', 3))) == 4          # train carries no noise here: any batch size


def test_every_other_dataset_ignores_the_keys(hp):
    hp.load(dict(NOISE_EVAL_DIR=7, NOISE_EVAL_SNR_MIN='loud', NOISE_EVAL_SNR_MAX=True))
    hp.digest()
    ds = hp.get_dataset()()
    ds.install_and_load()
    assert hp.DATASET_TYPE == 'toy' and next(iter(ds.epoch('train', 4)))[0].shape[0] == 4


def test_active_level_with_the_eval_folder_alone_is_valid(hp, tmp_path):
    from danet_amd import datasets
    ds = _loaded(hp, tmp_path, MIX_LEVEL_MEASURE='active', **_eval_keys(tmp_path))
    assert ds.level_key == 'active' and ds.noise_eval_on and not ds.noise_on
    hp.reset()
    root = str(tmp_path / 'noisy')
    hp.load(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, MIX_LEVEL_MEASURE='active', MIX_LEVEL_RANGE=3.0))
    hp.digest()
    with pytest.raises(ValueError, match='MIX_LEVEL_MEASURE') as e:           # the remaining case, its message kept
        datasets.WavDirData().install_and_load()
    assert 'would do nothing' in str(e.value)


def test_eval_noise_files_are_loaded_like_the_datasets_own(hp, tmp_path, capsys):
    from danet_amd import datasets
    ds = _loaded(hp, tmp_path, **_eval_keys(tmp_path))
    want = sorted(fn for fn in datasets.WavDirData.discover(hp.NOISE_EVAL_DIR) if 'noise02' not in fn)
    assert ds.noise_eval_files == want and ds.noise_eval_skipped == 1 and len(want) == len(EVAL_LENGTHS) - 1
    by_name = {os.path.basename(fn): int(n) for fn, n in zip(ds.noise_eval_files, ds.noise_eval_lengths)}
    assert by_name == {'noise%02d.wav' % i: L for i, L in enumerate(EVAL_LENGTHS) if i != 2}
    assert ds.noise_eval_pool_host.dtype == np.float32
    assert np.array_equal(ds.noise_eval_offsets, np.concatenate([[0], np.cumsum(ds.noise_eval_lengths)[:-1]]))
    for fn, o, n in zip(ds.noise_eval_files, ds.noise_eval_offsets, ds.noise_eval_lengths):
        assert np.array_equal(ds.noise_eval_pool_host[o:o + n], datasets.WavDirData.read_wave(fn))
    # the train pool was never read
    assert ds.noise_pool_host is None and ds.noise_files == [] and not ds.noise_on
    capsys.readouterr()
    datasets.WavDirData().load_host()
    out = capsys.readouterr().out
    assert 'NOISE_EVAL_DIR' in out and '4 files, 1 shorter than FFT_SIZE skipped' in out and 'wavdir noise:' not in out
    hp.reset()
    ds = _loaded(hp, tmp_path, **_train_keys(tmp_path))
    assert ds.noise_eval_pool_host is None and ds.noise_eval_files == []     # and the other way round
    for folder in (str(tmp_path / 'missing'),):
        hp.load(dict(NOISE_EVAL_DIR=folder, NOISE_EVAL_SNR_MIN=0, NOISE_EVAL_SNR_MAX=5))
        with pytest.raises(IOError, match='NOISE_EVAL_DIR'):
            datasets.WavDirData().install_and_load()


# ------------------------------------------------------------------------------------------ the plan
def _eval_stream(rank, subset):
    return np.random.RandomState([1337 + rank, ('train', 'valid', 'test').index(subset), 4])


def _same(got, ref):
    assert np.array_equal(got.files, ref['files']) and np.array_equal(got.snr, ref['snr'])
    assert np.array_equal(got.offsets, ref['offsets']) and np.array_equal(got.lengths, ref['lengths'])
    assert np.array_equal(got.pads, ref['pads'])
    assert got.gains.dtype == np.float32 and np.array_equal(got.gains.view(np.uint32), ref['gains'].view(np.uint32))
    assert np.array_equal(got.gains64, ref['gains64'])


def _plan(ds, subset, shuffle=False):
    return [tuple(None if f is None else (f.copy() if isinstance(f, np.ndarray) else f) for f in item)
            for item in ds.plan_epoch_noise(subset, 4, shuffle, 8, crop=True)]


def test_the_eval_plan_follows_the_restatement_and_repeats_every_sweep(hp, tmp_path, monkeypatch):
    ds = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0, **_eval_keys(tmp_path))
    calls = []
    real = ds.plan_noise

    def recording(powers, gains, rng, *rest):
        rec = NR.RecordingRandomState(0)
        rec.rng = rng
        out = real(powers, gains, rec, *rest)
        calls.append(rec.calls)
        return out
    monkeypatch.setattr(ds, 'plan_noise', recording)
    cases = set()
    for subset in ('valid', 'test'):
        random.seed(3)
        first = _plan(ds, subset)
        random.seed(3)
        second = _plan(ds, subset)                                   # a second sweep: the same noisy mixtures
        rng = _eval_stream(0, subset)
        for a, b in zip(first, second):
            assert a[8] is not None and len(a[8].gains) == 2
            _same(a[8], NR.plan(ds.power['test'][a[0]], a[5], rng, 2, ds.noise_eval_offsets, ds.noise_eval_lengths,
                                ds.noise_eval_power, a[1], 0.0, 15.0, 256, 64))
            _same(b[8], dict(files=a[8].files, snr=a[8].snr, offsets=a[8].offsets, lengths=a[8].lengths,
                             pads=a[8].pads, gains=a[8].gains, gains64=a[8].gains64))
            Lfull = NR.full_length(a[1], 64)
            cases |= set(bool(ds.noise_eval_lengths[f] >= Lfull) for f in a[8].files)
    assert cases == {True, False}                                    # both segment cases were drawn
    assert calls and all(c == [('randint', 2), ('random_sample', 2), ('uniform', 2)] for c in calls)
    # `valid` aliased to `test` still has its own subset index: the two sweeps differ
    random.seed(3)
    v = _plan(ds, 'valid')
    random.seed(3)
    t = _plan(ds, 'test')
    assert not all(np.array_equal(x[8].snr, y[8].snr) for x, y in zip(v, t))


def test_train_draws_what_it_draws_without_the_keys_and_the_other_streams_stay(hp, tmp_path):
    others = dict(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0, SPEED_PERTURB_RANGE=0.1, REVERB_RT60_MAX=0.3)

    def run(ev):
        hp.reset()
        keys = dict(others, **_train_keys(tmp_path))
        if ev:
            keys.update(_eval_keys(tmp_path))
        ds = _loaded(hp, tmp_path, **keys)
        random.seed(11)
        np.random.seed(12)
        plan = _plan(ds, 'train', shuffle=True) + _plan(ds, 'valid') + _plan(ds, 'train', shuffle=True)
        return plan, random.getstate(), np.random.get_state()[1].copy(), ds
    off, r0, n0, _ = run(False)
    on, r1, n1, ds = run(True)
    assert r0 == r1 and np.array_equal(n0, n1)                     # `random` and np.random: as without the keys
    assert len(off) == len(on) == 9
    for k, (a, b) in enumerate(zip(off, on)):
        assert np.array_equal(a[0], b[0]) and a[1:5] == b[1:5] and np.array_equal(a[5], b[5])
        if 3 <= k < 6:                                             # the valid sweep in between
            assert a[6] is None and a[7] is None and a[8] is None and b[6] is None and b[7] is None
            assert b[8] is not None
            continue
        assert np.array_equal(a[6][0], b[6][0]) and np.array_equal(a[7], b[7])
        _same(b[8], dict(files=a[8].files, snr=a[8].snr, offsets=a[8].offsets, lengths=a[8].lengths, pads=a[8].pads,
                         gains=a[8].gains, gains64=a[8].gains64))   # the train noise: its own pool, its own stream
    assert ds.noise_eval_stream('train') is None and ds.noise_stream('valid') is None


def test_the_eval_plan_is_unchanged_by_the_train_keys_and_ranks_differ(hp, tmp_path, monkeypatch):
    from danet_amd import dist
    ds_a = _loaded(hp, tmp_path, **_eval_keys(tmp_path))
    random.seed(5)
    a = _plan(ds_a, 'test')
    hp.reset()
    ds_b = _loaded(hp, tmp_path, **dict(_eval_keys(tmp_path), **_train_keys(tmp_path)))
    random.seed(5)
    b = _plan(ds_b, 'test')
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and x[1:5] == y[1:5]
        _same(y[8], dict(files=x[8].files, snr=x[8].snr, offsets=x[8].offsets, lengths=x[8].lengths, pads=x[8].pads,
                         gains=x[8].gains, gains64=x[8].gains64))
    monkeypatch.setattr(dist, 'rank', lambda: 1)
    random.seed(5)
    c = _plan(ds_a, 'test')
    assert not all(np.array_equal(x[8].snr, y[8].snr) for x, y in zip(a, c))
    rng = _eval_stream(1, 'test')
    for x in c:
        assert np.array_equal(x[8].snr, NR.plan(ds_a.power['test'][x[0]], None, rng, 2, ds_a.noise_eval_offsets,
                                                ds_a.noise_eval_lengths, ds_a.noise_eval_power, x[1], 0.0, 15.0, 256,
                                                64)['snr'])


def test_keys_null_plan_valid_and_test_as_before(hp, tmp_path):
    ds = _loaded(hp, tmp_path)
    for subset in ('valid', 'test'):
        assert all(item[8] is None for item in _plan(ds, subset))
    assert ds.noise_eval_pool_host is None and ds._noise_eval_pool_dev == {} and ds.noise_eval_power is None


def test_valid_step_and_evaluate_take_the_noise(hp):
    '''the signatures the route relies on (the behaviour is tested on the GPU)'''
    import inspect
    from danet_amd import cli
    from danet_amd.model import Model
    sig = inspect.signature(Model.valid_step)
    assert list(sig.parameters) == ['self', 's_src_signals', 's_noise', 's_noise_gain']
    assert sig.parameters['s_noise'].default is None and sig.parameters['s_noise_gain'].default is None
    assert list(inspect.signature(Model.forward).parameters) == ['self', 's_src_signals', 'with_valid', 'with_train',
                                                                 'fuse_heads', 's_dropout_keep']
    assert 'NoisyBatch' in inspect.getsource(cli.evaluate)
    assert 'ignores the noise' in cli._draw_aligned_sources.__doc__


# ------------------------------------------------------------------- known answers of the restatement
def _orthogonal(n_sig, L=64):
    '''n_sig mutually orthogonal +-1 signals of length L (rows of a Hadamard matrix, the constant row left out)'''
    import scipy.linalg
    return scipy.linalg.hadamard(L)[1:n_sig + 1].astype(np.float64)


def _gram(wav):
    return MR.gram_fsum(np.asarray(wav)[None])


def test_orthogonal_references_perfect_estimates_and_a_noise_of_known_power():
    C = 2
    s1, s2, z = _orthogonal(3)
    for amp, want_nsnr in ((1.0, 10.0 * math.log10(2.0)), (2.0, 10.0 * math.log10(0.5)), (0.5, 10.0 * math.log10(8.0))):
        wav = np.stack([s1, s2, s1, s2, amp * z])
        per_utt, perm, mean3 = NV.finalize(_gram(wav), C)
        assert per_utt[0, 0] == 100.0 and perm[0] == 0                 # estimates equal to the references
        # nSNR exact: cc = |s1|^2 + |s2|^2 = 128, nn = 64 amp^2
        assert per_utt[0, 2] == want_nsnr == NV.nsnr(128.0, 64.0 * amp * amp)
        # base_i by hand: <m, s_i> = 64, <m, m> = 128 + 64 amp^2: t = 64, r = 64 + 64 amp^2
        base = 10.0 * math.log10(64.0 / (64.0 + 64.0 * amp * amp))
        assert abs(per_utt[0, 1] - (100.0 - base)) <= 1e-12
        assert np.array_equal(mean3, per_utt[0])
    # a noise that is not orthogonal: z' = z + 0.5 s1.  <m, s_1> = 64 + 32, <m, s_2> = 64, <m, m> = |1.5 s1 + s2 + z|^2
    wav = np.stack([s1, s2, s2, s1, z + 0.5 * s1])
    per_utt, perm, _ = NV.finalize(_gram(wav), C)
    assert perm[0] == 1 and per_utt[0, 0] == 100.0
    mm = 64.0 * (2.25 + 1.0 + 1.0)
    b1 = MR.sdr(64.0, mm, 96.0)
    b2 = MR.sdr(64.0, mm, 64.0)
    assert abs(per_utt[0, 1] - (100.0 - 0.5 * (b1 + b2))) <= 1e-12
    assert abs(per_utt[0, 2] - 10.0 * math.log10(128.0 / (64.0 * 1.25))) <= 1e-12
    assert abs(b1 - 10.0 * math.log10(144.0 / (mm - 144.0))) <= 1e-12


def test_nsnr_clamps_silence_and_the_batch_mean():
    s1, s2, z = _orthogonal(3)
    zero = np.zeros_like(s1)
    assert NV.nsnr(0.0, 1.0) == -100.0 and NV.nsnr(1.0, 0.0) == 100.0 and NV.nsnr(0.0, 0.0) == -100.0
    assert NV.nsnr(1.0, 1e-30) == 100.0 and NV.nsnr(1e-30, 1.0) == -100.0
    # the references cancel (cc = 0): -100; a silent noise row: +100
    per_utt, _, _ = NV.finalize(_gram(np.stack([s1, -s1, s1, s1, z])), 2)
    assert per_utt[0, 2] == -100.0
    per_utt, _, _ = NV.finalize(_gram(np.stack([s1, s2, s1 + 0.1 * z, s2, zero])), 2)
    assert per_utt[0, 2] == 100.0
    # no live reference: (0, 0, 0), and the utterance does not count in the batch mean
    G = np.concatenate([_gram(np.stack([zero, zero, s1, s2, z])), _gram(np.stack([s1, s2, s1 + 0.1 * z, s2, 2 * z]))])
    per_utt, perm, mean3 = NV.finalize(G, 2)
    assert np.array_equal(per_utt[0], [0.0, 0.0, 0.0]) and perm[0] == 0
    assert np.array_equal(mean3, per_utt[1]) and per_utt[1, 2] == 10.0 * math.log10(0.5)
    assert np.array_equal(NV.finalize(G[:1], 2)[2], [0.0, 0.0, 0.0])
    # ties go to the first permutation
    assert NV.finalize(_gram(np.stack([s1, s2, s1 + s2, s1 + s2, z])), 2)[1][0] == 0


def _spectra(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_a_zero_noise_row_gives_the_clean_metric_exactly(C):
    rng = np.random.RandomState(C)
    w = _sqrt_hann(64)
    S = _spectra(rng, 3, C, 9, 33)
    E = (S[:, ::-1] + 0.3 * _spectra(rng, 3, C, 9, 33)).astype(np.complex64)
    S[1, 0] = 0                                                        # one silent reference
    Z = _spectra(rng, 3, 9, 33)
    for noise, gain in ((np.zeros_like(Z), None), (Z, np.zeros(3, np.float32))):
        wav = NV.synth(S, E, noise, gain, w, 16)
        assert not wav[:, 2 * C].any()
        G = MR.gram(wav)
        per_utt, perm, mean3 = NV.finalize(G, C)
        want = MR.finalize(G[:, :2 * C, :2 * C], C)
        assert np.array_equal(per_utt[:, :2], want[0]) and np.array_equal(perm, want[1])
        # (with C = 1 utterance 1 has no live reference: zeros)
        assert np.array_equal(mean3[:2], want[2])
        assert np.array_equal(per_utt[:, 2], [100.0, 100.0 if C > 1 else 0.0, 100.0])


@pytest.mark.parametrize('C,N,S', [(1, 64, 16), (2, 64, 32), (3, 256, 64), (4, 64, 16)])
def test_the_linear_baseline_is_the_direct_baseline(C, N, S):
    '''the rule derives <m, m> and <m, s_i> from the Gram matrix of the SEPARATE rows; the direct form synthesises
    the float64 mixture as one signal.  Synthesis is linear, so the two agree to the rounding of float64.'''
    rng = np.random.RandomState(10 * C + S)
    w = _sqrt_hann(N)
    B, T, F = 3, 11, N // 2 + 1
    Sr = _spectra(rng, B, C, T, F) * (10.0 ** rng.uniform(-1, 1, size=(B, C, 1, 1))).astype(np.float32)
    Z = _spectra(rng, B, T, F)
    worst = 0.0
    for gain in (None, np.asarray([0.3, 1.7, 9.1], np.float32), np.asarray([0.0, 1.0, 0.013], np.float32)):
        wav = NV.synth(Sr, Sr, Z, gain, w, S)                          # float64 synthesis of every row
        lin = NV.baseline_linear(MR.gram_fsum(wav), C)
        direct = NV.baseline_direct(Sr, Z, gain, w, S)
        assert np.isfinite(lin).all() and np.isfinite(direct).all()
        worst = max(worst, float(np.abs(lin - direct).max()))
    print('C %d N %d S %d: linear vs direct baseline, worst %.3g dB' % (C, N, S, worst))
    assert worst <= 1e-9


def test_the_noise_row_is_rounded_to_float32_before_anything_else():
    rng = np.random.RandomState(4)
    Z = _spectra(rng, 2, 5, 33)
    g = np.asarray([0.1, 3.3], np.float32)
    got = NV.scaled_noise(Z, g)
    assert got.dtype == np.complex64
    want_re = (g[:, None, None].astype(np.float64) * Z.real.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.real, want_re)
    assert np.array_equal(NV.scaled_noise(Z, None), Z) and np.array_equal(NV.scaled_noise(Z, np.ones(2, np.float32)), Z)
    assert not NV.scaled_noise(Z, np.zeros(2, np.float32)).any()
