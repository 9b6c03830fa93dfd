'''
CPU tests (no GPU) of the active speech level of the wavdir dataset (MIX_LEVEL_MEASURE): the extension library
libdanet_level_hip.so against its header (exports, prototypes, ABI, lazy load, host-visible argument errors), the
untouched other nine libraries, the open EXTENSIONS registry, the configuration key, the restatement
tests/level_ref.py against the standard's literal counter loop and known levels, the host finish
WavDirData.active_power against it, and the plan: equal active levels after gain, and not one draw moved.
'''
import ctypes
import importlib
import json
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import level_ref as LR
import noise_ref as NR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_level_hip.h')
LEVEL_SYMBOLS = ['danet_level_abi_version', 'danet_level_activity', 'danet_level_last_error',
                 'danet_level_workspace_bytes']
KEY = 'MIX_LEVEL_MEASURE'


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_level_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_level()
    syms = _header_symbols('danet_level_hip.h', 'danet_level_')
    assert syms == LEVEL_SYMBOLS
    assert sorted(_lib.LEVEL_PROTOTYPES) == syms
    assert _exports(_lib.LEVEL_LIB_PATH) == syms
    assert lib.danet_level_abi_version() == 1 == _lib.LEVEL_ABI_VERSION == _lib.LEVEL.abi
    txt = open(HEADER).read()
    assert '#define DANET_LEVEL_ABI_VERSION 1' in txt
    assert '#define DANET_LEVEL_THRESHOLDS %d' % ops.LEVEL_THRESHOLDS in txt and ops.LEVEL_THRESHOLDS == 16
    assert '#define DANET_LEVEL_TILE %d' % ops.LEVEL_TILE in txt
    rule = txt.split('#ifndef')[0]
    for words in ('g = exp(-1 / (0.03 fs))', 'I = ceil(0.2 fs)', 'M = 15.9 dB', 'c_j = sqrt(P) * 2^(j - 10)',
                  'p[n] = g p[n-1] + k |x[n]|', 'q[n] = g q[n-1] + k p[n]', 'n - m <= I', 'P_n stays its mean power'):
        assert words in rule, words
    assert '2^-34' in txt and '1e-9' in txt                   # the accuracy derivation and what it buys
    assert _lib.LEVEL.prototypes is _lib.LEVEL_PROTOTYPES and _lib.LEVEL.prefix == 'danet_level_'


def test_level_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'double': ctypes.c_double,
             'size_t': ctypes.c_size_t, 'const float*': ctypes.c_void_p, 'const int64_t*': ctypes.c_void_p,
             'const double*': ctypes.c_void_p, 'int64_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.LEVEL_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert len(_lib.LEVEL_PROTOTYPES['danet_level_activity'][1]) == 13


def test_level_is_appended_to_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.LEVEL in _lib.EXTENSIONS and build.LEVEL in build.EXTENSIONS
    assert isinstance(_lib.LEVEL, _lib.Library) and isinstance(build.LEVEL, build.Library)
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert _lib.LEVEL not in older and build.LEVEL not in build.LIBRARIES + build.LATER_LIBRARIES
    assert [lib.name for lib in _lib.EXTENSIONS] == [os.path.basename(spec.src_dir) for spec in build.EXTENSIONS]
    assert _lib.EXTENSIONS.index(_lib.LEVEL) > _lib.EXTENSIONS.index(_lib.NOISE)       # appended
    assert build.LEVEL_LIB == build.LEVEL.out == _lib.LEVEL_LIB_PATH
    assert os.path.basename(build.LEVEL_LIB) == _lib.LEVEL.so == 'libdanet_level_hip.so'
    assert os.path.isfile(os.path.join(build.LEVEL.src_dir, 'exports.map'))
    assert callable(build.build_level) and callable(_lib.load_level) and callable(_lib.level_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:2] == [build.METRIC, build.NOISE] and build.LEVEL in rest and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 10      # the nine older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_nine_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + (_lib.METRIC, _lib.NOISE)
    assert [spec.name for spec in older] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed', 'reverb', 'metric',
                                             'noise']
    assert [spec.abi for spec in older] == [7, 1, 1, 1, 1, 1, 1, 1, 1]
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_level_') for s in exported), spec.so
    assert sorted(_lib.MIX_PROTOTYPES) == ['danet_mix_abi_version', 'danet_mix_last_error', 'danet_mix_power',
                                           'danet_mix_scale_c64', 'danet_mix_workspace_bytes']
    assert sorted(_lib.NOISE_PROTOTYPES) == ['danet_noise_abi_version', 'danet_noise_frontend_fwd',
                                             'danet_noise_last_error']


def test_level_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.LEVEL_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'exp', 'log', 'pow', 'sqrt'):
        assert not re.search(r'\b%s[fl]?\b' % word, out.stdout), word       # and no libm call
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'level')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['level.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'level.hip')).read(), flags=re.S)
    code += csrc_scan.shared_code(code)              # and the shared headers it includes, same words
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic'):
        assert word not in code, word


def _write(path, data, rate=8000):
    import scipy.io.wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scipy.io.wavfile.write(path, rate, data)


def _tree(root, n=12):
    '''gated noise at very different stored scales; every third file pauses for 60 % of its length'''
    rng = np.random.RandomState(2)
    for subset in ('train', 'test'):
        for i in range(n):
            L = 16000 + 397 * ((i * 5) % n)
            w = LR.gated_noise(rng, L, 8000, rms=20.0 * 3 ** (i % 6), duty=0.4 if i % 3 == 0 else 1.0)
            _write(os.path.join(root, subset, 'u%02d.wav' % i), np.clip(np.rint(w), -32768, 32767).astype(np.int16))


def test_import_and_a_run_with_the_key_null_never_touch_the_library(tmp_path):
    root = str(tmp_path / 'lazy')
    _tree(root, n=4)
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "print('UNMAPPED:', _lib._level is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "def boom():\n"
        "    raise AssertionError('load_level called')\n"
        "real = _lib.load_level; _lib.load_level = boom\n"
        "hparams.load(json.loads(%r)); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.install_and_load()\n"
        "print('LOADED:', ds.is_loaded, ds.level_key, ds.mix_on)\n"
        "print('STILL:', _lib._level is None and 'libdanet_level' not in open('/proc/self/maps').read())\n"
        "_lib.load_level = real; _lib.LEVEL_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_level()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_level_hip.so' in str(e) and %r in str(e)\n"
        "          and 'MIX_LEVEL_MEASURE' in str(e))\n"
        "print('NONE:', _lib._level is None)\n"
    ) % (ROOT, json.dumps(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64, MIX_SNR_RANGE=0,
                               MIX_LEVEL_MEASURE=None)), nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'LOADED: True None True', 'STILL: True', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_level()
    big = 1 << 30
    ok = dict(stream=None, n_utt=2, pool=1024, pool_len=100, offsets=2048, lengths=4096, max_len=50, g=0.99,
              hang=1600, thr=8192, counts=16384, ws=32768, ws_bytes=big)
    need = lib.danet_level_workspace_bytes(2, 50)
    assert need == 2 * 1 * (16 + 12 * 16)
    assert lib.danet_level_workspace_bytes(3, 1025) == 3 * 2 * 208 and lib.danet_level_workspace_bytes(1, 0) == 208
    cases = [(dict(n_utt=0), b'n_utt must'), (dict(n_utt=-3), b'n_utt must'), (dict(pool_len=-1), b'pool_len'),
             (dict(max_len=-1), b'max_len'), (dict(max_len=(1 << 31) + 1), b'max_len'),
             (dict(n_utt=1 << 20, max_len=1 << 31), b'tiles per row'),
             (dict(g=0.0), b'g must'), (dict(g=1.0), b'g must'), (dict(g=-0.5), b'g must'), (dict(g=1.5), b'g must'),
             (dict(g=float('nan')), b'g must'), (dict(hang=-1), b'hang must'), (dict(hang=(1 << 40) + 1), b'hang must'),
             (dict(pool=None), b'null'), (dict(offsets=None), b'null'), (dict(lengths=None), b'null'),
             (dict(thr=None), b'null'), (dict(counts=None), b'null'), (dict(ws=None), b'null'),
             (dict(pool=1026), b'misaligned'), (dict(offsets=2052), b'misaligned'), (dict(lengths=4100), b'misaligned'),
             (dict(thr=8196), b'misaligned'), (dict(counts=16388), b'misaligned'), (dict(ws=32776), b'misaligned'),
             (dict(ws_bytes=need - 1), b'workspace too small'), (dict(ws_bytes=0), b'workspace too small')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_level_activity(*a.values()) == -1, kw
        assert msg in lib.danet_level_last_error(), (kw, lib.danet_level_last_error())
    for n, L in ((0, 10), (1, -1), (1, (1 << 31) + 1), (1 << 20, 1 << 31)):
        assert lib.danet_level_workspace_bytes(n, L) == ctypes.c_size_t(-1).value, (n, L)
    assert _lib.level_check(0) is None
    assert lib.danet_level_activity(None, 1, None, 0, None, None, 0, 0.5, 0, None, None, None, 0) == -1
    text = lib.danet_level_last_error().decode()
    assert 'null' in text
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.level_check(-1)
    assert str(e.value) == 'libdanet_level_hip error -1: %s' % text


# ----------------------------------------------------------------------------------- the key
def test_the_key_defaults_to_null_and_off(hp):
    from danet_amd import datasets
    H = sys.modules['danet_amd.hparams']
    assert KEY in H.DEFAULTS and H.DEFAULTS[KEY] is None and getattr(hp, KEY) is None
    assert re.fullmatch(hp.pattern, KEY) and KEY in H.__doc__ and KEY in datasets.WavDirData.__doc__
    assert datasets.WavDirData.level_measure() is None and datasets.WavDirData().level_key is None
    hp.load({KEY: 'active'})
    assert datasets.WavDirData.level_measure() == 'active'


@pytest.mark.parametrize('value', [True, False, 1, 0, 1.5, 'mean', 'Active', 'ACTIVE', ''])
def test_any_other_value_raises_and_names_the_key(hp, tmp_path, value):
    from danet_amd import datasets
    root = str(tmp_path / 'level')
    _tree(root, n=2)
    hp.load({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, 'MIX_SNR_RANGE': 3, KEY: value})
    hp.digest()
    ds = datasets.WavDirData()
    with pytest.raises(ValueError, match=KEY):
        ds.install_and_load()
    assert not ds.is_loaded
    with pytest.raises(ValueError, match=KEY):
        datasets.WavDirData.level_measure()


def test_active_without_a_key_that_uses_a_power_is_an_error_that_names_both(hp, tmp_path):
    from danet_amd import datasets
    root = str(tmp_path / 'level')
    _tree(root, n=2)
    for more in (dict(), dict(MIX_LEVEL_RANGE=6)):
        hp.reset()
        hp.load(dict({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, KEY: 'active'}, **more))
        hp.digest()
        ds = datasets.WavDirData()
        with pytest.raises(ValueError, match=KEY) as e:
            ds.install_and_load()
        assert 'MIX_SNR_RANGE' in str(e.value) and 'NOISE_DIR' in str(e.value) and not ds.is_loaded
    noise = str(tmp_path / 'noise')
    NR.write_noise(noise, (700, 5000))
    for more in (dict(MIX_SNR_RANGE=0), dict(MIX_SNR_RANGE=5, MIX_LEVEL_RANGE=6),
                 dict(NOISE_DIR=noise, NOISE_SNR_MIN=0, NOISE_SNR_MAX=10)):
        hp.reset()
        hp.load(dict({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, KEY: 'active'}, **more))
        hp.digest()
        ds = datasets.WavDirData()
        ds.load_host(out=open(os.devnull, 'w'))
        assert ds.level_key == 'active'


def test_every_other_dataset_ignores_the_key(hp):
    hp.load({KEY: 7})
    hp.digest()
    ds = hp.get_dataset()()
    ds.install_and_load()
    assert hp.DATASET_TYPE == 'toy' and next(iter(ds.epoch('train', 4)))[0].shape[0] == 4


def test_no_command_line_flag_is_added():
    from danet_amd import cli
    src = open(cli.__file__).read()
    assert 'level' not in src.lower().replace('mix_level_range', '')


# ----------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('L', [1, 2, 1601, 5000])
def test_the_vectorised_count_equals_the_literal_counter_loop(L):
    rng = np.random.RandomState(L)
    x = LR.gated_noise(rng, L, 8000)
    g, _k, _I = LR.params(8000)
    q = LR.envelope(x, g)
    assert np.array_equal(q, LR.envelope_loop(x, g))
    thr = LR.thresholds(LR.sum_squares(x) / L)
    for I in (0, 7, 1600):
        a = LR.counts(q, thr, I)
        assert np.array_equal(a, LR.counts_literal(q, thr, I)), (L, I)
        assert np.all(np.diff(a) <= 0) and a.max() <= L
    if L == 5000:
        assert len(set(LR.counts(q, thr, 1600).tolist())) >= 6            # the grid is not idle


def test_parameters_of_the_rule():
    g, k, I = LR.params(8000)
    assert g == math.exp(-1.0 / 240.0) and k == 1.0 - g and I == 1600
    assert LR.params(48000)[2] == 9600 and LR.params(44100)[2] == 8820 and LR.params(11025)[2] == 2205
    thr = LR.thresholds(4.0)
    assert thr[10] == 2.0 and thr[0] == 2.0 / 1024 and thr[15] == 64.0 and len(thr) == 16


def test_gated_noise_has_the_level_its_duty_says():
    rng = np.random.RandomState(0)
    for duty, want in ((0.5, 3.01), (1.0, 0.0)):
        x = LR.gated_noise(rng, 160000, 8000, duty=duty)
        rms_db = 10.0 * math.log10(LR.sum_squares(x) / len(x))
        assert abs(LR.active_level_db(x, 8000) - rms_db - want) <= 0.3, (duty, LR.active_level_db(x, 8000) - rms_db)


def test_a_one_sample_file_and_a_silent_file_take_the_fallbacks():
    one = np.asarray([1234.0], dtype=np.float32)
    g, _k, I = LR.params(8000)
    thr = LR.thresholds(1234.0 ** 2)
    assert LR.counts(LR.envelope(one, g), thr, I)[0] == 0                 # shorter than its own attack: a_0 = 0
    assert LR.active_power(one, 8000) == 1234.0 ** 2                     # -> the mean power
    assert LR.active_power(np.zeros(500, np.float32), 8000) == 0.0        # silent: 0, never finished


def test_the_level_does_not_depend_on_the_stored_scale():
    rng = np.random.RandomState(5)
    x = LR.gated_noise(rng, 24000, 8000, rms=50.0)
    y = (x * np.float32(128.0)).astype(np.float32)                        # exact in float32
    g, _k, I = LR.params(8000)
    qx, qy = LR.envelope(x, g), LR.envelope(y, g)
    tx, ty = LR.thresholds(LR.sum_squares(x) / len(x)), LR.thresholds(LR.sum_squares(y) / len(y))
    assert np.array_equal(LR.counts(qx, tx, I), LR.counts(qy, ty, I))
    d = LR.active_level_db(y, 8000) - LR.active_level_db(x, 8000)
    assert abs(d - 20.0 * math.log10(128.0)) <= 1e-9, d


# ----------------------------------------------------------------------------------- the host finish
def _cases(fs=8000):
    rng = np.random.RandomState(11)
    waves = [LR.gated_noise(rng, n, fs, rms=r, duty=d)
             for n, r, d in ((24000, 300.0, None), (16000, 20.0, 0.4), (8000, 5000.0, 1.0), (3000, 1.0, None),
                             (12000, 700.0, 0.25))]
    waves += [np.asarray([77.0], np.float32), np.zeros(900, np.float32)]
    g, _k, I = LR.params(fs)
    sums = np.asarray([LR.sum_squares(w) for w in waves])
    lens = np.asarray([len(w) for w in waves], dtype=np.int64)
    thr = np.stack([LR.thresholds(s / n) for s, n in zip(sums, lens)])
    cnt = np.stack([LR.counts(LR.envelope(w, g), t, I) for w, t in zip(waves, thr)])
    return waves, sums, lens, thr, cnt


def test_active_power_equals_the_restatement_on_its_counts():
    from danet_amd.datasets import WavDirData
    waves, sums, lens, thr, cnt = _cases()
    assert WavDirData.LEVEL_MARGIN_DB == LR.MARGIN_DB == 15.9
    assert WavDirData.level_params(8000) == LR.params(8000)[::2] and WavDirData.level_params(48000)[1] == 9600
    got_thr = WavDirData.level_thresholds(sums / lens)
    assert got_thr.shape == (len(waves), 16) and got_thr.dtype == np.float64
    live = sums > 0
    assert np.allclose(got_thr[live], thr[live], rtol=1e-15, atol=0) and np.all(got_thr[~live] == 0)
    got = WavDirData.active_power(sums, lens, cnt, thr)
    want = np.asarray([LR.active_power(w, 8000) for w in waves])
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.all(np.abs(got - want) <= 1e-12 * want), (got, want)
    assert got[-1] == 0.0 and got[-2] == 77.0 ** 2                        # silent; shorter than its attack
    assert want[1] > 1.8 * sums[1] / lens[1] and want[2] < 1.05 * sums[2] / lens[2]      # pauses count, noise not


def test_active_power_branches():
    from danet_amd.datasets import WavDirData
    sumsq, L = 1.0e6, 1000
    thr = LR.thresholds(sumsq / L)
    # j = 0: already the lowest threshold is within the margin of its level -> A_0
    thr0 = thr * 1024.0
    a = np.asarray([500] + [0] * 15)
    want = 10.0 ** (10.0 * math.log10(sumsq / 500) / 10.0)
    assert 10.0 * math.log10(sumsq / 500) - 20.0 * math.log10(thr0[0]) <= 15.9
    got = WavDirData.active_power([sumsq], [L], [a], [thr0])[0]
    assert abs(got - want) <= 1e-12 * want and abs(got - LR.finish(sumsq, L, a, thr0)) <= 1e-12 * want
    # no crossing: every live threshold stays further than the margin below its level -> the mean power
    far = thr / 4096.0
    a = np.asarray([1000] * 16)
    assert WavDirData.active_power([sumsq], [L], [a], [far])[0] == sumsq / L == LR.finish(sumsq, L, a, far)
    # no live threshold at all
    assert WavDirData.active_power([sumsq], [L], [np.zeros(16, np.int64)], [thr])[0] == sumsq / L
    # an interpolated crossing between two thresholds, by hand
    a = np.asarray([1000] * 8 + [800, 500] + [0] * 6)
    A = [10.0 * math.log10(sumsq / v) for v in (1000, 800, 500)]
    d7, d8 = A[0] - 20.0 * math.log10(thr[7]), A[1] - 20.0 * math.log10(thr[8])
    assert d7 > 15.9 >= d8
    w = (d7 - 15.9) / (d7 - d8)
    want = 10.0 ** ((A[0] + w * (A[1] - A[0])) / 10.0)
    got = WavDirData.active_power([sumsq], [L], [a], [thr])[0]
    assert abs(got - want) <= 1e-12 * want and sumsq / 1000 < got < sumsq / 800


# ----------------------------------------------------------------------------------- the plan
def _loaded(hp, tmp_path, level, **keys):
    '''a loaded dataset whose power tables come from the host restatement (the device half stubbed)'''
    from danet_amd import datasets
    root = str(tmp_path / 'level')
    if not os.path.isdir(root):
        _tree(root)
    noise = str(tmp_path / 'noise')
    if not os.path.isdir(noise):
        NR.write_noise(noise, (256, 700, 5000, 1300, 9000))
    hp.reset()
    hp.load(dict(dict(DATASET_TYPE='wavdir', DATASET_DIR=root, FFT_SIZE=256, FFT_STRIDE=64, BATCH_SIZE=2,
                      MAX_N_SIGNAL=2, MAX_TRAIN_LEN=8, MIX_SNR_RANGE=4.0, MIX_LEVEL_RANGE=3.0, SPEED_PERTURB_RANGE=0.1,
                      REVERB_RT60_MAX=0.2, NOISE_DIR=noise, NOISE_SNR_MIN=-5.0, NOISE_SNR_MAX=20.0,
                      MIX_LEVEL_MEASURE=level), **keys))
    hp.digest()
    ds = datasets.WavDirData()
    ds.load_host(out=open(os.devnull, 'w'))
    ds.is_loaded = True
    for subset in ('train', 'test'):
        rows = [ds.pool_host[subset][o:o + n] for o, n in zip(ds.offsets[subset], ds.lengths[subset])]
        ds.power[subset] = np.asarray([LR.active_power(w, 8000) if level else LR.sum_squares(w) / len(w)
                                       for w in rows])
    ds.noise_power = np.asarray([LR.sum_squares(ds.noise_pool_host[o:o + n]) / n
                                 for o, n in zip(ds.noise_offsets, ds.noise_lengths)])
    return ds


def test_plan_gains_fed_active_powers_equalises_the_active_levels(hp, tmp_path):
    from danet_amd.datasets import WavDirData
    ds = _loaded(hp, tmp_path, 'active')
    rows = [ds.pool_host['train'][o:o + n] for o, n in zip(ds.offsets['train'], ds.lengths['train'])]
    A = ds.power['train']
    mean = np.asarray([LR.sum_squares(w) / len(w) for w in rows])
    assert np.max(A / mean) > 1.6 and np.min(A / mean) < 1.1              # files with pauses, files without
    gains = WavDirData.plan_gains(A[:12], np.random.RandomState(0), 2, snr_range=0.0)
    after = 10.0 * np.log10(gains.astype(np.float64) ** 2 * A[:12]).reshape(-1, 2)
    assert np.all(np.abs(after[:, 0] - after[:, 1]) <= 2e-6)              # (float32 gains: 1e-7 relative)
    for b in range(6):                                                   # the scaled waveforms, measured again
        lv = [LR.active_level_db(rows[2 * b + c].astype(np.float64) * float(gains[2 * b + c]), 8000) for c in (0, 1)]
        assert abs(lv[0] - lv[1]) <= 1e-3, (b, lv)
    by_mean = WavDirData.plan_gains(mean[:12], np.random.RandomState(0), 2, snr_range=0.0)
    assert np.max(np.abs(20.0 * np.log10(by_mean / gains))) > 1.0         # the mean-power rule differs by dBs


def test_plan_epoch_with_the_key_draws_exactly_what_it_draws_without(hp, tmp_path):
    state = {}
    for level in (None, 'active'):
        ds = _loaded(hp, tmp_path, level)
        random.seed(7)
        np.random.seed(7)
        plans = []
        for _epoch in range(2):
            plans += list(ds.plan_epoch_noise('train', 4, True, 8, crop=True))
            plans += list(ds.plan_epoch_noise('valid', 4, False, 8, crop=True))
        streams = [ds._mix_rng['train'], ds._mix_rng['valid'], ds._speed_rng['train'], ds._reverb_rng['train'],
                   ds._noise_rng['train']]
        state[level] = (plans, random.getstate(), np.random.get_state(), [s.get_state() for s in streams])
    (p0, r0, n0, s0), (p1, r1, n1, s1) = state[None], state['active']
    assert r0 == r1 and all(np.array_equal(a, b) for a, b in zip(n0, n1))
    for a, b in zip(s0, s1):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(p0) == len(p1) and len(p0) > 6
    differ = 0
    for a, b in zip(p0, p1):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and list(a[2]) == list(b[2]) and a[3:5] == b[3:5]
        assert (a[6] is None) == (b[6] is None) and (a[7] is None) == (b[7] is None) and (a[8] is None) == (b[8] is None)
        if a[6] is not None:
            assert np.array_equal(a[6][0], b[6][0]) and np.array_equal(a[6][1], b[6][1]) and np.array_equal(a[7], b[7])
        if a[8] is not None:
            for f in ('offsets', 'lengths', 'pads', 'files', 'snr'):
                assert np.array_equal(getattr(a[8], f), getattr(b[8], f)), f
            differ += int(not np.array_equal(a[8].gains, b[8].gains))
        differ += int(not np.array_equal(a[5], b[5]))
    assert differ > len(p0) // 2                                          # same draws, other gains


def test_plan_noise_takes_the_active_table(hp, tmp_path):
    ds = _loaded(hp, tmp_path, 'active', SPEED_PERTURB_RANGE=None, REVERB_RT60_MAX=None)
    plans = list(ds.plan_epoch_noise('train', 4, False))
    A = ds.power['train']
    for item in plans:
        idx, gains, noise = item[0], item[5], item[8]
        g = gains.astype(np.float64).reshape(-1, 2)
        P_s = (g * g * A[idx].reshape(-1, 2)).sum(axis=1)
        P_n = ds.noise_power[noise.files]
        want = np.where((P_s > 0) & (P_n > 0), np.sqrt(P_s / np.where(P_n > 0, P_n, 1.0)) * 10.0 ** (-noise.snr / 20.0),
                        0.0)
        assert np.all(np.abs(noise.gains64 - want) <= 1e-12 * np.maximum(want, 1e-300))
