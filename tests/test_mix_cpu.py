'''
CPU tests (no GPU) of the mixture level control of the wavdir dataset (MIX_SNR_RANGE / MIX_LEVEL_RANGE):
the extension library libdanet_mix_hip.so against its header (exports, prototypes, no environment read, no
allocation, lazy load, host-visible argument errors), the untouched other four libraries, the two
configuration keys, and the gain rule of include/danet_mix_hip.h -- known answers, draw counts, draw
streams -- against the restatement tests/mix_ref.py.
'''
import ctypes
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mix_ref as M
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_mix_hip.h')
MIX_SYMBOLS = ['danet_mix_abi_version', 'danet_mix_last_error', 'danet_mix_power', 'danet_mix_scale_c64',
               'danet_mix_workspace_bytes']


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_mix_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_mix()
    syms = _header_symbols('danet_mix_hip.h', 'danet_mix_')
    assert syms == MIX_SYMBOLS
    assert set(_lib.MIX_PROTOTYPES) == set(syms)
    assert _exports(_lib.MIX_LIB_PATH) == syms
    assert lib.danet_mix_abi_version() == 1 == _lib.MIX_ABI_VERSION
    assert '#define DANET_MIX_ABI_VERSION 1' in open(HEADER).read()


def test_mix_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'size_t': ctypes.c_size_t,
             'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'double*': ctypes.c_void_p,
             'const int64_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.MIX_PROTOTYPES.items():
        m = re.search(r'([a-z_ ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)


def test_the_other_four_libraries_export_what_they_did():
    from danet_amd import _lib
    for path, header, prefix, table in (
            (_lib.LIB_PATH, 'danet_hip.h', 'danet_', _lib.PROTOTYPES),
            (_lib.CONV_LIB_PATH, 'danet_conv_hip.h', 'danet_conv_', _lib.CONV_PROTOTYPES),
            (_lib.DROPOUT_LIB_PATH, 'danet_dropout_hip.h', 'danet_dropout_', _lib.DROPOUT_PROTOTYPES),
            (_lib.PREP_LIB_PATH, 'danet_prep_hip.h', 'danet_prep_', _lib.PREP_PROTOTYPES)):
        exported = _exports(path)
        assert exported == _header_symbols(header, prefix) == sorted(table), path
        assert not any(s.startswith('danet_mix_') for s in exported), path
    assert len(_exports(_lib.LIB_PATH)) == 51
    assert _exports(_lib.PREP_LIB_PATH) == ['danet_prep_abi_version', 'danet_prep_last_error', 'danet_prep_num_frames',
                                            'danet_prep_stft_batch', 'danet_prep_stft_plan',
                                            'danet_prep_workspace_bytes']
    assert _exports(_lib.DROPOUT_LIB_PATH) == ['danet_dropout_abi_version', 'danet_dropout_apply',
                                               'danet_dropout_last_error']
    assert len(_exports(_lib.CONV_LIB_PATH)) == 7
    assert _lib.load().danet_abi_version() == 7
    assert _lib.load_conv().danet_conv_abi_version() == 1
    assert _lib.load_dropout().danet_dropout_abi_version() == 1
    assert _lib.load_prep().danet_prep_abi_version() == 1


def test_mix_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.MIX_LIB_PATH], capture_output=True, text=True, check=True)
    assert 'getenv' not in out.stdout and 'hipMalloc' not in out.stdout and 'hipFree' not in out.stdout
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'mix')
    srcs = [f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp'))]
    assert srcs == ['mix.hip']
    shared = csrc_scan.shared_headers(open(os.path.join(d, 'mix.hip')).read())
    assert [os.path.basename(p) for p in shared] == ['ext_core.h', 'ragged_rows.h', 'sumsq_f64.h']
    for f in srcs + shared:                                                                # same words
        src = open(os.path.join(d, f)).read()
        assert 'getenv' not in src and 'environ' not in src, f
        code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
        assert 'asm' not in code and 'atomic' not in code and 'Malloc' not in code, f      # plain HIP C++


def test_lazy_load_and_missing_library_is_a_loud_error(tmp_path):
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, cli, datasets\n"
        "from danet_amd.hparams import hparams\n"
        "hparams.load(dict(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE='loud'))\n"      # any other dataset ignores both keys
        "hparams.digest()\n"
        "ds = hparams.get_dataset()(); ds.install_and_load()\n"
        "next(iter(ds.epoch('train', 4)))\n"
        "maps = open('/proc/self/maps').read()\n"
        "print('TOY:', hparams.DATASET_TYPE, 'LAZY:', _lib._mix is None and 'libdanet_mix_hip' not in maps)\n"
        "_lib.MIX_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_mix()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_mix_hip.so' in str(e))\n"
    ) % (ROOT, str(tmp_path / 'nope.so'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'TOY: toy LAZY: True' in out.stdout and 'LOUD: True' in out.stdout, out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_mix()
    ok = dict(stream=None, n_utt=4, pool=1024, pool_len=1 << 20, offsets=2048, lengths=4096, max_len=1 << 20,
              out=8192, ws=16384, ws_bytes=4 * 16 * 8)
    assert lib.danet_mix_workspace_bytes(4, 1 << 20) == 4 * 16 * 8           # 16 slices of 65536
    assert lib.danet_mix_workspace_bytes(1000, 65536) == 0                   # one slice per row: no scratch
    assert lib.danet_mix_workspace_bytes(3, 1 << 30) == 3 * 256 * 8          # never more than 256 slices
    assert lib.danet_mix_workspace_bytes(0, 100) == ctypes.c_size_t(-1).value
    assert lib.danet_mix_workspace_bytes(1, -1) == ctypes.c_size_t(-1).value
    assert lib.danet_mix_workspace_bytes(1, (1 << 39) + 1) == ctypes.c_size_t(-1).value
    cases = [(dict(n_utt=0), b'n_utt'), (dict(pool_len=-1), b'pool_len'), (dict(max_len=-1), b'max_len'),
             (dict(max_len=(1 << 39) + 1), b'max_len'), (dict(pool=None), b'null'), (dict(offsets=None), b'null'),
             (dict(lengths=None), b'null'), (dict(out=None), b'null'), (dict(ws=None), b'null'),
             (dict(pool=1026), b'misaligned'), (dict(offsets=2052), b'misaligned'), (dict(lengths=4100), b'misaligned'),
             (dict(out=8196), b'misaligned'), (dict(ws=16388), b'misaligned'), (dict(ws_bytes=4 * 16 * 8 - 1), b'too small'),
             (dict(n_utt=1 << 30), b'2^31')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_mix_power(*a.values()) == -1, kw
        assert msg in lib.danet_mix_last_error(), (kw, lib.danet_mix_last_error())
    ok = dict(stream=None, n_utt=4, t_count=8, F=129, buf=4096, ld=129, gains=1024)
    cases = [(dict(n_utt=0), b'>= 1'), (dict(t_count=0), b'>= 1'), (dict(F=0), b'>= 1'), (dict(buf=None), b'null'),
             (dict(gains=None), b'null'), (dict(ld=128), b'ld must be >= F'), (dict(ld=1 << 40), b'too large'),
             (dict(buf=4100), b'misaligned'), (dict(gains=1026), b'misaligned'),
             (dict(n_utt=1 << 30, t_count=1 << 20, F=4097, ld=4098), b'2^31')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_mix_scale_c64(*a.values()) == -1, kw
        assert msg in lib.danet_mix_last_error(), (kw, lib.danet_mix_last_error())
    with pytest.raises(_lib.DanetHipError, match='ld must be'):
        _lib.mix_check(lib.danet_mix_scale_c64(*dict(ok, ld=1).values()))


# ----------------------------------------------------------------------------------- configuration
def test_key_defaults_are_null_and_off(hp):
    from danet_amd import datasets
    H = sys.modules['danet_amd.hparams']
    for key in ('MIX_SNR_RANGE', 'MIX_LEVEL_RANGE'):
        assert key in H.DEFAULTS and H.DEFAULTS[key] is None and getattr(hp, key) is None
        assert re.fullmatch(hp.pattern, key)
    ds = datasets.WavDirData()
    assert datasets.WavDirData.mix_ranges() == (None, None) and not ds.mix_on and ds.mix_stream('train') is None


def _write(path, data):
    import scipy.io.wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scipy.io.wavfile.write(path, 8000, data)


def _tree(root, n=11):
    rng = np.random.RandomState(2)
    for subset in ('train', 'test'):
        for i in range(n):
            _write(os.path.join(root, subset, 'u%02d.wav' % i),
                   (rng.randn(300 + 97 * ((i * 5) % n)) * 20 * 3 ** (i % 6)).astype(np.int16))


def _loaded(hp, tmp_path, **keys):
    '''a loaded dataset whose power table comes from the host restatement (no device)'''
    from danet_amd import datasets
    root = str(tmp_path / 'mix')
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
    return ds


@pytest.mark.parametrize('key', ['MIX_SNR_RANGE', 'MIX_LEVEL_RANGE'])
@pytest.mark.parametrize('bad', [-0.5, -1, 'six', float('nan'), float('inf'), True])
def test_bad_values_raise_and_name_the_key(hp, tmp_path, key, bad):
    from danet_amd import datasets
    root = str(tmp_path / 'mix')
    _tree(root, n=2)
    hp.load({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, key: bad})
    hp.digest()
    ds = datasets.WavDirData()
    with pytest.raises(ValueError, match=key):
        ds.install_and_load()
    assert not ds.is_loaded


def test_each_key_works_without_the_other_and_zero_is_a_value(hp, tmp_path):
    for keys, want in ((dict(MIX_SNR_RANGE=0), (0.0, None)), (dict(MIX_LEVEL_RANGE=3), (None, 3.0)),
                       (dict(MIX_SNR_RANGE=2.5, MIX_LEVEL_RANGE=0.0), (2.5, 0.0))):
        hp.reset()
        ds = _loaded(hp, tmp_path, **keys)
        assert (ds.mix_snr_range, ds.mix_level_range) == want and ds.mix_on


def test_batch_size_must_be_a_multiple_of_the_sources(hp, tmp_path):
    ds = _loaded(hp, tmp_path, MIX_LEVEL_RANGE=3.0)
    with pytest.raises(ValueError, match='multiple of MAX_N_SIGNAL'):
        next(ds.plan_epoch('train', 3))
    assert next(ds.plan_epoch('train', 4))[5].shape == (4,)
    hp.reset()
    ds = _loaded(hp, tmp_path)                                  # keys null: any batch size, as before
    assert next(ds.plan_epoch('train', 3))[5] is None


# ------------------------------------------------------------------------- the rule: known answers
def _plan(powers, C, R=None, L=None, seed=0):
    from danet_amd import datasets
    rng = M.CountingRandomState(seed)
    g = datasets.WavDirData.plan_gains(np.asarray(powers, np.float64), rng, C, R, L)
    assert g.dtype == np.float32 and g.shape == (len(powers),)
    return g, rng.draws


def test_r_zero_equalises_both_sources_to_the_geometric_mean():
    g, draws = _plan([4.0, 1.0], 2, R=0.0)
    assert np.array_equal(g, np.asarray([2 ** -0.5, 2 ** 0.5], np.float32))          # P = (4, 1): (2^-1/2, 2^1/2)
    assert len(draws) == 1 and draws[0][2] == 0.0
    P = np.asarray([3.7e6, 12.5])
    g, _ = _plan(P, 2, R=0.0)
    G = math.sqrt(P[0] * P[1])
    assert np.allclose(g.astype(np.float64) ** 2 * P, G, rtol=1e-6, atol=0)


def test_relative_level_of_two_sources_is_minus_u():
    P = np.asarray([9.0e5, 40.0, 1.0, 7.7e3, 123.0, 123.0])
    from danet_amd import datasets
    rng = M.CountingRandomState(5)
    g = datasets.WavDirData.plan_gains(P, rng, 2, 6.0, None).astype(np.float64)
    assert len(rng.draws) == 3
    for b, (lo, hi, u) in enumerate(rng.draws):
        assert (lo, hi) == (-6.0, 6.0) and -6.0 <= u <= 6.0
        # float64 gains before the float32 rounding: to 1e-9 dB
        g64 = M.group_gains(P[2 * b:2 * b + 2], [0.0, u], 0.0, True)
        ratio = 20 * math.log10(g64[0] * math.sqrt(P[2 * b]) / (g64[1] * math.sqrt(P[2 * b + 1])))
        assert abs(ratio - (-u)) < 1e-9
        # and the float32 gains the dataset plans are those, rounded once
        assert np.array_equal(np.asarray(g64).astype(np.float32), g[2 * b:2 * b + 2].astype(np.float32))
        ratio32 = 20 * math.log10(g[2 * b] * math.sqrt(P[2 * b]) / (g[2 * b + 1] * math.sqrt(P[2 * b + 1])))
        assert abs(ratio32 - (-u)) < 2e-6                            # two float32 roundings: 2 * 2^-24 * 8.7 dB
        # symmetric: (-u/2, +u/2) about the geometric mean
        G = math.sqrt(P[2 * b] * P[2 * b + 1])
        assert abs(20 * math.log10(g64[1] * math.sqrt(P[2 * b + 1] / G)) - u / 2) < 1e-9


def test_three_sources_offsets_sum_to_zero():
    P = np.asarray([100.0, 2500.0, 4.0e4])
    g, draws = _plan(P, 3, R=10.0, seed=3)
    assert len(draws) == 2
    G = math.exp(np.mean(np.log(P)))
    d = 20 * np.log10(g.astype(np.float64) * np.sqrt(P / G))
    assert abs(d.sum()) < 1e-5
    u = np.asarray([0.0, draws[0][2], draws[1][2]])
    assert np.allclose(d, u - u.mean(), atol=1e-5)


def test_silent_row_has_gain_one_and_is_left_out_of_g():
    g, draws = _plan([0.0, 50.0, 8.0, 0.0, 0.0, 0.0, 16.0, 4.0, 1.0], 3, R=0.0, L=None)
    assert len(draws) == 6                                             # drawn whether or not the row is silent
    assert g[0] == 1.0 and g[3] == 1.0 and np.array_equal(g[3:6], np.ones(3, np.float32))
    G = math.sqrt(50.0 * 8.0)                                          # over the rows with P > 0 only
    assert np.allclose(g[1:3].astype(np.float64) ** 2 * np.asarray([50.0, 8.0]), G, rtol=1e-6)
    assert np.allclose(g[6:9].astype(np.float64) ** 2 * np.asarray([16.0, 4.0, 1.0]), 4.0, rtol=1e-6)
    # with a level: the silent row still has exactly 1
    g, draws = _plan([0.0, 50.0], 2, R=None, L=6.0, seed=1)
    assert g[0] == 1.0 and g[1] == np.float32(10.0 ** (draws[0][2] / 20))


def test_level_only_shifts_the_group_and_equalises_nothing():
    P = [9.0e5, 40.0, 1.0, 7.7e3]
    g, draws = _plan(P, 2, R=None, L=6.0, seed=9)
    assert len(draws) == 2 and all((lo, hi) == (-6.0, 6.0) for lo, hi, _ in draws)
    for b, (_, _, l) in enumerate(draws):
        assert g[2 * b] == g[2 * b + 1] == np.float32(10.0 ** (l / 20.0))
    assert g[0] != g[2]


@pytest.mark.parametrize('B,C', [(1, 2), (4, 2), (3, 3), (5, 1)])
def test_draw_count_depends_on_shapes_and_keys_only(B, C):
    P = np.abs(np.random.RandomState(B + C).randn(B * C)) * 100
    P[0] = 0.0
    for R, L, n in ((4.0, 2.0, B * (C - 1) + B), (4.0, None, B * (C - 1)), (None, 2.0, B)):
        g, draws = _plan(P, C, R=R, L=L)
        assert len(draws) == n
        # order: group by group, the C - 1 offsets, then the level
        want = ([(-R, R)] * (C - 1) if R is not None else []) + ([(-L, L)] if L is not None else [])
        assert [(lo, hi) for lo, hi, _ in draws] == want * B
        assert np.array_equal(g, M.gains(P, np.random.RandomState(0), C, R, L))       # the restatement, same stream


# ------------------------------------------------------------------------------------ draw streams
def _epoch_plan(ds, subset, shuffle=False):
    return [(idx.copy(), T, list(p), b, c, None if g is None else g.copy())
            for idx, T, p, b, c, g in ds.plan_epoch(subset, 4, shuffle, 8, crop=True)]


def test_planning_with_the_keys_set_leaves_random_and_np_random_as_the_keys_null_do(hp, tmp_path):
    def run(**keys):
        hp.reset()
        ds = _loaded(hp, tmp_path, **keys)
        random.seed(11)
        np.random.seed(12)
        plan = _epoch_plan(ds, 'train', shuffle=True) + _epoch_plan(ds, 'train', shuffle=True)
        return plan, random.getstate(), np.random.get_state()[1].copy(), ds
    off, r0, n0, _ = run()
    on, r1, n1, ds = run(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0)
    assert r0 == r1 and np.array_equal(n0, n1)
    assert len(off) == len(on) == 6
    rng = M.stream(0, 'train')
    for a, b in zip(off, on):
        assert np.array_equal(a[0], b[0]) and a[1:5] == b[1:5]               # same indices, pads and crop
        assert a[5] is None
        assert np.array_equal(b[5], M.gains(ds.power['train'][b[0]], rng, 2, 5.0, 3.0))    # one stream, on across epochs


def test_valid_stream_repeats_and_train_stream_runs_on(hp, tmp_path):
    ds = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0)
    assert ds._alias                                                        # no valid folder: test's table
    for subset in ('valid', 'test'):
        a, b = _epoch_plan(ds, subset), _epoch_plan(ds, subset)
        assert len(a) == 3
        for x, y in zip(a, b):
            assert np.array_equal(x[5], y[5])
        rng = M.stream(0, subset)
        for x in a:
            assert np.array_equal(x[5], M.gains(ds.power['test'][x[0]], rng, 2, 5.0, 3.0))
    assert not np.array_equal(_epoch_plan(ds, 'valid')[0][5], _epoch_plan(ds, 'test')[0][5])
    a, b = _epoch_plan(ds, 'train'), _epoch_plan(ds, 'train')
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))            # same utterances ...
    assert not any(np.array_equal(x[5], y[5]) for x, y in zip(a, b))        # ... at new levels


def test_two_ranks_draw_differently(hp, tmp_path, monkeypatch):
    from danet_amd import dist
    ds0 = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0)
    a = _epoch_plan(ds0, 'train')
    monkeypatch.setattr(dist, 'rank', lambda: 1)
    ds1 = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0)
    b = _epoch_plan(ds1, 'train')
    assert not any(np.array_equal(x[5], y[5]) for x, y in zip(a, b))
    rng = M.stream(1, 'train')
    for x in b:
        assert np.array_equal(x[5], M.gains(ds1.power['train'][x[0]], rng, 2, 5.0, None))


def test_restated_power_is_exact_on_a_known_row():
    x = np.asarray([3.0, -4.0, 0.5, 2.0 ** -20, 1e4], np.float32)
    assert M.sum_squares(x) == 9.0 + 16.0 + 0.25 + 2.0 ** -40 + 1e8
    assert M.mean_power(x) == M.sum_squares(x) / 5
