'''
CPU tests (no GPU) of the reverberation of the wavdir dataset (REVERB_RT60_MAX): the extension library
libdanet_reverb_hip.so against its header (exports, prototypes, ABI, lazy load, host-visible argument errors),
the untouched other six libraries, the LATER_LIBRARIES records, the bank, the configuration key and the draw --
streams, what is left alone -- against the restatement tests/reverb_ref.py.
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
import reverb_ref as RR
import speed_ref as SR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_reverb_hip.h')
REVERB_SYMBOLS = ['danet_reverb_abi_version', 'danet_reverb_apply', 'danet_reverb_last_error']
KEY = 'REVERB_RT60_MAX'


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_reverb_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_reverb()
    syms = _header_symbols('danet_reverb_hip.h', 'danet_reverb_')
    assert syms == REVERB_SYMBOLS
    assert sorted(_lib.REVERB_PROTOTYPES) == syms
    assert _exports(_lib.REVERB_LIB_PATH) == syms
    assert lib.danet_reverb_abi_version() == 1 == _lib.REVERB_ABI_VERSION == _lib.REVERB.abi
    txt = open(HEADER).read()
    assert '#define DANET_REVERB_ABI_VERSION 1' in txt
    assert '#define DANET_REVERB_ROWS 32' in txt and '#define DANET_REVERB_MAX_TAPS 8192' in txt
    rule = txt.split('#ifndef')[0]
    assert 'NB = DANET_REVERB_ROWS = 32' in rule and 'DANET_REVERB_MAX_TAPS = 8192' in rule and '48 bytes' in rule
    assert _lib.REVERB.prototypes is _lib.REVERB_PROTOTYPES and _lib.REVERB.prefix == 'danet_reverb_'


def test_reverb_prototypes_match_the_header_text():
    from danet_amd import _lib, ops
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int,
             'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p,
             'const danet_reverb_utt_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.REVERB_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert ops.REVERB_DESC_DTYPE.itemsize == 48
    assert list(ops.REVERB_DESC_DTYPE.names) == re.findall(r'int(?:64|32)_t (\w+);', txt)
    assert list(ops.REVERB_DESC_DTYPE.names) == ['src_offset', 'src_length', 'dst_offset', 'out_begin', 'out_count',
                                                 'row', 'reserved']
    assert (ops.REVERB_ROWS, ops.REVERB_MAX_TAPS) == (RR.NB, RR.MAX_TAPS)


def test_later_libraries_records_and_a_build_of_seven():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.LATER_LIBRARIES == (_lib.REVERB,) and build.LATER_LIBRARIES == (build.REVERB,)
    assert isinstance(_lib.REVERB, _lib.Library) and isinstance(build.REVERB, build.Library)
    assert _lib.REVERB not in _lib.ALL_LIBRARIES and build.REVERB not in build.LIBRARIES
    assert len(_lib.LIBRARIES) == 5 and len(_lib.ALL_LIBRARIES) == 6 and len(build.LIBRARIES) == 6
    assert build.REVERB_LIB == build.REVERB.out == _lib.REVERB_LIB_PATH
    assert os.path.basename(build.REVERB_LIB) == _lib.REVERB.so == 'libdanet_reverb_hip.so'
    assert os.path.isfile(os.path.join(build.REVERB.src_dir, 'exports.map'))
    assert callable(build.build_reverb) and callable(_lib.load_reverb) and callable(_lib.reverb_check)
    built = []
    real = build._build_library
    try:
        build._build_library = lambda spec, force, verbose: built.append(spec)
        build.build(verbose=False)
    finally:
        build._build_library = real
    assert built == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(built) == 7
    assert all(os.path.isfile(spec.out) for spec in built)


def test_the_other_six_libraries_are_untouched():
    from danet_amd import _lib
    assert [spec.name for spec in _lib.ALL_LIBRARIES] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed']
    for spec in _lib.ALL_LIBRARIES:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_reverb_') for s in exported), spec.so


def test_reverb_library_reads_no_environment_allocates_nothing_and_has_no_math():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.REVERB_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', ' sin', ' cos', ' exp', ' pow', 'rand'):
        assert word not in out.stdout, word
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'reverb')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['reverb.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'reverb.hip')).read(), flags=re.S)
    code += csrc_scan.shared_code(code)              # and the shared headers it includes, same words
    for word in ('getenv', 'environ', 'Malloc', 'malloc', 'new ', 'sinf', 'cosf', 'expf', 'sin(', 'cos(', 'exp(',
                 'rand'):
        assert word not in code, word


def test_import_maps_nothing_and_a_missing_file_is_a_loud_error(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, datasets\n"
        "print('UNMAPPED:', _lib._reverb is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "_lib.REVERB_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_reverb()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_reverb_hip.so' in str(e) and %r in str(e))\n"
        "print('NONE:', _lib._reverb is None)\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'UNMAPPED: True' in out.stdout and 'LOUD: True' in out.stdout and 'NONE: True' in out.stdout, \
        out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_reverb()
    ok = dict(stream=None, n_utt=4, src=1024, src_len=1 << 20, desc=2048, bank=4096, n_taps=4000, dst=8192,
              dst_len=1 << 20)
    cases = [(dict(src=None), b'null'), (dict(desc=None), b'null'), (dict(bank=None), b'null'),
             (dict(dst=None), b'null'), (dict(n_utt=0), b'n_utt'), (dict(n_utt=-3), b'n_utt'),
             (dict(src=1026), b'misaligned'), (dict(dst=8194), b'misaligned'), (dict(desc=2052), b'misaligned'),
             (dict(bank=4104), b'misaligned'), (dict(src_len=-1), b'src_len'), (dict(dst_len=(1 << 40) + 1), b'dst_len'),
             (dict(n_taps=0), b'n_taps'), (dict(n_taps=-4), b'n_taps'), (dict(n_taps=3), b'n_taps'),
             (dict(n_taps=4002), b'n_taps'), (dict(n_taps=8196), b'n_taps')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_reverb_apply(*a.values()) == -1, kw
        assert msg in lib.danet_reverb_last_error(), (kw, lib.danet_reverb_last_error())
    assert _lib.reverb_check(0) is None
    assert lib.danet_reverb_apply(None, 1, None, 0, None, None, 4, None, 0) == -1
    text = lib.danet_reverb_last_error().decode()
    assert 'null' in text
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.reverb_check(-1)
    assert str(e.value) == 'libdanet_reverb_hip error -1: %s' % text


# ------------------------------------------------------------------------------------- the bank
def test_bank_known_answers(monkeypatch):
    from danet_amd import dist, ops
    assert RR.taps(0.5, 8000) == 4000 == ops.reverb_taps(0.5, 8000)
    assert [ops.reverb_taps(R, 8000) for R in (0, 0.0001, 0.0005, 0.00051, 1.0)] == [4, 4, 4, 8, 8000]
    impulse = np.zeros(8192, np.float32)
    impulse[0] = 1.0
    for R, rate in ((0.5, 8000), (0.05, 8000), (0.3, 16000)):
        got, ref = ops.reverb_bank(R, rate), RR.bank(R, rate)
        assert got.dtype == np.float32 and got.shape == ref.shape == (32, RR.taps(R, rate))
        assert np.isfinite(got).all()
        assert np.abs(got.astype(np.float64) - ref).max() <= 1e-6 * np.abs(ref).max()
        assert (np.abs(got.astype(np.float64) - ref) <= 1e-6 * np.abs(ref) + 1e-12).all()      # relative, per tap
        assert np.array_equal(got[0], impulse[:got.shape[1]])
        for b in (got, ref):
            assert np.abs((b.astype(np.float64) ** 2).sum(axis=1) - 1.0).max() <= 1e-6
    got = ops.reverb_bank(0.5, 8000)
    # direct-to-reverberant ratio: 10 dB at the driest row ... 0 dB at the last
    for k in (1, 16, 31):
        h = got[k].astype(np.float64)
        drr = 10 * np.log10(h[0] ** 2 / (h[1:] ** 2).sum())
        assert abs(drr - (10 - 10 * k / 31.0)) < 1e-3, (k, drr)
    z = ops.reverb_bank(0, 8000)
    assert z.shape == (32, 4) and np.array_equal(z, np.tile(impulse[:4], (32, 1)))
    monkeypatch.setattr(dist, 'rank', lambda: 1)                   # not shard-seeded: the same on every rank
    assert np.array_equal(ops.reverb_bank(0.5, 8000), got)
    with pytest.raises(ValueError, match='taps'):
        ops.reverb_bank(1.0, 16000)


def test_sequential_float32_sum_meets_the_bar_of_the_gpu_test():
    rng = np.random.RandomState(3)
    for R, rate, L in ((0.5, 8000, 4099), (0.51, 16000, 4099), (0.033, 8000, 1025), (0.0005, 8000, 257)):
        bank = RR.bank(R, rate)
        K = bank.shape[1]
        x = (rng.standard_normal(L) * 3000).astype(np.int16).astype(np.float32)
        for k in (0, 7, 31):
            y64, S = RR.apply(x, bank[k])
            y32 = RR.apply_f32(x, bank[k])
            err = np.abs(y32.astype(np.float64) - y64)
            print('K %d L %d row %d: worst error / bar %.3f' % (K, L, k, (err / RR.bound(S, K)).max()))
            assert (err <= RR.bound(S, K)).all()
            if k == 0:
                assert np.array_equal(y32, x) and np.array_equal(y64, x.astype(np.float64))


def test_span_covers_exactly_the_samples_the_cropped_frames_read():
    from danet_amd import datasets
    N, S = 256, 64
    for L, pad, beg, cnt in ((1000, 0, 0, 17), (1000, 3, 0, 8), (1000, 3, 5, 4), (1000, 0, 16, 1), (300, 10, 0, 5),
                             (300, 2, 9, 30), (5000, 1, 40, 8), (256, 0, 0, 5), (256, 0, 4, 1)):
        frames = RR.num_frames(L, N, S)
        need = np.zeros(L, bool)
        for t in range(max(beg - pad, 0), min(beg + cnt - pad, frames)):
            lo, hi = t * S - N // 2, t * S + N // 2
            need[max(lo, 0):max(min(hi, L), 0)] = True
        first, count = RR.span(L, pad, beg, cnt, N, S)
        assert need[first:first + count].all() and need.sum() == count, (L, pad, beg, cnt)
        f, c = datasets.WavDirData.reverb_span([L], [pad], beg, cnt, N, S)
        assert (int(f[0]), int(c[0])) == (first, count) and f.dtype == c.dtype == np.int64


# ----------------------------------------------------------------------------------- configuration
def _write(path, data):
    import scipy.io.wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scipy.io.wavfile.write(path, 8000, data)


def _tree(root, n=12):
    rng = np.random.RandomState(2)
    for subset in ('train', 'test'):
        for i in range(n):
            _write(os.path.join(root, subset, 'u%02d.wav' % i),
                   (rng.randn(300 + 97 * ((i * 5) % n)) * 20 * 3 ** (i % 6)).astype(np.int16))


def _loaded(hp, tmp_path, **keys):
    '''a loaded dataset whose power table comes from the host restatement (no device)'''
    from danet_amd import datasets
    root = str(tmp_path / 'reverb')
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


def test_key_default_is_null_and_off(hp):
    from danet_amd import datasets
    H = sys.modules['danet_amd.hparams']
    assert KEY in H.DEFAULTS and H.DEFAULTS[KEY] is None and getattr(hp, KEY) is None
    assert re.fullmatch(hp.pattern, KEY)
    assert KEY in H.__doc__
    ds = datasets.WavDirData()
    assert datasets.WavDirData.reverb_rt60_max() is None and ds.reverb_rt60 is None
    assert ds.reverb_stream('train') is None


@pytest.mark.parametrize('bad', [-0.1, 1.01, 'x', float('nan'), True])
def test_bad_values_raise_and_name_the_key(hp, tmp_path, bad):
    from danet_amd import datasets
    root = str(tmp_path / 'reverb')
    _tree(root, n=2)
    hp.load({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, KEY: bad})
    hp.digest()
    ds = datasets.WavDirData()
    with pytest.raises(ValueError, match=KEY):
        ds.install_and_load()
    assert not ds.is_loaded


def test_a_tap_count_beyond_the_header_names_the_key_and_the_sample_rate(hp, tmp_path):
    from danet_amd import datasets
    root = str(tmp_path / 'reverb')
    _tree(root, n=2)
    hp.load({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, KEY: 0.6, 'SMPRATE': 16000})
    hp.digest()
    ds = datasets.WavDirData()
    with pytest.raises(ValueError, match=KEY) as e:
        ds.install_and_load()
    assert 'SMPRATE' in str(e.value) and '9600' in str(e.value) and '8192' in str(e.value)
    hp.reset()
    hp.load({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, KEY: 0.512, 'SMPRATE': 16000})
    hp.digest()
    assert datasets.WavDirData.reverb_rt60_max() == 0.512           # 8192 taps: the envelope's edge


def test_every_other_dataset_ignores_the_key(hp):
    hp.load({KEY: 'wet'})
    hp.digest()
    ds = hp.get_dataset()()
    ds.install_and_load()
    assert hp.DATASET_TYPE == 'toy' and next(iter(ds.epoch('train', 4)))[0].shape[0] == 4


def _plan(ds, subset, shuffle=False):
    return [tuple(None if f is None else (f.copy() if isinstance(f, np.ndarray) else f) for f in item)
            for item in ds.plan_epoch_reverb(subset, 4, shuffle, 8, crop=True)]


def test_key_null_maps_nothing_and_plans_what_it_always_did(hp, tmp_path):
    ds = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0)
    assert ds.reverb_rt60 is None
    random.seed(11)
    np.random.seed(12)
    got = _plan(ds, 'train', shuffle=True)
    assert all(len(item) == 8 and item[6] is None and item[7] is None for item in got)
    assert ds._reverb_rng == {} and ds._reverb_bank == {} and ds._reverb_scratch == {}
    random.seed(11)
    np.random.seed(12)
    six = list(ds.plan_epoch('train', 4, True, 8, crop=True))
    random.seed(11)
    np.random.seed(12)
    seven = list(ds.plan_epoch_speed('train', 4, True, 8, crop=True))
    assert all(len(item) == 6 for item in six) and all(len(item) == 7 for item in seven)
    assert len(six) == len(seven) == len(got) == 3
    for a, b, c in zip(six, seven, got):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and a[1:5] == b[1:5] == c[1:5]
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, datasets\n"
        "from danet_amd.hparams import hparams\n"
        "hparams.load(json.loads(%r)); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.load_host(); ds.is_loaded = True\n"
        "n = len(list(ds.plan_epoch_reverb('train', 4, True, 8, crop=True)))\n"
        "print('PLANNED:', n, 'UNMAPPED:', _lib._reverb is None and 'libdanet_reverb' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, json.dumps(dict(DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'reverb'), FFT_SIZE=256,
                               FFT_STRIDE=64, REVERB_RT60_MAX=None)))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'PLANNED: 3 UNMAPPED: True' in out.stdout, out.stdout + out.stderr


def test_key_set_draws_one_call_per_batch_and_leaves_every_other_stream_alone(hp, tmp_path):
    def run(**keys):
        hp.reset()
        ds = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0, SPEED_PERTURB_RANGE=0.1, **keys)
        random.seed(11)
        np.random.seed(12)
        plan = _plan(ds, 'train', shuffle=True) + _plan(ds, 'train', shuffle=True)
        return plan, random.getstate(), np.random.get_state()[1].copy(), ds
    off, r0, n0, _ = run()
    on, r1, n1, ds = run(**{KEY: 0.5})
    assert r0 == r1 and np.array_equal(n0, n1)                     # `random` and np.random: as without the key
    assert len(off) == len(on) == 6
    rng = RR.stream(0, 'train')                                    # ONE stream, on across both epochs
    seen = set()
    for a, b in zip(off, on):
        assert a[7] is None and np.array_equal(a[0], b[0]) and a[1:5] == b[1:5]
        assert np.array_equal(a[5], b[5])                          # the mix draws
        assert np.array_equal(a[6][0], b[6][0]) and np.array_equal(a[6][1], b[6][1])       # the speed draws
        want = RR.draw(4, rng)
        assert np.array_equal(b[7], want) and b[7].dtype == np.int64 and b[7].shape == (4,)
        assert b[7].min() >= 0 and b[7].max() < 32
        seen.update(int(v) for v in b[7])
    assert len(seen) > 8
    # the speed stream is the one of tests/speed_ref.py still: seeded without regard to the new key
    srng = SR.stream(0, 'train')
    for b in on:
        assert np.array_equal(b[6][0], SR.draw(ds.lengths['train'][b[0]], srng, 0.1, 256)[0])


def test_reverb_draws_touch_neither_random_nor_np_random(hp, tmp_path):
    from danet_amd import datasets
    rng = np.random.RandomState(5)
    random.seed(1)
    np.random.seed(2)
    s0, n0 = random.getstate(), np.random.get_state()[1].copy()
    rows = datasets.WavDirData.plan_reverb(6, rng)
    assert random.getstate() == s0 and np.array_equal(np.random.get_state()[1], n0)
    assert np.array_equal(rows, RR.draw(6, np.random.RandomState(5)))
    ds = _loaded(hp, tmp_path, **{KEY: 1.0})
    assert ds.reverb_rt60 == 1.0 and ds.reverb_stream('train') is ds.reverb_stream('train')


def test_valid_and_test_draw_nothing_the_stream_runs_on_and_ranks_differ(hp, tmp_path, monkeypatch):
    from danet_amd import dist
    ds0 = _loaded(hp, tmp_path, **{KEY: 0.5})
    hp.reset()
    ds = _loaded(hp, tmp_path)
    for subset in ('valid', 'test'):
        assert ds0.reverb_stream(subset) is None
        random.seed(4)
        without = _plan(ds, subset)
        random.seed(4)
        with_key = _plan(ds0, subset)
        assert all(item[7] is None for item in with_key)
        for a, b in zip(without, with_key):
            assert np.array_equal(a[0], b[0]) and a[1:5] == b[1:5]
    assert ds0._reverb_rng == {}
    hp.reset()
    ds0 = _loaded(hp, tmp_path, **{KEY: 0.5})
    a = _plan(ds0, 'train')
    monkeypatch.setattr(dist, 'rank', lambda: 1)
    ds1 = _loaded(hp, tmp_path, **{KEY: 0.5})
    b = _plan(ds1, 'train')
    assert not all(np.array_equal(x[7], y[7]) for x, y in zip(a, b))
    rng = RR.stream(1, 'train')
    for x in b:
        assert np.array_equal(x[7], RR.draw(4, rng))
    c = _plan(ds1, 'train')                                        # the stream runs on: new rows in the second epoch
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(b, c))
    assert not all(np.array_equal(x[7], y[7]) for x, y in zip(b, c))
    for x in c:
        assert np.array_equal(x[7], RR.draw(4, rng))


def test_descriptor_validation_is_on_the_host():
    from danet_amd import ops
    ok = dict(src_offsets=[0, 100], src_lengths=[100, 50], dst_offsets=[0, 200], out_begin=[0, 10], out_count=[100, 40],
              rows=[0, 31], src_len=150, dst_len=400)
    d = ops.reverb_desc(**ok)
    assert d.dtype == ops.REVERB_DESC_DTYPE and d['row'].tolist() == [0, 31] and d['reserved'].tolist() == [0, 0]
    assert d['out_begin'].tolist() == [0, 10] and d['out_count'].tolist() == [100, 40]
    for kw, msg in ((dict(rows=[-1, 0]), 'row = -1'), (dict(rows=[0, 32]), 'row = 32'),
                    (dict(src_lengths=[100, 51]), 'outside the pool'), (dict(src_offsets=[-1, 100]), 'outside the pool'),
                    (dict(out_count=[101, 40]), 'outside its 100 samples'), (dict(out_begin=[-1, 10]), 'outside its'),
                    (dict(dst_offsets=[0, 80]), 'apart from each other'), (dict(dst_offsets=[0, 351]), 'inside the buffer')):
        with pytest.raises(ValueError, match=msg):
            ops.reverb_desc(**dict(ok, **kw))
