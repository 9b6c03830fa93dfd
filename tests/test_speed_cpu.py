'''
CPU tests (no GPU) of the speed perturbation of the wavdir dataset (SPEED_PERTURB_RANGE): the extension
library libdanet_speed_hip.so against its header (exports, prototypes, ABI, lazy load, host-visible argument
errors, danet_speed_out_len), the untouched other five libraries, the filter table, the configuration key
and the draw -- lengths, streams, what is left alone -- against the restatement tests/speed_ref.py.
'''
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mix_ref as M
import speed_ref as SR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_speed_hip.h')
SPEED_SYMBOLS = ['danet_speed_abi_version', 'danet_speed_last_error', 'danet_speed_out_len', 'danet_speed_resample']
KEY = 'SPEED_PERTURB_RANGE'


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_speed_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_speed()
    syms = _header_symbols('danet_speed_hip.h', 'danet_speed_')
    assert syms == SPEED_SYMBOLS
    assert sorted(_lib.SPEED_PROTOTYPES) == syms
    assert _exports(_lib.SPEED_LIB_PATH) == syms
    assert lib.danet_speed_abi_version() == 1 == _lib.SPEED_ABI_VERSION == _lib.SPEED.abi
    txt = open(HEADER).read()
    assert '#define DANET_SPEED_ABI_VERSION 1' in txt
    assert '#define DANET_SPEED_PHASES 512' in txt and '#define DANET_SPEED_TAPS 32' in txt
    assert _lib.SPEED.prototypes is _lib.SPEED_PROTOTYPES and _lib.SPEED.prefix == 'danet_speed_'
    assert _lib.ALL_LIBRARIES == _lib.LIBRARIES + (_lib.SPEED,)


def test_speed_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int,
             'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p,
             'const danet_speed_utt_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.SPEED_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    # the descriptor row of the header is the record the binding uploads
    from danet_amd import ops
    assert ops.SPEED_DESC_DTYPE.itemsize == 40
    assert list(ops.SPEED_DESC_DTYPE.names) == re.findall(r'int(?:64|32)_t (\w+);', txt)


def test_binding_and_build_name_the_sixth_library():
    import importlib
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert len(build.LIBRARIES) == 6 and build.LIBRARIES[5] is build.SPEED
    assert build.SPEED_LIB == build.SPEED.out == _lib.SPEED_LIB_PATH
    assert os.path.basename(build.SPEED_LIB) == _lib.SPEED.so == 'libdanet_speed_hip.so'
    assert os.path.isfile(os.path.join(build.SPEED.src_dir, 'exports.map'))
    assert callable(build.build_speed)


def test_the_other_five_libraries_are_untouched():
    from danet_amd import _lib
    assert [spec.name for spec in _lib.LIBRARIES] == ['', 'conv', 'dropout', 'prep', 'mix']
    for spec in _lib.LIBRARIES:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_speed_') for s in exported), spec.so


def test_speed_library_reads_no_environment_allocates_nothing_and_has_no_math():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.SPEED_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', ' sin', ' cos', ' sincos'):
        assert word not in out.stdout, word
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'speed')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['speed.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'speed.hip')).read(), flags=re.S)
    code += csrc_scan.shared_code(code)              # and the shared headers it includes, same words
    for word in ('getenv', 'environ', 'Malloc', 'sinf', 'cosf', 'sin(', 'cos('):
        assert word not in code, word


def test_import_maps_nothing_and_a_missing_file_is_a_loud_error(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, datasets\n"
        "print('UNMAPPED:', _lib._speed is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "_lib.SPEED_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_speed()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_speed_hip.so' in str(e) and %r in str(e))\n"
        "print('NONE:', _lib._speed is None)\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'UNMAPPED: True' in out.stdout and 'LOUD: True' in out.stdout and 'NONE: True' in out.stdout, \
        out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_speed()
    ok = dict(stream=None, n_utt=4, src=1024, src_len=1 << 20, desc=2048, table=4096, dst=8192, dst_len=1 << 20)
    cases = [(dict(src=None), b'null'), (dict(desc=None), b'null'), (dict(table=None), b'null'),
             (dict(dst=None), b'null'), (dict(n_utt=0), b'n_utt'), (dict(n_utt=-3), b'n_utt'),
             (dict(src=1026), b'misaligned'), (dict(dst=8194), b'misaligned'), (dict(desc=2052), b'misaligned'),
             (dict(table=4104), b'misaligned'), (dict(src_len=-1), b'src_len'), (dict(dst_len=(1 << 40) + 1), b'dst_len')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_speed_resample(*a.values()) == -1, kw
        assert msg in lib.danet_speed_last_error(), (kw, lib.danet_speed_last_error())
    assert _lib.speed_check(0) is None
    assert lib.danet_speed_resample(None, 1, None, 0, None, None, None, 0) == -1
    text = lib.danet_speed_last_error().decode()
    assert 'null' in text
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.speed_check(-1)
    assert str(e.value) == 'libdanet_speed_hip error -1: %s' % text


# ------------------------------------------------------------------------------------- the rule
def test_out_len_against_the_restatement():
    from danet_amd import _lib, ops
    lib = _lib.load_speed()
    assert lib.danet_speed_out_len(1000, 576) == 889 == SR.out_len(1000, 576)
    for L in (1, 2, 255, 256, 1000, 8128, 160000):
        assert lib.danet_speed_out_len(L, 512) == L
        for p in (384, 487, 511, 512, 513, 541, 576, 640):
            want = SR.out_len(L, p)
            assert lib.danet_speed_out_len(L, p) == want == int(ops.speed_out_len(L, p)), (L, p)
            # the last output's centre tap lies inside the utterance, the next one's would not
            assert (want - 1) * p <= (L - 1) * 512 < want * p
    for L, p in ((0, 512), (-5, 512), (100, 383), (100, 641), ((1 << 40) + 1, 512)):
        assert lib.danet_speed_out_len(L, p) == -1
        assert b'out_len' in lib.danet_speed_last_error()


def test_table_is_the_restated_one():
    from danet_amd import ops
    t0 = ops.speed_table(0.0)
    assert t0.dtype == np.float32 and t0.shape == (SR.Q, 2 * SR.Z)
    impulse = np.zeros(2 * SR.Z, np.float32)
    impulse[SR.Z - 1] = 1.0
    assert np.array_equal(t0[0].view(np.uint32), impulse.view(np.uint32))      # fc = 1: the unit impulse, +0 elsewhere
    for P in (0.0, 0.1, 0.25):
        ref = SR.table(P)
        assert np.array_equal(ops.speed_table(P).view(np.uint32), ref.view(np.uint32)), P
    # DC gain: a Hann-windowed sinc of 16 lobes a side ripples less than 1e-3 about 1 -- first on the
    # restatement, then on the table the dataset uploads
    for tab in (SR.table(0.1), ops.speed_table(0.1)):
        sums = tab.astype(np.float64).sum(axis=1)
        print('DC gain of the P = 0.1 table: %.3g ... %.3g about 1' % (sums.min() - 1, sums.max() - 1))
        assert np.abs(sums - 1.0).max() <= 1e-3
    assert abs(float(SR.table(0.1)[0, SR.Z - 1]) - 1 / 1.1) < 1e-7              # h(0) = fc


def test_sequential_float32_sum_meets_the_bar_of_the_gpu_test():
    rng = np.random.RandomState(3)
    tab = SR.table(0.1)
    for L, p in ((33, 384), (257, 487), (4097, 541), (4097, 640), (1000, 512)):
        x = (rng.standard_normal(L) * 3000).astype(np.int16).astype(np.float32)
        y64, S = SR.resample(x, p, tab)
        y32 = SR.resample_f32(x, p, tab)
        assert len(y64) == SR.out_len(L, p)
        err = np.abs(y32.astype(np.float64) - y64)
        print('L %d p %d: worst error / bar %.3f' % (L, p, (err / SR.bound(S)).max()))
        assert (err <= SR.bound(S)).all()
    # the P = 0 table at p = Q is the identity
    x = (rng.standard_normal(500) * 3000).astype(np.float32)
    assert np.array_equal(SR.resample_f32(x, 512, SR.table(0.0)).view(np.uint32), x.view(np.uint32))


# ----------------------------------------------------------------------------------- configuration
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
        _write(os.path.join(root, subset, 'u%02d.wav' % n), (rng.randn(260) * 500).astype(np.int16))    # 260 * 0.9 < 256


def _loaded(hp, tmp_path, **keys):
    '''a loaded dataset whose power table comes from the host restatement (no device)'''
    from danet_amd import datasets
    root = str(tmp_path / 'speed')
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
    ds = datasets.WavDirData()
    assert datasets.WavDirData.speed_perturb_range() is None and ds.speed_range is None
    assert ds.speed_stream('train') is None


@pytest.mark.parametrize('bad', [-0.1, 0.3, 'x', float('nan'), True])
def test_bad_values_raise_and_name_the_key(hp, tmp_path, bad):
    from danet_amd import datasets
    root = str(tmp_path / 'speed')
    _tree(root, n=2)
    hp.load({'DATASET_TYPE': 'wavdir', 'DATASET_DIR': root, KEY: bad})
    hp.digest()
    ds = datasets.WavDirData()
    with pytest.raises(ValueError, match=KEY):
        ds.install_and_load()
    assert not ds.is_loaded


def test_every_other_dataset_ignores_the_key(hp):
    hp.load({KEY: 'fast'})
    hp.digest()
    ds = hp.get_dataset()()
    ds.install_and_load()
    assert hp.DATASET_TYPE == 'toy' and next(iter(ds.epoch('train', 4)))[0].shape[0] == 4


def _epoch_plan(ds, subset, shuffle=False):
    return [(idx.copy(), T, list(p), b, c, None if g is None else g.copy(),
             None if s is None else (s[0].copy(), s[1].copy()))
            for idx, T, p, b, c, g, s in ds.plan_epoch_speed(subset, 4, shuffle, 8, crop=True)]


def test_key_null_maps_nothing_and_plans_what_it_always_did(hp, tmp_path):
    import prep_ref as P
    ds = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0)
    assert ds.speed_range is None
    random.seed(11)
    np.random.seed(12)
    got = _epoch_plan(ds, 'train', shuffle=True)
    state = random.getstate(), np.random.get_state()[1].copy()
    assert ds._speed_rng == {} and ds._speed_table == {} and ds._speed_scratch == {}
    random.seed(11)
    np.random.seed(12)
    rng = M.stream(0, 'train')
    for (idx, T_max, pads, beg, cnt, gains, speed), want_idx in zip(got, P.index_plan(12, 4, True)):
        assert np.array_equal(idx, want_idx) and speed is None
        assert (T_max, pads) == P.draw_pads([int(ds.frames['train'][i]) for i in idx])
        assert (beg, cnt) == P.draw_crop(T_max, 8)
        assert np.array_equal(gains, M.gains(ds.power['train'][idx], rng, 2, 5.0, None))
    assert state[0] == random.getstate() and np.array_equal(state[1], np.random.get_state()[1])
    # and a process that plans an epoch with the key null never maps the library
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, datasets\n"
        "from danet_amd.hparams import hparams\n"
        "hparams.load(json.loads(%r)); hparams.digest()\n"
        "ds = datasets.WavDirData(); ds.load_host(); ds.is_loaded = True\n"
        "n = len(list(ds.plan_epoch('train', 4, True, 8, crop=True)))\n"
        "print('PLANNED:', n, 'UNMAPPED:', _lib._speed is None and 'libdanet_speed' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, __import__('json').dumps(dict(DATASET_TYPE='wavdir', DATASET_DIR=str(tmp_path / 'speed'), FFT_SIZE=256,
                                            FFT_STRIDE=64, SPEED_PERTURB_RANGE=None)))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'PLANNED: 3 UNMAPPED: True' in out.stdout, out.stdout + out.stderr


def test_key_set_plans_the_drawn_lengths_and_leaves_every_other_stream_alone(hp, tmp_path):
    import prep_ref as P

    def run(**keys):
        hp.reset()
        ds = _loaded(hp, tmp_path, MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0, **keys)
        random.seed(11)
        np.random.seed(12)
        plan = _epoch_plan(ds, 'train', shuffle=True) + _epoch_plan(ds, 'train', shuffle=True)
        return plan, np.random.get_state()[1].copy(), ds
    off, n0, _ = run()
    on, n1, ds = run(SPEED_PERTURB_RANGE=0.1)
    assert np.array_equal(n0, n1)                                  # np.random: the shuffles only
    assert len(off) == len(on) == 6
    rng = SR.stream(0, 'train')                                    # ONE stream, on across both epochs
    random.seed(11)
    seen = set()
    for a, b in zip(off, on):
        idx, T_max, pads, beg, cnt, gains, (p, Lp) = b
        assert np.array_equal(a[0], idx) and a[6] is None
        assert np.array_equal(a[5], gains)                         # the mix draws: the same with the key on or off
        want_p, want_L = SR.draw(ds.lengths['train'][idx], rng, 0.1, 256)
        assert np.array_equal(p, want_p) and np.array_equal(Lp, want_L) and p.dtype == Lp.dtype == np.int64
        assert all(int(l) == SR.out_len(L, q) for l, L, q in zip(Lp, ds.lengths['train'][idx], p))
        assert p.min() >= 512 - 51 and p.max() <= 512 + 51 and Lp.min() >= 256
        seen.update(int(v) for v in p)
        for i, q in zip(idx, p):                                   # the 260-sample file cannot be sped up
            if ds.lengths['train'][i] == 260:
                assert q <= 512 and SR.out_len(260, int(q)) >= 256
        # `random`: the pads and the crop of the NEW lengths, nothing else
        frames = [P.num_frames(int(l), 256, 64) for l in Lp]
        assert (T_max, pads) == P.draw_pads(frames)
        assert (beg, cnt) == P.draw_crop(T_max, 8)
    assert len(seen) > 10 and any(v != 512 for v in seen)
    # the short file drew a speed that would have left it under FFT_SIZE at least once in the restatement
    # (u > 0.016 does it: 260 * 512 / 521 < 256), so the rule's exception was exercised
    rng = SR.stream(0, 'train')
    hit = 0
    for b in on:
        u = rng.uniform(-0.1, 0.1, size=4)
        hit += int(np.any((ds.lengths['train'][b[0]] == 260) & (512 + np.rint(512 * u) > 520)))
    assert hit >= 1


def test_speed_draws_touch_neither_random_nor_np_random(hp, tmp_path):
    from danet_amd import datasets
    rng = np.random.RandomState(5)
    random.seed(1)
    np.random.seed(2)
    s0, n0 = random.getstate(), np.random.get_state()[1].copy()
    p, Lp = datasets.WavDirData.plan_speed(np.asarray([300, 5000, 260, 100000]), rng, 0.1, 256)
    assert random.getstate() == s0 and np.array_equal(np.random.get_state()[1], n0)
    want = SR.draw([300, 5000, 260, 100000], np.random.RandomState(5), 0.1, 256)
    assert np.array_equal(p, want[0]) and np.array_equal(Lp, want[1])
    # P = 0 still draws (the number of draws depends on shapes alone) and every p is Q
    a = np.random.RandomState(9)
    p, Lp = datasets.WavDirData.plan_speed(np.asarray([300, 5000]), a, 0.0, 256)
    assert p.tolist() == [512, 512] and Lp.tolist() == [300, 5000]
    b = np.random.RandomState(9)
    b.uniform(size=2)
    assert a.randint(1 << 30) == b.randint(1 << 30)
    ds = _loaded(hp, tmp_path, SPEED_PERTURB_RANGE=0.25)
    assert ds.speed_range == 0.25 and ds.speed_stream('train') is ds.speed_stream('train')


def test_valid_and_test_are_never_perturbed_and_ranks_draw_differently(hp, tmp_path, monkeypatch):
    from danet_amd import dist
    ds0 = _loaded(hp, tmp_path, SPEED_PERTURB_RANGE=0.1)
    for subset in ('valid', 'test'):
        assert ds0.speed_stream(subset) is None
        random.seed(4)
        with_key = _epoch_plan(ds0, subset)
        assert all(item[6] is None for item in with_key)
    hp.reset()
    ds = _loaded(hp, tmp_path)
    for subset in ('valid', 'test'):
        random.seed(4)
        without = _epoch_plan(ds, subset)
        random.seed(4)
        with_key = _epoch_plan(ds0, subset)
        for a, b in zip(without, with_key):
            assert np.array_equal(a[0], b[0]) and a[1:5] == b[1:5]
    assert list(ds0._speed_rng) in ([], ['train'])
    hp.reset()
    ds0 = _loaded(hp, tmp_path, SPEED_PERTURB_RANGE=0.1)
    a = _epoch_plan(ds0, 'train')
    monkeypatch.setattr(dist, 'rank', lambda: 1)
    ds1 = _loaded(hp, tmp_path, SPEED_PERTURB_RANGE=0.1)
    b = _epoch_plan(ds1, 'train')
    assert not any(np.array_equal(x[6][0], y[6][0]) for x, y in zip(a, b))
    rng = SR.stream(1, 'train')
    for x in b:
        assert np.array_equal(x[6][0], SR.draw(ds1.lengths['train'][x[0]], rng, 0.1, 256)[0])
    # the train stream runs on: a second epoch over the same utterances draws new speeds
    c = _epoch_plan(ds1, 'train')
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(b, c))
    assert not any(np.array_equal(x[6][0], y[6][0]) for x, y in zip(b, c))


def test_descriptor_validation_is_on_the_host():
    from danet_amd import ops
    d = ops.speed_desc([0, 100], [100, 50], [0, 200], [100, 50], [512, 640], 150, 400)
    assert d.dtype == ops.SPEED_DESC_DTYPE and d['p'].tolist() == [512, 640] and d['reserved'].tolist() == [0, 0]
    for kw, msg in ((dict(p=[383, 512]), 'p = 383'), (dict(p=[512, 641]), 'p = 641'),
                    (dict(src_lengths=[100, 51]), 'outside the pool'), (dict(src_offsets=[-1, 100]), 'outside the pool'),
                    (dict(dst_offsets=[0, 99]), 'apart from each other'), (dict(dst_offsets=[0, 351]), 'inside the buffer')):
        a = dict(src_offsets=[0, 100], src_lengths=[100, 50], dst_offsets=[0, 200], dst_lengths=[100, 50], p=[512, 640],
                 src_len=150, dst_len=400)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.speed_desc(**a)
