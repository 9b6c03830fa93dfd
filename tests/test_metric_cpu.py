'''
CPU tests (no GPU) of the waveform metric of valid / test (EVAL_SI_SDR): the extension library
libdanet_metric_hip.so against its header (exports, prototypes, ABI, lazy load, host-visible argument errors), the
untouched other seven libraries, the open EXTENSIONS registry and build_all, the configuration key, and known
answers of the restatement tests/metric_ref.py.
'''
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import metric_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_metric_hip.h')
METRIC_SYMBOLS = ['danet_metric_abi_version', 'danet_metric_gram', 'danet_metric_last_error', 'danet_metric_si_sdr',
                  'danet_metric_synth', 'danet_metric_workspace_bytes']
KEY = 'EVAL_SI_SDR'


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
def test_metric_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_metric()
    syms = _header_symbols('danet_metric_hip.h', 'danet_metric_')
    assert syms == METRIC_SYMBOLS
    assert sorted(_lib.METRIC_PROTOTYPES) == syms
    assert _exports(_lib.METRIC_LIB_PATH) == syms
    assert lib.danet_metric_abi_version() == 1 == _lib.METRIC_ABI_VERSION == _lib.METRIC.abi
    txt = open(HEADER).read()
    assert '#define DANET_METRIC_ABI_VERSION 1' in txt and '#define DANET_METRIC_MAX_C 4' in txt
    assert 'COMPUTED IN THE KERNEL' in txt                     # where the twiddles come from
    assert _lib.METRIC.prototypes is _lib.METRIC_PROTOTYPES and _lib.METRIC.prefix == 'danet_metric_'
    out = subprocess.run(['nm', '-D', _lib.METRIC_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree'):
        assert word not in out.stdout, word


def test_the_wave_metric_core_is_defined_once_and_in_the_shared_header():
    build = importlib.import_module('danet-tensorflow_amd._build')
    csrc = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc')
    shared = os.path.join(csrc, 'wave_metric.h')
    files = [shared] + [os.path.join(csrc, n, n + '.hip') for n in ('metric', 'neval', 'wavloss')]
    code = {f: re.sub(r'/\*.*?\*/', '', open(f).read(), flags=re.S) for f in files}
    # radix2_stages: the radix-2 stage loop over all frames of a tile, of the synthesis and of wavloss_bwd_kernel
    for name in ('floor_div', 'block_sum_f64', 'nth_perm', 'sdr_db', 'tiling_of', 'radix2_stages'):
        # a definition: the name after a type, its parameter list, then a body
        define = re.compile(r'[\w>&*]\s+%s\s*\([^;{}()]*\)\s*\{' % name)
        counts = {f: len(define.findall(txt)) for f, txt in code.items()}
        assert counts[shared] == 1 and sum(counts.values()) == 1, (name, counts)
    for f in files[1:]:
        assert '#include "wave_metric.h"' in code[f], f
        assert re.search(r'\bblock_sum_f64\s*\(', code[f]), f                 # and every library uses the core
    # its two callers: synth_tile in the header, wavloss_bwd_kernel
    assert code[shared].count('radix2_stages(') == 2 and code[files[3]].count('radix2_stages(') == 1
    for spec in (build.METRIC, build.NEVAL, build.WAVLOSS):
        assert shared in spec.headers, spec.out
        assert spec.headers[0] == os.path.join(ROOT, 'include', 'danet_%s_hip.h' % os.path.basename(spec.src_dir))


def test_metric_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'const float*': ctypes.c_void_p,
             'float*': ctypes.c_void_p, 'const double*': ctypes.c_void_p, 'double*': ctypes.c_void_p,
             'int32_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.METRIC_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)


def test_extensions_is_an_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.METRIC in _lib.EXTENSIONS and build.METRIC in build.EXTENSIONS
    assert isinstance(_lib.METRIC, _lib.Library) and isinstance(build.METRIC, build.Library)
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert _lib.METRIC not in older and build.METRIC not in build.LIBRARIES + build.LATER_LIBRARIES
    assert [lib.name for lib in _lib.EXTENSIONS] == [os.path.basename(spec.src_dir) for spec in build.EXTENSIONS]
    assert build.METRIC_LIB == build.METRIC.out == _lib.METRIC_LIB_PATH
    assert os.path.basename(build.METRIC_LIB) == _lib.METRIC.so == 'libdanet_metric_hip.so'
    assert os.path.isfile(os.path.join(build.METRIC.src_dir, 'exports.map'))
    assert callable(build.build_metric) and callable(_lib.load_metric) and callable(_lib.metric_check)
    # a stubbed build helper: build() still builds the seven older libraries, build_all() those and metric
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
    assert build.METRIC in rest and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 8
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_seven_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert [spec.name for spec in older] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed', 'reverb']
    assert [spec.abi for spec in older] == [7, 1, 1, 1, 1, 1, 1]
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_metric_') for s in exported), spec.so


def test_import_maps_nothing_and_a_missing_file_is_a_loud_error(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, datasets\n"
        "print('UNMAPPED:', _lib._metric is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "_lib.METRIC_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_metric()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_metric_hip.so' in str(e) and %r in str(e)\n"
        "          and 'EVAL_SI_SDR' in str(e))\n"
        "print('NONE:', _lib._metric is None)\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'UNMAPPED: True' in out.stdout and 'LOUD: True' in out.stdout and 'NONE: True' in out.stdout, \
        out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_metric()
    ok = dict(stream=None, B=2, C=2, T=9, N=256, S=64, ref=1024, est=2048, window=4096, wav=8192)
    cases = [(dict(T=1), b'T must be >= 2'), (dict(T=0), b'T must'), (dict(N=192), b'power of two'),
             (dict(N=32, S=8), b'power of two'), (dict(N=2048, S=512), b'power of two'), (dict(S=129), b'S must'),
             (dict(S=31), b'S must'), (dict(S=0), b'S must'), (dict(B=0), b'B and C'), (dict(C=0), b'B and C'),
             (dict(ref=None), b'null'), (dict(est=None), b'null'), (dict(window=None), b'null'), (dict(wav=None), b'null'),
             (dict(ref=1028), b'misaligned'), (dict(est=2052), b'misaligned'), (dict(window=4098), b'misaligned'),
             (dict(wav=8193), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_metric_synth(*a.values()) == -1, kw
        assert msg in lib.danet_metric_last_error(), (kw, lib.danet_metric_last_error())
    ok = dict(stream=None, B=2, M=4, Ls=100, wav=1024, G=2048)
    for kw, msg in [(dict(B=0), b'B must'), (dict(M=0), b'M must'), (dict(M=9), b'M must'), (dict(Ls=0), b'Ls must'),
                    (dict(Ls=1 << 31), b'Ls must'), (dict(wav=None), b'null'), (dict(G=None), b'null'),
                    (dict(wav=1026), b'misaligned'), (dict(G=2052), b'misaligned')]:
        a = dict(ok, **kw)
        assert lib.danet_metric_gram(*a.values()) == -1, kw
        assert msg in lib.danet_metric_last_error(), (kw, lib.danet_metric_last_error())
    ok = dict(stream=None, B=2, C=2, G=1024, per_utt=2048, perm_idx=4096, mean2=8192)
    for kw, msg in [(dict(B=0), b'B must'), (dict(C=0), b'C must'), (dict(C=5), b'C must'), (dict(G=None), b'null'),
                    (dict(per_utt=None), b'null'), (dict(perm_idx=None), b'null'), (dict(mean2=None), b'null'),
                    (dict(G=1028), b'misaligned'), (dict(perm_idx=4098), b'misaligned')]:
        a = dict(ok, **kw)
        assert lib.danet_metric_si_sdr(*a.values()) == -1, kw
        assert msg in lib.danet_metric_last_error(), (kw, lib.danet_metric_last_error())
    # the layout the header gives: five parts, each rounded up to a multiple of 256 bytes
    r = lambda n: (n + 255) & ~255
    for B, C, T, N, S in ((32, 2, 128, 256, 64), (1, 1, 2, 64, 32), (3, 4, 130, 1024, 128)):
        Ls = (T - 1) * S
        want = r(B * 2 * C * Ls * 4) + r(B * 4 * C * C * 8) + r(B * 16) + r(16) + r(B * 4)
        assert lib.danet_metric_workspace_bytes(B, C, T, N, S) == want
    bad = ctypes.c_size_t(-1).value
    for args in ((1, 5, 9, 256, 64), (1, 1, 1, 256, 64), (1, 1, 9, 100, 25), (1, 1, 9, 256, 192), (0, 1, 9, 256, 64)):
        assert lib.danet_metric_workspace_bytes(*args) == bad, args
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.metric_check(-1)
    assert str(e.value).startswith('libdanet_metric_hip error -1: ')
    assert _lib.metric_check(0) is None


# ----------------------------------------------------------------------------------- configuration
def test_key_default_is_null_and_off(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    assert KEY in H.DEFAULTS and H.DEFAULTS[KEY] is None and getattr(hp, KEY) is None
    assert re.fullmatch(hp.pattern, KEY)
    assert KEY in H.__doc__
    hp.digest()
    assert Model._check_eval_si_sdr() is False
    hp.load({KEY: False})
    assert Model._check_eval_si_sdr() is False
    hp.load({KEY: True})
    assert Model._check_eval_si_sdr() is True


@pytest.mark.parametrize('keys,name', [({KEY: 1}, KEY), ({KEY: 'yes'}, KEY), ({KEY: 0.5}, KEY),
                                       ({KEY: True, 'FFT_SIZE': 64, 'FFT_STRIDE': 48}, 'FFT_STRIDE'),
                                       ({KEY: True, 'FFT_SIZE': 256, 'FFT_STRIDE': 16}, 'FFT_STRIDE'),
                                       ({KEY: True, 'FFT_SIZE': 2048, 'FFT_STRIDE': 512}, 'FFT_SIZE'),
                                       ({KEY: True, 'FFT_SIZE': 96, 'FFT_STRIDE': 24}, 'FFT_SIZE'),
                                       ({KEY: True, 'MAX_N_SIGNAL': 5}, 'MAX_N_SIGNAL')])
def test_build_raises_and_names_the_offending_key(hp, keys, name):
    from danet_amd.model import Model
    hp.load(keys)
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('metric', device='cuda:0').build()             # raised before anything touches a device
    assert re.search(r'\b%s\b' % name, str(e.value))
    if keys.get('FFT_STRIDE') == 48:
        assert 'window edges' in str(e.value) and 'LDS' not in str(e.value)
    if keys.get('FFT_STRIDE') == 16:
        assert 'LDS' in str(e.value) and 'window edges' not in str(e.value)
    others = {KEY, 'FFT_STRIDE', 'MAX_N_SIGNAL'} - {name}
    if name != KEY:
        assert not any(re.search(r'\b%s (must|=)' % o, str(e.value)) for o in others - {KEY})
    # with the key off none of them is looked at
    hp.load({KEY: None})
    assert Model._check_eval_si_sdr() is False
    hp.load({KEY: False})
    assert Model._check_eval_si_sdr() is False


def test_window_sum_stays_away_from_zero_up_to_half_a_window():
    '''the figures of the FFT_STRIDE rule: min over n of sum_t w^2 for the project's sqrt-hann window'''
    assert abs(MR.window_sum_min(_sqrt_hann(64), 32) - 0.975) < 2e-3
    for N in (64, 256, 1024):
        assert abs(MR.window_sum_min(_sqrt_hann(N), N // 4) - 1.5) < 0.05
        assert MR.window_sum_min(_sqrt_hann(N), N // 8) > 1.5
    # beyond N/2 the cover thins out towards the window edges, down to nothing
    assert MR.window_sum_min(_sqrt_hann(64), 48) < 0.3 and MR.window_sum_min(_sqrt_hann(64), 64) == 0.0


# ------------------------------------------------------------------- known answers of the restatement
def _spectra(rng, B, C, T, N):
    F = N // 2 + 1
    return (rng.standard_normal((B, C, T, F)) + 1j * rng.standard_normal((B, C, T, F))).astype(np.complex64)


def test_swapped_estimates_give_100_db_and_the_swapped_permutation():
    rng = np.random.RandomState(0)
    w = _sqrt_hann(64)
    S = _spectra(rng, 3, 2, 9, 64)
    per_utt, perm, mean2 = MR.si_sdr(S, S[:, ::-1], w, 16)
    assert np.array_equal(per_utt[:, 0], [100.0] * 3) and np.array_equal(perm, [1, 1, 1]) and mean2[0] == 100.0
    S3 = _spectra(rng, 2, 3, 9, 64)
    per_utt, perm, _ = MR.si_sdr(S3, S3[:, [2, 0, 1]], w, 16)      # estimate j = reference order[j]
    assert np.array_equal(per_utt[:, 0], [100.0] * 2)
    import itertools
    assert [list(itertools.permutations(range(3)))[p] for p in perm] == [(1, 2, 0)] * 2


def test_scaling_changes_nothing():
    rng = np.random.RandomState(1)
    w = _sqrt_hann(64)
    S = _spectra(rng, 2, 2, 12, 64)
    E = (S[:, ::-1] + 0.3 * _spectra(rng, 2, 2, 12, 64)).astype(np.complex64)
    base = MR.si_sdr(S, E, w, 16)
    for which, c, k in (('E', 0, 7.5), ('E', 1, 0.01), ('S', 0, 3.0), ('S', 1, 0.125)):
        S2, E2 = S.astype(np.complex128), E.astype(np.complex128)
        (E2 if which == 'E' else S2)[:, c] *= k
        got = MR.si_sdr(S2, E2, w, 16)
        if which == 'E':
            assert np.abs(got[0] - base[0]).max() <= 1e-9          # SI-SDR and SI-SDRi
        else:
            assert np.abs(got[0][:, 0] - base[0][:, 0]).max() <= 1e-9      # (the mixture changes with a reference)
        assert np.array_equal(got[1], base[1])
    assert np.array_equal(base[1], [1, 1])


def test_mixture_as_estimate_has_no_improvement():
    rng = np.random.RandomState(2)
    w = _sqrt_hann(64)
    for C in (1, 2, 3):
        S = _spectra(rng, 2, C, 10, 64).astype(np.complex128)
        E = np.repeat(S.sum(axis=1, keepdims=True), C, axis=1)
        per_utt, _, mean2 = MR.si_sdr(S, E, w, 32)
        assert np.abs(per_utt[:, 1]).max() <= 1e-9 and abs(mean2[1]) <= 1e-9


def test_hand_made_cases():
    # s and n orthogonal, e = s + 0.1 n: 10 log10(|s|^2 / |0.1 n|^2) = 20 dB
    s, n = np.array([1.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, -1.0])
    wav = np.stack([s, s + 0.1 * n])[None]
    per_utt, perm, mean2 = MR.finalize(MR.gram(wav), 1)
    assert abs(per_utt[0, 0] - 20.0) <= 1e-9 and perm[0] == 0 and abs(mean2[0] - 20.0) <= 1e-9
    assert MR.sdr(2.0, 2.0, 0.0) == -100.0 and MR.sdr(2.0, 0.0, 0.0) == -100.0 and MR.sdr(2.0, 2.0, 2.0) == 100.0
    # one silent reference is left out of the mean: (20 dB, silent) -> 20, not 10 or -40
    z = np.zeros(4)
    wav = np.stack([s, z, s + 0.1 * n, n])[None]
    per_utt, perm, _ = MR.finalize(MR.gram(wav), 2)
    assert abs(per_utt[0, 0] - 20.0) <= 1e-9 and perm[0] == 0
    wav = np.stack([z, s, s + 0.1 * n, n])[None]                    # the live reference is the second one
    per_utt, perm, _ = MR.finalize(MR.gram(wav), 2)
    assert abs(per_utt[0, 0] - 20.0) <= 1e-9 and perm[0] == 1
    # all references silent: 0, and the utterance does not count in the batch mean
    wav = np.stack([np.stack([z, z, s, n]), np.stack([s, n, s + 0.1 * n, n + 0.1 * s])])
    per_utt, perm, mean2 = MR.finalize(MR.gram(wav), 2)
    assert np.array_equal(per_utt[0], [0.0, 0.0]) and perm[0] == 0
    assert abs(per_utt[1, 0] - 20.0) <= 1e-9 and abs(mean2[0] - 20.0) <= 1e-9
    per_utt, perm, mean2 = MR.finalize(MR.gram(wav[:1]), 2)
    assert np.array_equal(mean2, [0.0, 0.0])
    # ties go to the first permutation
    wav = np.stack([s, n, s + n, s + n])[None]
    assert MR.finalize(MR.gram(wav), 2)[1][0] == 0


@pytest.mark.parametrize('N,S', [(64, 16), (64, 32), (256, 64), (512, 128)])
def test_synthesis_inverts_the_stft(N, S):
    rng = np.random.RandomState(N + S)
    w = _sqrt_hann(N)
    for L in (N, N + 1, 5 * S + 3, 8128):
        x = rng.standard_normal(L)
        X = MR.stft(x, w, N, S)                                    # scipy's, cast to complex64
        y = MR.synth(X, w, S) * float(np.sum(w.astype(np.float64)))
        n = min(L, y.shape[-1])
        err = np.abs(y[:n] - x[:n]).max() / np.abs(x).max()
        print('N %d S %d L %d: T %d, worst error %.3g of max|x|' % (N, S, L, X.shape[0], err))
        assert n >= min(L, (X.shape[0] - 1) * S) and err <= 1e-6
