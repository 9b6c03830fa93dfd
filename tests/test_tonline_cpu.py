'''
CPU tests (no GPU) of the truth-online estimator (TRAIN_ESTIMATOR_METHOD = "truth-online"): the extension library
libdanet_tonline_hip.so against its header (exports, prototypes, ABI, lazy load, every host-visible argument error),
the untouched other twenty libraries, the open MORE_EXTENSIONS registry, the registry entry and every ValueError, and
the numpy restatement of tests/tonline_ref.py against itself: the closed-form backward against torch float64 autograd,
the oracle's truth-weighted attractors, causality, the silent prefix, and the float32 run inside the header's bound.
'''
import ctypes
import hashlib
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import csrc_scan
import online_ref as OR
import tonline_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_tonline_hip.h')
ENTRY_POINTS = ['frame_sums', 'scan', 'scan_bwd', 'separate_bwd', 'sums_bwd']
TONLINE_SYMBOLS = sorted(['danet_tonline_abi_version', 'danet_tonline_last_error']
                         + ['danet_tonline_' + n for n in ENTRY_POINTS])
# the export lists of the twenty older libraries: sha1 of their sorted, space-joined names (first 12 digits)
OLDER = {'': (51, '35c97f3a2452'), 'conv': (7, '9446af6b053c'), 'dropout': (3, '31a0846a9f05'),
         'prep': (6, '4528d8ffdc78'), 'mix': (5, 'a519a2795d7a'), 'speed': (4, 'e1adf1c490af'),
         'reverb': (3, '05ef787913e5'), 'metric': (6, 'eff9d5e3632c'), 'noise': (3, 'cf88e352bf83'),
         'level': (4, '7fdea6b0fb6a'), 'wavloss': (4, 'e9c25e57750d'), 'gclip': (5, 'a9921dcbc5d9'),
         'dpcl': (7, '8021ee69c5d3'), 'neval': (6, '44b1be58a6d8'), 'stitch': (7, '2ab75117a25c'),
         'bss': (7, '265172254200'), 'stoi': (8, '476adf4d55ec'), 'phase': (6, 'abe3128b0d70'),
         'online': (6, '37411e8747f2'), 'causal': (7, 'e4e4a3d9d800')}


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_tonline_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_tonline()
    syms = _header_symbols('danet_tonline_hip.h', 'danet_tonline_')
    assert syms == TONLINE_SYMBOLS
    assert sorted(_lib.TONLINE_PROTOTYPES) == syms
    assert _exports(_lib.TONLINE_LIB_PATH) == syms
    assert lib.danet_tonline_abi_version() == 1 == _lib.TONLINE_ABI_VERSION == _lib.TONLINE.abi
    txt = open(HEADER).read()
    assert '#define DANET_TONLINE_ABI_VERSION 1' in txt
    for name, value in (('C', TR.MAX_C), ('E', TR.MAX_E), ('F', TR.MAX_F), ('T', TR.MAX_T)):
        assert re.search(r'#define DANET_TONLINE_MAX_%s %d\b' % (name, value), txt), name
        assert re.search(r'#define DANET_ONLINE_MAX_%s %d\b' % (name, value),
                         open(os.path.join(ROOT, 'include', 'danet_online_hip.h')).read()), name   # the same envelope
    rule = txt.split('#ifndef')[0]
    for words in ('THE RULE', 'the lowest c that maximises P[c][t][f]', 'tf.argmax',
                  's_t[c][e] = sum_{f: k(t,f) = c} W[t][f] V[t][f][e]', 'q_t[c] = sum_{f: k(t,f) = c} W[t][f]',
                  'function of F alone', 'S_t = lambda S_{t-1} + s_t and n_t = lambda n_{t-1} + q_t, in float64 from zero',
                  'tau(t) = min(max(t, T0 - 1), T - 1)', 'A_t[c] = (float)(S_tau[c] / (n_tau[c] + eps))',
                  'rounded once', 'A source with no bin so far has A = 0', 'R_u = H_u + lambda R_{u+1} with R_T = 0',
                  'dV[u][f][e] = W[u][f] * (float)R_u[k(u,f)][e]', 'There is no gradient to W or P',
                  'silent over a prefix', 'softmax: dl_c = m_c (g_c - sum_j m_j g_j)', 'sigmoid: dl_c = (m_c (1 - m_c)) g_c',
                  'dA_t[c][e] = sum_f dl_c[f] V[t][f][e]', 'SUMMATION ORDER', 'blocks of 16', 'ERROR BOUND',
                  'N_s = ceil(F / G) + min(G, 16) + ceil(G / 16)', 'N_q = ceil(F / 256) + 9', 'no atomics',
                  'no persistent grid', 'B T F E, B C T F and B T C E below 2^31'):
        assert words in rule, words
    assert _lib.TONLINE.prototypes is _lib.TONLINE_PROTOTYPES and _lib.TONLINE.prefix == 'danet_tonline_'


def test_tonline_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    ctype = {'void*': p, 'int': ctypes.c_int, 'const float*': p, 'float*': p, 'void': None, 'double': ctypes.c_double,
             'const double*': p, 'double*': p}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.TONLINE_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.TONLINE_PROTOTYPES['danet_tonline_' + n][1]) for n in ENTRY_POINTS] == [11, 12, 10, 13, 10]


def test_tonline_is_in_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.TONLINE in _lib.MORE_EXTENSIONS and build.TONLINE in build.MORE_EXTENSIONS
    assert isinstance(_lib.TONLINE, _lib.Library) and isinstance(build.TONLINE, build.Library)
    closed = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert _lib.TONLINE not in closed and len(closed) == 14
    assert build.TONLINE not in build.LIBRARIES + build.LATER_LIBRARIES + build.EXTENSIONS
    # it follows the records that were there
    assert _lib.MORE_EXTENSIONS.index(_lib.TONLINE) > _lib.MORE_EXTENSIONS.index(_lib.CAUSAL) == 5
    assert build.MORE_EXTENSIONS.index(build.TONLINE) > build.MORE_EXTENSIONS.index(build.CAUSAL) == 5
    assert [lib.name for lib in _lib.MORE_EXTENSIONS] == [os.path.basename(spec.src_dir)
                                                          for spec in build.MORE_EXTENSIONS]
    assert build.TONLINE_LIB == build.TONLINE.out == _lib.TONLINE_LIB_PATH
    assert os.path.basename(build.TONLINE_LIB) == _lib.TONLINE.so == 'libdanet_tonline_hip.so'
    assert os.path.isfile(os.path.join(build.TONLINE.src_dir, 'exports.map'))
    assert build.TONLINE.headers == (HEADER, os.path.join(csrc_scan.CSRC, 'ext_core.h'))
    src = open(os.path.join(build.TONLINE.src_dir, 'tonline.hip')).read()
    assert set(csrc_scan.shared_headers(src)) == set(build.TONLINE.headers[1:])
    assert callable(build.build_tonline) and callable(_lib.load_tonline) and callable(_lib.tonline_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:13] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL,
                         build.STITCH, build.BSS, build.STOI, build.PHASE, build.ONLINE, build.CAUSAL]
    assert build.TONLINE in rest[13:] and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 21      # the twenty older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_twenty_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS + _lib.MORE_EXTENSIONS[:6]
    assert [spec.name for spec in older] == list(OLDER)
    assert [spec.abi for spec in older] == [7] + [1] * 19
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_tonline_') for s in exported), spec.so
        assert (len(exported), hashlib.sha1(' '.join(exported).encode()).hexdigest()[:12]) == OLDER[spec.name], spec.so


def test_tonline_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.TONLINE_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset', 'hipStreamSynchronize', 'hipDeviceSynchronize'):
        assert not re.search(r'\b%s\w*\b' % word, out.stdout), word
    d = os.path.join(csrc_scan.CSRC, 'tonline')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['tonline.hip']
    own = csrc_scan.strip_comments(open(os.path.join(d, 'tonline.hip')).read())
    code = own + csrc_scan.shared_code(own)           # and the shared header it includes
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', 'common.h', 'Synchronize',
                 'hipMemcpy', 'hipMemset', 'asm', 'cooperative', 'volatile'):
        assert word not in code, word
    # the preamble of every extension source
    assert own.count('#include "danet_tonline_hip.h"\n#define DANET_EXT tonline\n#define DANET_EXT_UPPER TONLINE\n'
                     '#include "ext_core.h"\n') == 1
    # five kernels, one per entry point; the frame sums and the separator's backward share one contraction
    assert len(re.findall(r'__global__', own)) == 5 and own.count('CHECK_LAUNCH();') == 5
    assert own.count('contract<') == 2 and own.count('block_sum(') == 3 and own.count('bin_label(') == 3
    # the logits and the activation are those of danet_online_separate, statement for statement
    online = csrc_scan.strip_comments(open(os.path.join(csrc_scan.CSRC, 'online', 'online.hip')).read())
    for fn in ('fma_chunk', 'bin_logits', 'activate'):
        body = lambda text: re.sub(r'\s*//[^\n]*', '', text[text.index('__device__ __forceinline__ void %s(' % fn):]
                                   .split('\n}\n')[0])
        assert body(own) == body(online), fn
    # every launch comes after every argument check of its entry point
    bodies = re.split(r'extern "C"', own)[1:]
    assert len(bodies) == 5
    for body in bodies:
        launches = [m.start() for m in re.finditer(r'<<<', body)]
        checks = [m.start() for m in re.finditer(r'CHECK_ARG\(|envelope_ok\(', body)]
        assert len(launches) == 1 and max(checks) < min(launches)


def test_import_and_a_model_with_another_estimator_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, modules, ozers, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "real, _lib.load_tonline = _lib.load_tonline, None         # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._tonline is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "hparams.load(dict(TRAIN_ESTIMATOR_METHOD='truth-online', INFER_ESTIMATOR_METHOD='online'))\n"
        "print('ON:', model.Model._check_online())\n"
        "_lib.load_tonline = real\n"
        "_lib.TONLINE_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_tonline()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_tonline_hip.so' in str(e) and %r in str(e)\n"
        "          and '\"truth-online\"' in str(e))\n"
        "print('NONE:', _lib._tonline is None and 'libdanet_tonline' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'ON: (32, 1.0)', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------- argument errors
FRAME_SHAPES = [(dict(B=0), b'need B >= 1'), (dict(T=0), b'need B >= 1'), (dict(T=65537), b'need B >= 1'),
                (dict(F=0), b'need 1 <= F'), (dict(F=1026), b'need 1 <= F'), (dict(C=0), b'need 1 <= C <= 4'),
                (dict(C=5), b'need 1 <= C <= 4'), (dict(E=0), b'need 1 <= C <= 4'), (dict(E=65), b'need 1 <= C <= 4'),
                (dict(B=64, T=65536, F=1025, E=1), b'must be < 2^31'), (dict(B=1 << 15, T=65536, F=1, E=1, C=1), b'must be < 2^31'),
                (dict(B=1024, T=65536, F=1, E=16, C=4), b'must be < 2^31'), (dict(B=1024, T=65536, F=16, E=1, C=4), b'must be < 2^31')]
SCAN_SHAPES = [(dict(B=0), b'need B >= 1'), (dict(T=0), b'need B >= 1'), (dict(T=65537), b'need B >= 1'),
               (dict(C=0), b'need 1 <= C <= 4'), (dict(C=5), b'need 1 <= C <= 4'), (dict(E=0), b'need 1 <= C <= 4'),
               (dict(E=65), b'need 1 <= C <= 4'), (dict(B=1024, T=65536, E=16, C=4), b'must be < 2^31')]
VALUES = [(dict(lam=0.0), b'0 < lambda <= 1'), (dict(lam=1.0000001), b'0 < lambda <= 1'), (dict(lam=-0.5), b'0 < lambda <= 1'),
          (dict(lam=float('nan')), b'0 < lambda <= 1'), (dict(T0=0), b'T0 >= 1'), (dict(T0=-3), b'T0 >= 1')]


def test_argument_errors_without_gpu():
    '''every host-visible argument error of the five entry points is returned before any launch: no device is needed
    to see them'''
    from danet_amd import _lib
    lib = _lib.load_tonline()
    err = lib.danet_tonline_last_error

    def refused(fn, who, ok, cases):
        for kw, msg in cases:
            assert fn(*dict(ok, **kw).values()) == -1, (who, kw)
            assert who in err() and msg in err(), (who, kw, err())

    ok = dict(stream=None, B=2, C=2, T=9, F=33, E=20, embed=4096, src_pwr=8192, w=16384, s=32768, q=65536)
    cases = list(FRAME_SHAPES) + [({k: None}, b'null') for k in ('embed', 'src_pwr', 'w', 's', 'q')]
    cases += [(dict(embed=4100), b'misaligned'), (dict(embed=4104), b'misaligned'), (dict(src_pwr=8194), b'misaligned'),
              (dict(w=16385), b'misaligned'), (dict(s=32770), b'misaligned'), (dict(q=65538), b'misaligned'),
              (dict(E=7, embed=4098), b'misaligned')]
    refused(lib.danet_tonline_frame_sums, b'frame_sums: ', ok, cases)
    ok = dict(stream=None, B=2, C=2, T=9, E=20, lam=0.9, T0=4, eps=1e-7, s=4096, q=8192, attr=16384, den=32768)
    cases = list(SCAN_SHAPES) + list(VALUES) + [(dict(eps=-1e-9), b'eps must be'), (dict(eps=float('inf')), b'eps must be'),
                                                (dict(eps=float('nan')), b'eps must be')]
    cases += [({k: None}, b'null') for k in ('s', 'q', 'attr', 'den')]
    cases += [(dict(s=4098), b'misaligned'), (dict(q=8193), b'misaligned'), (dict(attr=16386), b'misaligned'),
              (dict(den=32772), b'misaligned')]
    refused(lib.danet_tonline_scan, b'scan: ', ok, cases)
    ok = dict(stream=None, B=2, C=2, T=9, E=20, lam=0.9, T0=4, dattr=4096, den=8192, r=16384)
    cases = list(SCAN_SHAPES) + list(VALUES) + [({k: None}, b'null') for k in ('dattr', 'den', 'r')]
    cases += [(dict(dattr=4098), b'misaligned'), (dict(den=8196), b'misaligned'), (dict(r=16385), b'misaligned')]
    refused(lib.danet_tonline_scan_bwd, b'scan_bwd: ', ok, cases)
    ok = dict(stream=None, B=2, C=2, T=9, F=33, E=20, src_pwr=4096, w=8192, r=16384, dembed=32768)
    cases = list(FRAME_SHAPES) + [({k: None}, b'null') for k in ('src_pwr', 'w', 'r', 'dembed')]
    cases += [(dict(dembed=32772), b'misaligned'), (dict(src_pwr=4098), b'misaligned'), (dict(w=8193), b'misaligned'),
              (dict(r=16386), b'misaligned'), (dict(E=7, dembed=32770), b'misaligned')]
    refused(lib.danet_tonline_sums_bwd, b'sums_bwd: ', ok, cases)
    ok = dict(stream=None, act=0, B=2, C=2, T=9, F=33, E=20, w=4096, attr=8192, embed=16384, dout=32768, dembed=65536,
              dattr=131072)
    cases = list(FRAME_SHAPES) + [(dict(act=2), b'act must be'), (dict(act=-1), b'act must be')]
    cases += [({k: None}, b'null') for k in ('w', 'attr', 'embed', 'dout', 'dembed', 'dattr')]
    cases += [(dict(embed=16388), b'misaligned'), (dict(dembed=65544), b'misaligned'), (dict(w=4098), b'misaligned'),
              (dict(attr=8193), b'misaligned'), (dict(dout=32770), b'misaligned'), (dict(dattr=131074), b'misaligned'),
              (dict(E=7, dembed=65538), b'misaligned')]
    refused(lib.danet_tonline_separate_bwd, b'separate_bwd: ', ok, cases)
    assert _lib.tonline_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.tonline_check(-1)
    assert str(e.value).startswith('libdanet_tonline_hip error -1: separate_bwd: misaligned pointer')


# ----------------------------------------------------------------------------------- the registry and the keys
def test_the_estimator_is_registered_and_uses_the_truth(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    from danet_amd import modules, ops
    assert 'truth-online' in hp.estimator_registry and hp.get_estimator('truth-online') is modules.TruthOnlineEstimator
    assert modules.TruthOnlineEstimator.USE_TRUTH is True and issubclass(modules.TruthOnlineEstimator, modules.Estimator)
    assert 'truth-online' in H.__doc__ and hp.TRAIN_ESTIMATOR_METHOD == 'truth-weighted'
    assert not [k for k in H.DEFAULTS if 'TRUTH_ONLINE' in k or 'TONLINE' in k]         # no key of its own
    assert issubclass(ops.TruthOnlineAttractorFn, __import__('torch').autograd.Function)
    assert issubclass(ops.OnlineSeparateFn, __import__('torch').autograd.Function)
    for di, want in ((dict(), (32, 1.0)), (dict(ONLINE_INIT_FRAMES=4, ONLINE_MEMORY_FRAMES=8), (4, float(np.exp(-1 / 8))))):
        hp.reset()
        hp.load(dict(di, TRAIN_ESTIMATOR_METHOD='truth-online', INFER_ESTIMATOR_METHOD='online'))
        hp.digest()
        got = Model._check_online()
        assert got[0] == want[0] and abs(got[1] - want[1]) <= 1e-15


@pytest.mark.parametrize('keys,di', [
    (('TRAIN_ESTIMATOR_METHOD', 'INFER_ESTIMATOR_METHOD', 'truth-online'), dict(TRAIN_ESTIMATOR_METHOD='truth-online')),
    (('TRAIN_ESTIMATOR_METHOD', 'INFER_ESTIMATOR_METHOD', 'truth-online'),
     dict(TRAIN_ESTIMATOR_METHOD='truth-online', INFER_ESTIMATOR_METHOD='kmeans')),
    (('TRAIN_ESTIMATOR_METHOD', 'INFER_ESTIMATOR_METHOD', 'truth-online'),
     dict(TRAIN_ESTIMATOR_METHOD='truth-online', INFER_ESTIMATOR_METHOD='truth-online')),
    (('TRAIN_ESTIMATOR_METHOD', 'INFER_ESTIMATOR_METHOD', 'ONLINE_INIT_FRAMES'),
     dict(TRAIN_ESTIMATOR_METHOD='truth-online', ONLINE_INIT_FRAMES=4)),
    (('TRAIN_ESTIMATOR_METHOD', 'online'), dict(TRAIN_ESTIMATOR_METHOD='online')),
    (('TRAIN_ESTIMATOR_METHOD', 'online'), dict(TRAIN_ESTIMATOR_METHOD='online', INFER_ESTIMATOR_METHOD='online')),
    (('INFER_ESTIMATOR_METHOD', 'SEPARATOR_TYPE'),
     dict(TRAIN_ESTIMATOR_METHOD='truth-online', INFER_ESTIMATOR_METHOD='online', SEPARATOR_TYPE='no-act')),
    (('INFER_ESTIMATOR_METHOD', 'EMBED_SIZE'),
     dict(TRAIN_ESTIMATOR_METHOD='truth-online', INFER_ESTIMATOR_METHOD='online', EMBED_SIZE=65))])
def test_build_raises_and_names_the_keys(hp, keys, di):
    from danet_amd.model import Model
    from danet_amd import modules
    if di.get('SEPARATOR_TYPE') == 'no-act':
        @hp.register_separator('no-act')
        class NoAct(modules.Separator):
            pass
    try:
        hp.load(di)
        hp.digest()
        with pytest.raises(ValueError) as e:
            Model('tonline', device='cuda:0').build()         # raised before anything touches a device
        for key in keys:
            assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)
        if di == dict(TRAIN_ESTIMATOR_METHOD='online'):
            assert str(e.value) == ('TRAIN_ESTIMATOR_METHOD cannot be "online": the online estimator has no backward, it '
                                    'is an inference estimator (INFER_ESTIMATOR_METHOD)')
    finally:
        type(hp).separator_registry.pop('no-act', None)


def test_truth_online_as_the_inference_estimator_fails_like_any_truth_estimator(hp):
    from danet_amd.model import Model
    hp.load(dict(INFER_ESTIMATOR_METHOD='truth-online'))
    hp.digest()
    assert Model._check_online() is None
    with pytest.raises(AssertionError):
        Model('tonline', device='cuda:0').build()


# ----------------------------------------------------------------------------------- the restatement
def _grad_case(T, F, E, C, seed):
    V, W, P = TR.case(2, T, F, E, C, seed=seed)
    G, D = TR.grads(2, T, F, E, C, seed=seed)
    return V, W, P, G, D


@pytest.mark.parametrize('T0', [1, 4, 'T + 3'])
@pytest.mark.parametrize('lam', TR.LAMBDAS)
def test_the_closed_form_estimator_backward_is_torch_float64_autograd(lam, T0):
    import torch
    T = 9
    T0 = T + 3 if T0 == 'T + 3' else T0
    V, W, P, G, _ = _grad_case(T, 7, 5, 3, seed=T0)
    v = torch.tensor(V, dtype=torch.float64, requires_grad=True)
    attr = TR.torch_attractors(v, W, P, lam, T0, TR.EPS)
    want_attr, den = TR.attractors(V, W, P, lam, T0, TR.EPS)
    assert np.abs(attr.detach().numpy() - want_attr).max() <= 1e-12 * np.abs(want_attr).max()
    attr.backward(torch.tensor(G, dtype=torch.float64))
    want = v.grad.numpy()
    got = TR.attractors_bwd(G, den, W, P, lam, T0)
    assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('act', [0, 1])
def test_the_closed_form_separator_backward_is_torch_float64_autograd(act):
    import torch
    V, W, P, _, D = _grad_case(6, 9, 5, 3, seed=20 + act)
    A = TR.attractors(V, W, P, 0.9, 2, TR.EPS)[0]
    v = torch.tensor(V, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(A, dtype=torch.float64, requires_grad=True)
    out = TR.torch_separate(v, W, a, act)
    assert np.abs(out.detach().numpy() - OR.separate(V, W, A, act)).max() <= 1e-12 * np.abs(W).max()
    out.backward(torch.tensor(D, dtype=torch.float64))
    dV, dA = TR.separate_bwd(V, W, A, D, act)
    for got, want in ((dV, v.grad.numpy()), (dA, a.grad.numpy())):
        assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('T0', [1, 4, 'T + 3'])
@pytest.mark.parametrize('lam', TR.LAMBDAS)
def test_the_heads_chained_are_torch_float64_autograd(lam, T0, act):
    '''estimator and separator together: the embedding gradient is the sum of the two contributions'''
    import torch
    T = 9
    T0 = T + 3 if T0 == 'T + 3' else T0
    V, W, P, _, D = _grad_case(T, 7, 5, 2, seed=40 + act)
    v = torch.tensor(V, dtype=torch.float64, requires_grad=True)
    TR.torch_separate(v, W, TR.torch_attractors(v, W, P, lam, T0, TR.EPS), act).backward(torch.tensor(D, dtype=torch.float64))
    A, den = TR.attractors(V, W, P, lam, T0, TR.EPS)
    dV, dA = TR.separate_bwd(V, W, A, D, act)
    got = dV + TR.attractors_bwd(dA, den, W, P, lam, T0)
    want = v.grad.numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_lambda_one_and_a_hold_over_everything_is_the_oracles_truth_weighted():
    from oracle import danet_oracle
    V, W, P = TR.case(3, 11, 17, 6, 3, seed=5)
    want = danet_oracle.est_truth_weighted(V.astype(np.float64), P.astype(np.float64), W.astype(np.float64), eps=TR.EPS)
    for T0 in (11, 12, 500):
        attr = TR.attractors(V, W, P, 1.0, T0, TR.EPS)[0]
        assert np.abs(attr - want[:, None]).max() <= 1e-12 * np.abs(want).max()
    # a shorter hold or a forgetting factor gives something else
    assert np.abs(TR.attractors(V, W, P, 1.0, 4, TR.EPS)[0][:, :10] - want[:, None]).max() > 1e-4
    assert np.abs(TR.attractors(V, W, P, 0.8, 11, TR.EPS)[0] - want[:, None]).max() > 1e-4


def test_changing_later_frames_leaves_earlier_attractors_unchanged():
    V, W, P = TR.case(1, 30, 17, 5, 2, seed=6)
    rng = np.random.RandomState(0)
    base = TR.attractors(V, W, P, 0.9, TR.T0, TR.EPS)[0]
    for t in (TR.T0 - 1, TR.T0, 15, 28):
        V2, W2, P2 = V.copy(), W.copy(), P.copy()
        V2[:, t + 1:] = -3 * V2[:, t + 1:] + 1
        W2[:, t + 1:] *= 7
        P2[:, :, t + 1:] = rng.random_sample(P2[:, :, t + 1:].shape)
        other = TR.attractors(V2, W2, P2, 0.9, TR.T0, TR.EPS)[0]
        assert np.array_equal(other[:, TR.T0 - 1:t + 1], base[:, TR.T0 - 1:t + 1])
        assert np.array_equal(other[:, :TR.T0 - 1], base[:, :TR.T0 - 1])          # the hold is frame T0 - 1's
        assert not np.array_equal(other[:, t + 1:], base[:, t + 1:])
    # inside the hold a later frame of the hold does reach back
    V2 = V.copy()
    V2[:, TR.T0 - 1] += 1
    assert not np.array_equal(TR.attractors(V2, W, P, 0.9, TR.T0, TR.EPS)[0][:, 0], base[:, 0])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_a_silent_prefix_gives_zero_attractors_and_finite_gradients(dtype):
    T, p, C = 20, 12, 3
    V, W, P = TR.case(2, T, 9, 4, C, seed=7, silent=p)
    G, _ = TR.grads(2, T, 9, 4, C, seed=7)
    assert (TR.labels(P)[:, :p] != C - 1).all() and (TR.labels(P)[:, p:] == C - 1).any()
    attr, den = TR.attractors(V, W, P, 0.9, TR.T0, TR.EPS, dtype)
    assert not attr[:, :p, C - 1].any() and np.abs(attr[:, p:, C - 1]).min() > 0.01 and np.isfinite(attr).all()
    assert np.array_equal(den[:, :p, C - 1], np.full((2, p), TR.EPS))
    dV = TR.attractors_bwd(G, den, W, P, 0.9, TR.T0, dtype)
    assert np.isfinite(dV).all() and np.abs(dV).max() < 1e3
    # G / eps of the silent frames is carried by no bin: the gradient does not depend on it
    G2 = G.copy()
    G2[:, :p, C - 1] *= -5
    assert np.array_equal(TR.attractors_bwd(G2, den, W, P, 0.9, TR.T0, dtype), dV)
    # eps = 0: the attractor of a source without a bin is 0, not 0 / 0, and the gradient stays finite
    attr0, den0 = TR.attractors(V, W, P, 0.9, TR.T0, 0.0, dtype)
    assert not attr0[:, :p, C - 1].any() and not den0[:, :p, C - 1].any()
    assert np.isfinite(TR.attractors_bwd(G, den0, W, P, 0.9, TR.T0, dtype)).all()


def test_ties_take_the_lowest_source():
    P = np.zeros((1, 3, 1, 4), np.float32)
    P[0, :, 0, 1] = [1, 2, 2]
    P[0, :, 0, 2] = [3, 3, 3]
    P[0, :, 0, 3] = [0, 1, 5]
    assert TR.labels(P).tolist() == [[[0, 1, 0, 2]]]


@pytest.mark.parametrize('i', range(len(TR.CASES)))
def test_the_float32_restatement_stays_inside_the_headers_bound(i):
    '''the cases of the GPU tests, on the CPU first: the float32 run of the rule in the header's summation order lies
    inside the header's ERROR BOUND, the bound is below 1e-5 of max |attr|, and the three backward outputs of the
    float32 run lie under half of the 1e-5 bar'''
    B, T, F, E, C, lam = TR.CASES[i]
    V, W, P = TR.case(B, T, F, E, C, seed=i)
    G, D = TR.grads(B, T, F, E, C, seed=i)
    a64, den = TR.attractors(V, W, P, lam, TR.T0, TR.EPS)
    a32, den32 = TR.attractors(V, W, P, lam, TR.T0, TR.EPS, np.float32)
    bound = TR.attr_bound(V, W, P, lam, TR.T0, TR.EPS)
    top = np.abs(a64).max()
    print('case %d B %d T %d F %d E %d C %d lambda %.3f: float32 %.3g, bound %.3g of max |attr|'
          % (i, B, T, F, E, C, lam, np.abs(a32 - a64).max() / top, bound.max() / top))
    assert (np.abs(a32 - a64) <= bound).all() and 0 < bound.max() < 1e-5 * top
    worst = {}
    for act in (0, 1):
        dV64, dA64 = TR.separate_bwd(V, W, a32, D, act)
        dV32, dA32 = TR.separate_bwd(V, W, a32, D, act, np.float32)
        worst['dV'] = max(worst.get('dV', 0), TR.rel(dV32, dV64))
        worst['dattr'] = max(worst.get('dattr', 0), TR.rel(dA32, dA64))
    e64 = TR.attractors_bwd(G, den, W, P, lam, TR.T0)
    e32 = TR.attractors_bwd(G, den32, W, P, lam, TR.T0, np.float32)
    worst['dV estimator'] = TR.rel(e32, e64)
    print('    float32 backward: %s of each maximum' % ', '.join('%s %.3g' % kv for kv in worst.items()))
    assert max(worst.values()) <= 0.5 * TR.BAR
