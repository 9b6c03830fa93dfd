'''
CPU tests (no GPU) of the online attractor estimator (INFER_ESTIMATOR_METHOD = "online"): the extension library
libdanet_online_hip.so against its header (exports, prototypes, ABI, lazy load, the state layout, every host-visible
argument error), the untouched other eighteen libraries, the open MORE_EXTENSIONS registry, the two configuration keys
and every ValueError, and the numpy restatement of tests/online_ref.py against known answers.
'''
import ctypes
import hashlib
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import csrc_scan
import online_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_online_hip.h')
ONLINE_SYMBOLS = ['danet_online_abi_version', 'danet_online_init', 'danet_online_last_error', 'danet_online_scan',
                  'danet_online_separate', 'danet_online_state_bytes']
NO_BYTES = ctypes.c_size_t(-1).value
# the export lists of the eighteen older libraries: sha1 of their sorted, space-joined names (first 12 digits)
OLDER = {'': (51, '35c97f3a2452'), 'conv': (7, '9446af6b053c'), 'dropout': (3, '31a0846a9f05'),
         'prep': (6, '4528d8ffdc78'), 'mix': (5, 'a519a2795d7a'), 'speed': (4, 'e1adf1c490af'),
         'reverb': (3, '05ef787913e5'), 'metric': (6, 'eff9d5e3632c'), 'noise': (3, 'cf88e352bf83'),
         'level': (4, '7fdea6b0fb6a'), 'wavloss': (4, 'e9c25e57750d'), 'gclip': (5, 'a9921dcbc5d9'),
         'dpcl': (7, '8021ee69c5d3'), 'neval': (6, '44b1be58a6d8'), 'stitch': (7, '2ab75117a25c'),
         'bss': (7, '265172254200'), 'stoi': (8, '476adf4d55ec'), 'phase': (6, 'abe3128b0d70')}


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_online_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_online()
    syms = _header_symbols('danet_online_hip.h', 'danet_online_')
    assert syms == ONLINE_SYMBOLS
    assert sorted(_lib.ONLINE_PROTOTYPES) == syms
    assert _exports(_lib.ONLINE_LIB_PATH) == syms
    assert lib.danet_online_abi_version() == 1 == _lib.ONLINE_ABI_VERSION == _lib.ONLINE.abi
    txt = open(HEADER).read()
    assert '#define DANET_ONLINE_ABI_VERSION 1' in txt
    for name, value in (('C', OR.MAX_C), ('E', OR.MAX_E), ('F', OR.MAX_F), ('T', OR.MAX_T)):
        assert re.search(r'#define DANET_ONLINE_MAX_%s %d\b' % (name, value), txt), name
        assert getattr(ops, 'ONLINE_MAX_' + name) == value
    rule = txt.split('#ifndef')[0]
    for words in ('THE RULE', 'causal IN THE EMBEDDING', 'It does NOT make the model streaming',
                  'centre their\n * input and their last layer over the whole utterance', 'start from a zero state',
                  'End-to-end streaming needs a causal encoder too', 'danet_online_init sets S = 0, n = 0, A = A0',
                  'l[f][c] = V[t][f] . A[c]: float32 fused multiply-adds, e ascending from +0',
                  'Softmax subtracts the row maximum', 's[c][e] = sum_f W[t][f] m[f][c] V[t][f][e]',
                  'q[c] = sum_f W[t][f] m[f][c]', 'function of F alone', 'S = lambda S + s and n = lambda n + q, in float64',
                  'for every c with n[c] > eps, A[c] = (float)(S[c] / n[c])', 'If t < T0, A is unchanged: the hold',
                  'attr[t] = A', "Frame t's attractors depend on frames <= t only", 'BIT FOR BIT one call over the whole',
                  'STATE LAYOUT', '8 (2 C E + C) bytes per utterance', 'S  [C][E]     n  [C]     A  [C][E]',
                  'SUMMATION ORDER', 'ERROR BOUND', 'dl = (E + 1) 2^-24 sum_e |v_e a_e|',
                  '|out - exact| <= |W| (max_c dl_c / 2 + 8 * 2^-24)', 'no atomics', 'no persistent grid',
                  'B T F E, B C T F and B T C E below 2^31'):
        assert words in rule, words
    assert _lib.ONLINE.prototypes is _lib.ONLINE_PROTOTYPES and _lib.ONLINE.prefix == 'danet_online_'


def test_online_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    ctype = {'void*': p, 'int': ctypes.c_int, 'const float*': p, 'float*': p, 'void': None, 'double': ctypes.c_double,
             'int64_t': ctypes.c_int64}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.ONLINE_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.ONLINE_PROTOTYPES['danet_online_' + n][1])
            for n in ('state_bytes', 'init', 'scan', 'separate')] == [2, 6, 15, 11]


def test_online_is_in_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.ONLINE in _lib.MORE_EXTENSIONS and build.ONLINE in build.MORE_EXTENSIONS
    assert isinstance(_lib.ONLINE, _lib.Library) and isinstance(build.ONLINE, build.Library)
    closed = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert _lib.ONLINE not in closed and len(closed) == 14
    assert build.ONLINE not in build.LIBRARIES + build.LATER_LIBRARIES + build.EXTENSIONS
    # it follows the records that were there
    assert _lib.MORE_EXTENSIONS.index(_lib.ONLINE) > _lib.MORE_EXTENSIONS.index(_lib.PHASE) == 3
    assert build.MORE_EXTENSIONS.index(build.ONLINE) > build.MORE_EXTENSIONS.index(build.PHASE) == 3
    assert [lib.name for lib in _lib.MORE_EXTENSIONS] == [os.path.basename(spec.src_dir)
                                                          for spec in build.MORE_EXTENSIONS]
    assert build.ONLINE_LIB == build.ONLINE.out == _lib.ONLINE_LIB_PATH
    assert os.path.basename(build.ONLINE_LIB) == _lib.ONLINE.so == 'libdanet_online_hip.so'
    assert os.path.isfile(os.path.join(build.ONLINE.src_dir, 'exports.map'))
    assert build.ONLINE.headers == (HEADER, os.path.join(csrc_scan.CSRC, 'ext_core.h'))
    src = open(os.path.join(build.ONLINE.src_dir, 'online.hip')).read()
    assert set(csrc_scan.shared_headers(src)) == set(build.ONLINE.headers[1:])
    assert callable(build.build_online) and callable(_lib.load_online) and callable(_lib.online_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:11] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL,
                         build.STITCH, build.BSS, build.STOI, build.PHASE]
    assert build.ONLINE in rest[11:] and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 19      # the eighteen older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_eighteen_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS + _lib.MORE_EXTENSIONS[:4]
    assert [spec.name for spec in older] == list(OLDER)
    assert [spec.abi for spec in older] == [7] + [1] * 17
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_online_') for s in exported), spec.so
        assert (len(exported), hashlib.sha1(' '.join(exported).encode()).hexdigest()[:12]) == OLDER[spec.name], spec.so


def test_online_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.ONLINE_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset', 'hipStreamSynchronize', 'hipDeviceSynchronize'):
        assert not re.search(r'\b%s\w*\b' % word, out.stdout), word
    d = os.path.join(csrc_scan.CSRC, 'online')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['online.hip']
    own = csrc_scan.strip_comments(open(os.path.join(d, 'online.hip')).read())
    code = own + csrc_scan.shared_code(own)           # and the shared header it includes
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', 'common.h', 'Synchronize',
                 'hipMemcpy', 'hipMemset', 'asm', 'cooperative', 'volatile'):
        assert word not in code, word
    # the preamble of every extension source
    assert own.count('#include "danet_online_hip.h"\n#define DANET_EXT online\n#define DANET_EXT_UPPER ONLINE\n'
                     '#include "ext_core.h"\n') == 1
    # three kernels, one workgroup size; the scan and the separator share the logit and the activation code
    assert len(re.findall(r'__global__', own)) == 3 and 'CHECK_LAUNCH();' in own
    assert own.count('bin_logits(') == 3 and own.count('activate(') == 3
    # every launch comes after every argument check of its entry point
    for body in re.split(r'extern "C"', own)[1:]:
        launches = [m.start() for m in re.finditer(r'<<<', body)]
        checks = [m.start() for m in re.finditer(r'CHECK_ARG\(|envelope_ok\(|ce_ok\(', body)]
        assert not launches or max(checks) < min(launches)


def test_import_and_a_model_with_another_estimator_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, modules, ozers, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "real, _lib.load_online = _lib.load_online, None         # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._online is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model._check_online())\n"
        "m = model.Model('x', device='cpu'); print('STATE:', m.online)\n"
        "hparams.load(dict(INFER_ESTIMATOR_METHOD='online')); print('ON:', model.Model._check_online())\n"
        "_lib.load_online = real\n"
        "_lib.ONLINE_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_online()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_online_hip.so' in str(e) and %r in str(e)\n"
        "          and '\"online\" estimator' in str(e))\n"
        "print('NONE:', _lib._online is None and 'libdanet_online' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: None', 'STATE: None', 'ON: (32, 1.0)', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------- state bytes and argument errors
def test_state_bytes_and_its_layout():
    from danet_amd import _lib, ops
    lib = _lib.load_online()
    for C, E in ((1, 1), (2, 20), (3, 40), (4, 64), (2, 7)):
        assert lib.danet_online_state_bytes(C, E) == 8 * OR.state_doubles(C, E) == ops.online_state_bytes(C, E)
    for C, E in ((0, 4), (5, 4), (2, 0), (2, 65), (-1, -1)):
        assert lib.danet_online_state_bytes(C, E) == NO_BYTES, (C, E)
        assert b'state_bytes: need 1 <= C <= 4 and 1 <= E <= 64' in lib.danet_online_last_error()
    with pytest.raises(_lib.DanetHipError) as e:
        ops.online_state_bytes(5, 4)
    assert str(e.value).startswith('libdanet_online_hip error -1: state_bytes: need 1 <= C <= 4')
    # the parts, cut from a host tensor, and the restatement's packing: the header's order
    import torch
    B, C, E = 3, 2, 5
    flat = torch.arange(B * OR.state_doubles(C, E), dtype=torch.float64).view(B, -1)
    S, n, A = ops.online_state_parts(flat, C, E)
    assert (tuple(S.shape), tuple(n.shape), tuple(A.shape)) == ((B, C, E), (B, C), (B, C, E))
    assert [int(t.flatten()[0]) for t in (S, n, A)] == [0, C * E, C * E + C]
    back = OR.pack(OR.unpack(flat.numpy(), C, E))
    assert np.array_equal(back, flat.numpy())
    for got, want in zip(OR.unpack(flat.numpy(), C, E), (S, n, A)):
        assert np.array_equal(got, want.numpy())


SHAPES = [(dict(B=0), b'need B >= 1'), (dict(T=0), b'need B >= 1'), (dict(T=65537), b'need B >= 1'),
          (dict(F=0), b'need B >= 1'), (dict(F=1026), b'need B >= 1'), (dict(C=0), b'need 1 <= C <= 4'),
          (dict(C=5), b'need 1 <= C <= 4'), (dict(E=0), b'need 1 <= C <= 4'), (dict(E=65), b'need 1 <= C <= 4'),
          (dict(B=64, T=65536, F=1025, E=1), b'must be < 2^31'), (dict(B=1 << 15, T=65536, F=1, E=1, C=1), b'must be < 2^31'),
          (dict(B=1024, T=65536, F=1, E=16, C=4), b'must be < 2^31'), (dict(B=1024, T=65536, F=16, E=1, C=4), b'must be < 2^31')]


def test_argument_errors_without_gpu():
    '''every host-visible argument error is returned before any launch: no device is needed to see them'''
    from danet_amd import _lib
    lib = _lib.load_online()
    err = lib.danet_online_last_error
    ok = dict(stream=None, B=2, C=2, E=20, a0=4096, state=8192)
    cases = [(dict(B=0), b'need B >= 1'), (dict(C=0), b'need 1 <= C'), (dict(C=5), b'need 1 <= C'), (dict(E=0), b'need 1 <= C'),
             (dict(E=65), b'need 1 <= C'), (dict(B=1 << 23, C=4, E=64), b'must be < 2^31'), (dict(a0=None), b'null'),
             (dict(state=None), b'null'), (dict(a0=4098), b'misaligned'), (dict(state=8196), b'misaligned')]
    for kw, msg in cases:
        assert lib.danet_online_init(*dict(ok, **kw).values()) == -1, kw
        assert b'init: ' in err() and msg in err(), (kw, err())
    ok = dict(stream=None, B=2, C=2, T=9, F=33, E=20, act=1, lam=0.9, T0=4, t_first=0, eps=1e-7, embed=4096, w=8192,
              state=16384, attr=32768)
    cases = list(SHAPES) + [(dict(act=2), b'act must be'), (dict(act=-1), b'act must be'), (dict(lam=0.0), b'0 < lambda <= 1'),
                            (dict(lam=1.0000001), b'0 < lambda <= 1'), (dict(lam=-0.5), b'0 < lambda <= 1'),
                            (dict(lam=float('nan')), b'0 < lambda <= 1'), (dict(T0=0), b'T0 >= 1'), (dict(T0=-3), b'T0 >= 1'),
                            (dict(t_first=-1), b't_first >= 0'), (dict(eps=-1e-9), b'eps must be'),
                            (dict(eps=float('inf')), b'eps must be'), (dict(eps=float('nan')), b'eps must be')]
    cases += [({k: None}, b'null') for k in ('embed', 'w', 'state', 'attr')]
    cases += [(dict(embed=4100), b'misaligned'), (dict(embed=4104), b'misaligned'), (dict(w=8194), b'misaligned'),
              (dict(state=16388), b'misaligned'), (dict(attr=32770), b'misaligned'), (dict(E=7, embed=4098), b'misaligned')]
    for kw, msg in cases:
        assert lib.danet_online_scan(*dict(ok, **kw).values()) == -1, kw
        assert b'scan: ' in err() and msg in err(), (kw, err())
    ok = dict(stream=None, act=0, B=2, C=2, T=9, F=33, E=20, w=4096, attr=8192, embed=16384, out=32768)
    cases = list(SHAPES) + [(dict(act=2), b'act must be')] + [({k: None}, b'null') for k in ('w', 'attr', 'embed', 'out')]
    cases += [(dict(embed=16388), b'misaligned'), (dict(w=4098), b'misaligned'), (dict(attr=8193), b'misaligned'),
              (dict(out=32770), b'misaligned')]
    for kw, msg in cases:
        assert lib.danet_online_separate(*dict(ok, **kw).values()) == -1, kw
        assert b'separate: ' in err() and msg in err(), (kw, err())
    assert _lib.online_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.online_check(-1)
    assert str(e.value).startswith('libdanet_online_hip error -1: separate: misaligned pointer')


# ----------------------------------------------------------------------------------- the keys
def test_the_keys_default_to_null_and_the_estimator_is_registered(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    from danet_amd import modules
    for key in ('ONLINE_INIT_FRAMES', 'ONLINE_MEMORY_FRAMES'):
        assert key in H.DEFAULTS and H.DEFAULTS[key] is None and getattr(hp, key) is None
        assert re.fullmatch(hp.pattern, key) and key in H.__doc__
    assert 'a choice, not' in H.__doc__ and hp.INFER_ESTIMATOR_METHOD == 'anchor'
    assert 'online' in hp.estimator_registry and hp.get_estimator('online') is modules.OnlineEstimator
    assert hp.get_estimator('online').USE_TRUTH is False and issubclass(modules.OnlineEstimator, modules.Estimator)
    hp.digest()
    assert Model._check_online() is None
    for di, want in ((dict(), (32, 1.0)), (dict(ONLINE_INIT_FRAMES=1), (1, 1.0)), (dict(ONLINE_INIT_FRAMES=500), (500, 1.0)),
                     (dict(ONLINE_MEMORY_FRAMES=100), (32, math.exp(-1.0 / 100))),
                     (dict(ONLINE_MEMORY_FRAMES=0.5, ONLINE_INIT_FRAMES=8), (8, math.exp(-1.0 / 0.5))),
                     (dict(SEPARATOR_TYPE='dot-softmax-orig', MAX_N_SIGNAL=4, EMBED_SIZE=64, FFT_SIZE=2048,
                           FFT_STRIDE=512, EVAL_SI_SDR=True, PHASE_REFINE_ITERS=2), (32, 1.0))):
        hp.reset()
        hp.load(dict(di, INFER_ESTIMATOR_METHOD='online'))
        hp.digest()
        got = Model._check_online()
        assert got == want and type(got[0]) is int and type(got[1]) is float and 0 < got[1] <= 1, (di, got)


@pytest.mark.parametrize('keys,di', [
    (('TRAIN_ESTIMATOR_METHOD', 'online'), dict(TRAIN_ESTIMATOR_METHOD='online')),
    (('TRAIN_ESTIMATOR_METHOD', 'online'), dict(TRAIN_ESTIMATOR_METHOD='online', INFER_ESTIMATOR_METHOD='online')),
    (('INFER_ESTIMATOR_METHOD', 'SEPARATOR_TYPE'), dict(INFER_ESTIMATOR_METHOD='online', SEPARATOR_TYPE='no-act')),
    (('INFER_ESTIMATOR_METHOD', 'INFER_CHUNK_LEN'), dict(INFER_ESTIMATOR_METHOD='online', INFER_CHUNK_LEN=64)),
    (('ONLINE_INIT_FRAMES', 'INFER_ESTIMATOR_METHOD'), dict(ONLINE_INIT_FRAMES=16)),
    (('ONLINE_MEMORY_FRAMES', 'INFER_ESTIMATOR_METHOD'), dict(ONLINE_MEMORY_FRAMES=50.0)),
    (('ONLINE_MEMORY_FRAMES', 'INFER_ESTIMATOR_METHOD'), dict(ONLINE_MEMORY_FRAMES=50, INFER_ESTIMATOR_METHOD='kmeans')),
    (('ONLINE_INIT_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=True)),
    (('ONLINE_INIT_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=8.0)),
    (('ONLINE_INIT_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES='8')),
    (('ONLINE_INIT_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=0)),
    (('ONLINE_INIT_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=-4)),
    (('ONLINE_MEMORY_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_MEMORY_FRAMES=False)),
    (('ONLINE_MEMORY_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_MEMORY_FRAMES='100')),
    (('ONLINE_MEMORY_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_MEMORY_FRAMES=0)),
    (('ONLINE_MEMORY_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_MEMORY_FRAMES=-1.5)),
    (('ONLINE_MEMORY_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_MEMORY_FRAMES=float('inf'))),
    (('ONLINE_MEMORY_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_MEMORY_FRAMES=float('nan'))),
    (('ONLINE_MEMORY_FRAMES',), dict(INFER_ESTIMATOR_METHOD='online', ONLINE_MEMORY_FRAMES=1e-3)),
    (('INFER_ESTIMATOR_METHOD', 'MAX_N_SIGNAL'), dict(INFER_ESTIMATOR_METHOD='online', MAX_N_SIGNAL=5, NUM_ANCHOR=7)),
    (('INFER_ESTIMATOR_METHOD', 'EMBED_SIZE'), dict(INFER_ESTIMATOR_METHOD='online', EMBED_SIZE=65)),
    (('INFER_ESTIMATOR_METHOD', 'FFT_SIZE'), dict(INFER_ESTIMATOR_METHOD='online', FFT_SIZE=4096, FFT_STRIDE=1024))])
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
            Model('online', device='cuda:0').build()         # raised before anything touches a device
        for key in keys:
            assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)
    finally:
        type(hp).separator_registry.pop('no-act', None)


def test_no_flag_is_added_and_the_train_step_never_looks(hp):
    import inspect
    from danet_amd import cli
    from danet_amd.model import Model
    assert 'online' not in open(cli.__file__).read().lower()
    opts = [a.dest for a in cli.build_parser()._actions]
    assert len(opts) == 15 and not any('online' in o for o in opts)
    for fn in (Model.train_step, Model.debug_fetch, Model.infer_chunks, Model.infer_long):
        assert 'online' not in inspect.getsource(fn) and '_separate(' not in inspect.getsource(fn), fn.__name__
    for fn in (Model.infer, Model.forward):
        assert inspect.getsource(fn).count('self._separate(') == 1, fn.__name__
    # the train branch of forward keeps the separator: the one call of the helper is the validation branch's
    src = inspect.getsource(Model.forward)
    assert src.index('self._separate(') > src.index('if with_valid:') and src.count('self.separator(') == 2
    assert 's_attractors.dim() == 4' in inspect.getsource(Model._separate)


# ----------------------------------------------------------------------------------- the restatement
def _one_hot_case(T=6, F=5, C=2, scale=30.0, seed=0):
    '''one-hot, widely separated embeddings: bin (t, f) is scale * unit vector of its class'''
    rng = np.random.RandomState(seed)
    which = rng.randint(C, size=(1, T, F))
    which[0, :, :C] = np.arange(C)                       # every class in every frame
    V = scale * np.eye(C)[which]                         # [1, T, F, E = C]
    W = 1 + rng.randint(1, 5, size=(1, T, F)).astype(np.float64)
    A0 = np.eye(C)[None] * 1.0
    return V, W, A0, which


@pytest.mark.parametrize('act', [0, 1])
def test_one_hot_embeddings_give_the_weighted_class_means(act):
    V, W, A0, which = _one_hot_case()
    T, C = V.shape[1], A0.shape[1]
    attr = OR.attractors(V, W, A0, act, 1.0, 1, OR.EPS)
    assert np.array_equal(attr[0, 0], A0[0])                 # t = 0 < T0 = 1: the hold
    if act == 0:
        # softmax: the logits are 30 apart, the assignment is hard to 1e-13, and the attractor of class c after frame
        # t is the W-weighted mean of its bins so far, which are all 30 e_c: 30 e_c itself
        for t in range(1, T):
            assert np.abs(attr[0, t] - 30.0 * np.eye(C)).max() <= 1e-9
    else:
        # sigmoid under A0 = I (frames 0 and 1 are both assigned under it): a bin of class k has m[c] = sigmoid(30) = 1
        # to 1e-13 for c = k and sigmoid(0) = 1/2 otherwise, so A[c] after frame 1 is this mixture of the 30 e_k
        seen = np.array([W[0, :2][which[0, :2] == k].sum() for k in range(C)])
        for c in range(C):
            m = np.where(np.arange(C) == c, 1.0, 0.5)
            assert np.abs(attr[0, 1, c] - 30.0 * seen * m / (seen * m).sum()).max() <= 1e-9
    # the weighted mean, literally, with well separated but not one-hot data and hard assignments
    rng = np.random.RandomState(3)
    cen = np.array([[40.0, 0.0, 0.0], [0.0, 40.0, 0.0]])
    which = rng.randint(2, size=(1, 4, 7))
    V = cen[which] + rng.standard_normal((1, 4, 7, 3))
    W = 1 + rng.random_sample((1, 4, 7))
    attr = OR.attractors(V, W, cen[None] / 40, 0, 1.0, 1, OR.EPS)
    for t in range(1, 4):
        for c in range(2):
            sel = which[0, :t + 1] == c
            want = (W[0, :t + 1][sel][:, None] * V[0, :t + 1][sel]).sum(0) / W[0, :t + 1][sel].sum()
            assert np.abs(attr[0, t, c] - want).max() <= 1e-9 * 40


def test_the_hold_the_zero_weights_and_the_eps_rule():
    V, W, A0 = OR.clustered_case(2, 20, 9, 4, 2, seed=1)
    attr, (S, n, A) = OR.scan(V, W, OR.init(A0), 1, 0.9, OR.T0, OR.EPS)
    assert np.array_equal(attr[:, :OR.T0], np.broadcast_to(A0[:, None].astype(np.float64), attr[:, :OR.T0].shape))
    assert np.abs(attr[:, OR.T0] - A0).max() > 1e-3 and (n > 0).all()       # the state accumulated during the hold
    assert np.array_equal(attr[:, -1], A)
    # an all-zero-weight utterance keeps A0 throughout, finite
    W0 = W.copy()
    W0[1] = 0
    attr0, (S0, n0, A00) = OR.scan(V, W0, OR.init(A0), 1, 0.9, OR.T0, OR.EPS)
    assert np.array_equal(attr0[1], np.broadcast_to(A0[1].astype(np.float64), attr0[1].shape)) and np.isfinite(attr0).all()
    assert not n0[1].any() and not S0[1].any() and np.array_equal(attr0[0], attr[0])
    # n[c] <= eps keeps that row: a large eps holds class 1 only
    big = float(np.sort(n.ravel())[0] * 10)
    state = OR.init(A0)
    state[1][:] = [[5 * big, 0.0], [0.0, 5 * big]]           # class 1 of utterance 0 and class 0 of utterance 1 start empty
    W1 = W * 1e-6
    attr1, (S1, n1, _) = OR.scan(V, W1, state, 0, 1.0, 1, big, t_first=1)
    assert (n1[0, 1] <= big) and (n1[1, 0] <= big) and n1[0, 0] > big and n1[1, 1] > big
    assert np.array_equal(attr1[0, :, 1], np.broadcast_to(A0[0, 1].astype(np.float64), attr1[0, :, 1].shape))
    assert np.array_equal(attr1[1, :, 0], np.broadcast_to(A0[1, 0].astype(np.float64), attr1[1, :, 0].shape))
    assert np.isfinite(attr1).all()


@pytest.mark.parametrize('cut', [1, OR.T0 - 1, OR.T0, OR.T0 + 1, 35])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_two_calls_over_a_split_equal_one_call(cut, dtype):
    V, W, A0 = OR.clustered_case(2, 50, 17, 5, 3, seed=2)
    whole, end = OR.scan(V, W, OR.init(A0), 0, 0.95, OR.T0, OR.EPS, 0, dtype)
    a, mid = OR.scan(V[:, :cut], W[:, :cut], OR.init(A0), 0, 0.95, OR.T0, OR.EPS, 0, dtype)
    b, end2 = OR.scan(V[:, cut:], W[:, cut:], mid, 0, 0.95, OR.T0, OR.EPS, cut, dtype)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    assert all(np.array_equal(x, y) for x, y in zip(end, end2))
    assert np.array_equal(OR.pack(end), OR.pack(OR.unpack(OR.pack(end2), 3, 5)))


def test_changing_later_frames_leaves_earlier_attractors_unchanged():
    V, W, A0 = OR.clustered_case(1, 40, 17, 5, 2, seed=3)
    base = OR.attractors(V, W, A0, 1, 0.9, OR.T0, OR.EPS)
    for t in (0, OR.T0 - 1, OR.T0, 20, 38):
        V2, W2 = V.copy(), W.copy()
        V2[:, t + 1:] = -3 * V2[:, t + 1:] + 1
        W2[:, t + 1:] *= 7
        other = OR.attractors(V2, W2, A0, 1, 0.9, OR.T0, OR.EPS)
        assert np.array_equal(other[:, :t + 1], base[:, :t + 1])
        assert t + 1 < OR.T0 or not np.array_equal(other[:, t + 1:], base[:, t + 1:])


@pytest.mark.parametrize('case', range(len(OR.TRAJECTORY_CASES)))
def test_the_input_condition_float32_stays_within_1e_6_of_float64(case):
    '''what the 1e-5 bar of the GPU tests rests on: on every trajectory case the float32 run of the rule is within
    1e-6 of max |A| of the float64 run (measured when written: at most 2.4e-7)'''
    T, F, E, C, lam, act = OR.TRAJECTORY_CASES[case]
    V, W, A0 = OR.clustered_case(2, T, F, E, C, seed=case)
    a64 = OR.attractors(V, W, A0, act, lam, OR.T0, OR.EPS)
    a32 = OR.attractors(V, W, A0, act, lam, OR.T0, OR.EPS, np.float32)
    err = np.abs(a32 - a64).max() / np.abs(a64).max()
    print('T %d F %d E %d C %d lambda %g act %d: float32 vs float64 %.3g of max |A|' % (T, F, E, C, lam, act, err))
    assert 0 < err <= 1e-6
    assert np.abs(a64[:, OR.T0:] - A0[:, None]).max() > 1e-2             # the track moved
    # a 1e-6 relative change of A0 comes out damped
    moved = OR.attractors(V, W, A0.astype(np.float64) * (1 + 1e-6), act, lam, OR.T0, OR.EPS)
    assert np.abs(moved[:, OR.T0:] - a64[:, OR.T0:]).max() <= 0.5 * 1e-6 * np.abs(A0).max()


def test_the_separator_of_the_restatement_and_its_bound():
    V, W, A0 = OR.clustered_case(2, 5, 9, 20, 3, seed=5)
    attr = OR.attractors(V, W, A0, 0, 1.0, 2, OR.EPS, np.float32)          # float32 values, as the kernel's
    assert np.array_equal(attr, attr.astype(np.float32))
    for act in (0, 1):
        out = OR.separate(V, W, attr, act)
        assert out.shape == (2, 3, 5, 9) and out.dtype == np.float64
        b, c, t, f = 1, 2, 3, 4
        l = V[b, t, f].astype(np.float64) @ attr[b, t].T
        m = np.exp(l - l.max()) / np.exp(l - l.max()).sum() if act == 0 else 1 / (1 + np.exp(-l))
        assert abs(out[b, c, t, f] - W[b, t, f] * m[c]) <= 1e-12 * abs(out[b, c, t, f])
        if act == 0:
            assert np.abs(out.sum(1) - W).max() <= 1e-12 * W.max()
        out32 = OR.separate(V, W, attr, act, np.float32)
        bound = OR.separate_bound(V, W, attr)
        assert out32.dtype == np.float32 and bound.shape == out.shape
        assert (np.abs(out32 - out) <= bound).all() and bound.max() < 1e-3 * np.abs(out).max()
