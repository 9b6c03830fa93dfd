'''
CPU tests (no GPU) of the causal encoder and block-wise streaming inference: the extension library
libdanet_causal_hip.so against its header (exports, prototypes, ABI, lazy load, every host-visible argument error),
the untouched other nineteen libraries, the open MORE_EXTENSIONS registry, the key INFER_STREAM_BLOCK and every
ValueError of it and of Model.open_stream, the `lstm-causal` plugin's variables, and the numpy restatement of
tests/causal_ref.py.

RESTATEMENT ONLY: the tests from test_causality_of_the_restatement down check tests/causal_ref.py, the reference the
GPU tests hold the kernels against, and no line of the product: causality, split invariance, the adjoint identity,
torch autograd, the hand-computed answer, the torch twin and the input condition of the GPU bar.
'''
import ctypes
import hashlib
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import causal_ref as CR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_causal_hip.h')
CAUSAL_SYMBOLS = ['danet_causal_abi_version', 'danet_causal_center_bwd', 'danet_causal_center_fwd',
                  'danet_causal_last_error', 'danet_causal_lstm_block', 'danet_causal_lstm_ws_bytes',
                  'danet_causal_project']
NO_BYTES = ctypes.c_size_t(-1).value
# the export lists of the nineteen older libraries: sha1 of their sorted, space-joined names (first 12 digits)
OLDER = {'': (51, '35c97f3a2452'), 'conv': (7, '9446af6b053c'), 'dropout': (3, '31a0846a9f05'),
         'prep': (6, '4528d8ffdc78'), 'mix': (5, 'a519a2795d7a'), 'speed': (4, 'e1adf1c490af'),
         'reverb': (3, '05ef787913e5'), 'metric': (6, 'eff9d5e3632c'), 'noise': (3, 'cf88e352bf83'),
         'level': (4, '7fdea6b0fb6a'), 'wavloss': (4, 'e9c25e57750d'), 'gclip': (5, 'a9921dcbc5d9'),
         'dpcl': (7, '8021ee69c5d3'), 'neval': (6, '44b1be58a6d8'), 'stitch': (7, '2ab75117a25c'),
         'bss': (7, '265172254200'), 'stoi': (8, '476adf4d55ec'), 'phase': (6, 'abe3128b0d70'),
         'online': (6, '37411e8747f2')}


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_causal_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_causal()
    syms = _header_symbols('danet_causal_hip.h', 'danet_causal_')
    assert syms == CAUSAL_SYMBOLS
    assert sorted(_lib.CAUSAL_PROTOTYPES) == syms
    assert _exports(_lib.CAUSAL_LIB_PATH) == syms
    assert lib.danet_causal_abi_version() == 1 == _lib.CAUSAL_ABI_VERSION == _lib.CAUSAL.abi
    txt = open(HEADER).read()
    assert '#define DANET_CAUSAL_ABI_VERSION 1' in txt
    for name in ('B', 'TB', 'H', 'D0', 'L', 'M'):
        value = getattr(CR, 'MAX_' + name)
        assert re.search(r'#define DANET_CAUSAL_MAX_%s %d\b' % (name, value), txt), name
        assert getattr(ops, 'CAUSAL_MAX_' + name) == value
    assert re.search(r'#define DANET_CAUSAL_MAX_T %d\b' % CR.MAX_T, txt) and re.search(r'#define DANET_CAUSAL_MAX_D %d\b' % CR.MAX_D, txt)
    rule = txt.split('#ifndef')[0]
    for words in ('THE RULE', 'no atomics', 'within a launch every output\n * element is written once, by one thread',
                  'No waiting between workgroups and no\n * persistent grid',
                  'S    = S + r_t          (float64, sequentially in t)', 'mu_t = (float)(S / (n * D))',
                  'out[t][d] = in[t][d] - mu_t', 'BIT FOR BIT two\n *    calls over its halves', 'ROW SUM ORDER',
                  'a function of D alone', '|out - exact| <= 2^-23 (|x| + |mu|)',
                  's_t\'  = sum over t >= t\' of g_t / ((t + 1) D)', 'din[t\'][d] = dout[t\'][d] - (float)s_t\'',
                  'The order is a function of K alone', 'gate order g | i | f | o', 'c_t = i g + f c_(t-1),   h_t = o tanh(c_t)',
                  'depends neither\n *    on Tb, nor on where the block starts, nor on the other rows of the batch'):
        assert words in rule, words
    assert _lib.CAUSAL.prototypes is _lib.CAUSAL_PROTOTYPES and _lib.CAUSAL.prefix == 'danet_causal_'


def test_causal_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    pp = ctypes.POINTER(p)
    ctype = {'void*': p, 'int': ctypes.c_int, 'const float*': p, 'float*': p, 'void': None, 'size_t': ctypes.c_size_t,
             'const float* const*': pp}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.CAUSAL_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.CAUSAL_PROTOTYPES['danet_causal_' + n][1])
            for n in ('center_fwd', 'center_bwd', 'lstm_ws_bytes', 'lstm_block', 'project')] == [11, 10, 4, 16, 10]


def test_causal_is_in_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.CAUSAL in _lib.MORE_EXTENSIONS and build.CAUSAL in build.MORE_EXTENSIONS
    assert isinstance(_lib.CAUSAL, _lib.Library) and isinstance(build.CAUSAL, build.Library)
    closed = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert _lib.CAUSAL not in closed and len(closed) == 14
    assert build.CAUSAL not in build.LIBRARIES + build.LATER_LIBRARIES + build.EXTENSIONS
    # it follows the records that were there
    assert _lib.MORE_EXTENSIONS.index(_lib.CAUSAL) > _lib.MORE_EXTENSIONS.index(_lib.ONLINE) == 4
    assert build.MORE_EXTENSIONS.index(build.CAUSAL) > build.MORE_EXTENSIONS.index(build.ONLINE) == 4
    assert [lib.name for lib in _lib.MORE_EXTENSIONS] == [os.path.basename(spec.src_dir)
                                                          for spec in build.MORE_EXTENSIONS]
    assert build.CAUSAL_LIB == build.CAUSAL.out == _lib.CAUSAL_LIB_PATH
    assert os.path.basename(build.CAUSAL_LIB) == _lib.CAUSAL.so == 'libdanet_causal_hip.so'
    assert os.path.isfile(os.path.join(build.CAUSAL.src_dir, 'exports.map'))
    assert build.CAUSAL.headers == (HEADER, os.path.join(csrc_scan.CSRC, 'ext_core.h'))
    src = open(os.path.join(build.CAUSAL.src_dir, 'causal.hip')).read()
    assert set(csrc_scan.shared_headers(src)) == set(build.CAUSAL.headers[1:])
    assert callable(build.build_causal) and callable(_lib.load_causal) and callable(_lib.causal_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:12] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL,
                         build.STITCH, build.BSS, build.STOI, build.PHASE, build.ONLINE]
    assert build.CAUSAL in rest[12:] and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 20      # the nineteen older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_nineteen_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS + _lib.MORE_EXTENSIONS[:5]
    assert [spec.name for spec in older] == list(OLDER)
    assert [spec.abi for spec in older] == [7] + [1] * 18
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_causal_') for s in exported), spec.so
        assert (len(exported), hashlib.sha1(' '.join(exported).encode()).hexdigest()[:12]) == OLDER[spec.name], spec.so


def test_causal_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.CAUSAL_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset', 'hipStreamSynchronize', 'hipDeviceSynchronize'):
        assert not re.search(r'\b%s\w*\b' % word, out.stdout), word
    d = os.path.join(csrc_scan.CSRC, 'causal')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['causal.hip']
    own = csrc_scan.strip_comments(open(os.path.join(d, 'causal.hip')).read())
    code = own + csrc_scan.shared_code(own)           # and the shared header it includes
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', 'common.h', 'Synchronize',
                 'hipMemcpy', 'hipMemset', 'asm', 'cooperative', 'volatile'):
        assert word not in code, word
    assert own.count('#include "danet_causal_hip.h"\n#define DANET_EXT causal\n#define DANET_EXT_UPPER CAUSAL\n'
                     '#include "ext_core.h"\n') == 1
    # four kernels; ONE skinny-product core with two callers: the LSTM step and the projection
    assert len(re.findall(r'__global__', own)) == 4 and 'CHECK_LAUNCH();' in own
    for fn in ('skinny_partials<NR>(', 'skinny_exchange<NR>(', 'skinny_sum<NR>('):
        assert fn in own.split('lstm_diag_kernel(LstmArgs a, int k)')[1].split('__global__')[0], fn
        assert fn in own.split('void project_kernel(')[1].split('// ---- the host side')[0], fn
    # every launch comes after every argument check of its entry point
    for body in re.split(r'extern "C"', own)[1:]:
        body = body.split('\n}\n')[0]                     # the entry point alone, not the helpers defined behind it
        launches = [m.start() for m in re.finditer(r'<<<|launch_diag<', body)]
        checks = [m.start() for m in re.finditer(r'CHECK_ARG\(|center_ok\(|lstm_dims_ok\(', body)]
        assert not launches or max(checks) < min(launches)


def test_import_and_a_model_with_another_encoder_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, modules, ozers, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "real, _lib.load_causal = _lib.load_causal, None         # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._causal is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model._check_stream_block())\n"
        "m = model.Model('x', device='cpu'); print('STATE:', m.stream_block)\n"
        "hparams.load(dict(INFER_STREAM_BLOCK=4, ENCODER_TYPE='lstm-causal', INFER_ESTIMATOR_METHOD='online'))\n"
        "print('ON:', model.Model._check_stream_block())\n"
        "_lib.load_causal = real\n"
        "_lib.CAUSAL_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_causal()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_causal_hip.so' in str(e) and %r in str(e)\n"
        "          and 'lstm-causal' in str(e))\n"
        "print('NONE:', _lib._causal is None and 'libdanet_causal' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: None', 'STATE: None', 'ON: 4', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu():
    '''every host-visible argument error is returned before any launch: no device is needed to see them'''
    from danet_amd import _lib, ops
    lib = _lib.load_causal()
    err = lib.danet_causal_last_error
    ok = dict(stream=None, B=2, T=9, D=33, x=4096, lin=0, ldi=33, out=8192, lout=1, ldo=36, state=16384)
    cases = [(dict(B=0), b'need B >= 1'), (dict(T=0), b'need B >= 1'), (dict(T=65537), b'need B >= 1'),
             (dict(D=0), b'need B >= 1'), (dict(D=4097, ldi=4097, ldo=4097), b'need B >= 1'), (dict(lin=2), b'layout'),
             (dict(lout=-1), b'layout'), (dict(ldi=32), b'leading dimension'), (dict(ldo=32), b'leading dimension'),
             (dict(B=1 << 20, T=65536, ldi=1 << 20), b'2^40'), (dict(x=None), b'null'), (dict(out=None), b'null'),
             (dict(x=4097), b'misaligned'), (dict(out=8194), b'misaligned')]
    for kw, msg in cases + [(dict(state=None), b'state'), (dict(state=16388), b'state')]:
        assert lib.danet_causal_center_fwd(*dict(ok, **kw).values()) == -1, kw
        assert b'center_fwd: ' in err() and msg in err(), (kw, err())
    del ok['state']
    for kw, msg in cases:
        assert lib.danet_causal_center_bwd(*dict(ok, **kw).values()) == -1, kw
        assert b'center_bwd: ' in err() and msg in err(), (kw, err())
    # the workspace size and its envelope
    for L, B, Tb, H in ((1, 1, 1, 4), (4, 1, 64, 600), (8, 16, 64, 608), (2, 3, 5, 8)):
        assert lib.danet_causal_lstm_ws_bytes(L, B, Tb, H) == 4 * L * B * Tb * H == ops.causal_lstm_ws_bytes(L, B, Tb, H)
    bad_dims = [dict(L=0), dict(L=9), dict(B=0), dict(B=17), dict(Tb=0), dict(Tb=65), dict(H=0), dict(H=6), dict(H=612)]
    for kw in bad_dims:
        a = dict(dict(L=2, B=2, Tb=3, H=8), **kw)
        assert lib.danet_causal_lstm_ws_bytes(*a.values()) == NO_BYTES, kw
        assert b'lstm_ws_bytes: need 1 <= L <= 8, 1 <= B <= 16, 1 <= Tb <= 64' in err()
    with pytest.raises(_lib.DanetHipError) as e:
        ops.causal_lstm_ws_bytes(9, 1, 1, 4)
    assert str(e.value).startswith('libdanet_causal_hip error -1: lstm_ws_bytes: need 1 <= L <= 8')
    W = (ctypes.c_void_p * 2)(4096, 8192)
    Wbad = (ctypes.c_void_p * 2)(4096, 8196)
    Wnull = (ctypes.c_void_p * 2)(4096, None)
    ok = dict(stream=None, L=2, B=2, Tb=3, D0=33, H=8, x=4096, ldx=36, W=W, bias=W, h=4096, c=4096, y=4096, ldy=8,
              ws=4096, ws_bytes=4 * 2 * 2 * 3 * 8)
    cases = [(kw, b'need 1 <= L <= 8') for kw in bad_dims]
    cases += [(dict(D0=0), b'1 <= D0'), (dict(D0=1029, ldx=1032), b'1 <= D0'), (dict(ldx=32), b'ldx >= D0'),
              (dict(ldy=7), b'ldx >= D0'), (dict(ws_bytes=4 * 2 * 2 * 3 * 8 - 1), b'workspace too small'),
              (dict(W=Wbad), b'misaligned'), (dict(W=Wnull), b'null'), (dict(bias=Wnull), b'null'), (dict(ws=4100), b'misaligned'),
              (dict(x=4097), b'misaligned'), (dict(h=4098), b'misaligned')]
    cases += [({k: None}, b'null') for k in ('x', 'W', 'bias', 'h', 'c', 'y', 'ws')]
    for kw, msg in cases:
        assert lib.danet_causal_lstm_block(*dict(ok, **kw).values()) == -1, kw
        assert b'lstm_' in err() and msg in err(), (kw, err())
    ok = dict(stream=None, M=5, K=8, N=33, A=4096, lda=8, W=8192, ldw=33, out=16384, ldo=33)
    cases = [(dict(M=0), b'need 1 <= M'), (dict(M=1025), b'need 1 <= M'), (dict(K=0), b'need 1 <= M'),
             (dict(K=1637, lda=1637), b'need 1 <= M'), (dict(N=0), b'need 1 <= M'), (dict(N=1 << 24, ldw=1 << 24, ldo=1 << 24), b'need 1 <= M'),
             (dict(lda=7), b'lda >= K'), (dict(ldw=32), b'lda >= K'), (dict(ldo=32), b'lda >= K'), (dict(A=4098), b'misaligned'),
             (dict(W=8193), b'misaligned'), (dict(out=16386), b'misaligned')]
    cases += [({k: None}, b'null') for k in ('A', 'W', 'out')]
    for kw, msg in cases:
        assert lib.danet_causal_project(*dict(ok, **kw).values()) == -1, kw
        assert b'project: ' in err() and msg in err(), (kw, err())
    assert _lib.causal_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.causal_check(-1)
    assert str(e.value).startswith('libdanet_causal_hip error -1: project: null pointer')


# ----------------------------------------------------------------------------------- the key and the session
STREAM = dict(ENCODER_TYPE='lstm-causal', INFER_ESTIMATOR_METHOD='online')


def test_the_key_defaults_to_null_and_the_encoder_is_registered(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    from danet_amd import modules
    key = 'INFER_STREAM_BLOCK'
    assert key in H.DEFAULTS and H.DEFAULTS[key] is None and getattr(hp, key) is None
    assert re.fullmatch(hp.pattern, key) and key in H.__doc__ and 'lstm-causal' in H.__doc__
    assert 'lstm-causal' in hp.encoder_registry and hp.encoder_registry['lstm-causal'] is modules.LstmCausalEncoder
    assert issubclass(modules.LstmCausalEncoder, modules.LstmEncoder) and modules.LstmCausalEncoder.NDIR == 1
    assert modules.LstmCausalEncoder._dims is modules.LstmEncoder._dims
    hp.digest()
    assert Model._check_stream_block() is None and Model('x', device='cpu').stream_block is None
    for n in (1, 4, 64):
        hp.reset()
        hp.load(dict(STREAM, INFER_STREAM_BLOCK=n))
        hp.digest()
        got = Model._check_stream_block()
        assert got == n and type(got) is int


@pytest.mark.parametrize('keys,di', [
    (('INFER_STREAM_BLOCK',), dict(STREAM, INFER_STREAM_BLOCK=True)),
    (('INFER_STREAM_BLOCK',), dict(STREAM, INFER_STREAM_BLOCK=4.0)),
    (('INFER_STREAM_BLOCK',), dict(STREAM, INFER_STREAM_BLOCK='4')),
    (('INFER_STREAM_BLOCK',), dict(STREAM, INFER_STREAM_BLOCK=0)),
    (('INFER_STREAM_BLOCK',), dict(STREAM, INFER_STREAM_BLOCK=-1)),
    (('INFER_STREAM_BLOCK',), dict(STREAM, INFER_STREAM_BLOCK=65)),
    (('INFER_STREAM_BLOCK', 'ENCODER_TYPE'), dict(INFER_ESTIMATOR_METHOD='online', INFER_STREAM_BLOCK=4)),
    (('INFER_STREAM_BLOCK', 'ENCODER_TYPE'), dict(STREAM, ENCODER_TYPE='lstm-orig', INFER_STREAM_BLOCK=4)),
    (('INFER_STREAM_BLOCK', 'INFER_ESTIMATOR_METHOD'), dict(ENCODER_TYPE='lstm-causal', INFER_STREAM_BLOCK=4)),
    (('INFER_STREAM_BLOCK', 'INFER_ESTIMATOR_METHOD'), dict(STREAM, INFER_ESTIMATOR_METHOD='kmeans', INFER_STREAM_BLOCK=4)),
    (('INFER_STREAM_BLOCK', 'PHASE_REFINE_ITERS'), dict(STREAM, INFER_STREAM_BLOCK=4, PHASE_REFINE_ITERS=2)),
    # (INFER_CHUNK_LEN with the "online" estimator is refused by that estimator's own check first; both name the key)
    (('INFER_CHUNK_LEN',), dict(STREAM, INFER_STREAM_BLOCK=4, INFER_CHUNK_LEN=64))])
def test_build_raises_and_names_the_keys(hp, keys, di):
    from danet_amd.model import Model
    hp.load(di)
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('causal', device='cuda:0').build()         # raised before anything touches a device
    for key in keys:
        assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)


def test_the_chunk_key_is_named_by_the_stream_check_itself(hp):
    from danet_amd.model import Model
    hp.load(dict(STREAM, INFER_STREAM_BLOCK=4, INFER_CHUNK_LEN=64))
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model._check_stream_block()
    assert 'INFER_STREAM_BLOCK' in str(e.value) and 'INFER_CHUNK_LEN' in str(e.value)


def test_infer_with_the_key_refuses_a_batch_size_above_16(hp):
    from danet_amd.model import Model
    hp.load(dict(STREAM, INFER_STREAM_BLOCK=4, BATCH_SIZE=17))
    hp.digest()
    m = Model('x', device='cpu')
    m.stream_block = Model._check_stream_block()
    with pytest.raises(ValueError) as e:
        m.infer(torch.zeros(17, 4, hp.FEATURE_SIZE, dtype=torch.complex64))
    assert 'INFER_STREAM_BLOCK' in str(e.value) and 'BATCH_SIZE' in str(e.value)


@pytest.mark.parametrize('keys,di,batch', [
    (('open_stream', 'ENCODER_TYPE'), dict(INFER_ESTIMATOR_METHOD='online'), 1),
    (('open_stream', 'ENCODER_TYPE'), dict(STREAM, ENCODER_TYPE='bilstm-orig'), 1),
    (('open_stream', 'INFER_ESTIMATOR_METHOD'), dict(ENCODER_TYPE='lstm-causal'), 1),
    (('open_stream', 'SEPARATOR_TYPE'), dict(STREAM, SEPARATOR_TYPE='no-act'), 1),
    (('open_stream', 'batch', 'BATCH_SIZE'), dict(STREAM), 17),
    (('open_stream', 'batch'), dict(STREAM), 0),
    (('open_stream', 'batch'), dict(STREAM), True),
    (('open_stream', 'batch'), dict(STREAM), 2.0),
    (('open_stream', 'built'), dict(STREAM), 1)])
def test_open_stream_raises_and_names_the_key(hp, keys, di, batch):
    from danet_amd.model import Model, SeparationStream
    from danet_amd import modules
    if di.get('SEPARATOR_TYPE') == 'no-act':
        @hp.register_separator('no-act')
        class NoAct(modules.Separator):
            pass
    try:
        hp.load(di)
        hp.digest()
        with pytest.raises(ValueError) as e:
            Model('x', device='cpu').open_stream(batch)
        for key in keys:
            assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)
    finally:
        type(hp).separator_registry.pop('no-act', None)
    assert [n for n in ('push', 'flush', 'reset') if callable(getattr(SeparationStream, n))] == ['push', 'flush', 'reset']


def test_no_flag_is_added_and_the_steps_never_look(hp):
    from danet_amd import cli
    from danet_amd.model import Model
    assert 'stream' not in open(cli.__file__).read().lower()
    assert len([a.dest for a in cli.build_parser()._actions]) == 15
    for fn in (Model.train_step, Model.valid_step, Model.forward, Model.debug_fetch, Model.infer_chunks, Model.infer_long):
        src = inspect.getsource(fn)
        assert 'stream_block' not in src and 'INFER_STREAM_BLOCK' not in src and 'open_stream' not in src, fn.__name__
    assert inspect.getsource(Model.infer).count('self.stream_block') == 1


class _FakeModel(object):
    def __init__(self, seed):
        self.names, self.shapes, self.values = [], [], []
        self._gen = torch.Generator().manual_seed(seed)

    def get_variable(self, name, shape, init):
        self.names.append(name)
        self.shapes.append(list(shape))
        self.values.append(init(list(shape), self._gen))
        return self.values[-1]


def test_lstm_causal_creates_the_variables_of_lstm_orig(hp, monkeypatch):
    '''names, shapes, initial values and creation order; the kernels behind the two Functions are stubbed out'''
    from danet_amd import modules, ops
    hp.load(dict(BATCH_SIZE=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=3, LSTM_HDIM=8))
    hp.digest()
    calls = []

    def stub(kind):
        def apply(x, H, L, *rest):
            calls.append((kind, H, L, len(rest)))
            return torch.zeros(x.shape[0], x.shape[1], hp.FEATURE_SIZE * hp.EMBED_SIZE)
        return type('Stub', (), dict(apply=staticmethod(apply)))
    monkeypatch.setattr(ops, 'RnnEncoderFn', stub('orig'))
    monkeypatch.setattr(ops, 'CausalRnnEncoderFn', stub('causal'))
    made = {}
    for name in ('lstm-orig', 'lstm-causal'):
        fake = _FakeModel(7)
        out = hp.encoder_registry[name](fake, 'encoder')(torch.zeros(2, 5, hp.FEATURE_SIZE), 0.5)
        assert tuple(out.shape) == (2, 5, hp.FEATURE_SIZE, hp.EMBED_SIZE)
        made[name] = fake
    a, b = made['lstm-orig'], made['lstm-causal']
    assert a.names == b.names and a.shapes == b.shapes and len(a.names) == 7
    assert a.names[0] == 'encoder/lstm0/LSTM/linear/W' and a.names[-1] == 'encoder/output/W'
    assert all(torch.equal(x, y) for x, y in zip(a.values, b.values))
    # (orig: x, H, L, ndir, 7 params; causal: x, H, L, 7 params -- no ndir)
    assert calls == [('orig', 8, 3, 8), ('causal', 8, 3, 7)]
    hp.reset()
    hp.load(dict(ENCODER_TYPE='lstm-causal'))
    hp.digest()
    assert hp.get_encoder() is modules.LstmCausalEncoder and modules.LstmCausalEncoder(None, 'e')._dims() == (600, hp.NUM_LSTM_LAYERS)


# ----------------------------------------------------------------------------------- RESTATEMENT ONLY from here on
def _x(B, T, D, seed):
    return np.random.RandomState(seed).standard_normal((B, T, D)).astype(np.float32) * 2 + 0.5


def test_causality_of_the_restatement():
    x = _x(2, 30, 7, 0)
    case = CR.lstm_case(2, 8, 7, 2, 30, seed=1)
    Wout = CR.f32(np.random.RandomState(2).standard_normal((8, 12)))
    for dtype in (np.float64, np.float32):
        base_c = CR.center_fwd(x, None, dtype)[0]
        base_e = CR.encoder(x, case['Ws'], case['bs'], Wout, dtype)
        for t in (0, 7, 28):
            x2 = x.copy()
            x2[:, t + 1:] = -3 * x2[:, t + 1:] + 1
            assert np.array_equal(CR.center_fwd(x2, None, dtype)[0][:, :t + 1], base_c[:, :t + 1])
            assert not np.array_equal(CR.center_fwd(x2, None, dtype)[0][:, t + 1:], base_c[:, t + 1:])
            other = CR.encoder(x2, case['Ws'], case['bs'], Wout, dtype)
            assert np.array_equal(other[:, :t + 1], base_e[:, :t + 1])
            assert not np.array_equal(other[:, t + 1:], base_e[:, t + 1:])


@pytest.mark.parametrize('cut', [1, 7, 8, 9, 35])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_two_calls_over_a_split_equal_one_call(cut, dtype):
    T = 70
    x = _x(3, T, 9, 3)
    whole, mu, end = CR.center_fwd(x, None, dtype)
    a, _, mid = CR.center_fwd(x[:, :cut], None, dtype)
    b, _, end2 = CR.center_fwd(x[:, cut:], mid, dtype)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole) and np.array_equal(end, end2)
    assert np.array_equal(end[:, 1], np.full(3, T))
    case = CR.lstm_case(2, 8, 9, 3, T, seed=4)
    xt = x.transpose(1, 0, 2)
    y, h, c = CR.lstm_block(xt, case['Ws'], case['bs'], case['h'], case['c'], dtype)
    y1, h1, c1 = CR.lstm_block(xt[:cut], case['Ws'], case['bs'], case['h'], case['c'], dtype)
    y2, h2, c2 = CR.lstm_block(xt[cut:], case['Ws'], case['bs'], h1, c1, dtype)
    assert np.array_equal(np.concatenate([y1, y2]), y) and np.array_equal(h2, h) and np.array_equal(c2, c)
    assert np.array_equal(h[-1], y[-1])


def test_the_adjoint_identity_and_torch_autograd():
    rng = np.random.RandomState(5)
    for B, T, D in ((1, 1, 1), (2, 3, 2), (3, 70, 9), (1, 300, 33)):
        x, g = rng.standard_normal((B, T, D)), rng.standard_normal((B, T, D))
        lhs = (CR.center_fwd(x)[0] * g).sum()
        rhs = (x * CR.center_bwd(g)[0]).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (B, T, D, lhs, rhs)
        xt = torch.tensor(x, requires_grad=True)
        n = torch.arange(1, T + 1, dtype=torch.float64)[None, :] * D
        out = xt - (torch.cumsum(xt.sum(dim=2), dim=1) / n)[:, :, None]
        assert np.abs(out.detach().numpy() - CR.center_fwd(x)[0]).max() <= 1e-12 * np.abs(x).max()
        (out * torch.tensor(g)).sum().backward()
        assert np.abs(xt.grad.numpy() - CR.center_bwd(g)[0]).max() <= 1e-12 * np.abs(g).max(), (B, T, D)


def test_a_hand_computed_answer():
    # T = 3, D = 2: running sums 4, 4 + 8 = 12, 12 + 6 = 18 over 2, 4, 6 values: means 2, 3, 3
    x = np.array([[[1.0, 3.0], [2.0, 6.0], [5.0, 1.0]]])
    out, mu, state = CR.center_fwd(x)
    assert np.array_equal(mu, [[2.0, 3.0, 3.0]]) and np.array_equal(state, [[18.0, 3.0]])
    assert np.array_equal(out, [[[-1.0, 1.0], [-1.0, 3.0], [2.0, -2.0]]])
    # and from that state, one more frame (3, 3): the sum 24 over 8 values, mean 3
    out2, mu2, state2 = CR.center_fwd(np.array([[[3.0, 3.0]]]), state)
    assert np.array_equal(mu2, [[3.0]]) and np.array_equal(out2, [[[0.0, 0.0]]]) and np.array_equal(state2, [[24.0, 4.0]])
    # the adjoint: row sums of g 1, 2, 4; s_2 = 4 / 6, s_1 = 4 / 6 + 2 / 4, s_0 = 4 / 6 + 2 / 4 + 1 / 2
    g = np.array([[[1.0, 0.0], [1.0, 1.0], [3.0, 1.0]]])
    din, s = CR.center_bwd(g)
    assert np.allclose(s, [[4 / 6 + 0.5 + 0.5, 4 / 6 + 0.5, 4 / 6]], rtol=0, atol=1e-15)
    assert np.allclose(din, g - s[:, :, None], rtol=0, atol=0)
    # one LSTM step by hand: H = 1 would break H % 4, the rule does not care: x = 1, h = 0, c = 2, W = 0 -> a = b
    b = np.array([0.5, 0.0, 0.0, 0.0])
    y, h, c = CR.lstm_block(np.ones((1, 1, 1)), [np.zeros((2, 4))], [b], np.zeros((1, 1, 1)), np.full((1, 1, 1), 2.0))
    assert abs(c[0, 0, 0] - (0.5 * 0.5 + 0.5 * 2.0)) <= 1e-15 and abs(y[0, 0, 0] - 0.5 * np.tanh(1.25)) <= 1e-15


def test_the_torch_twin_is_the_numpy_encoder():
    x = _x(2, 12, 7, 6)
    case = CR.lstm_case(2, 8, 7, 2, 12, seed=7)
    Wout = np.random.RandomState(8).standard_normal((8, 12))
    want = CR.encoder(x, case['Ws'], case['bs'], Wout)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    got = CR.encoder_torch(t64(x), [t64(W) for W in case['Ws']], [t64(b) for b in case['bs']], t64(Wout))
    assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('case', range(len(CR.LSTM_CASES)))
def test_the_input_condition_float32_stays_within_1e_5_of_float64(case):
    '''what the 1e-5 bar of the GPU test of the LSTM block rests on: on every one of its cases, from the same random
    carried state, the float32 run of the restatement is within 1e-5 of each output's maximum of the float64 run'''
    L, H, D0, B, Tb = CR.LSTM_CASES[case]
    d = CR.lstm_case(L, H, D0, B, Tb)
    r64 = CR.lstm_block(d['x'], d['Ws'], d['bs'], d['h'], d['c'])
    r32 = CR.lstm_block(d['x'], d['Ws'], d['bs'], d['h'], d['c'], np.float32)
    errs = [CR.relmax(a, b) for a, b in zip(r32, r64)]
    print('L %d H %d D0 %d B %d Tb %d: float32 vs float64 y %.3g h %.3g c %.3g of the maximum' % ((L, H, D0, B, Tb) + tuple(errs)))
    assert all(r.dtype == np.float32 for r in r32) and 0 < max(errs) <= CR.F32_BAR


def test_the_case_table_covers_every_value_of_every_axis():
    shapes = {(L, H, D0) for L, H, D0, _, _ in CR.LSTM_CASES}
    assert shapes == {(1, 4, 1), (2, 8, 33), (3, 64, 129), (1, 600, 257), (2, 608, 600), (8, 12, 5)}
    for shape in shapes:
        assert {B for L, H, D0, B, _ in CR.LSTM_CASES if (L, H, D0) == shape} == {1, 3, 16}
    assert {Tb for *_, Tb in CR.LSTM_CASES} == {1, 2, 5, 64}
    assert all(Tb <= 5 for L, H, D0, B, Tb in CR.LSTM_CASES if H >= 600)
