'''
CPU tests (no GPU) of the BSS-eval figures (EVAL_BSS_SDR): the extension library libdanet_bss_hip.so against its
header (exports, prototypes, ABI, lazy load, every host-visible argument error), the untouched other fifteen
libraries, the open MORE_EXTENSIONS registry, the two configuration keys and every ValueError, and the two float64
restatements of tests/bss_ref.py against each other and against known answers.
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

import bss_ref as BR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_bss_hip.h')
BSS_SYMBOLS = ['danet_bss_abi_version', 'danet_bss_chol_solve', 'danet_bss_finalize', 'danet_bss_last_error',
               'danet_bss_systems', 'danet_bss_workspace_bytes', 'danet_bss_xcorr']
KEYS = ('EVAL_BSS_SDR', 'EVAL_BSS_FILTER_LEN')
NO_WS = ctypes.c_size_t(-1).value
# the export lists of the fifteen older libraries: sha1 of their sorted, space-joined names (first 12 digits)
OLDER = {'': (51, '35c97f3a2452'), 'conv': (7, '9446af6b053c'), 'dropout': (3, '31a0846a9f05'),
         'prep': (6, '4528d8ffdc78'), 'mix': (5, 'a519a2795d7a'), 'speed': (4, 'e1adf1c490af'),
         'reverb': (3, '05ef787913e5'), 'metric': (6, 'eff9d5e3632c'), 'noise': (3, 'cf88e352bf83'),
         'level': (4, '7fdea6b0fb6a'), 'wavloss': (4, 'e9c25e57750d'), 'gclip': (5, 'a9921dcbc5d9'),
         'dpcl': (7, '8021ee69c5d3'), 'neval': (6, '44b1be58a6d8'), 'stitch': (7, '2ab75117a25c')}
# (a) against (b): the grid of the issue
GRID = [(1, 40, 1), (2, 300, 8), (3, 200, 16), (2, 64, 32), (4, 120, 4)]


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_bss_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_bss()
    syms = _header_symbols('danet_bss_hip.h', 'danet_bss_')
    assert syms == BSS_SYMBOLS
    assert sorted(_lib.BSS_PROTOTYPES) == syms
    assert _exports(_lib.BSS_LIB_PATH) == syms
    assert lib.danet_bss_abi_version() == 1 == _lib.BSS_ABI_VERSION == _lib.BSS.abi
    txt = open(HEADER).read()
    assert '#define DANET_BSS_ABI_VERSION 1' in txt
    for name, value in (('MAX_C', BR.MAX_C), ('MAX_L', BR.MAX_L), ('MAX_N', BR.MAX_N), ('MAX_RHS', BR.MAX_RHS),
                        ('MAX_BATCH', BR.MAX_BATCH), ('BLOCK', BR.BLOCK)):
        assert re.search(r'#define DANET_BSS_%s %d\b' % (name, value), txt), name
    assert ops.BSS_MAX_C == BR.MAX_C and ops.BSS_MAX_L == BR.MAX_L and BR.MAX_N == BR.MAX_C * BR.MAX_L
    rule = txt.split('#ifndef')[0]
    for words in ('R_ik[tau] = sum_n s_i[n] s_k[n + tau]', 'D_ji[tau] = sum_n e_j[n] s_i[n - tau]',
                  'G[(i, t1), (k, t2)] = R_ik[t1 - t2]', 'is silent', 'pall_j = D_j^T G^-1 D_j',
                  'st_ij = D_ji^T G_ii^-1 D_ji', 'SDR(i, j) = q(st_ij, ee_j - st_ij)',
                  'SIR(i, j) = q(st_ij, pall_j - st_ij)', 'SAR(j) = q(pall_j, ee_j - pall_j)',
                  'p maximises sum_i SIR(i, p(i))', 'itertools.permutations(range(C)) order',
                  'D_mi[tau] = sum_k R_ik[tau]', 'base_i = q(st_mi, mm - st_mi)', 'NO least-squares fallback',
                  'left out of the batch means', 'symmetric bit for bit by construction'):
        assert words in rule, words
    assert _lib.BSS.prototypes is _lib.BSS_PROTOTYPES and _lib.BSS.prefix == 'danet_bss_'


def test_bss_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    ctype = {'void*': p, 'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'const float*': p,
             'double*': p, 'const double*': p, 'int32_t*': p, 'const int32_t*': p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.BSS_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.BSS_PROTOTYPES['danet_bss_' + n][1]) for n in ('xcorr', 'systems', 'chol_solve', 'finalize')] \
        == [9, 10, 7, 17]


def test_bss_is_in_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.BSS in _lib.MORE_EXTENSIONS and build.BSS in build.MORE_EXTENSIONS
    assert isinstance(_lib.BSS, _lib.Library) and isinstance(build.BSS, build.Library)
    closed = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert _lib.BSS not in closed and len(closed) == 14
    assert build.BSS not in build.LIBRARIES + build.LATER_LIBRARIES + build.EXTENSIONS
    # it follows the records that were there
    assert _lib.MORE_EXTENSIONS.index(_lib.BSS) > _lib.MORE_EXTENSIONS.index(_lib.STITCH) == 0
    assert build.MORE_EXTENSIONS.index(build.BSS) > build.MORE_EXTENSIONS.index(build.STITCH) == 0
    assert [lib.name for lib in _lib.MORE_EXTENSIONS] == [os.path.basename(spec.src_dir)
                                                          for spec in build.MORE_EXTENSIONS]
    assert build.BSS_LIB == build.BSS.out == _lib.BSS_LIB_PATH
    assert os.path.basename(build.BSS_LIB) == _lib.BSS.so == 'libdanet_bss_hip.so'
    assert os.path.isfile(os.path.join(build.BSS.src_dir, 'exports.map'))
    assert build.BSS.headers == (HEADER, os.path.join(csrc_scan.CSRC, 'ext_core.h'))
    assert callable(build.build_bss) and callable(_lib.load_bss) and callable(_lib.bss_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:8] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL,
                        build.STITCH]
    assert build.BSS in rest[8:] and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 16      # the fifteen older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_fifteen_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS + _lib.MORE_EXTENSIONS[:1]
    assert [spec.name for spec in older] == list(OLDER)
    assert [spec.abi for spec in older] == [7] + [1] * 14
    assert len(_lib.LIBRARIES) == 5 and len(_lib.ALL_LIBRARIES) == 6 and len(_lib.LATER_LIBRARIES) == 1 \
        and len(_lib.EXTENSIONS) == 7
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_bss_') for s in exported), spec.so
        assert (len(exported), hashlib.sha1(' '.join(exported).encode()).hexdigest()[:12]) == OLDER[spec.name], spec.so


def test_bss_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.BSS_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipStreamSynchronize', 'hipDeviceSynchronize'):
        assert not re.search(r'\b%s\w*\b' % word, out.stdout), word
    d = os.path.join(csrc_scan.CSRC, 'bss')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['bss.hip']
    code = csrc_scan.strip_comments(open(os.path.join(d, 'bss.hip')).read())
    code += csrc_scan.shared_code(code)              # and the shared header it includes
    assert csrc_scan.shared_headers(code) == [os.path.join(csrc_scan.CSRC, 'ext_core.h')]
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', 'common.h', 'Synchronize',
                 'hipMemcpy', 'asm'):
        assert word not in code, word
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64(' in code      # the trailing update is on the f64 matrix unit


def test_import_and_a_model_with_the_keys_null_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, ozers, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "real, _lib.load_bss = _lib.load_bss, None          # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._bss is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model._check_eval_bss())\n"
        "hparams.load(dict(EVAL_BSS_SDR=False)); print('FALSE:', model.Model._check_eval_bss())\n"
        "_lib.load_bss = real\n"
        "_lib.BSS_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_bss()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_bss_hip.so' in str(e) and %r in str(e)\n"
        "          and 'EVAL_BSS_SDR' in str(e))\n"
        "print('NONE:', _lib._bss is None and 'libdanet_bss' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: None', 'FALSE: None', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------- argument errors
def test_workspace_bytes_and_its_envelope():
    from danet_amd import _lib, ops
    lib = _lib.load_bss()
    for B, C, L in ((1, 1, 1), (3, 2, 8), (2, 4, 512), (32, 2, 512), (65535, 1, 1), (7, 3, 33)):
        assert lib.danet_bss_workspace_bytes(B, C, L) == BR.workspace_bytes(B, C, L) == ops.bss_workspace_bytes(B, C, L)
        assert BR.workspace_bytes(B, C, L) % 256 == 0
        assert [p[0] for p in ops.bss_parts(B, C, L)] == ['R', 'D', 'ee', 'G', 'Gs', 'Xg', 'Xs', 'fg', 'fs', 'per_utt',
                                                          'perm_idx', 'flags', 'mean4']
    assert BR.workspace_bytes(1, 4, 512) > 32 << 20                 # G alone is 32 MiB per utterance there
    assert ops.bss_group(32, 4, 512) == 6 and ops.bss_workspace_bytes(6, 4, 512) <= ops.BSS_SCRATCH_BYTES \
        < ops.bss_workspace_bytes(7, 4, 512)
    assert ops.bss_group(32, 2, 512) == 21 and ops.bss_group(4, 2, 8) == 4 and ops.bss_group(1, 4, 512) == 1
    for bad in ((0, 2, 8), (65536, 2, 8), (1, 0, 8), (1, 5, 8), (1, 2, 0), (1, 2, 513), (-1, 2, 8)):
        assert lib.danet_bss_workspace_bytes(*bad) == NO_WS, bad
        assert b'workspace_bytes: need 1 <= B' in lib.danet_bss_last_error()
    with pytest.raises(_lib.DanetHipError) as e:
        ops.bss_workspace_bytes(1, 5, 8)
    assert str(e.value).startswith('libdanet_bss_hip error -1: workspace_bytes: need 1 <= B')


def test_argument_errors_without_gpu():
    '''every host-visible argument error is returned before any launch: no device is needed to see them'''
    from danet_amd import _lib
    lib = _lib.load_bss()
    shapes = [(dict(B=0), b'need 1 <= B'), (dict(B=65536), b'need 1 <= B'), (dict(C=0), b'need 1 <= B'),
              (dict(C=5), b'need 1 <= B'), (dict(L=0), b'need 1 <= B'), (dict(L=513), b'need 1 <= B')]
    ok = dict(stream=None, B=2, C=2, Ls=300, L=8, wav=4096, R=8192, D=16384, ee=32768)
    cases = shapes + [(dict(Ls=0), b'Ls must be'), (dict(Ls=1 << 31), b'Ls must be'), (dict(Ls=-5), b'Ls must be')]
    cases += [({k: None}, b'null') for k in ('wav', 'R', 'D', 'ee')]
    cases += [(dict(wav=4098), b'misaligned')] + [({k: ok[k] + 4}, b'misaligned') for k in ('R', 'D', 'ee')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_bss_xcorr(*a.values()) == -1, kw
        assert b'xcorr: ' + msg in lib.danet_bss_last_error(), (kw, lib.danet_bss_last_error())
    ok = dict(stream=None, B=2, C=2, L=8, R=8192, D=16384, G=32768, Gs=65536, Xg=1024, Xs=2048)
    ptrs = ('R', 'D', 'G', 'Gs', 'Xg', 'Xs')
    cases = shapes + [({k: None}, b'null') for k in ptrs] + [({k: ok[k] + 4}, b'misaligned') for k in ptrs]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_bss_systems(*a.values()) == -1, kw
        assert b'systems: ' + msg in lib.danet_bss_last_error(), (kw, lib.danet_bss_last_error())
    ok = dict(stream=None, nmat=3, n=100, nrhs=2, A=8192, X=16384, flags=1024)
    cases = [(dict(nmat=0), b'nmat must be'), (dict(nmat=65536), b'nmat must be'), (dict(n=0), b'n must be'),
             (dict(n=2049), b'n must be'), (dict(nrhs=0), b'nrhs must be'), (dict(nrhs=17), b'nrhs must be')]
    cases += [({k: None}, b'null') for k in ('A', 'X', 'flags')]
    cases += [(dict(A=8196), b'misaligned'), (dict(X=16388), b'misaligned'), (dict(flags=1026), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_bss_chol_solve(*a.values()) == -1, kw
        assert b'chol_solve: ' + msg in lib.danet_bss_last_error(), (kw, lib.danet_bss_last_error())
    ok = dict(stream=None, B=2, C=2, L=8, R=8192, D=16384, ee=32768, Xg=1024, Xs=2048, fg=512, fs=768, b0=0, B_all=2,
              per_utt=65536, perm_idx=256, flags=128, mean4=131072)
    p8, p4 = ('R', 'D', 'ee', 'Xg', 'Xs', 'per_utt', 'mean4'), ('fg', 'fs', 'perm_idx', 'flags')
    cases = shapes + [(dict(b0=-1), b'need b0 >= 0'), (dict(b0=1), b'need b0 >= 0'), (dict(B_all=1), b'need b0 >= 0'),
                      (dict(B_all=65536), b'need b0 >= 0')]
    cases += [({k: None}, b'null') for k in p8 + p4]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in p8] + [({k: ok[k] + 2}, b'misaligned') for k in p4]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_bss_finalize(*a.values()) == -1, kw
        assert b'finalize: ' + msg in lib.danet_bss_last_error(), (kw, lib.danet_bss_last_error())
    assert _lib.bss_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.bss_check(-1)
    assert str(e.value).startswith('libdanet_bss_hip error -1: finalize: misaligned')


# ----------------------------------------------------------------------------------- the keys
def test_the_keys_default_to_null_and_mean_off(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    for key in KEYS:
        assert key in H.DEFAULTS and H.DEFAULTS[key] is None and getattr(hp, key) is None
        assert re.fullmatch(hp.pattern, key) and key in H.__doc__
    hp.digest()
    assert Model._check_eval_bss() is None
    for di, want in ((dict(EVAL_BSS_SDR=False), None), (dict(EVAL_BSS_SDR=True), 512),
                     (dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=1), 1),
                     (dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=512), 512),
                     (dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=64, EVAL_SI_SDR=True), 64),
                     (dict(EVAL_BSS_SDR=True, MAX_N_SIGNAL=4, FFT_SIZE=64, FFT_STRIDE=8), 512),
                     (dict(MAX_N_SIGNAL=5, FFT_SIZE=48), None)):       # off: the envelope is not looked at
        hp.reset()
        hp.load(di)
        assert Model._check_eval_bss() == want, di


@pytest.mark.parametrize('keys,di', [
    (('EVAL_BSS_SDR',), dict(EVAL_BSS_SDR=1)), (('EVAL_BSS_SDR',), dict(EVAL_BSS_SDR='true')),
    (('EVAL_BSS_SDR',), dict(EVAL_BSS_SDR=0.0)),
    (('EVAL_BSS_FILTER_LEN',), dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=True)),
    (('EVAL_BSS_FILTER_LEN',), dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=64.0)),
    (('EVAL_BSS_FILTER_LEN',), dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN='64')),
    (('EVAL_BSS_FILTER_LEN',), dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=0)),
    (('EVAL_BSS_FILTER_LEN',), dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=513)),
    (('EVAL_BSS_FILTER_LEN',), dict(EVAL_BSS_SDR=True, EVAL_BSS_FILTER_LEN=-8)),
    (('EVAL_BSS_FILTER_LEN', 'EVAL_BSS_SDR'), dict(EVAL_BSS_FILTER_LEN=64)),
    (('EVAL_BSS_FILTER_LEN', 'EVAL_BSS_SDR'), dict(EVAL_BSS_SDR=False, EVAL_BSS_FILTER_LEN=64)),
    (('EVAL_BSS_SDR', 'MAX_N_SIGNAL'), dict(EVAL_BSS_SDR=True, MAX_N_SIGNAL=5)),
    (('EVAL_BSS_SDR', 'FFT_SIZE'), dict(EVAL_BSS_SDR=True, FFT_SIZE=48, FFT_STRIDE=12)),
    (('EVAL_BSS_SDR', 'FFT_SIZE'), dict(EVAL_BSS_SDR=True, FFT_SIZE=2048, FFT_STRIDE=512)),
    (('EVAL_BSS_SDR', 'FFT_STRIDE'), dict(EVAL_BSS_SDR=True, FFT_SIZE=256, FFT_STRIDE=192)),
    (('EVAL_BSS_SDR', 'FFT_STRIDE'), dict(EVAL_BSS_SDR=True, FFT_SIZE=256, FFT_STRIDE=16)),
    (('EVAL_BSS_SDR', 'NOISE_EVAL_DIR'), dict(EVAL_BSS_SDR=True, NOISE_EVAL_DIR='/nowhere')),
    (('EVAL_BSS_SDR', 'NOISE_EVAL_DIR'), dict(EVAL_BSS_SDR=True, EVAL_SI_SDR=True, NOISE_EVAL_DIR='/nowhere'))])
def test_build_raises_and_names_the_key(hp, keys, di):
    from danet_amd.model import Model
    hp.load(di)
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('bss', device='cuda:0').build()                # raised before anything touches a device
    for key in keys:
        assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)
    if 'FFT_SIZE' in keys or 'FFT_STRIDE' in keys or 'MAX_N_SIGNAL' in keys:
        assert 'EVAL_SI_SDR' not in str(e.value)             # the shared rules speak under this key's name


def test_the_si_sdr_messages_are_unchanged_and_no_flag_is_added(hp):
    from danet_amd.model import Model
    from danet_amd import cli
    hp.load(dict(EVAL_SI_SDR=True, FFT_SIZE=256, FFT_STRIDE=192))
    with pytest.raises(ValueError) as e:
        Model._check_eval_si_sdr()
    assert str(e.value).startswith('EVAL_SI_SDR needs FFT_STRIDE <= FFT_SIZE / 2 (got FFT_STRIDE = 192 at FFT_SIZE = 256)')
    src = open(cli.__file__).read().lower()
    assert 'bss' not in src
    opts = [a.dest for a in cli.build_parser()._actions]
    assert len(opts) == 15 and not any('bss' in o for o in opts)


# ----------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize('C,Ls,L', GRID)
def test_literal_against_quadratic_form(C, Ls, L):
    wav = BR.make_case(C, Ls, L, seed=100 * C + L)[0]
    pa, ia, fa, (sdr, sir, sar) = BR.evaluate_literal(wav, L, with_table=True)
    pb, ib, fb, cond = BR.evaluate(wav, L, with_cond=True)
    print('C %d Ls %d L %d: cond(G) %.2e  (a) %s  (b) %s  max |a - b| %.2e dB'
          % (C, Ls, L, cond, pa.round(3), pb.round(3), np.abs(pa - pb).max()))
    assert cond <= 1e6
    assert ia == ib and fa == fb == 0
    assert np.abs(pa - pb).max() <= 1e-9
    flat = [v for row in sdr for v in row] + sar
    if C > 1:
        flat += [v for row in sir for v in row]
    else:
        assert sir == [[100.0]] and pa[1] == pb[1] == 100.0  # one reference: nothing to interfere, pall = st exactly
    assert all(-100.0 < v < 100.0 for v in flat)             # nothing else clamped: the comparison is of real figures


def test_estimate_equal_to_the_reference_gives_plus_100():
    wav = BR.make_case(2, 200, 4, seed=1)[0]
    wav[2:] = wav[:2]
    for ev in (BR.evaluate, BR.evaluate_literal):
        per, idx, fl = ev(wav, 4)
        assert per[0] == 100.0 and idx == 0 and fl == 0, (ev.__name__, per)
        assert per[3] > 90.0                                 # the mixture of two white sources sits near 0 dB


def test_a_filtered_reference_is_no_distortion_when_the_filter_fits():
    rng = np.random.RandomState(5)
    wav = np.zeros((2, 400), np.float32)
    wav[0, :398] = rng.standard_normal(398)                  # (the filtered reference ends inside the Ls samples)
    wav[1] = np.convolve(wav[0].astype(np.float64), [0.9, -0.4, 0.25])[:400]
    for ev in (BR.evaluate, BR.evaluate_literal):
        assert ev(wav, 3)[0][0] == 100.0 and ev(wav, 8)[0][0] == 100.0, ev.__name__
        assert ev(wav, 2)[0][0] < 20.0 and ev(wav, 1)[0][0] < 10.0            # too short a filter: real distortion
    s, e = wav[0].astype(np.float64), wav[1].astype(np.float64)
    t = np.dot(s, e) ** 2 / np.dot(s, s)
    assert 10 * np.log10(t / (np.dot(e, e) - t)) < 10.0                       # what SI-SDR makes of it


def test_the_other_reference_gives_minus_100_sir_and_swapped_estimates_perm_1():
    wav = BR.make_case(2, 300, 4, seed=9, noise=0.0, leak=0.0)[0]
    swapped = wav.copy()
    swapped[2], swapped[3] = wav[1], wav[0]                  # estimate 0 IS reference 1 and the other way round
    for ev in (BR.evaluate_literal,):
        sdr, sir, sar = ev(swapped, 4, with_table=True)[3]
        assert sir[1][0] == 100.0 and sir[0][1] == 100.0
    R, D, ee = BR.correlations(swapped, 4)
    G, Gs, Xg, Xs = BR.systems(R, D)
    per, idx, fl = BR.evaluate(swapped, 4)
    assert idx == 1 and fl == 0 and per[0] == 100.0 and per[1] == 100.0
    assert BR.evaluate_literal(swapped, 4)[1] == 1
    # an estimate that is exactly the OTHER reference: its target part against its own reference is what leaks through
    # the correlation of two white signals, so SIR sits far below 0; with orthogonal references it is -100
    orth = np.zeros((4, 8), np.float32)
    orth[0, :4] = [1, 2, -1, 3]
    orth[1, 4:] = [2, -1, 1, 1]
    orth[2], orth[3] = orth[1], orth[0]
    for ev in (BR.evaluate, BR.evaluate_literal):
        per, idx, fl = ev(orth, 1)
        assert idx == 1 and per[0] == 100.0, ev.__name__
    st = [[0.0, 7.0], [15.0, 0.0]]
    per, idx, fl = BR.scores(st, [1.0, 1.0], [15.0, 7.0], [15.0, 7.0], 22.0, [True, True])
    assert idx == 1
    sir = [[BR.q(st[i][j], [15.0, 7.0][j] - st[i][j]) for j in range(2)] for i in range(2)]
    assert sir[0][0] == -100.0 and sir[1][1] == -100.0 and sir[0][1] == 100.0


def test_one_silent_reference_takes_no_part():
    wav = BR.make_case(3, 200, 4, seed=4)[0]
    wav[1] = 0.0
    two = np.concatenate([wav[[0, 2]], wav[[3, 5]]])
    R, D, ee = BR.correlations(wav, 4)
    assert BR.live_refs(R) == [True, False, True]
    G, Gs, Xg, Xs = BR.systems(R, D)
    assert (G[4:8, 4:8] == np.eye(4)).all() and not G[4:8, :4].any() and not G[:4, 4:8].any() and not G[8:, 4:8].any()
    assert (Gs[1] == np.eye(4)).all() and not Xg[:, 4:8].any() and not Xs[1].any()
    pb, ib, fb = BR.evaluate(wav, 4)
    pa, ia, fa = BR.evaluate_literal(wav, 4)
    assert fb == fa == 0 and ib == ia and np.abs(pa - pb).max() <= 1e-9
    # SDR(i, j) of the live references against their own estimates is that of the two-source problem
    p2 = BR.evaluate(two, 4)[0]
    assert abs(pb[0] - p2[0]) <= 1e-9
    silent = np.zeros((4, 200), np.float32)
    silent[2:] = 1.0
    for ev in (BR.evaluate, BR.evaluate_literal):
        per, idx, fl = ev(silent, 4)
        assert not per.any() and idx == 0 and fl == BR.FLAG_SILENT
    mean4, per_utt, perm, flags = BR.evaluate_batch(np.stack([silent, wav[[0, 2, 3, 5]]]), 4)
    assert flags.tolist() == [BR.FLAG_SILENT, 0] and (mean4 == per_utt[1]).all()


def test_a_filter_as_long_as_the_signal_clamps_sar():
    C, Ls, L = 2, 9, 8                                       # C L = 16 >= Ls + L - 1 = 16: the delays span everything
    assert C * L >= Ls + L - 1
    wav = BR.make_case(C, Ls, L, seed=2)[0]
    sdr, sir, sar = BR.evaluate_literal(wav, L, with_table=True)[3]
    assert sar == [100.0, 100.0]
    per, idx, fl = BR.evaluate_literal(wav, L)
    assert per[2] == 100.0


def test_clamp_flag_and_tie_rules():
    assert BR.q(0.0, 1.0) == -100.0 and BR.q(-1.0, -1.0) == -100.0 and BR.q(1.0, 0.0) == 100.0
    assert BR.q(1.0, -1e-30) == 100.0 and BR.q(1.0, 1e-30) == 100.0 and BR.q(1e-30, 1.0) == -100.0
    assert BR.q(10.0, 1.0) == 10.0 and BR.q(float('nan'), 1.0) == -100.0
    tie = [[3.0, 3.0], [3.0, 3.0]]
    assert BR.search(tie, [True, True])[0] == 0
    tie3 = [[0.0, 2.0, 2.0], [2.0, 0.0, 2.0], [2.0, 2.0, 0.0]]          # (1, 2, 0) and (2, 0, 1) tie at 6
    assert BR.search(tie3, [True, True, True]) == (3, (1, 2, 0))
    assert BR.search(tie3, [False, False, False]) == (0, (0, 1, 2))
    assert BR.search([[1.0, 5.0], [9.0, 0.0]], [True, False])[0] == 1   # the silent row does not vote
    x, f = BR.chol_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones((1, 2)))
    assert f == 1
    x, f = BR.chol_solve(np.array([[4.0, 2.0], [2.0, 3.0]]), np.array([[2.0, 1.0]]))
    assert f == 0 and np.allclose(x, [[0.5, 0.0]])
    per, idx, fl = BR.scores([[1.0]], [1.0], [1.0], [2.0], 2.0, [True], flag=1)
    assert not per.any() and idx == 0 and fl == BR.FLAG_PIVOT
    assert (BR.batch_mean([[1, 2, 3, 4], [5, 6, 7, 8], [9, 9, 9, 9]], [0, 1, 0]) == [5.0, 5.5, 6.0, 6.5]).all()
    assert not BR.batch_mean([[1, 2, 3, 4]], [2]).any()
    assert BR.backward_error(np.eye(2), np.ones(2), np.ones(2)) == 0.0
