'''
CPU tests (no GPU) of the intelligibility figures (EVAL_STOI): the extension library libdanet_stoi_hip.so against its
header (exports, prototypes, ABI, lazy load, every host-visible argument error), the untouched other sixteen
libraries, the open MORE_EXTENSIONS registry, the configuration key and every ValueError, and the float64 restatement
of tests/stoi_ref.py against scipy, against a literal loop and against known answers.
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
import stoi_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_stoi_hip.h')
STOI_SYMBOLS = ['danet_stoi_abi_version', 'danet_stoi_bands', 'danet_stoi_finalize', 'danet_stoi_frames',
                'danet_stoi_last_error', 'danet_stoi_resample', 'danet_stoi_segments', 'danet_stoi_workspace_bytes']
NO_WS = ctypes.c_size_t(-1).value
# the export lists of the sixteen older libraries: sha1 of their sorted, space-joined names (first 12 digits)
OLDER = {'': (51, '35c97f3a2452'), 'conv': (7, '9446af6b053c'), 'dropout': (3, '31a0846a9f05'),
         'prep': (6, '4528d8ffdc78'), 'mix': (5, 'a519a2795d7a'), 'speed': (4, 'e1adf1c490af'),
         'reverb': (3, '05ef787913e5'), 'metric': (6, 'eff9d5e3632c'), 'noise': (3, 'cf88e352bf83'),
         'level': (4, '7fdea6b0fb6a'), 'wavloss': (4, 'e9c25e57750d'), 'gclip': (5, 'a9921dcbc5d9'),
         'dpcl': (7, '8021ee69c5d3'), 'neval': (6, '44b1be58a6d8'), 'stitch': (7, '2ab75117a25c'),
         'bss': (7, '265172254200')}


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_stoi_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_stoi()
    syms = _header_symbols('danet_stoi_hip.h', 'danet_stoi_')
    assert syms == STOI_SYMBOLS
    assert sorted(_lib.STOI_PROTOTYPES) == syms
    assert _exports(_lib.STOI_LIB_PATH) == syms
    assert lib.danet_stoi_abi_version() == 1 == _lib.STOI_ABI_VERSION == _lib.STOI.abi
    txt = open(HEADER).read()
    assert '#define DANET_STOI_ABI_VERSION 1' in txt
    for name, value in (('MAX_C', SR.MAX_C), ('MAX_BATCH', SR.MAX_BATCH), ('MAX_TABLE', SR.MAX_TABLE),
                        ('FRAME', SR.FRAME), ('HOP', SR.HOP), ('BANDS', SR.BANDS), ('SEG', SR.SEG)):
        assert re.search(r'#define DANET_STOI_%s %d\b' % (name, value), txt), name
    assert ops.STOI_MAX_C == SR.MAX_C and ops.STOI_MAX_TABLE == SR.MAX_TABLE and ops.STOI_MIN_RATE == SR.MIN_RATE \
        and ops.STOI_FS == SR.FS
    rule = txt.split('#ifndef')[0]
    for words in ('m[n] = s_0[n] + s_1[n] + ...', 'H = 10 max(U, D)', "firwin(2H + 1, 1 / max(U, D), window = ('kaiser', 5.0))",
                  'L10 = ceil(Ls U / D)', 'y[n] = sum_k h[n D + H - k U] x[k]', 'scipy.signal.resample_poly(x, U, D)',
                  'nf = floor((L10 - 256) / 128) + 1', 'hanning(258)[1:-1]', 'E_f > 1e-4 * max_f E_f',
                  'w[n + 128] z[128 k(q - 1) + n + 128]', 'w[n - 128] z[128 k(q + 1) + n - 128]', 'FFT_512',
                  '150 * 2^((2b - 1) / 6)', 'alpha = |X_b| / |Y_b|', '6.623413251903491', 'there is no epsilon',
                  'itertools.permutations(range(C)) order', 'left out of the\n *    batch means', 'no atomics',
                  'no transcendental math'):
        assert words in rule, words
    assert _lib.STOI.prototypes is _lib.STOI_PROTOTYPES and _lib.STOI.prefix == 'danet_stoi_'


def test_the_band_table_equals_the_integers_of_the_header():
    rule = open(HEADER).read().split('#ifndef')[0]
    pairs = re.findall(r'\{(\d+), (\d+)\}', rule)
    assert tuple((int(a), int(b)) for a, b in pairs) == SR.BAND_BINS == SR.band_table() and len(pairs) == 15
    assert abs(SR.CLIP - (1 + 10 ** (15 / 20))) < 1e-15
    # consecutive, inside the 257 bins, from 150 Hz / 2^(1/6) up to 4.3 kHz
    assert all(SR.BAND_BINS[b][1] == SR.BAND_BINS[b + 1][0] for b in range(14)) and SR.BAND_BINS[-1][1] <= 257


def test_stoi_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    ctype = {'void*': p, 'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'const float*': p,
             'float*': p, 'double*': p, 'const double*': p, 'int32_t*': p, 'const int32_t*': p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.STOI_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.STOI_PROTOTYPES['danet_stoi_' + n][1])
            for n in ('workspace_bytes', 'resample', 'frames', 'bands', 'segments', 'finalize')] == [5, 9, 11, 11, 7, 14]


def test_stoi_is_in_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.STOI in _lib.MORE_EXTENSIONS and build.STOI in build.MORE_EXTENSIONS
    assert isinstance(_lib.STOI, _lib.Library) and isinstance(build.STOI, build.Library)
    closed = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert _lib.STOI not in closed and len(closed) == 14
    assert build.STOI not in build.LIBRARIES + build.LATER_LIBRARIES + build.EXTENSIONS
    # it follows the records that were there
    assert _lib.MORE_EXTENSIONS.index(_lib.STOI) > _lib.MORE_EXTENSIONS.index(_lib.BSS) == 1
    assert build.MORE_EXTENSIONS.index(build.STOI) > build.MORE_EXTENSIONS.index(build.BSS) == 1
    assert [lib.name for lib in _lib.MORE_EXTENSIONS] == [os.path.basename(spec.src_dir)
                                                          for spec in build.MORE_EXTENSIONS]
    assert build.STOI_LIB == build.STOI.out == _lib.STOI_LIB_PATH
    assert os.path.basename(build.STOI_LIB) == _lib.STOI.so == 'libdanet_stoi_hip.so'
    assert os.path.isfile(os.path.join(build.STOI.src_dir, 'exports.map'))
    assert build.STOI.headers == (HEADER, os.path.join(csrc_scan.CSRC, 'ext_core.h'))
    assert callable(build.build_stoi) and callable(_lib.load_stoi) and callable(_lib.stoi_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:9] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL,
                        build.STITCH, build.BSS]
    assert build.STOI in rest[9:] and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 17      # the sixteen older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_sixteen_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS + _lib.MORE_EXTENSIONS[:2]
    assert [spec.name for spec in older] == list(OLDER)
    assert [spec.abi for spec in older] == [7] + [1] * 15
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_stoi_') for s in exported), spec.so
        assert (len(exported), hashlib.sha1(' '.join(exported).encode()).hexdigest()[:12]) == OLDER[spec.name], spec.so


def test_stoi_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.STOI_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipStreamSynchronize', 'hipDeviceSynchronize'):
        assert not re.search(r'\b%s\w*\b' % word, out.stdout), word
    d = os.path.join(csrc_scan.CSRC, 'stoi')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['stoi.hip']
    code = csrc_scan.strip_comments(open(os.path.join(d, 'stoi.hip')).read())
    code += csrc_scan.shared_code(code)              # and the shared header it includes
    assert csrc_scan.shared_headers(code) == [os.path.join(csrc_scan.CSRC, 'ext_core.h')]
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', 'common.h', 'Synchronize',
                 'hipMemcpy', 'asm', 'sincos', 'cos(', 'sin(', 'exp(', 'log', 'pow('):
        assert word not in code, word


def test_import_and_a_model_with_the_key_null_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, ozers, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "real, _lib.load_stoi = _lib.load_stoi, None          # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._stoi is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model._check_eval_stoi())\n"
        "hparams.load(dict(EVAL_STOI=False)); print('FALSE:', model.Model._check_eval_stoi())\n"
        "hparams.load(dict(EVAL_STOI=True)); print('TRUE:', model.Model._check_eval_stoi(), model.Model._stoi_key())\n"
        "_lib.load_stoi = real\n"
        "_lib.STOI_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_stoi()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_stoi_hip.so' in str(e) and %r in str(e)\n"
        "          and 'EVAL_STOI' in str(e))\n"
        "print('NONE:', _lib._stoi is None and 'libdanet_stoi' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: False', 'FALSE: False', 'TRUE: True True', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------- argument errors
def _parts_bytes(parts):
    import torch
    return sum(((int(np.prod(s)) * (8 if d == torch.float64 else 4)) + 255) & ~255 for _, s, d in parts)


def test_workspace_bytes_and_its_envelope():
    from danet_amd import _lib, ops
    lib = _lib.load_stoi()
    for B, C, Ls, U, D in ((1, 1, 1, 5, 4), (3, 2, 255, 1, 1), (2, 4, 8128, 5, 4), (32, 2, 8128, 5, 8),
                           (16383, 1, 300, 100, 441), (7, 3, 2049, 100, 819)):
        assert lib.danet_stoi_workspace_bytes(B, C, Ls, U, D) == _parts_bytes(ops.stoi_parts(B, C, Ls, U, D)) \
            == ops.stoi_workspace_bytes(B, C, Ls, U, D)
        assert [p[0] for p in ops.stoi_parts(B, C, Ls, U, D)] == [
            'sig', 'E', 'mask', 'kidx', 'M', 'Emax', 'T', 'd', 'per_utt', 'perm_idx', 'flags', 'mean4', 'count']
        assert ops.stoi_lengths(Ls, U, D) == (SR.out_len(Ls, U, D), SR.num_frames(SR.out_len(Ls, U, D)))
    assert ops.stoi_group(32, 2, 8128, 5, 4) == 32 and ops.stoi_group(1, 4, 100, 5, 4) == 1
    for bad in ((0, 2, 100, 5, 4), (16384, 2, 100, 5, 4), (1, 0, 100, 5, 4), (1, 5, 100, 5, 4), (1, 2, 0, 5, 4),
                (1, 2, 1 << 31, 5, 4), (1, 2, (1 << 31) - 1, 5, 4), (1, 2, 100, 0, 4), (1, 2, 100, 5, 0),
                (1, 2, 100, 10, 8), (1, 2, 100, 820, 1), (1, 2, 100, 1, 8001), (-1, 2, 100, 5, 4)):
        assert lib.danet_stoi_workspace_bytes(*bad) == NO_WS, bad
        assert b'workspace_bytes: need 1 <= B' in lib.danet_stoi_last_error()
    with pytest.raises(_lib.DanetHipError) as e:
        ops.stoi_workspace_bytes(1, 5, 100, 5, 4)
    assert str(e.value).startswith('libdanet_stoi_hip error -1: workspace_bytes: need 1 <= B')


def test_argument_errors_without_gpu():
    '''every host-visible argument error is returned before any launch: no device is needed to see them'''
    from danet_amd import _lib
    lib = _lib.load_stoi()
    batch = [(dict(B=0), b'need 1 <= B'), (dict(B=16384), b'need 1 <= B'), (dict(C=0), b'need 1 <= B'),
             (dict(C=5), b'need 1 <= B')]
    rates = [(dict(U=0), b'U and D must be'), (dict(D=0), b'U and D must be'), (dict(U=10, D=8), b'U and D must be'),
             (dict(U=820, D=1), b'U and D must be'), (dict(U=1, D=8001), b'U and D must be'),
             (dict(U=-5), b'U and D must be')]
    bins = (ctypes.c_int32 * 30)(*[v for lo_hi in SR.BAND_BINS for v in lo_hi])
    ok = dict(stream=None, B=2, C=2, Ls=300, U=5, D=4, wav=4096, h=8192, sig=16384)
    cases = batch + rates + [(dict(Ls=0), b'Ls and ceil(Ls U / D) must be'), (dict(Ls=1 << 31), b'Ls and ceil(Ls U / D) must be'),
                             (dict(Ls=(1 << 31) - 1), b'Ls and ceil(Ls U / D) must be'), (dict(Ls=-5), b'Ls and ceil(Ls U / D) must be')]
    cases += [({k: None}, b'null') for k in ('wav', 'h', 'sig')]
    cases += [(dict(wav=4098), b'misaligned'), (dict(sig=16386), b'misaligned'), (dict(h=8196), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_stoi_resample(*a.values()) == -1, kw
        assert b'resample: ' + msg in lib.danet_stoi_last_error(), (kw, lib.danet_stoi_last_error())
    ok = dict(stream=None, B=2, C=2, L10=375, sig=4096, w=8192, E=16384, mask=32768, kidx=65536, M=1024, Emax=2048)
    cases = batch + [(dict(L10=0), b'L10 must be'), (dict(L10=1 << 31), b'L10 must be')]
    cases += [({k: None}, b'null') for k in ('sig', 'w', 'E', 'mask', 'kidx', 'M', 'Emax')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('sig', 'w', 'mask', 'kidx', 'M')]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in ('E', 'Emax')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_stoi_frames(*a.values()) == -1, kw
        assert b'frames: ' + msg in lib.danet_stoi_last_error(), (kw, lib.danet_stoi_last_error())
    ok = dict(stream=None, B=2, C=2, L10=375, sig=4096, w=8192, tw=16384, bands=ctypes.addressof(bins), kidx=65536,
              M=1024, T=2048)
    cases = batch + [(dict(L10=0), b'L10 must be'), (dict(L10=1 << 31), b'L10 must be')]
    cases += [({k: None}, b'null') for k in ('sig', 'w', 'tw', 'bands', 'kidx', 'M', 'T')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('sig', 'w', 'kidx', 'M', 'bands')]
    cases += [(dict(tw=16392), b'misaligned'), (dict(T=2052), b'misaligned')]
    for lo, hi in ((-1, 3), (5, 4), (250, 258)):
        bad = (ctypes.c_int32 * 30)(*bins)
        bad[8], bad[9] = lo, hi
        cases.append((dict(bands=ctypes.addressof(bad), _keep=bad), b'band 4 must have'))
    for kw, msg in cases:
        a = dict(ok, **kw)
        a.pop('_keep', None)
        assert lib.danet_stoi_bands(*a.values()) == -1, kw
        assert b'bands: ' + msg in lib.danet_stoi_last_error(), (kw, lib.danet_stoi_last_error())
    # a row shorter than a frame: nothing to launch, and no device is needed to learn it
    assert lib.danet_stoi_bands(*dict(ok, L10=255).values()) == 0
    ok = dict(stream=None, B=2, C=2, nf=40, T=4096, M=1024, d=2048)
    cases = batch + [(dict(nf=-1), b'nf must be'), (dict(nf=1 << 24), b'nf must be')]
    cases += [({k: None}, b'null') for k in ('T', 'M', 'd')]
    cases += [(dict(T=4100), b'misaligned'), (dict(d=2052), b'misaligned'), (dict(M=1026), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_stoi_segments(*a.values()) == -1, kw
        assert b'segments: ' + msg in lib.danet_stoi_last_error(), (kw, lib.danet_stoi_last_error())
    ok = dict(stream=None, B=2, C=2, nf=40, d=8192, M=1024, Emax=2048, b0=0, B_all=2, per_utt=65536, perm_idx=256,
              flags=128, mean4=131072, count=512)
    p8, p4 = ('d', 'Emax', 'per_utt', 'mean4'), ('M', 'perm_idx', 'flags', 'count')
    cases = batch + [(dict(nf=-1), b'nf must be'), (dict(nf=1 << 24), b'nf must be'), (dict(b0=-1), b'need b0 >= 0'),
                     (dict(b0=1), b'need b0 >= 0'), (dict(B_all=1), b'need b0 >= 0'), (dict(B_all=16384), b'need b0 >= 0')]
    cases += [({k: None}, b'null') for k in p8 + p4]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in p8] + [({k: ok[k] + 2}, b'misaligned') for k in p4]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_stoi_finalize(*a.values()) == -1, kw
        assert b'finalize: ' + msg in lib.danet_stoi_last_error(), (kw, lib.danet_stoi_last_error())
    assert _lib.stoi_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.stoi_check(-1)
    assert str(e.value).startswith('libdanet_stoi_hip error -1: finalize: misaligned')


# ----------------------------------------------------------------------------------- the key
def test_the_key_defaults_to_null_and_means_off(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    assert 'EVAL_STOI' in H.DEFAULTS and H.DEFAULTS['EVAL_STOI'] is None and hp.EVAL_STOI is None
    assert re.fullmatch(hp.pattern, 'EVAL_STOI') and 'EVAL_STOI' in H.__doc__
    hp.digest()
    assert Model._check_eval_stoi() is False
    for di, want in ((dict(EVAL_STOI=False), False), (dict(EVAL_STOI=True), True),
                     (dict(EVAL_STOI=True, EVAL_SI_SDR=True, EVAL_BSS_SDR=True), True),
                     (dict(EVAL_STOI=True, SMPRATE=16000), True), (dict(EVAL_STOI=True, SMPRATE=44100), True),
                     (dict(EVAL_STOI=True, SMPRATE=10000), True), (dict(EVAL_STOI=True, SMPRATE=81900), True),
                     (dict(EVAL_STOI=True, MAX_N_SIGNAL=4, FFT_SIZE=64, FFT_STRIDE=8), True),
                     (dict(MAX_N_SIGNAL=5, FFT_SIZE=48, SMPRATE=4000), False)):   # off: nothing is looked at
        hp.reset()
        hp.load(di)
        assert Model._check_eval_stoi() is want, di


@pytest.mark.parametrize('keys,di', [
    (('EVAL_STOI',), dict(EVAL_STOI=1)), (('EVAL_STOI',), dict(EVAL_STOI='true')), (('EVAL_STOI',), dict(EVAL_STOI=0.0)),
    (('EVAL_STOI', 'MAX_N_SIGNAL'), dict(EVAL_STOI=True, MAX_N_SIGNAL=5)),
    (('EVAL_STOI', 'FFT_SIZE'), dict(EVAL_STOI=True, FFT_SIZE=48, FFT_STRIDE=12)),
    (('EVAL_STOI', 'FFT_SIZE'), dict(EVAL_STOI=True, FFT_SIZE=2048, FFT_STRIDE=512)),
    (('EVAL_STOI', 'FFT_STRIDE'), dict(EVAL_STOI=True, FFT_SIZE=256, FFT_STRIDE=192)),
    (('EVAL_STOI', 'FFT_STRIDE'), dict(EVAL_STOI=True, FFT_SIZE=256, FFT_STRIDE=16)),
    (('EVAL_STOI', 'NOISE_EVAL_DIR'), dict(EVAL_STOI=True, NOISE_EVAL_DIR='/nowhere')),
    (('EVAL_STOI', 'NOISE_EVAL_DIR'), dict(EVAL_STOI=True, EVAL_SI_SDR=True, NOISE_EVAL_DIR='/nowhere')),
    (('EVAL_STOI', 'SMPRATE'), dict(EVAL_STOI=True, SMPRATE=7999)),
    (('EVAL_STOI', 'SMPRATE'), dict(EVAL_STOI=True, SMPRATE=4000)),
    (('EVAL_STOI', 'SMPRATE'), dict(EVAL_STOI=True, SMPRATE=8001)),          # D = 8001: 160021 entries
    (('EVAL_STOI', 'SMPRATE'), dict(EVAL_STOI=True, SMPRATE=82100)),         # 100 / 821: 16421 entries
    (('EVAL_STOI', 'SMPRATE'), dict(EVAL_STOI=True, SMPRATE=16000.0))])
def test_build_raises_and_names_the_key(hp, keys, di):
    from danet_amd.model import Model
    hp.load(di)
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('stoi', device='cuda:0').build()               # raised before anything touches a device
    for key in keys:
        assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)
    if 'FFT_SIZE' in keys or 'FFT_STRIDE' in keys or 'MAX_N_SIGNAL' in keys:
        assert 'EVAL_SI_SDR' not in str(e.value) and 'EVAL_BSS_SDR' not in str(e.value)


def test_the_table_limit_is_the_headers_and_no_flag_is_added(hp):
    from danet_amd import cli, ops
    assert ops.stoi_rate(8000) == SR.rate(8000) == (5, 4, 50) and ops.stoi_rate(44100) == SR.rate(44100) == (100, 441, 4410)
    assert ops.stoi_rate(10000) == SR.rate(10000) == (1, 1, 0) and ops.stoi_rate(16000) == (5, 8, 80)
    assert ops.stoi_rate(81900) == (100, 819, 8190)           # 16381 entries: the longest table that fits
    with pytest.raises(ValueError):
        ops.stoi_rate(82100)                                  # 100 / 821: 16421 entries
    src = open(cli.__file__).read().lower()
    assert 'stoi' not in src
    opts = [a.dest for a in cli.build_parser()._actions]
    assert len(opts) == 15 and not any('stoi' in o for o in opts)


# ----------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('smprate', [8000, 16000, 44100])
def test_the_resampler_is_resample_poly(smprate):
    import scipy.signal
    U, D, H = SR.rate(smprate)
    h = SR.table(smprate)
    assert len(h) == 2 * H + 1 <= SR.MAX_TABLE
    for Ls in (1, 2, 37, 1000, 2049):
        x = np.random.RandomState(Ls).standard_normal(Ls)
        y, taps, a = SR.resample(x, U, D, H, h, with_bound=True)
        want = scipy.signal.resample_poly(x, U, D)
        assert y.shape == want.shape == (SR.out_len(Ls, U, D),)
        assert np.abs(y - want).max() <= 1e-12, (smprate, Ls)
        assert taps.min() >= 1 and taps.max() <= 2 * H // U + 1 and (a >= np.abs(y) - 1e-12).all()
    assert SR.rate(10000) == (1, 1, 0) and np.array_equal(SR.resample([1.5, -2.0], 1, 1, 0, SR.table(10000)), [1.5, -2.0])


def test_silent_frame_removal_equals_a_literal_loop():
    w = SR.window()
    assert w.dtype == np.float32 and w.shape == (256,) and w[0] > 0 and np.allclose(w, w[::-1])
    rng = np.random.RandomState(3)
    for n, period in ((10160, 1500), (4000, 900), (1500, 1200)):
        x = SR.make_signal(rng, n, period)
        z = (x + 0.1 * rng.standard_normal(n)).astype(np.float32)
        mask, k, E = SR.kept(x, w)
        assert 0 < len(k) < len(mask) == SR.num_frames(n) and SR.margin_db(E) > 1e-6
        # the mask, literally
        want = [sum((float(w[i]) * float(x[128 * f + i])) ** 2 for i in range(256)) for f in range(len(mask))]
        assert np.allclose(E, want, rtol=1e-12) and [e > 1e-4 * max(want) for e in want] == mask.tolist()
        for sig in (x, z):
            assert np.array_equal(SR.compact(sig, w, k), SR.compact_loop(sig, w, mask))
    assert SR.num_frames(255) == 0 and SR.num_frames(256) == 1 and SR.num_frames(383) == 1 and SR.num_frames(384) == 2 \
        and SR.num_frames(385) == 2
    assert SR.kept(np.zeros(1000, np.float32), w)[0].tolist() == [False] * 6           # no energy: nothing is kept


def _speech(seed, n=10160):
    return SR.make_signal(np.random.RandomState(seed), n, 1700)


def test_identity_monotony_and_gain_invariance():
    x = _speech(1)
    a, e = SR.stoi(x, x)
    assert abs(a - 1) <= 1e-12 and abs(e - 1) <= 1e-12
    rng = np.random.RandomState(2)
    n = rng.standard_normal(len(x)) * np.std(x)
    got = [SR.stoi(x, (x + n * 10 ** (-snr / 20)).astype(np.float32)) for snr in (20, 10, 0, -10)]
    print('STOI / ESTOI at 20, 10, 0, -10 dB: %s' % (np.round(got, 4).tolist(),))
    assert all(got[i][0] > got[i + 1][0] and got[i][1] > got[i + 1][1] for i in range(3))
    assert got[0][0] < 1 and got[3][0] > 0
    y = (x + n * 10 ** (-5 / 20)).astype(np.float32)
    base = SR.stoi(x, y)
    for gx, gy in ((4.0, 1.0), (1.0, 0.25), (0.5, 8.0)):     # powers of two: the float32 rows scale exactly
        assert np.abs(np.subtract(SR.stoi(gx * x, gy * y), base)).max() <= 1e-12
    for gx, gy in ((3.0, 1.0), (1.0, 0.7)):                  # any gain: up to the float32 rounding of the rows
        assert np.abs(np.subtract(SR.stoi((gx * x).astype(np.float32), (gy * y).astype(np.float32)), base)).max() <= 1e-5


def test_the_zero_norm_guards_and_the_float32_run():
    rng = np.random.RandomState(4)
    X, Y = np.abs(rng.standard_normal((15, 40))), np.abs(rng.standard_normal((15, 40)))
    a, e = SR.segment_values(X, X)
    assert np.abs(a - 1).max() <= 1e-12 and np.abs(e - 1).max() <= 1e-12 and a.shape == (11,)
    Y0 = Y.copy()
    Y0[3] = 0.0                                              # a band row of zeros: it contributes 0, nothing is NaN
    a0, e0 = SR.segment_values(X, Y0)
    assert np.isfinite(a0).all() and np.isfinite(e0).all()
    full = SR.segment_values(X, Y)[0]
    r3 = SR.segment_values(np.tile(X[3], (15, 1)), np.tile(Y[3], (15, 1)))[0]       # the row's own coefficient
    assert np.abs(a0 - (full - r3 / 15)).max() <= 1e-12
    Xc = np.ones((15, 40))                                   # constant rows: every norm is zero
    assert not SR.segment_values(Xc, Y)[0].any() and not SR.segment_values(Xc, Y)[1].any()
    a32, e32 = SR.segment_values(X, Y, np.float32)
    assert a32.dtype == np.float32 and 0 < np.abs(a32 - SR.segment_values(X, Y)[0]).max() < 1e-5
    assert SR.segments(X[:, :29], Y[:, :29]) == (0.0, 0.0)


def test_m_29_is_flagged_and_m_30_is_not():
    w = SR.window()
    for M, flagged in ((29, True), (30, False)):
        x = _speech(5, 128 * (M - 1) + 256)[None]            # M frames in all
        x = np.concatenate([x, (x + 0.1).astype(np.float32)])
        mask, k, E = SR.kept(x[0], w)
        loud = np.random.RandomState(6).standard_normal(x.shape[1]).astype(np.float32)
        wav = np.stack([loud, (loud + 0.3 * x[1]).astype(np.float32)])
        assert SR.kept(loud, w)[0].all() and len(SR.kept(loud, w)[1]) == M
        per, idx, fl = SR.evaluate(wav, SR.FS)
        assert (fl == SR.FLAG_SHORT) == flagged and fl in (0, SR.FLAG_SHORT), (M, fl)
        assert (not per.any()) == flagged and idx == 0
    st, es = [[0.9, 0.5]], [[0.8, 0.4]]
    assert SR.scores(st, es, [29], [True])[2] == SR.FLAG_SHORT and SR.scores(st, es, [30], [True])[2] == 0
    assert np.allclose(SR.scores(st, es, [30], [True])[0], [0.9, 0.8, 0.4, 0.4])
    assert SR.scores(st, es, [0], [False])[2] == SR.FLAG_SILENT
    # a silent reference takes no part: neither in the flag nor in the search
    st2 = [[0.1, 0.9, 0.3], [0.7, 0.2, 0.3]]
    per, idx, fl = SR.scores(st2, st2, [40, 0], [True, False])
    assert fl == 0 and idx == 1 and np.allclose(per, [0.9, 0.9, 0.6, 0.6])
    assert SR.search([[3.0, 3.0], [3.0, 3.0]], [True, True])[0] == 0
    tie3 = [[0.0, 2.0, 2.0], [2.0, 0.0, 2.0], [2.0, 2.0, 0.0]]
    assert SR.search(tie3, [True, True, True]) == (3, (1, 2, 0)) and SR.search_gap(tie3, [True] * 3) == 0.0
    mean4, count = SR.batch_mean([[1, 2, 3, 4], [5, 6, 7, 8], [9, 9, 9, 9]], [0, 1, 0])
    assert (mean4 == [5.0, 5.5, 6.0, 6.5]).all() and count == 2
    mean4, count = SR.batch_mean([[1, 2, 3, 4]], [2])
    assert not mean4.any() and count == 0


def test_the_whole_rule_on_two_sources():
    wav = SR.make_case(2, 8128, seed=3)
    per, idx, fl = SR.evaluate(wav, 8000)
    assert fl == 0 and idx == 0 and 0.5 < per[0] < 1 and 0.3 < per[1] < per[0] and per[2] > 0 and per[3] > 0
    swapped = np.concatenate([wav[:2], wav[[3, 2]]])
    per2, idx2, fl2 = SR.evaluate(swapped, 8000)
    assert idx2 == 1 and np.abs(per2 - per).max() <= 1e-12
    p32 = SR.evaluate(wav, 8000, dtype=np.float32)[0]
    assert 0 < np.abs(p32 - per).max() < 1e-5
    mean4, per_utt, perm, flags, count = SR.evaluate_batch(np.stack([wav, np.zeros_like(wav)]), 8000)
    assert flags.tolist() == [0, SR.FLAG_SILENT] and count == 1 and np.array_equal(mean4, per_utt[0])
