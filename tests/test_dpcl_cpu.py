'''
CPU tests (no GPU) of the deep-clustering auxiliary loss (DPCL_WEIGHT): the extension library libdanet_dpcl_hip.so
against its header (exports, prototypes, ABI, lazy load, host-visible argument errors), the untouched other twelve
libraries, the open EXTENSIONS registry, the configuration key, and the restatement tests/dpcl_ref.py against torch
float64 autograd of the literal N x N loss and against known answers.
'''
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dpcl_ref as DR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_dpcl_hip.h')
DPCL_SYMBOLS = ['danet_dpcl_abi_version', 'danet_dpcl_bwd', 'danet_dpcl_chunks', 'danet_dpcl_finalize',
                'danet_dpcl_last_error', 'danet_dpcl_stats', 'danet_dpcl_workspace_bytes']
KEY = 'DPCL_WEIGHT'
NO_WS = ctypes.c_size_t(-1).value


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


def _case(N, E, C, seed=0, ties=True):
    '''normal embeddings, uniform magnitudes, and (N permitting) rows with exact ties and exact zeros'''
    rng = np.random.RandomState(1000 * N + 10 * E + C + seed)
    V = rng.standard_normal((N, E))
    S = rng.uniform(0.0, 2.0, (C, N)).astype(np.float32)
    if ties and N >= 4:
        S[:, 1] = S[0, 1]              # an exact tie of every source
        S[:, 2] = 0.0                  # an all-zero bin
        if C > 1:
            S[-1, 3] = S[-2, 3]        # a tie of the last two
    return V, S


# ------------------------------------------------------------------------------------------ ABI
def test_dpcl_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_dpcl()
    syms = _header_symbols('danet_dpcl_hip.h', 'danet_dpcl_')
    assert syms == DPCL_SYMBOLS
    assert sorted(_lib.DPCL_PROTOTYPES) == syms
    assert _exports(_lib.DPCL_LIB_PATH) == syms
    assert lib.danet_dpcl_abi_version() == 1 == _lib.DPCL_ABI_VERSION == _lib.DPCL.abi
    txt = open(HEADER).read()
    assert '#define DANET_DPCL_ABI_VERSION 1' in txt
    assert '#define DANET_DPCL_MAX_E %d' % DR.MAX_E in txt and ops.DPCL_MAX_E == DR.MAX_E
    assert '#define DANET_DPCL_MAX_C %d' % DR.MAX_C in txt and ops.DPCL_MAX_C == DR.MAX_C
    assert '#define DANET_DPCL_MAX_CHUNKS %d' % DR.MAX_CHUNKS in txt
    assert '#define DANET_DPCL_TILE_ROWS %d' % DR.TILE_ROWS in txt
    rule = txt.split('#ifndef')[0]
    for words in ('the lowest c with S_ci = max_c', 'w_i        = s_i / sum_j s_j', 'A          = sum_i w_i v_i v_i^T',
                  'L_b        = ||A||_F^2 - 2 ||Bm||_F^2 + sum_k c_k^2', 'dpcl       = (1 / B) sum_b L_b',
                  'total      = main + alpha * dpcl', 'dloss * (alpha / B) * 4 w_i (A v_i - Bm[:, y_i])',
                  'L_b = 0 and a zero gradient', 'chunk_rows(N) = 128 * ceil(ceil(N / DANET_DPCL_MAX_CHUNKS) / 128)'):
        assert words in rule, words
    assert '16-byte loads; otherwise' in txt and 'never an error' in txt          # the misaligned embedding
    assert _lib.DPCL.prototypes is _lib.DPCL_PROTOTYPES and _lib.DPCL.prefix == 'danet_dpcl_'


def test_dpcl_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    ctype = {'void*': p, 'const void*': p, 'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
             'size_t': ctypes.c_size_t, 'const float*': p, 'double*': p, 'float*': p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.DPCL_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.DPCL_PROTOTYPES['danet_dpcl_' + n][1]) for n in ('stats', 'finalize', 'bwd')] == [9, 14, 12]


def test_dpcl_is_appended_to_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.DPCL in _lib.EXTENSIONS and build.DPCL in build.EXTENSIONS
    assert isinstance(_lib.DPCL, _lib.Library) and isinstance(build.DPCL, build.Library)
    assert _lib.DPCL not in _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert build.DPCL not in build.LIBRARIES + build.LATER_LIBRARIES
    assert [lib.name for lib in _lib.EXTENSIONS] == [os.path.basename(spec.src_dir) for spec in build.EXTENSIONS]
    assert _lib.EXTENSIONS.index(_lib.DPCL) > _lib.EXTENSIONS.index(_lib.GCLIP)       # appended
    assert build.EXTENSIONS.index(build.DPCL) > build.EXTENSIONS.index(build.GCLIP)
    assert build.DPCL_LIB == build.DPCL.out == _lib.DPCL_LIB_PATH
    assert os.path.basename(build.DPCL_LIB) == _lib.DPCL.so == 'libdanet_dpcl_hip.so'
    assert os.path.isfile(os.path.join(build.DPCL.src_dir, 'exports.map'))
    assert callable(build.build_dpcl) and callable(_lib.load_dpcl) and callable(_lib.dpcl_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:5] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP] and build.DPCL in rest
    assert not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 13     # the twelve older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_twelve_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + (_lib.METRIC, _lib.NOISE, _lib.LEVEL, _lib.WAVLOSS, _lib.GCLIP)
    assert [spec.name for spec in older] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed', 'reverb', 'metric',
                                             'noise', 'level', 'wavloss', 'gclip']
    assert [spec.abi for spec in older] == [7] + [1] * 11
    assert len(_lib.LIBRARIES) == 5 and len(_lib.ALL_LIBRARIES) == 6 and len(_lib.LATER_LIBRARIES) == 1
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_dpcl_') for s in exported), spec.so
    assert sorted(_lib.GCLIP_PROTOTYPES) == ['danet_gclip_abi_version', 'danet_gclip_adam_step',
                                             'danet_gclip_last_error', 'danet_gclip_partials', 'danet_gclip_sumsq']


def test_dpcl_library_reads_no_environment_allocates_nothing_and_has_no_atomics():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.DPCL_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree'):
        assert not re.search(r'\b%s\b' % word, out.stdout), word
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'dpcl')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['dpcl.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'dpcl.hip')).read(), flags=re.S)
    code += csrc_scan.shared_code(code)              # and the shared headers it includes, same words: the
    assert '} while (0)' in code and '#include "ext_core.h"' in code       # allowance is for their macros
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', '__threadfence', 'while',
                 'common.h'):
        assert word not in code.replace('} while (0)', ''), word


def test_import_and_a_model_with_the_key_null_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, ozers, datasets, feed, cli\n"
        "real, _lib.load_dpcl = _lib.load_dpcl, None          # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._dpcl is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model('m', device='cpu').dpcl_weight, model.Model._check_dpcl_weight())\n"
        "_lib.load_dpcl = real\n"
        "_lib.DPCL_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_dpcl()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_dpcl_hip.so' in str(e) and %r in str(e)\n"
        "          and 'DPCL_WEIGHT' in str(e))\n"
        "print('NONE:', _lib._dpcl is None and 'libdanet_dpcl' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: None None', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


def test_chunks_and_workspace_are_the_headers_pure_functions():
    from danet_amd import _lib
    lib = _lib.load_dpcl()
    for N in (1, 2, 127, 128, 129, 2047, 2048, 2049, 4097, 16512, 100000, 1 << 20, (1 << 31) - 1, 1 << 31):
        n = lib.danet_dpcl_chunks(N)
        rows = DR.chunk_rows(N)
        assert n == DR.chunks(N) and 1 <= n <= DR.MAX_CHUNKS, N
        assert rows % DR.TILE_ROWS == 0 and (n - 1) * rows < N <= n * rows
        for B, E, C in ((1, 1, 1), (32, 20, 2), (9, 64, 4)):
            assert lib.danet_dpcl_workspace_bytes(B, N, E, C) == DR.workspace_bytes(B, N, E, C)
    assert DR.chunks(16512) == 15 and DR.chunk_rows(16512) == 1152 and DR.chunks(129) == 2
    for N in (0, -1, (1 << 31) + 1):
        assert lib.danet_dpcl_chunks(N) == 0 and b'N must be' in lib.danet_dpcl_last_error()
    for bad in ((0, 8, 4, 2), (65536, 8, 4, 2), (1, 0, 4, 2), (1, (1 << 31) + 1, 4, 2), (1, 8, 0, 2), (1, 8, 65, 2),
                (1, 8, 4, 0), (1, 8, 4, 5)):
        assert lib.danet_dpcl_workspace_bytes(*bad) == NO_WS, bad
        assert b'workspace_bytes: need' in lib.danet_dpcl_last_error()


def test_argument_errors_without_gpu():
    '''every host-visible argument error is returned before any launch: no device is needed to see them'''
    from danet_amd import _lib
    lib = _lib.load_dpcl()
    B, N, E, C = 3, 300, 20, 2
    need = DR.workspace_bytes(B, N, E, C)
    sizes = [(dict(B=0), b'need 1 <= B'), (dict(B=65536), b'need 1 <= B'), (dict(N=0), b'need 1 <= B'),
             (dict(N=(1 << 31) + 1), b'need 1 <= B'), (dict(E=0), b'need 1 <= B'), (dict(E=65), b'need 1 <= B'),
             (dict(C=0), b'need 1 <= B'), (dict(C=5), b'need 1 <= B')]
    ok = dict(stream=None, B=B, N=N, E=E, C=C, embed=4096, src_pwr=8192, ws=16384, ws_bytes=need)
    cases = sizes + [({k: None}, b'null') for k in ('embed', 'src_pwr', 'ws')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('embed', 'src_pwr', 'ws')]
    cases += [(dict(ws_bytes=need - 1), b'workspace too small'), (dict(ws_bytes=0), b'workspace too small')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_dpcl_stats(*a.values()) == -1, kw
        assert b'stats: ' + msg in lib.danet_dpcl_last_error(), (kw, lib.danet_dpcl_last_error())
    ok = dict(stream=None, B=B, N=N, E=E, C=C, ws=16384, ws_bytes=need, main=None, alpha=0.5, per_utt=4096, dpcl=8192,
              total=8196, tables=32768, cs=65536)
    cases = sizes + [({k: None}, b'null') for k in ('ws', 'per_utt', 'dpcl', 'total', 'tables', 'cs')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('ws', 'dpcl', 'total', 'tables', 'cs')]
    cases += [(dict(per_utt=4100), b'misaligned'), (dict(main=8194), b'misaligned')]
    cases += [(dict(alpha=v), b'alpha must') for v in (-1.0, float('inf'), float('nan'))]
    cases += [(dict(ws_bytes=need - 1), b'workspace too small')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_dpcl_finalize(*a.values()) == -1, kw
        assert b'finalize: ' + msg in lib.danet_dpcl_last_error(), (kw, lib.danet_dpcl_last_error())
    ok = dict(stream=None, B=B, N=N, E=E, C=C, embed=4096, src_pwr=8192, tables=16384, cs=32768, dloss=None,
              scale=0.25, dembed=65536)
    cases = sizes + [({k: None}, b'null') for k in ('embed', 'src_pwr', 'tables', 'cs', 'dembed')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('embed', 'src_pwr', 'tables', 'cs', 'dembed')]
    cases += [(dict(dloss=1026), b'misaligned')]
    cases += [(dict(scale=v), b'scale must') for v in (float('inf'), float('nan'))]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_dpcl_bwd(*a.values()) == -1, kw
        assert b'bwd: ' + msg in lib.danet_dpcl_last_error(), (kw, lib.danet_dpcl_last_error())
    assert _lib.dpcl_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.dpcl_check(-1)
    assert str(e.value).startswith('libdanet_dpcl_hip error -1: bwd: scale must')


# ----------------------------------------------------------------------------------- the key
def test_the_key_defaults_to_null_and_means_off(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    assert KEY in H.DEFAULTS and H.DEFAULTS[KEY] is None and getattr(hp, KEY) is None
    assert re.fullmatch(hp.pattern, KEY) and KEY in H.__doc__
    hp.digest()
    assert Model._check_dpcl_weight() is None and Model('m', device='cpu').dpcl_weight is None
    for v, want in ((0, 0.0), (0.0, 0.0), (0.1, 0.1), (3, 3.0), (1e30, 1e30)):          # 0.0 is ON
        hp.load({KEY: v})
        got = Model._check_dpcl_weight()
        assert got == want and isinstance(got, float)


@pytest.mark.parametrize('value', [True, False, 'x', '0.1', '', -1, -0.5, -1e-30, float('inf'), float('-inf'),
                                   float('nan')])
def test_build_raises_and_names_the_key(hp, value):
    from danet_amd.model import Model
    hp.load({KEY: value})
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('dpcl', device='cuda:0').build()               # raised before anything touches a device
    assert re.search(r'\b%s\b' % KEY, str(e.value))


@pytest.mark.parametrize('other,value', [('EMBED_SIZE', 65), ('EMBED_SIZE', 100), ('MAX_N_SIGNAL', 5)])
def test_build_raises_outside_the_headers_envelope_and_names_the_other_key(hp, other, value):
    from danet_amd.model import Model
    hp.load({KEY: 0.1, other: value})
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('dpcl', device='cuda:0').build()
    assert re.search(r'\b%s\b' % other, str(e.value)) and KEY in str(e.value)
    hp.load({KEY: None})
    assert Model._check_dpcl_weight() is None                # without the key the envelope is not looked at


def test_no_command_line_flag_is_added():
    from danet_amd import cli
    src = open(cli.__file__).read().lower()
    assert 'dpcl' not in src


# ----------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('N,E,C', [(1, 1, 1), (2, 1, 2), (65, 3, 2), (516, 20, 2), (516, 40, 3), (300, 64, 4)])
def test_restatement_against_float64_autograd_of_the_literal_loss(N, E, C):
    V, S = _case(N, E, C)
    L, g, st = DR.utterance(V, S)
    Lw, gw = DR.literal(V, S)
    scale = max(abs(Lw), DR.term_size(st))
    print('N=%d E=%d C=%d  loss %.3e (diff %.1e)  grad diff %.1e of %.3e'
          % (N, E, C, Lw, abs(L - Lw), np.abs(g - gw).max(), np.abs(gw).max()))
    assert abs(L - Lw) <= 1e-10 * scale
    assert np.abs(g - gw).max() <= 1e-10 * max(np.abs(gw).max(), DR.grad_bar(V, st))
    r = DR.batch(np.stack([V, 2 * V]), np.stack([S, S]), main=1.5, alpha=0.25, dloss=3.0)
    L2 = DR.utterance(2 * V, S)[0]
    assert abs(r['dpcl'] - (L + L2) / 2) <= 1e-15 * scale * 16 and r['total'] == 1.5 + 0.25 * r['dpcl']
    assert np.abs(r['dembed'][0] - g * (3.0 * 0.25 / 2)).max() <= 1e-15 * max(np.abs(g).max(), 1e-300)


def test_one_hot_embedding_has_zero_loss_and_zero_gradient():
    for N, E, C in ((65, 2, 2), (300, 5, 3), (129, 4, 4)):
        _, S = _case(N, E, C)
        V = np.zeros((N, E))
        V[np.arange(N), DR.labels(S)] = 1.0
        L, g, st = DR.utterance(V, S)
        assert abs(L) <= 1e-15 and np.abs(g).max() <= 1e-15
        assert DR.grad_bar(V, st) > 1e-4                     # the bar of the gradient test does not vanish with it


def test_zero_embedding_gives_the_sum_of_squared_class_weights():
    V, S = _case(300, 7, 3)
    L, g, st = DR.utterance(0 * V, S)
    assert L == float((st['c'] ** 2).sum()) and 1.0 / 3 <= L <= 1.0 and not g.any()
    assert abs(st['c'].sum() - 1.0) <= 1e-15 and abs(st['w'].sum() - 1.0) <= 1e-13


def test_silent_utterance_gives_zero_and_a_zero_gradient():
    V, S = _case(130, 6, 2)
    L, g, st = DR.utterance(V, 0 * S)
    assert L == 0.0 and not g.any() and not st['A'].any() and not st['c'].any() and st['S'] == 0.0
    assert not (DR.labels(0 * S)).any()                      # an all-zero bin gets label 0
    r = DR.batch(np.stack([V, V]), np.stack([S, 0 * S]))
    assert r['per_utt'][1] == 0.0 and np.isfinite(r['dembed']).all() and not r['dembed'][1].any()


def test_a_tie_goes_to_the_lowest_index():
    S = np.array([[1.0, 2.0, 0.0, 3.0], [1.0, 2.0, 0.0, 3.0], [1.0, 1.0, 0.0, 3.0]], np.float32)
    assert DR.labels(S).tolist() == [0, 0, 0, 0]
    S = np.array([[0.5, 2.0], [1.0, 2.0], [1.0, 1.0]], np.float32)
    assert DR.labels(S).tolist() == [1, 0]


def test_invariant_to_a_common_scale_of_the_magnitudes_and_to_the_order_of_rows():
    V, S = _case(516, 20, 3)
    L, g, _ = DR.utterance(V, S)
    L2, g2, _ = DR.utterance(V, S * np.float32(4.0))          # (a power of two: the float32 values scale exactly)
    assert abs(L2 - L) <= 1e-14 * abs(L) and np.abs(g2 - g).max() <= 1e-14 * np.abs(g).max()
    perm = np.random.RandomState(5).permutation(516)
    L3, g3, _ = DR.utterance(V[perm], S[:, perm])
    assert abs(L3 - L) <= 1e-13 * abs(L) and np.abs(g3 - g[perm]).max() <= 1e-13 * np.abs(g).max()


def test_float32_order_of_the_stats_pass_is_far_inside_the_bar():
    V, S = _case(4097, 20, 2)
    st = DR.stats(V.astype(np.float32), S)
    A, Bm, c, _ = DR.stats_f32(V, S)
    for got, want in ((A, st['A']), (Bm, st['Bm']), (c, st['c'])):
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()
