'''
CPU tests (no GPU) of chunked inference (INFER_CHUNK_LEN): the extension library libdanet_stitch_hip.so against its
header (exports, prototypes, ABI, lazy load, host-visible argument errors), the untouched other fourteen libraries,
the open MORE_EXTENSIONS registry, the three configuration keys, the plan over an exhaustive grid, and known answers
of the restatement tests/stitch_ref.py.
'''
import ctypes
import hashlib
import importlib
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stitch_ref as SR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_stitch_hip.h')
STITCH_SYMBOLS = ['danet_stitch_abi_version', 'danet_stitch_affinity', 'danet_stitch_assign', 'danet_stitch_chunks',
                  'danet_stitch_last_error', 'danet_stitch_merge', 'danet_stitch_workspace_bytes']
KEYS = ('INFER_CHUNK_LEN', 'INFER_CHUNK_OVERLAP', 'INFER_CHUNK_BATCH')
NO_WS = ctypes.c_size_t(-1).value
# the export lists of the fourteen older libraries: sha1 of their sorted, space-joined names (first 12 digits)
OLDER = {'': (51, '35c97f3a2452'), 'conv': (7, '9446af6b053c'), 'dropout': (3, '31a0846a9f05'),
         'prep': (6, '4528d8ffdc78'), 'mix': (5, 'a519a2795d7a'), 'speed': (4, 'e1adf1c490af'),
         'reverb': (3, '05ef787913e5'), 'metric': (6, 'eff9d5e3632c'), 'noise': (3, 'cf88e352bf83'),
         'level': (4, '7fdea6b0fb6a'), 'wavloss': (4, 'e9c25e57750d'), 'gclip': (5, 'a9921dcbc5d9'),
         'dpcl': (7, '8021ee69c5d3'), 'neval': (6, '44b1be58a6d8')}


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_stitch_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_stitch()
    syms = _header_symbols('danet_stitch_hip.h', 'danet_stitch_')
    assert syms == STITCH_SYMBOLS
    assert sorted(_lib.STITCH_PROTOTYPES) == syms
    assert _exports(_lib.STITCH_LIB_PATH) == syms
    assert lib.danet_stitch_abi_version() == 1 == _lib.STITCH_ABI_VERSION == _lib.STITCH.abi
    txt = open(HEADER).read()
    assert '#define DANET_STITCH_ABI_VERSION 1' in txt
    assert '#define DANET_STITCH_MAX_C %d' % SR.MAX_C in txt and ops.STITCH_MAX_C == SR.MAX_C
    assert '#define DANET_STITCH_MAX_CHUNKS %d' % SR.MAX_CHUNKS in txt
    assert '#define DANET_STITCH_TILE %d' % SR.TILE in txt
    rule = txt.split('#ifndef')[0]
    for words in ('n   = 1 + ceil((T - L) / H)', 's_{n-1} = T - L', 'NOT zero-padded', 'F_i = [e_i - V, e_i)',
                  'at most two contributing chunks', 'S_i[c][c\'] = sum over t in O_i and f',
                  'itertools.permutations order', 'an all-zero overlap gives the\n * identity',
                  'P_{i+1}[c] = pi_i[P_i[c]]', 'the owner is the smallest i with t < e_i',
                  'mag = fma(w_k, fl(b - a), a)', 'w_k = (k + 1) / (V + 1)', 'is pointwise in (t, f)'):
        assert words in rule, words
    assert _lib.STITCH.prototypes is _lib.STITCH_PROTOTYPES and _lib.STITCH.prefix == 'danet_stitch_'


def test_stitch_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    ctype = {'void*': p, 'const void*': p, 'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'const float*': p,
             'double*': p, 'float*': p, 'int32_t*': p, 'const int32_t*': p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.STITCH_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.STITCH_PROTOTYPES['danet_stitch_' + n][1]) for n in ('affinity', 'assign', 'merge')] == [9, 10, 11]


def test_stitch_is_in_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.STITCH in _lib.MORE_EXTENSIONS and build.STITCH in build.MORE_EXTENSIONS
    assert isinstance(_lib.STITCH, _lib.Library) and isinstance(build.STITCH, build.Library)
    closed = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert _lib.STITCH not in closed and len(closed) == 14
    assert build.STITCH not in build.LIBRARIES + build.LATER_LIBRARIES + build.EXTENSIONS
    assert [lib.name for lib in _lib.MORE_EXTENSIONS] == [os.path.basename(spec.src_dir)
                                                          for spec in build.MORE_EXTENSIONS]
    assert build.STITCH_LIB == build.STITCH.out == _lib.STITCH_LIB_PATH
    assert os.path.basename(build.STITCH_LIB) == _lib.STITCH.so == 'libdanet_stitch_hip.so'
    assert os.path.isfile(os.path.join(build.STITCH.src_dir, 'exports.map'))
    assert build.STITCH.headers == (HEADER, os.path.join(csrc_scan.CSRC, 'ext_core.h'))
    assert callable(build.build_stitch) and callable(_lib.load_stitch) and callable(_lib.stitch_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:7] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL]
    assert build.STITCH in rest and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 15     # the fourteen older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_fourteen_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert [spec.name for spec in older] == list(OLDER)
    assert [spec.abi for spec in older] == [7] + [1] * 13
    assert len(_lib.LIBRARIES) == 5 and len(_lib.ALL_LIBRARIES) == 6 and len(_lib.LATER_LIBRARIES) == 1
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_stitch_') for s in exported), spec.so
        assert (len(exported), hashlib.sha1(' '.join(exported).encode()).hexdigest()[:12]) == OLDER[spec.name], spec.so


def test_stitch_library_reads_no_environment_allocates_nothing_and_has_no_transcendental_math():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.STITCH_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipStreamSynchronize', 'hipDeviceSynchronize'):
        assert not re.search(r'\b%s\w*\b' % word, out.stdout), word
    d = os.path.join(csrc_scan.CSRC, 'stitch')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['stitch.hip']
    code = csrc_scan.strip_comments(open(os.path.join(d, 'stitch.hip')).read())
    code += csrc_scan.shared_code(code)              # and the shared header it includes
    assert csrc_scan.shared_headers(code) == [os.path.join(csrc_scan.CSRC, 'ext_core.h')]
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', 'common.h', 'math.h',
                 'Synchronize', 'hipMemcpy'):
        assert word not in code, word
    for fn in ('exp', 'log', 'log1p', 'sin', 'cos', 'tan', 'atan2', 'sincos', 'sqrt', 'rsqrt', 'pow', 'hypot', 'tanh'):
        assert not re.search(r'\b_*%sf?\s*\(' % fn, code), fn
    assert '__fmaf_rn(' in code                        # the one rounding of the cross-fade is spelled out


def test_import_and_a_model_with_the_key_null_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, ozers, datasets, feed, cli\n"
        "real, _lib.load_stitch = _lib.load_stitch, None          # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._stitch is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model('m', device='cpu').infer_chunk, model.Model._check_infer_chunk())\n"
        "_lib.load_stitch = real\n"
        "_lib.STITCH_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_stitch()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_stitch_hip.so' in str(e) and %r in str(e)\n"
        "          and 'INFER_CHUNK_LEN' in str(e))\n"
        "print('NONE:', _lib._stitch is None and 'libdanet_stitch' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: None None', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu():
    '''every host-visible argument error is returned before any launch: no device is needed to see them'''
    from danet_amd import _lib
    lib = _lib.load_stitch()
    T, L, V, C, F = 40, 8, 3, 2, 33
    need = SR.workspace_bytes(T, L, V, C, F)
    assert lib.danet_stitch_workspace_bytes(T, L, V, C, F) == need > 0
    plans = [(dict(T=0), b'need T >= 1'), (dict(L=1), b'need T >= 1'), (dict(V=0), b'need T >= 1'),
             (dict(V=5), b'need T >= 1'), (dict(T=8), b'need T > L'), (dict(T=5), b'need T > L'),
             (dict(C=0), b'need 1 <= C'), (dict(C=5), b'need 1 <= C'), (dict(F=0), b'need 1 <= C'),
             (dict(T=65538, L=2, V=1), b'need at most 65536 chunks'), (dict(L=1 << 30, V=1, F=2, T=(1 << 30) + 1),
                                                                          b'need L * F < 2^31'),
             (dict(T=1 << 30, F=1 << 10, L=1 << 20, V=1), b'need L * F < 2^31')]
    for kw, msg in plans:
        a = dict(dict(T=T, L=L, V=V, C=C, F=F), **kw)
        assert lib.danet_stitch_workspace_bytes(*a.values()) == NO_WS, kw
        assert b'workspace_bytes: ' + msg in lib.danet_stitch_last_error(), (kw, lib.danet_stitch_last_error())
    assert lib.danet_stitch_workspace_bytes(65537, 2, 1, 1, 1) == 65535 * 8      # n = 65536 is inside
    ok = dict(stream=None, T=T, L=L, V=V, C=C, F=F, mags=4096, ws=16384, ws_bytes=need)
    cases = plans + [({k: None}, b'null') for k in ('mags', 'ws')]
    cases += [(dict(mags=4098), b'misaligned'), (dict(ws=16388), b'misaligned')]
    cases += [(dict(ws_bytes=need - 1), b'workspace too small'), (dict(ws_bytes=0), b'workspace too small')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_stitch_affinity(*a.values()) == -1, kw
        assert b'affinity: ' + msg in lib.danet_stitch_last_error(), (kw, lib.danet_stitch_last_error())
    ok = dict(stream=None, T=T, L=L, V=V, C=C, F=F, ws=16384, ws_bytes=need, S_out=4096, perm_out=8192)
    cases = plans + [({k: None}, b'null') for k in ('ws', 'S_out', 'perm_out')]
    cases += [(dict(ws=16388), b'misaligned'), (dict(S_out=4100), b'misaligned'), (dict(perm_out=8194), b'misaligned')]
    cases += [(dict(ws_bytes=need - 1), b'workspace too small')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_stitch_assign(*a.values()) == -1, kw
        assert b'assign: ' + msg in lib.danet_stitch_last_error(), (kw, lib.danet_stitch_last_error())
    ok = dict(stream=None, T=T, L=L, V=V, C=C, F=F, mags=4096, phasor=8192, fade=1024, perm=2048, out=16384)
    cases = plans + [({k: None}, b'null') for k in ('mags', 'phasor', 'fade', 'perm', 'out')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('mags', 'fade', 'perm')]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in ('phasor', 'out')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_stitch_merge(*a.values()) == -1, kw
        assert b'merge: ' + msg in lib.danet_stitch_last_error(), (kw, lib.danet_stitch_last_error())
    for bad in ((0, 8, 3), (40, 1, 1), (40, 8, 0), (40, 8, 5), (-3, 8, 3)):
        assert lib.danet_stitch_chunks(*bad) < 0 and b'chunks: need T >= 1' in lib.danet_stitch_last_error(), bad
    assert _lib.stitch_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.stitch_check(-1)
    assert str(e.value).startswith('libdanet_stitch_hip error -1: chunks: need T >= 1')


# ----------------------------------------------------------------------------------- the keys
def test_the_keys_default_to_null_and_mean_off(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    for key in KEYS:
        assert key in H.DEFAULTS and H.DEFAULTS[key] is None and getattr(hp, key) is None
        assert re.fullmatch(hp.pattern, key) and key in H.__doc__
    hp.digest()
    assert Model._check_infer_chunk() is None and Model('m', device='cpu').infer_chunk is None
    for di, want in ((dict(INFER_CHUNK_LEN=128), (128, 32, 16)), (dict(INFER_CHUNK_LEN=4), (4, 1, 16)),
                     (dict(INFER_CHUNK_LEN=8, INFER_CHUNK_OVERLAP=4, INFER_CHUNK_BATCH=1), (8, 4, 1)),
                     (dict(INFER_CHUNK_LEN=512, INFER_CHUNK_OVERLAP=128, INFER_CHUNK_BATCH=24), (512, 128, 24)),
                     (dict(INFER_CHUNK_LEN=2, LENGTH_ALIGN=1), (2, 1, 16))):
        hp.reset()
        hp.load(di)
        assert Model._check_infer_chunk() == want


@pytest.mark.parametrize('key,di', [
    ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN=True)), ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN=128.0)),
    ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN='128')), ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN=0)),
    ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN=1, LENGTH_ALIGN=1)), ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN=-4)),
    ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN=130)), ('INFER_CHUNK_LEN', dict(INFER_CHUNK_LEN=6)),
    ('INFER_CHUNK_OVERLAP', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_OVERLAP=False)),
    ('INFER_CHUNK_OVERLAP', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_OVERLAP=1.5)),
    ('INFER_CHUNK_OVERLAP', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_OVERLAP=0)),
    ('INFER_CHUNK_OVERLAP', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_OVERLAP=65)),
    ('INFER_CHUNK_OVERLAP', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_OVERLAP='32')),
    ('INFER_CHUNK_BATCH', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_BATCH=True)),
    ('INFER_CHUNK_BATCH', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_BATCH=0)),
    ('INFER_CHUNK_BATCH', dict(INFER_CHUNK_LEN=128, INFER_CHUNK_BATCH=2.0)),
    ('INFER_CHUNK_OVERLAP', dict(INFER_CHUNK_OVERLAP=32)), ('INFER_CHUNK_BATCH', dict(INFER_CHUNK_BATCH=16)),
    ('MAX_N_SIGNAL', dict(INFER_CHUNK_LEN=128, MAX_N_SIGNAL=5))])
def test_build_raises_and_names_the_key(hp, key, di):
    from danet_amd.model import Model
    hp.load(di)
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('stitch', device='cuda:0').build()             # raised before anything touches a device
    assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)
    if 'INFER_CHUNK_LEN' not in di or key == 'MAX_N_SIGNAL':
        assert 'INFER_CHUNK_LEN' in str(e.value)             # the key that is set alone names the one it needs


def test_without_the_key_the_envelope_is_not_looked_at_and_no_flag_is_added(hp):
    from danet_amd.model import Model
    from danet_amd import cli
    hp.load(dict(MAX_N_SIGNAL=5))
    assert Model._check_infer_chunk() is None
    src = open(cli.__file__).read().lower()
    assert 'chunk' not in src and 'stitch' not in src
    opts = [a.dest for a in cli.build_parser()._actions]
    assert len(opts) == 15 and not any('chunk' in o for o in opts)


# ----------------------------------------------------------------------------------- the plan
def test_plan_over_the_exhaustive_grid():
    from danet_amd import _lib, ops
    lib = _lib.load_stitch()
    cases = 0
    for L in (2, 4, 8, 12):
        for V in range(1, L // 2 + 1):
            H = L - V
            assert lib.danet_stitch_chunks(L, L, V) == 1 == lib.danet_stitch_chunks(1, L, V) == SR.chunks(L, L, V)
            assert ops.stitch_plan(L, L, V) == [0]
            for T in range(L + 1, 5 * L + 1):
                starts = SR.plan(T, L, V)
                n = len(starts)
                assert lib.danet_stitch_chunks(T, L, V) == n == SR.chunks(T, L, V) == ops.stitch_chunks(T, L, V) >= 2
                assert ops.stitch_plan(T, L, V) == starts
                assert n == 1 + -(-(T - L) // H)
                assert starts[0] == 0 and starts[-1] + L == T and all(b > a for a, b in zip(starts, starts[1:]))
                assert 1 <= starts[-1] - starts[-2] <= H and all(b - a == H for a, b in zip(starts[:-2], starts[1:-1]))
                fades = [set(range(s + L - V, s + L)) for s in starts[:-1]]
                assert all(not (a & b) for a, b in itertools.combinations(fades, 2))           # disjoint
                owners = np.zeros(T, int)
                for t in range(T):
                    i = SR.owner(t, starts, L)
                    owners[t] += 1
                    assert i == min(j for j in range(n) if t < starts[j] + L)
                    assert 0 <= t - starts[i] < L                                              # the owner's row
                    if i < n - 1 and t >= starts[i] + L - V:
                        assert t in fades[i] and 0 <= t - starts[i + 1] < L                    # the partner's row
                        assert 0 <= t - (starts[i] + L - V) < V
                    else:
                        assert not any(t in f for f in fades)
                assert (owners == 1).all()
                for i in range(n - 1):
                    ov = starts[i] + L - starts[i + 1]
                    assert V <= ov <= L - 1 and (ov == V or i == n - 2)
                    assert starts[i + 1] <= starts[i] + L - V              # the partner covers the whole fade
                assert lib.danet_stitch_workspace_bytes(T, L, V, 3, 5) == SR.workspace_bytes(T, L, V, 3, 5) \
                    == (n - 1) * 9 * 8
                cases += 1
    assert cases == sum((L // 2) * 4 * L for L in (2, 4, 8, 12))
    assert SR.chunks(7500, 512, 128) == 20 and SR.plan(7500, 512, 128)[-2:] == [6912, 6988]
    assert SR.workspace_bytes(7500, 512, 128, 2, 129) == 19 * 9 * 4 * 8


# ----------------------------------------------------------------------------------- the restatement
def _speakers(C, T, F, seed):
    '''C magnitude tracks with distinct spectral envelopes and distinct frame patterns, float32 [C, T, F]'''
    rng = np.random.RandomState(seed)
    f = np.arange(F)[None, None, :]
    t = np.arange(T)[None, :, None]
    c = np.arange(C)[:, None, None]
    env = 1.0 + 4.0 * (f % C == c) + 2.0 * ((t + c) % (C + 1) == 0)
    return (env * rng.uniform(0.5, 1.5, (C, T, F))).astype(np.float32)


def test_one_channel_is_a_cross_fade_of_itself():
    T, L, V, F = 23, 8, 3, 5
    truth = _speakers(1, T, F, 0)
    mags = SR.cut(truth, T, L, V)
    ph = np.ones((len(mags), L, F, 2), np.float32)
    r = SR.stitch(mags, ph, T, V)
    assert r['perm'].tolist() == [[0]] * len(mags) and SR.margin(r['S'][0]) == float('inf')
    assert (r['mag'] == truth).all() and r['faded'].sum() == V * (len(mags) - 1)


def test_an_all_zero_overlap_gives_the_identity_and_a_tie_goes_to_the_first_permutation():
    T, L, V, C, F = 20, 8, 2, 3, 4
    mags = SR.cut(_speakers(C, T, F, 1), T, L, V)
    starts = SR.plan(T, L, V)
    mags[1, :, :starts[0] + L - starts[1]] = 0.0             # chunk 1's side of pair 0's overlap
    S = SR.affinity(mags, T, V)
    assert not S[0].any() and SR.local_perm(S[0]) == [0, 1, 2] and SR.margin(S[0]) == 0.0
    assert SR.chain(S)[1].tolist() == [0, 1, 2]
    tie = np.array([[1.0, 1.0], [1.0, 1.0]])
    assert SR.local_perm(tie) == [0, 1]
    tie3 = np.array([[0.0, 2.0, 2.0], [2.0, 0.0, 2.0], [2.0, 2.0, 0.0]])       # (1, 2, 0) and (2, 0, 1) tie at 6
    assert SR.local_perm(tie3) == [1, 2, 0]


@pytest.mark.parametrize('C,T,L,V,F', [(2, 23, 8, 3, 5), (3, 41, 8, 4, 3), (4, 30, 4, 1, 7), (4, 9, 4, 2, 1),
                                       (2, 300, 128, 32, 9)])
def test_swapped_channels_are_undone(C, T, L, V, F):
    truth = _speakers(C, T, F, 10 * C + F)
    chunks = SR.cut(truth, T, L, V).transpose(0, 1, 2, 3)            # [n, C, L, F]
    rng = np.random.RandomState(T)
    swaps = [list(range(C))] + [list(rng.permutation(C)) for _ in range(len(chunks) - 1)]
    mags = np.stack([ch[sw] for ch, sw in zip(chunks, swaps)])       # chunk i's channel k is speaker swaps[i][k]
    ph = np.stack([np.cos(chunks[:, 0]), np.sin(chunks[:, 0])], axis=-1).astype(np.float32)
    r = SR.stitch(mags, ph, T, V)
    assert min(SR.margin(S) for S in r['S']) > 1e-9
    for i, sw in enumerate(swaps):
        assert [sw[k] for k in r['perm'][i]] == list(range(C)), i    # output channel c is speaker c in every chunk
    assert (r['a'] == truth).all() and (r['b'] == truth).all() and (r['mag'] == truth).all()
    want = truth[..., None].astype(np.float64) * SR.owner_phasor(ph, T, V)[None].astype(np.float64)
    assert (r['out'].real == want[..., 0]).all() and (r['out'].imag == want[..., 1]).all()
    exact, absum = SR.affinity_exact(mags, T, V)
    assert (np.abs(r['S'] - exact) <= 1e-12 * absum).all()
