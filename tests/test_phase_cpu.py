'''
CPU tests (no GPU) of the MISI phase refinement (PHASE_REFINE_ITERS): the extension library libdanet_phase_hip.so
against its header (exports, prototypes, ABI, lazy load, the workspace layout, every host-visible argument error), the
untouched other seventeen libraries, the open MORE_EXTENSIONS registry, the configuration key and every ValueError,
and the float64 restatement of tests/phase_ref.py against the metric's restatement and against known answers.
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
import metric_ref as MR
import phase_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_phase_hip.h')
PHASE_SYMBOLS = ['danet_phase_abi_version', 'danet_phase_init', 'danet_phase_last_error', 'danet_phase_project',
                 'danet_phase_synth', 'danet_phase_workspace_bytes']
NO_WS = ctypes.c_size_t(-1).value
# the export lists of the seventeen older libraries: sha1 of their sorted, space-joined names (first 12 digits)
OLDER = {'': (51, '35c97f3a2452'), 'conv': (7, '9446af6b053c'), 'dropout': (3, '31a0846a9f05'),
         'prep': (6, '4528d8ffdc78'), 'mix': (5, 'a519a2795d7a'), 'speed': (4, 'e1adf1c490af'),
         'reverb': (3, '05ef787913e5'), 'metric': (6, 'eff9d5e3632c'), 'noise': (3, 'cf88e352bf83'),
         'level': (4, '7fdea6b0fb6a'), 'wavloss': (4, 'e9c25e57750d'), 'gclip': (5, 'a9921dcbc5d9'),
         'dpcl': (7, '8021ee69c5d3'), 'neval': (6, '44b1be58a6d8'), 'stitch': (7, '2ab75117a25c'),
         'bss': (7, '265172254200'), 'stoi': (8, '476adf4d55ec')}


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_phase_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_phase()
    syms = _header_symbols('danet_phase_hip.h', 'danet_phase_')
    assert syms == PHASE_SYMBOLS
    assert sorted(_lib.PHASE_PROTOTYPES) == syms
    assert _exports(_lib.PHASE_LIB_PATH) == syms
    assert lib.danet_phase_abi_version() == 1 == _lib.PHASE_ABI_VERSION == _lib.PHASE.abi
    txt = open(HEADER).read()
    assert '#define DANET_PHASE_ABI_VERSION 1' in txt and re.search(r'#define DANET_PHASE_MAX_C %d\b' % PR.MAX_C, txt)
    assert ops.PHASE_MAX_C == PR.MAX_C == MR.MAX_C
    rule = txt.split('#ifndef')[0]
    for words in ('THE RULE', 'mixrows[.][0] + mixrows[.][1] + ...', 'rounded ONCE to float32', 'X^0 = est0',
                  "danet_metric_synth's rule", 'y = synth(mix)', 'x_c = synth(X^k_c)',
                  'z_c[n] = x_c[n] + (y[n] - (x_0[n] + x_1[n] + ...)) / C', 'UNSCALED windowed real FFT',
                  '[tS - N/2, tS + N/2)', 'No 1 / sum(w) is applied', 'm2 = re^2 + im^2',
                  'X^{k+1} = A * (Z / sqrtf(m2))', 'both parts are +0 there where A = 0', 'X^{k+1} = X^k at that bin',
                  'K = 0 returns est0 bit for bit', 'the noise is therefore shared among the refined sources',
                  'B * (C + 1) * Ls below 2^31', 'each rounded up to a multiple of 256 bytes', 'no atomics',
                  'no persistent grid'):
        assert words in rule, words
    assert _lib.PHASE.prototypes is _lib.PHASE_PROTOTYPES and _lib.PHASE.prefix == 'danet_phase_'
    # the tile of the projection: the formula of the header
    m = re.search(r'#define DANET_PHASE_TILE_FRAMES\(N\) \\\n\s*(.*)\n', txt)
    frames = lambda N: eval(m.group(1).replace('/', '//').replace('?', 'and').replace(':', 'or'), {'N': N})
    assert [frames(N) for N in (64, 128, 256, 512, 1024)] == [32, 32, 32, 20, 9]
    for N in (64, 128, 256, 512, 1024):                      # twiddles + frames + span at S = N/2: within 64 KiB
        assert N + frames(N) * N + (frames(N) - 1) * (N // 2) + N <= 16384


def test_phase_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    p = ctypes.c_void_p
    ctype = {'void*': p, 'int': ctypes.c_int, 'const float*': p, 'float*': p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p, 'size_t': ctypes.c_size_t}
    for name, (res, args) in _lib.PHASE_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert [len(_lib.PHASE_PROTOTYPES['danet_phase_' + n][1])
            for n in ('workspace_bytes', 'init', 'synth', 'project')] == [5, 12, 9, 10]


def test_phase_is_in_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.PHASE in _lib.MORE_EXTENSIONS and build.PHASE in build.MORE_EXTENSIONS
    assert isinstance(_lib.PHASE, _lib.Library) and isinstance(build.PHASE, build.Library)
    closed = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS
    assert _lib.PHASE not in closed and len(closed) == 14
    assert build.PHASE not in build.LIBRARIES + build.LATER_LIBRARIES + build.EXTENSIONS
    # it follows the records that were there
    assert _lib.MORE_EXTENSIONS.index(_lib.PHASE) > _lib.MORE_EXTENSIONS.index(_lib.STOI) == 2
    assert build.MORE_EXTENSIONS.index(build.PHASE) > build.MORE_EXTENSIONS.index(build.STOI) == 2
    assert [lib.name for lib in _lib.MORE_EXTENSIONS] == [os.path.basename(spec.src_dir)
                                                          for spec in build.MORE_EXTENSIONS]
    assert build.PHASE_LIB == build.PHASE.out == _lib.PHASE_LIB_PATH
    assert os.path.basename(build.PHASE_LIB) == _lib.PHASE.so == 'libdanet_phase_hip.so'
    assert os.path.isfile(os.path.join(build.PHASE.src_dir, 'exports.map'))
    assert build.PHASE.headers == (HEADER, os.path.join(csrc_scan.CSRC, 'ext_core.h'),
                                   os.path.join(csrc_scan.CSRC, 'wave_metric.h'))
    src = open(os.path.join(build.PHASE.src_dir, 'phase.hip')).read()
    assert set(csrc_scan.shared_headers(src)) == set(build.PHASE.headers[1:])
    assert callable(build.build_phase) and callable(_lib.load_phase) and callable(_lib.phase_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:10] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS, build.GCLIP, build.DPCL, build.NEVAL,
                         build.STITCH, build.BSS, build.STOI]
    assert build.PHASE in rest[10:] and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 18      # the seventeen older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_seventeen_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + _lib.EXTENSIONS + _lib.MORE_EXTENSIONS[:3]
    assert [spec.name for spec in older] == list(OLDER)
    assert [spec.abi for spec in older] == [7] + [1] * 16
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_phase_') for s in exported), spec.so
        assert (len(exported), hashlib.sha1(' '.join(exported).encode()).hexdigest()[:12]) == OLDER[spec.name], spec.so


def test_phase_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.PHASE_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset', 'hipStreamSynchronize', 'hipDeviceSynchronize'):
        assert not re.search(r'\b%s\w*\b' % word, out.stdout), word
    d = os.path.join(csrc_scan.CSRC, 'phase')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['phase.hip']
    own = csrc_scan.strip_comments(open(os.path.join(d, 'phase.hip')).read())
    code = own + csrc_scan.shared_code(own)           # and the shared headers it includes
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', 'common.h', 'Synchronize',
                 'hipMemcpy', 'hipMemset', 'asm', '__builtin_amdgcn', 'cooperative', 'volatile'):
        assert word not in code, word
    # the preamble of every extension source, and the shared cores used rather than restated
    assert own.count('#include "danet_phase_hip.h"\n#define DANET_EXT phase\n#define DANET_EXT_UPPER PHASE\n'
                     '#include "ext_core.h"\n') == 1
    assert own.count('synth_tile(') == 1 and own.count('radix2_stages(') == 1 and 'CHECK_LAUNCH();' in own
    assert not re.search(r'\b(synth_tile|radix2_stages|tiling_of|round256)\s*\([^;{}()]*\)\s*\{', own)
    # three kernels; every launch comes after every argument check of its entry point
    assert len(re.findall(r'__global__', own)) == 3
    for body in re.split(r'extern "C"', own)[1:]:
        launches = [m.start() for m in re.finditer(r'<<<|launch_synth\(', body)]
        checks = [m.start() for m in re.finditer(r'CHECK_ARG\(|envelope_ok\(', body)]
        assert not launches or max(checks) < min(launches)


def test_import_and_a_model_with_the_key_null_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, ozers, datasets, feed, cli\n"
        "from danet_amd.hparams import hparams\n"
        "real, _lib.load_phase = _lib.load_phase, None          # any call would raise TypeError\n"
        "print('UNMAPPED:', _lib._phase is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model._check_phase_refine())\n"
        "m = model.Model('x', device='cpu'); print('STATE:', m.phase_refine, m._refined('est', 'mix'))\n"
        "hparams.load(dict(PHASE_REFINE_ITERS=5)); print('ON:', model.Model._check_phase_refine())\n"
        "_lib.load_phase = real\n"
        "_lib.PHASE_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_phase()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_phase_hip.so' in str(e) and %r in str(e)\n"
        "          and 'PHASE_REFINE_ITERS' in str(e))\n"
        "print('NONE:', _lib._phase is None and 'libdanet_phase' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: None', 'STATE: None est', 'ON: 5', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------- workspace and argument errors
def _layout(B, C, T, N, S):
    F, Ls = N // 2 + 1, (T - 1) * S
    return [(n + 255) & ~255 for n in (B * C * T * F * 4, B * T * F * 8, B * (C + 1) * Ls * 4)]


ENVELOPE = [(dict(B=0), b'need B >= 1'), (dict(B=-3), b'need B >= 1'), (dict(C=0), b'need B >= 1'),
            (dict(C=5), b'need B >= 1'), (dict(T=1), b'need B >= 1'), (dict(N=32), b'need B >= 1'),
            (dict(N=2048), b'need B >= 1'), (dict(N=96), b'need B >= 1'), (dict(S=40), b'need B >= 1'),
            (dict(S=4), b'need B >= 1'), (dict(S=0), b'need B >= 1'), (dict(B=1 << 20, T=4096), b'must be < 2^31'),
            (dict(B=1 << 14, C=1, T=1 << 14, N=64, S=32), b'must be < 2^31')]


def test_workspace_bytes_and_its_layout():
    from danet_amd import _lib, ops
    lib = _lib.load_phase()
    for shape in ((1, 1, 2, 64, 8), (3, 2, 9, 64, 16), (2, 4, 40, 256, 64), (32, 2, 128, 256, 64), (1, 2, 1251, 512, 128),
                  (5, 3, 7, 1024, 512), (1, 4, 2, 1024, 128)):
        assert lib.danet_phase_workspace_bytes(*shape) == sum(_layout(*shape)) == ops.phase_workspace_bytes(*shape)
    # the parts, cut from a host buffer: three views in the header's order, each starting on a multiple of 256 bytes
    import torch
    B, C, T, N, S = 3, 2, 9, 64, 16
    buf = torch.zeros(sum(_layout(B, C, T, N, S)), dtype=torch.uint8)
    A, mix, wav = ops.phase_parts(buf, B, C, T, N, S)
    assert (A.dtype, mix.dtype, wav.dtype) == (torch.float32, torch.complex64, torch.float32)
    assert (tuple(A.shape), tuple(mix.shape), tuple(wav.shape)) == ((B, C, T, 33), (B, T, 33), (B, C + 1, 8 * S))
    offs = [t.data_ptr() - buf.data_ptr() for t in (A, mix, wav)]
    assert offs == [0, _layout(B, C, T, N, S)[0], sum(_layout(B, C, T, N, S)[:2])] and all(o % 256 == 0 for o in offs)
    ok = dict(B=2, C=2, T=9, N=64, S=16)
    for kw, msg in ENVELOPE:
        assert lib.danet_phase_workspace_bytes(*dict(ok, **kw).values()) == NO_WS, kw
        assert b'workspace_bytes: ' in lib.danet_phase_last_error() and msg in lib.danet_phase_last_error(), kw
    with pytest.raises(_lib.DanetHipError) as e:
        ops.phase_workspace_bytes(1, 5, 9, 64, 16)
    assert str(e.value).startswith('libdanet_phase_hip error -1: workspace_bytes: need B >= 1')


def test_argument_errors_without_gpu():
    '''every host-visible argument error is returned before any launch: no device is needed to see them'''
    from danet_amd import _lib
    lib = _lib.load_phase()
    ok = dict(stream=None, B=2, C=2, Cm=1, T=9, N=64, S=16, est0=4096, mixrows=8192, window=16384, ws=32768, x=65536)
    cases = list(ENVELOPE) + [(dict(Cm=0), b'need B >= 1'), (dict(Cm=5), b'need B >= 1'),
                              (dict(B=1 << 14, C=1, Cm=4, T=1 << 10, N=64, S=8), b'must be < 2^31')]
    cases += [({k: None}, b'null') for k in ('est0', 'mixrows', 'window', 'ws', 'x')]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in ('est0', 'mixrows', 'ws', 'x')] + [(dict(window=16386), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_phase_init(*a.values()) == -1, kw
        assert b'init: ' in lib.danet_phase_last_error() and msg in lib.danet_phase_last_error(), (kw, lib.danet_phase_last_error())
    ok = dict(stream=None, B=2, C=2, T=9, N=64, S=16, x=65536, window=16384, ws=32768)
    cases = list(ENVELOPE) + [({k: None}, b'null') for k in ('x', 'window', 'ws')]
    cases += [(dict(x=65540), b'misaligned'), (dict(ws=32772), b'misaligned'), (dict(window=16385), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_phase_synth(*a.values()) == -1, kw
        assert b'synth: ' in lib.danet_phase_last_error() and msg in lib.danet_phase_last_error(), (kw, lib.danet_phase_last_error())
    ok = dict(stream=None, B=2, C=2, T=9, N=64, S=16, window=16384, ws=32768, x=65536, z_out=131072)
    cases = list(ENVELOPE) + [({k: None}, b'null') for k in ('x', 'window', 'ws')]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in ('x', 'ws', 'z_out')] + [(dict(window=16386), b'misaligned')]
    cases += [(dict(z_out=65536), b'z_out must not be x')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_phase_project(*a.values()) == -1, kw
        assert b'project: ' in lib.danet_phase_last_error() and msg in lib.danet_phase_last_error(), (kw, lib.danet_phase_last_error())
    assert _lib.phase_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.phase_check(-1)
    assert str(e.value).startswith('libdanet_phase_hip error -1: project: z_out must not be x')


# ----------------------------------------------------------------------------------- the key
def test_the_key_defaults_to_null_and_means_off(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    assert 'PHASE_REFINE_ITERS' in H.DEFAULTS and H.DEFAULTS['PHASE_REFINE_ITERS'] is None and hp.PHASE_REFINE_ITERS is None
    assert re.fullmatch(hp.pattern, 'PHASE_REFINE_ITERS') and 'PHASE_REFINE_ITERS' in H.__doc__
    hp.digest()
    assert Model._check_phase_refine() is None
    for di, want in ((dict(PHASE_REFINE_ITERS=1), 1), (dict(PHASE_REFINE_ITERS=100), 100),
                     (dict(PHASE_REFINE_ITERS=5, EVAL_SI_SDR=True, EVAL_BSS_SDR=True, EVAL_STOI=True), 5),
                     (dict(PHASE_REFINE_ITERS=3, MAX_N_SIGNAL=4, FFT_SIZE=64, FFT_STRIDE=8), 3),
                     (dict(PHASE_REFINE_ITERS=3, FFT_SIZE=1024, FFT_STRIDE=512), 3),
                     (dict(MAX_N_SIGNAL=5, FFT_SIZE=48, NOISE_EVAL_DIR='/nowhere'), None)):   # off: nothing is looked at
        hp.reset()
        hp.load(di)
        assert Model._check_phase_refine() == want and type(Model._check_phase_refine()) is type(want), di


@pytest.mark.parametrize('keys,di', [
    (('PHASE_REFINE_ITERS',), dict(PHASE_REFINE_ITERS=True)), (('PHASE_REFINE_ITERS',), dict(PHASE_REFINE_ITERS=False)),
    (('PHASE_REFINE_ITERS',), dict(PHASE_REFINE_ITERS=2.0)), (('PHASE_REFINE_ITERS',), dict(PHASE_REFINE_ITERS='3')),
    (('PHASE_REFINE_ITERS',), dict(PHASE_REFINE_ITERS=0)), (('PHASE_REFINE_ITERS',), dict(PHASE_REFINE_ITERS=-1)),
    (('PHASE_REFINE_ITERS',), dict(PHASE_REFINE_ITERS=101)),
    (('PHASE_REFINE_ITERS', 'MAX_N_SIGNAL'), dict(PHASE_REFINE_ITERS=2, MAX_N_SIGNAL=5)),
    (('PHASE_REFINE_ITERS', 'FFT_SIZE'), dict(PHASE_REFINE_ITERS=2, FFT_SIZE=48, FFT_STRIDE=12)),
    (('PHASE_REFINE_ITERS', 'FFT_SIZE'), dict(PHASE_REFINE_ITERS=2, FFT_SIZE=2048, FFT_STRIDE=512)),
    (('PHASE_REFINE_ITERS', 'FFT_STRIDE'), dict(PHASE_REFINE_ITERS=2, FFT_SIZE=256, FFT_STRIDE=192)),
    (('PHASE_REFINE_ITERS', 'FFT_STRIDE'), dict(PHASE_REFINE_ITERS=2, FFT_SIZE=256, FFT_STRIDE=16)),
    (('PHASE_REFINE_ITERS', 'NOISE_EVAL_DIR'), dict(PHASE_REFINE_ITERS=2, NOISE_EVAL_DIR='/nowhere')),
    (('PHASE_REFINE_ITERS', 'NOISE_EVAL_DIR'), dict(PHASE_REFINE_ITERS=2, EVAL_SI_SDR=True, NOISE_EVAL_DIR='/nowhere'))])
def test_build_raises_and_names_the_key(hp, keys, di):
    from danet_amd.model import Model
    hp.load(di)
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('phase', device='cuda:0').build()              # raised before anything touches a device
    for key in keys:
        assert re.search(r'\b%s\b' % key, str(e.value)), str(e.value)
    assert not re.search(r'EVAL_SI_SDR|EVAL_BSS_SDR|EVAL_STOI', str(e.value))


def test_no_flag_is_added_and_the_train_step_never_looks(hp):
    import inspect
    from danet_amd import cli
    from danet_amd.model import Model
    assert 'phase' not in open(cli.__file__).read().lower()
    opts = [a.dest for a in cli.build_parser()._actions]
    assert len(opts) == 15 and not any('phase' in o for o in opts)
    for fn in (Model.train_step, Model.debug_fetch, Model.forward, Model.forward_noisy, Model.infer_chunks):
        assert 'phase_refine' not in inspect.getsource(fn) and '_refined' not in inspect.getsource(fn), fn.__name__
    for fn in (Model.infer, Model.infer_long, Model.valid_step):
        assert '_refined(' in inspect.getsource(fn), fn.__name__
    assert 'self.phase_refine is None' in inspect.getsource(Model._refined)


# ----------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('N,S,T', [(64, 16, 9), (64, 8, 12), (256, 64, 40), (128, 64, 3), (1024, 256, 6)])
def test_the_analysis_is_the_metrics_stft_unscaled(N, S, T):
    w = PR.window('sqrt_hann', N)
    Ls = (T - 1) * S
    x = np.random.RandomState(N + T).standard_normal((2, Ls))
    Z = PR.analyse(x, w, S, T)
    assert Z.shape == (2, T, N // 2 + 1) and Z.dtype == np.complex128
    if Ls >= N:                                              # scipy refuses a signal shorter than its window
        want = np.stack([MR.stft(v, w, N, S, np.complex128) for v in x]) * w.astype(np.float64).sum()
        assert np.abs(Z - want).max() <= 1e-12 * np.abs(want).max()
    # a consistent spectrum maps to itself: analyse(synth(stft(x))) = stft(x)
    back = PR.analyse(MR.synth(Z, w, S), w, S, T)
    assert np.abs(back - Z).max() <= 1e-12 * np.abs(Z).max()
    # frame t, literally
    t = T // 2
    frame = np.array([x[0, n] if 0 <= n < Ls else 0.0 for n in range(t * S - N // 2, t * S + N // 2)]) * w
    assert np.abs(Z[0, t] - np.fft.rfft(frame)).max() <= 1e-12 * np.abs(Z).max()
    assert not Z[..., 0].imag.any() and not Z[..., -1].imag.any()
    Z32 = PR.analyse(x, w, S, T, np.float32)
    assert Z32.dtype == np.complex64 and 0 < np.abs(Z32 - Z).max() <= 1e-5 * np.abs(Z).max()


@pytest.mark.parametrize('N,S,T,C,wname', PR.DESCENT_CASES)
def test_the_objective_falls_in_each_of_twelve_iterations(N, S, T, C, wname):
    est0, src, w = PR.oracle_case(1, C, T, N, S, wname, seed=3)
    A, mix, y, X = PR.start(est0, src, w, S)
    assert np.abs(A - np.abs(est0.astype(np.complex128))).max() <= 1e-15 * A.max() and X.dtype == np.complex128
    J = []
    for k in range(13):                                      # J_0 .. J_12: twelve steps down
        X, Z, new = PR.step(X, A, y, w, S)
        J.append(PR.objective(A, Z))
        assert new.all() and np.abs(np.abs(X) - A).max() <= 1e-12 * A.max()
    drops = -np.diff(J) / J[0]
    print('J_k / J_0: %s' % np.round(np.asarray(J) / J[0], 5).tolist())
    assert len(drops) == 12 and (drops > 1e-4).all(), drops
    assert abs(PR.objective_of(est0, A, y, w, S) - J[0]) <= 1e-12 * J[0]
    # after the redistribution the sources sum to the mixture's waveform
    z = PR.redistribute(MR.synth(X, w, S), y)
    assert np.abs(z.sum(1) - y).max() <= 1e-12 * np.abs(y).max()


def test_one_source_is_a_fixed_point_after_one_iteration():
    N, S, T = 64, 16, 9
    est0, src, w = PR.oracle_case(2, 1, T, N, S, seed=4)
    rng = np.random.RandomState(5)
    est0 = (np.abs(est0) * np.exp(2j * np.pi * rng.random_sample(est0.shape))).astype(np.complex64)   # any phase
    X1 = PR.refine(est0, src, w, S, 1)
    X2 = PR.refine(est0, src, w, S, 2)
    assert np.abs(X1 - est0).max() > 1e-3 * np.abs(est0).max()
    assert np.abs(X2 - X1).max() <= 1e-12 * np.abs(X1).max()
    # C = 1: z = y whatever x is, so X^1 is the mixture's own spectrum (the magnitudes are its own)
    assert np.abs(X1 - PR.mixture(src)[:, None]).max() <= 1e-6 * np.abs(X1).max()


def test_the_zero_bin_rule_and_the_float32_run():
    A = np.array([[2.0, 0.0, 3.0, 0.0, 1.0, 1.0]])
    Z = np.array([[3 + 4j, 1 - 1j, 0j, 0j, np.inf + 0j, -2.0 + 0j]])
    old = np.array([[1j, 5 + 0j, -0.0 + 3j, 7 - 7j, 0.6 + 0.8j, 1 + 0j]])
    with np.errstate(all='ignore'):
        X, new = PR.project(Z, A, old)
    assert new.tolist() == [[True, True, False, False, False, True]]
    assert np.allclose(X[0, 0], 1.2 + 1.6j, rtol=1e-15) and X[0, 5] == -1.0
    assert X[0, 1] == 0 and not np.signbit(X[0, 1].real) and not np.signbit(X[0, 1].imag)       # A = 0: +0, +0
    for i in (2, 3, 4):                                      # the old value, bit for bit (the sign of -0 too)
        assert X[0, i] == old[0, i] and np.signbit(X[0, i].real) == np.signbit(old[0, i].real)
    # K = 0 is the input; the float32 run stays close to the float64 one for one step
    est0, src, w = PR.oracle_case(1, 2, 9, 64, 16, seed=6)
    assert np.array_equal(PR.refine(est0, src, w, 16, 0), est0.astype(np.complex128))
    X64, X32 = PR.refine(est0, src, w, 16, 1), PR.refine(est0, src, w, 16, 1, np.float32)
    assert X32.dtype == np.complex64 and 0 < np.abs(X32 - X64).max() <= 1e-4 * np.abs(X64).max()
    assert PR.mixture(src, np.float32).dtype == np.complex64 and PR.magnitudes(est0, np.float32).dtype == np.float32


def test_si_sdr_rises_by_more_than_6_db_with_oracle_magnitudes():
    N, S, T, B, C = 256, 64, 40, 2, 2
    est0, src, w = PR.oracle_case(B, C, T, N, S, seed=0)
    got = [MR.si_sdr(src, PR.refine(est0, src, w, S, K), w, S)[2][0] for K in (0, 1, 8)]
    print('SI-SDR with oracle magnitudes and the mixture phase, K = 0, 1, 8: %s dB' % np.round(got, 2).tolist())
    assert got[0] < got[1] < got[2] and got[2] - got[0] > 6.0
    ref = MR.synth(src, w, S)
    plain = [PR.si_sdr_db(ref, MR.synth(PR.refine(est0, src, w, S, K), w, S)) for K in (0, 8)]
    assert abs(plain[0] - got[0]) <= 1e-9 and abs(plain[1] - got[2]) <= 1e-9      # the identity permutation wins
