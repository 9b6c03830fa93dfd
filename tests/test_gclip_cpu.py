'''
CPU tests (no GPU) of global-norm gradient clipping (GRAD_CLIP_NORM): the extension library libdanet_gclip_hip.so
against its header (exports, prototypes, ABI, lazy load, host-visible argument errors), the untouched other eleven
libraries, the open EXTENSIONS registry, the configuration key, the optimizer's unchanged default branch, and the
restatement tests/gclip_ref.py against known answers and torch.nn.utils.clip_grad_norm_.
'''
import ctypes
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gclip_ref as GR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_gclip_hip.h')
GCLIP_SYMBOLS = ['danet_gclip_abi_version', 'danet_gclip_adam_step', 'danet_gclip_last_error', 'danet_gclip_partials',
                 'danet_gclip_sumsq']
KEY = 'GRAD_CLIP_NORM'


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_gclip_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_gclip()
    syms = _header_symbols('danet_gclip_hip.h', 'danet_gclip_')
    assert syms == GCLIP_SYMBOLS
    assert sorted(_lib.GCLIP_PROTOTYPES) == syms
    assert _exports(_lib.GCLIP_LIB_PATH) == syms
    assert lib.danet_gclip_abi_version() == 1 == _lib.GCLIP_ABI_VERSION == _lib.GCLIP.abi
    txt = open(HEADER).read()
    assert '#define DANET_GCLIP_ABI_VERSION 1' in txt
    assert '#define DANET_GCLIP_MAX_PARTIALS %d' % GR.MAX_PARTIALS in txt
    assert '#define DANET_GCLIP_MIN_SLICE %d' % GR.MIN_SLICE in txt
    rule = txt.split('#ifndef')[0]
    for words in ('slice(n)    = max(4096, 4 * ceil(ceil(n / 1024) / 4))', 'partials(n) = ceil(n / slice(n))',
                  'terms(n)    = ceil(slice(n) / 1024) + 2', '(x0^2 + x1^2) + (x2^2 + x3^2)', '(w0 + w1) + (w2 + w3)',
                  'norm = |s| * sqrt(S)', 'coef = M / (norm + 1e-6) if norm + 1e-6 > M, else 1',
                  'k = (float)((double)s * coef)', 'AFTER the scaling', 'no skip logic', 'terms(n) + 22'):
        assert words in rule, words
    assert _lib.GCLIP.prototypes is _lib.GCLIP_PROTOTYPES and _lib.GCLIP.prefix == 'danet_gclip_'


def test_gclip_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
             'double': ctypes.c_double, 'const float*': ctypes.c_void_p, 'const double*': ctypes.c_void_p,
             'double*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.GCLIP_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert len(_lib.GCLIP_PROTOTYPES['danet_gclip_sumsq'][1]) == 5
    assert len(_lib.GCLIP_PROTOTYPES['danet_gclip_adam_step'][1]) == 17


def test_gclip_is_appended_to_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.GCLIP in _lib.EXTENSIONS and build.GCLIP in build.EXTENSIONS
    assert isinstance(_lib.GCLIP, _lib.Library) and isinstance(build.GCLIP, build.Library)
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert _lib.GCLIP not in older and build.GCLIP not in build.LIBRARIES + build.LATER_LIBRARIES
    assert [lib.name for lib in _lib.EXTENSIONS] == [os.path.basename(spec.src_dir) for spec in build.EXTENSIONS]
    assert _lib.EXTENSIONS.index(_lib.GCLIP) > _lib.EXTENSIONS.index(_lib.WAVLOSS)       # appended
    assert build.EXTENSIONS.index(build.GCLIP) > build.EXTENSIONS.index(build.WAVLOSS)
    assert build.GCLIP_LIB == build.GCLIP.out == _lib.GCLIP_LIB_PATH
    assert os.path.basename(build.GCLIP_LIB) == _lib.GCLIP.so == 'libdanet_gclip_hip.so'
    assert os.path.isfile(os.path.join(build.GCLIP.src_dir, 'exports.map'))
    assert callable(build.build_gclip) and callable(_lib.load_gclip) and callable(_lib.gclip_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:4] == [build.METRIC, build.NOISE, build.LEVEL, build.WAVLOSS] and build.GCLIP in rest
    assert not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 12     # the eleven older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_eleven_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + (_lib.METRIC, _lib.NOISE, _lib.LEVEL, _lib.WAVLOSS)
    assert [spec.name for spec in older] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed', 'reverb', 'metric',
                                             'noise', 'level', 'wavloss']
    assert [spec.abi for spec in older] == [7, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    assert len(_lib.LIBRARIES) == 5 and len(_lib.ALL_LIBRARIES) == 6 and len(_lib.LATER_LIBRARIES) == 1
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_gclip_') for s in exported), spec.so
    # the core's optimizer entry point keeps its prototype: the factor still comes from the host by value
    f32 = ctypes.c_float
    assert _lib.PROTOTYPES['danet_adam_clip_step'] == (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, f32, f32,
        f32, f32, f32, f32, ctypes.c_int])
    assert sorted(_lib.WAVLOSS_PROTOTYPES) == ['danet_wavloss_abi_version', 'danet_wavloss_bwd', 'danet_wavloss_fwd',
                                               'danet_wavloss_last_error']


def test_gclip_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.GCLIP_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree'):
        assert not re.search(r'\b%s\b' % word, out.stdout), word
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'gclip')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['gclip.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'gclip.hip')).read(), flags=re.S)
    code += csrc_scan.shared_code(code)              # and the shared headers it includes, same words: the
    assert '} while (0)' in code and '#include "ext_core.h"' in code       # allowance is for their macros
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic', '__threadfence', 'while'):
        assert word not in code.replace('} while (0)', ''), word
    # adam_one is the core's: one definition, in the header both pointwise.hip and gclip.hip include
    csrc = os.path.dirname(d)
    one = re.compile(r'__device__ __forceinline__ void adam_one\(.*?\n}\n', flags=re.S)
    texts = {f: open(os.path.join(csrc, f)).read() for f in ('adam_one.h', 'pointwise.hip', 'gclip/gclip.hip')}
    assert [len(one.findall(texts[f])) for f in texts] == [1, 0, 0]
    for f in ('pointwise.hip', 'gclip/gclip.hip'):
        assert '#include "adam_one.h"' in texts[f] and texts[f].count('adam_one(') == 2, f


def test_import_and_a_model_with_the_key_null_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, ozers, datasets, feed, cli\n"
        "print('UNMAPPED:', _lib._gclip is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('OFF:', model.Model('m', device='cpu').grad_clip_norm, model.Model._check_grad_clip_norm())\n"
        "_lib.GCLIP_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_gclip()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_gclip_hip.so' in str(e) and %r in str(e)\n"
        "          and 'GRAD_CLIP_NORM' in str(e))\n"
        "print('NONE:', _lib._gclip is None and 'libdanet_gclip' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'OFF: None None', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


def test_partials_is_the_headers_pure_function():
    from danet_amd import _lib
    lib = _lib.load_gclip()
    for n in (1, 2, 4095, 4096, 4097, 8192, 8193, 1000003, 4194303, 4194304, 4194305, 4194308, 6904920, 35615000,
              1 << 31, (1 << 31) + 5, 1 << 40):
        p = lib.danet_gclip_partials(n)
        assert p == GR.partials_of(n) and 1 <= p <= 1024, n
        assert GR.slice_of(n) % 4 == 0 and GR.slice_of(n) >= 4096 and (p - 1) * GR.slice_of(n) < n <= p * GR.slice_of(n)
    assert GR.partials_of(4194304) == 1024 and GR.slice_of(4194305) == 4100 and GR.partials_of(6904920) == 1024
    assert GR.serial_terms(1) == 6 and GR.serial_terms(6904920) == 9 and GR.serial_terms(35615000) == 36
    for n in (0, -1, (1 << 40) + 1):
        assert lib.danet_gclip_partials(n) == 0 and b'n must be' in lib.danet_gclip_last_error()


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_gclip()
    n = 10000
    P = GR.partials_of(n)
    ok = dict(stream=None, n=n, grad=1024, partials=2048, n_partials=P)
    cases = [(dict(n=0), b'n must'), (dict(n=-3), b'n must'), (dict(n=(1 << 40) + 1), b'n must'),
             (dict(grad=None), b'null'), (dict(partials=None), b'null'), (dict(grad=1026), b'misaligned'),
             (dict(partials=2052), b'misaligned'), (dict(n_partials=P + 1), b'n_partials'),
             (dict(n_partials=0), b'n_partials'), (dict(n_partials=1024), b'n_partials')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_gclip_sumsq(*a.values()) == -1, kw
        assert msg in lib.danet_gclip_last_error(), (kw, lib.danet_gclip_last_error())
    ok = dict(stream=None, n=n, theta=1024, grad=2048, m=4096, v=8192, lr_t=1e-3, b1=0.9, b2=0.999, eps=1e-8,
              clip=100.0, grad_scale=1.0, zero_grad=1, max_norm=5.0, partials=16384, n_partials=P, norm_out=32768)
    cases = [(dict(n=0), b'n must'), (dict(n=-1), b'n must'), (dict(n_partials=P - 1), b'n_partials'),
             (dict(n_partials=P + 1), b'n_partials'), (dict(max_norm=0.0), b'max_norm'),
             (dict(max_norm=-1.0), b'max_norm'), (dict(max_norm=float('inf')), b'max_norm'),
             (dict(max_norm=float('nan')), b'max_norm')]
    cases += [({k: None}, b'null') for k in ('theta', 'grad', 'm', 'v', 'partials', 'norm_out')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('theta', 'grad', 'm', 'v')]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in ('partials', 'norm_out')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_gclip_adam_step(*a.values()) == -1, kw
        assert msg in lib.danet_gclip_last_error(), (kw, lib.danet_gclip_last_error())
    assert _lib.gclip_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.gclip_check(-1)
    assert str(e.value).startswith('libdanet_gclip_hip error -1: adam_step: misaligned')


# ----------------------------------------------------------------------------------- the key
def test_the_key_defaults_to_null_and_means_off(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    assert KEY in H.DEFAULTS and H.DEFAULTS[KEY] is None and getattr(hp, KEY) is None
    assert re.fullmatch(hp.pattern, KEY) and KEY in H.__doc__
    hp.digest()
    assert Model._check_grad_clip_norm() is None and Model('m', device='cpu').grad_clip_norm is None
    for v, want in ((5, 5.0), (0.25, 0.25), (1e30, 1e30)):
        hp.load({KEY: v})
        got = Model._check_grad_clip_norm()
        assert got == want and isinstance(got, float)


@pytest.mark.parametrize('value', [True, False, 'x', '5', '', 0, 0.0, -1, -0.5, float('inf'), float('-inf'),
                                   float('nan')])
def test_build_raises_and_names_the_key(hp, value):
    from danet_amd.model import Model
    hp.load({KEY: value})
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('gclip', device='cuda:0').build()              # raised before anything touches a device
    assert re.search(r'\b%s\b' % KEY, str(e.value))


def test_build_raises_with_the_early_optimizer_piece(hp, monkeypatch):
    from danet_amd import _lib
    from danet_amd.model import Model
    monkeypatch.setattr(_lib, '_expert', {'early_adam': '1'})
    hp.load({KEY: 5.0})
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('gclip', device='cuda:0').build()
    assert KEY in str(e.value) and 'early_adam' in str(e.value)
    hp.load({KEY: None})
    assert Model._check_grad_clip_norm() is None             # without the key the expert setting is not looked at


def test_no_command_line_flag_is_added():
    from danet_amd import cli
    src = open(cli.__file__).read().lower()
    assert 'grad_clip_norm' not in src and 'gclip' not in src and 'clip_coef' not in src


# ----------------------------------------------------------------------------------- the optimizer's default branch
class _StubOps(object):
    def __init__(self):
        self.calls = []

    def adam_clip_step(self, *args, **kw):
        self.calls.append(('adam_clip_step', args, kw))

    def grad_sumsq(self, *args, **kw):
        self.calls.append(('grad_sumsq', args, kw))
        return 'partials'

    def adam_gclip_step(self, *args, **kw):
        self.calls.append(('adam_gclip_step', args, kw))


def test_adam_step_without_the_new_arguments_is_todays_call(monkeypatch):
    from danet_amd import ozers
    stub = _StubOps()
    monkeypatch.setattr(ozers, 'ops', stub)
    o = ozers.TfAdam(3e-4)
    o.bind(torch.zeros(10), torch.ones(10))
    o.step(3, 3e-4, clip=100.0, grad_scale=0.5, zero_grad=True)
    o.step(3, 3e-4, clip=None, ranges=[(0, 4), (6, 10)])
    lr_t = 3e-4 * math.sqrt(1. - 0.999 ** 3) / (1. - 0.9 ** 3)
    assert [c[0] for c in stub.calls] == ['adam_clip_step'] * 3
    name, args, kw = stub.calls[0]
    assert not kw and len(args) == 11 and args[4:] == (lr_t, 0.9, 0.999, 1e-8, 100.0, 0.5, True)
    assert [a.data_ptr() for a in args[:4]] == [t.data_ptr() for t in (o.theta, o.grad, o.m, o.v)]
    assert all(a.numel() == 10 for a in args[:4])
    assert stub.calls[1][1][4:] == (lr_t, 0.9, 0.999, 1e-8, 0.0, 1.0, False)
    assert [stub.calls[i][1][0].numel() for i in (1, 2)] == [4, 4]
    assert stub.calls[2][1][0].data_ptr() == o.theta.data_ptr() + 24
    # with the key: one sum of squares over the whole gradient, one fused step, never in pieces
    del stub.calls[:]
    o.step(3, 3e-4, clip=100.0, grad_scale=0.5, zero_grad=True, max_norm=2.0, norm_out='out')
    assert [c[0] for c in stub.calls] == ['grad_sumsq', 'adam_gclip_step']
    assert stub.calls[1][1][4:] == (lr_t, 0.9, 0.999, 1e-8, 100.0, 0.5, True, 2.0, 'partials', 'out')
    del stub.calls[:]
    o.step(3, 3e-4, max_norm=2.0, partials='mine', norm_out='out')
    assert [c[0] for c in stub.calls] == ['adam_gclip_step'] and stub.calls[0][1][-2:] == ('mine', 'out')
    with pytest.raises(AssertionError):
        o.step(3, 3e-4, max_norm=2.0, norm_out='out', ranges=[(0, 4)])


# ----------------------------------------------------------------------------------- the restatement
def test_known_answers():
    g = np.array([3.0, 4.0], np.float32)
    r = GR.clip(g, 1.0, 1.0)
    assert r['norm'] == 5.0 and r['coef'] == 1.0 / (5.0 + 1e-6) and r['k'] == np.float32(1.0 / (5.0 + 1e-6))
    r = GR.clip(g, 1.0, 10.0)
    assert r['norm'] == 5.0 and r['coef'] == 1.0 and r['k'] == np.float32(1.0)
    r = GR.clip(g, 0.5, 1.0)                                  # the data-parallel scale is part of the norm
    assert r['norm'] == 2.5 and r['coef'] == 1.0 / (2.5 + 1e-6) and r['k'] == np.float32(0.5 / (2.5 + 1e-6))
    r = GR.clip(g, -0.5, 1.0)
    assert r['norm'] == 2.5 and r['k'] == np.float32(-0.5 / (2.5 + 1e-6))
    r = GR.clip(np.array([3.0, np.nan, 4.0], np.float32), 1.0, 1.0)       # a NaN norm compares false
    assert np.isnan(r['norm']) and r['coef'] == 1.0 and r['k'] == np.float32(1.0)
    r = GR.clip(np.array([3.0, np.inf], np.float32), 1.0, 1.0)           # an infinite norm gives 0
    assert np.isinf(r['norm']) and r['coef'] == 0.0 and r['k'] == np.float32(0.0)
    r = GR.clip(np.array([3e38, 3e38], np.float32), 1.0, 1.0)            # float64 squares do not overflow
    assert np.isfinite(r['norm']) and 0.0 < r['coef'] < 1e-38
    r = GR.clip(np.zeros(7, np.float32), 1.0, 1.0)
    assert r['norm'] == 0.0 and r['coef'] == 1.0
    # the value clip comes after the scaling, and keeps a NaN
    gp = GR.scaled_value_clip(np.array([400.0, -8.0, np.nan], np.float32), np.float32(0.5), 100.0)
    assert gp[0] == 100.0 and gp[1] == -4.0 and np.isnan(gp[2])
    assert np.array_equal(GR.scaled_value_clip([400.0, -8.0], np.float32(0.5), 0), [200.0, -4.0])


@pytest.mark.parametrize('n,residue', [(1, 0), (3, 1), (5, 3), (257, 2), (1025, 0), (4097, 1), (9001, 3), (70001, 2)])
def test_the_fixed_tree_meets_the_headers_bound(n, residue):
    rng = np.random.RandomState(n)
    g = (10.0 ** rng.uniform(-6, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p = GR.sumsq_partials(g, residue)
    assert p.shape == (GR.partials_of(n),) and p.dtype == np.float64
    want = math.fsum((g.astype(np.float64) ** 2).tolist())
    assert abs(math.fsum(p.tolist()) - want) <= GR.sum_bar(n) * want
    assert abs(GR.total(p) - want) <= GR.sum_bar(n) * want
    assert np.array_equal(GR.sumsq_partials(g, residue), p)


@pytest.mark.parametrize('M', [0.25, 3.0, 1e30])
@pytest.mark.parametrize('n', [2, 1000, 9001])
def test_restatement_against_torch_clip_grad_norm(n, M):
    rng = np.random.RandomState(n)
    g = rng.standard_normal(n).astype(np.float32)
    r = GR.clip(g, 1.0, M)
    p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
    p.grad = torch.tensor(g.astype(np.float64))
    total = float(torch.nn.utils.clip_grad_norm_([p], M))
    assert abs(r['norm'] - total) <= 1e-15 * total
    got = p.grad.numpy()
    want = g.astype(np.float64) * r['coef']
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
    assert (r['coef'] < 1.0) == (total + 1e-6 > M)
    if M == 1e30:
        assert r['coef'] == 1.0 and np.array_equal(got, g.astype(np.float64))
