'''
CPU tests (no GPU) of the waveform training loss (TRAIN_LOSS = "si-sdr"): the extension library
libdanet_wavloss_hip.so against its header (exports, prototypes, ABI, lazy load, host-visible argument errors), the
untouched other ten libraries, the open EXTENSIONS registry, the configuration key, and the restatement
tests/wavloss_ref.py against torch float64 autograd through its own synthesis, the adjoint identity and known
answers.
'''
import ctypes
import importlib
import itertools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import metric_ref as MR
import wavloss_ref as WR
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'danet_wavloss_hip.h')
WAVLOSS_SYMBOLS = ['danet_wavloss_abi_version', 'danet_wavloss_bwd', 'danet_wavloss_fwd', 'danet_wavloss_last_error']
KEY = 'TRAIN_LOSS'


def _sqrt_hann(N):
    import scipy.signal
    return np.sqrt(scipy.signal.windows.hann(N)).astype(np.float32)


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True)
    return sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())


# ------------------------------------------------------------------------------------------ ABI
def test_wavloss_library_exports_exactly_its_header():
    from danet_amd import _lib, ops
    lib = _lib.load_wavloss()
    syms = _header_symbols('danet_wavloss_hip.h', 'danet_wavloss_')
    assert syms == WAVLOSS_SYMBOLS
    assert sorted(_lib.WAVLOSS_PROTOTYPES) == syms
    assert _exports(_lib.WAVLOSS_LIB_PATH) == syms
    assert lib.danet_wavloss_abi_version() == 1 == _lib.WAVLOSS_ABI_VERSION == _lib.WAVLOSS.abi
    txt = open(HEADER).read()
    assert '#define DANET_WAVLOSS_ABI_VERSION 1' in txt
    assert '#define DANET_WAVLOSS_MAX_C %d' % ops.WAVLOSS_MAX_C in txt and ops.WAVLOSS_MAX_C == ops.METRIC_MAX_C
    rule = txt.split('#ifndef')[0]
    for words in ('pair[b][j] = i when p(i) = j', '(alpha, beta) = -(1 / (n_live_b * n_utt_live))', 'K = 10 / ln 10',
                  'rounded ONCE to float32', 'f_t[k] = w[k] * u[tS - N/2 + k]', 'dX_t[f] = dloss * (c_f / N) * rfft_N(f_t)[f]',
                  'exactly 0', 'dL/dRe + i dL/dIm', 'cos(phi) Re(dX) + sin(phi) Im(dX)'):
        assert words in rule, words
    assert _lib.WAVLOSS.prototypes is _lib.WAVLOSS_PROTOTYPES and _lib.WAVLOSS.prefix == 'danet_wavloss_'
    # the tile length is a function of N alone, the same in the header's macro, ops and the restatement
    assert '#define DANET_WAVLOSS_TILE_FRAMES(N)' in txt and 'min(32, (16384 - 3N/2) / (3N/2))' in txt
    for N, want in ((64, 32), (128, 32), (256, 32), (512, 20), (1024, 9)):
        assert ops.wavloss_tile_frames(N) == WR.tile_frames(N) == want, N
        assert 3 * N // 2 * (1 + want) <= 16384                           # twiddles + frames + the span at S = N/2


def test_wavloss_prototypes_match_the_header_text():
    from danet_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ctype = {'void*': ctypes.c_void_p, 'int': ctypes.c_int, 'const float*': ctypes.c_void_p,
             'const double*': ctypes.c_void_p, 'const int32_t*': ctypes.c_void_p, 'double*': ctypes.c_void_p,
             'float*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p, 'void': None}
    rtype = {'int': ctypes.c_int, 'const char*': ctypes.c_char_p}
    for name, (res, args) in _lib.WAVLOSS_PROTOTYPES.items():
        m = re.search(r'([a-z_0-9 ]+?\*?)\s*%s\((.*?)\);' % name, txt, flags=re.S)
        assert m, name
        assert rtype[m.group(1).strip()] == res, name
        want = [ctype[a.strip().rsplit(' ', 1)[0] if ' ' in a.strip() else a.strip()]
                for a in m.group(2).replace('\n', ' ').split(',')]
        assert args == [w for w in want if w is not None], (name, args, want)
    assert len(_lib.WAVLOSS_PROTOTYPES['danet_wavloss_fwd'][1]) == 10
    assert len(_lib.WAVLOSS_PROTOTYPES['danet_wavloss_bwd'][1]) == 13


def test_wavloss_is_appended_to_the_open_registry_and_build_all_builds_it():
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    assert _lib.WAVLOSS in _lib.EXTENSIONS and build.WAVLOSS in build.EXTENSIONS
    assert isinstance(_lib.WAVLOSS, _lib.Library) and isinstance(build.WAVLOSS, build.Library)
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES
    assert _lib.WAVLOSS not in older and build.WAVLOSS not in build.LIBRARIES + build.LATER_LIBRARIES
    assert [lib.name for lib in _lib.EXTENSIONS] == [os.path.basename(spec.src_dir) for spec in build.EXTENSIONS]
    assert _lib.EXTENSIONS.index(_lib.WAVLOSS) > _lib.EXTENSIONS.index(_lib.LEVEL)       # appended
    assert build.WAVLOSS_LIB == build.WAVLOSS.out == _lib.WAVLOSS_LIB_PATH
    assert os.path.basename(build.WAVLOSS_LIB) == _lib.WAVLOSS.so == 'libdanet_wavloss_hip.so'
    assert os.path.isfile(os.path.join(build.WAVLOSS.src_dir, 'exports.map'))
    assert callable(build.build_wavloss) and callable(_lib.load_wavloss) and callable(_lib.wavloss_check)
    seven, rest = [], []
    real_library, real_spec = build._build_library, build._build_spec
    try:
        build._build_library = lambda spec, force, verbose: seven.append(spec)
        build._build_spec = lambda spec, force, verbose: rest.append(spec)
        outs = build.build_all(verbose=False)
    finally:
        build._build_library, build._build_spec = real_library, real_spec
    assert seven == list(build.LIBRARIES + build.LATER_LIBRARIES) and len(seven) == 7
    assert rest[:3] == [build.METRIC, build.NOISE, build.LEVEL] and build.WAVLOSS in rest and not set(rest) & set(seven)
    assert set(spec.out for spec in seven + rest) == set(outs) and len(outs) >= 11      # the ten older and this one
    assert all(os.path.isfile(out) for out in outs)


def test_the_other_ten_libraries_are_untouched():
    from danet_amd import _lib
    older = _lib.ALL_LIBRARIES + _lib.LATER_LIBRARIES + (_lib.METRIC, _lib.NOISE, _lib.LEVEL)
    assert [spec.name for spec in older] == ['', 'conv', 'dropout', 'prep', 'mix', 'speed', 'reverb', 'metric',
                                             'noise', 'level']
    assert [spec.abi for spec in older] == [7, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    assert len(_lib.LIBRARIES) == 5 and len(_lib.ALL_LIBRARIES) == 6 and len(_lib.LATER_LIBRARIES) == 1
    for spec in older:
        exported = _exports(getattr(_lib, spec.path_var))
        assert exported == _header_symbols(spec.prefix + 'hip.h', spec.prefix) == sorted(spec.prototypes), spec.so
        assert not any(s.startswith('danet_wavloss_') for s in exported), spec.so
    assert sorted(_lib.METRIC_PROTOTYPES) == ['danet_metric_abi_version', 'danet_metric_gram', 'danet_metric_last_error',
                                              'danet_metric_si_sdr', 'danet_metric_synth',
                                              'danet_metric_workspace_bytes']
    assert sorted(_lib.LEVEL_PROTOTYPES) == ['danet_level_abi_version', 'danet_level_activity', 'danet_level_last_error',
                                             'danet_level_workspace_bytes']


def test_wavloss_library_reads_no_environment_and_allocates_nothing():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.WAVLOSS_LIB_PATH], capture_output=True, text=True, check=True)
    for word in ('getenv', 'hipMalloc', 'hipFree'):
        assert not re.search(r'\b%s\b' % word, out.stdout), word
    d = os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'wavloss')
    srcs = sorted(f for f in os.listdir(d) if f.endswith(('.hip', '.h', '.cpp')))
    assert srcs == ['wavloss.hip']
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(d, 'wavloss.hip')).read(), flags=re.S)
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic'):
        assert word not in code, word
    shared = csrc_scan.shared_code(code)               # wave_metric.h, ext_core.h
    assert '#include "wave_metric.h"' in code and '#include "ext_core.h"' in code
    for word in ('getenv', 'environ', 'hipMalloc', 'hipFree', 'malloc', 'new ', 'atomic'):
        assert word not in shared, word


def test_import_and_a_model_with_the_key_null_never_touch_the_library(tmp_path):
    nope = str(tmp_path / 'nope.so')
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model, datasets, feed, cli\n"
        "print('UNMAPPED:', _lib._wavloss is None and 'libdanet_' not in open('/proc/self/maps').read())\n"
        "print('MSE:', model.Model('m', device='cpu').train_loss, model.Model._check_train_loss())\n"
        "_lib.WAVLOSS_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_wavloss()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e) and 'libdanet_wavloss_hip.so' in str(e) and %r in str(e)\n"
        "          and 'TRAIN_LOSS' in str(e))\n"
        "print('NONE:', _lib._wavloss is None and 'libdanet_wavloss' not in open('/proc/self/maps').read())\n"
    ) % (ROOT, nope, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('UNMAPPED: True', 'MSE: pit-mse pit-mse', 'LOUD: True', 'NONE: True'):
        assert words in out.stdout, out.stdout + out.stderr


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_wavloss()
    ok = dict(stream=None, B=2, C=2, G=1024, loss64=2048, loss32=4096, per_utt=8192, perm_idx=16384, pair=32768,
              coef=65536)
    cases = [(dict(B=0), b'B must'), (dict(B=-1), b'B must'), (dict(C=0), b'C must'), (dict(C=5), b'C must'),
             (dict(B=1 << 27, C=4), b'2^31')]
    cases += [({k: None}, b'null') for k in list(ok)[3:]]
    cases += [({k: ok[k] + 4}, b'misaligned') for k in ('G', 'loss64', 'per_utt', 'coef')]
    cases += [({k: ok[k] + 2}, b'misaligned') for k in ('loss32', 'perm_idx', 'pair')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_wavloss_fwd(*a.values()) == -1, kw
        assert msg in lib.danet_wavloss_last_error(), (kw, lib.danet_wavloss_last_error())
    ok = dict(stream=None, B=2, C=2, T=9, N=256, S=64, wav=1024, pair=2048, coef=4096, window=8192, dloss=16384,
              phasor=32768, out=65536)
    cases = [(dict(B=0), b'B must'), (dict(C=0), b'C must'), (dict(C=5), b'C must'), (dict(T=1), b'T must be >= 2'),
             (dict(T=0), b'T must'), (dict(N=192), b'power of two'), (dict(N=32, S=8), b'power of two'),
             (dict(N=2048, S=512), b'power of two'), (dict(S=129), b'S must'), (dict(S=31), b'S must'),
             (dict(S=0), b'S must'), (dict(T=(1 << 31) - 1, N=1024, S=512), b'(T - 1) * S'),
             (dict(T=1 << 23, N=1024, S=128), b'T * F'),
             (dict(B=1 << 15, C=4, T=1 << 20, N=64, S=8), b'B * C * tiles'),
             (dict(wav=None), b'null'), (dict(pair=None), b'null'), (dict(coef=None), b'null'),
             (dict(window=None), b'null'), (dict(out=None), b'null'),
             (dict(wav=1026), b'misaligned'), (dict(pair=2050), b'misaligned'), (dict(coef=4100), b'misaligned'),
             (dict(window=8194), b'misaligned'), (dict(dloss=16386), b'misaligned'), (dict(phasor=32772), b'misaligned'),
             (dict(out=65538), b'misaligned'), (dict(phasor=None, out=65540), b'misaligned')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_wavloss_bwd(*a.values()) == -1, kw
        assert msg in lib.danet_wavloss_last_error(), (kw, lib.danet_wavloss_last_error())
    assert _lib.wavloss_check(0) is None
    with pytest.raises(_lib.DanetHipError) as e:
        _lib.wavloss_check(-1)
    assert str(e.value).startswith('libdanet_wavloss_hip error -1: bwd: misaligned')


# ----------------------------------------------------------------------------------- the key
def test_the_key_defaults_to_null_and_means_mse(hp):
    H = sys.modules['danet_amd.hparams']
    from danet_amd.model import Model
    assert KEY in H.DEFAULTS and H.DEFAULTS[KEY] is None and getattr(hp, KEY) is None
    assert re.fullmatch(hp.pattern, KEY) and KEY in H.__doc__
    hp.digest()
    assert Model._check_train_loss() == 'pit-mse' and Model('m', device='cpu').train_loss == 'pit-mse'
    hp.load({KEY: 'pit-mse'})
    assert Model._check_train_loss() == 'pit-mse'
    hp.load({KEY: 'si-sdr'})
    assert Model._check_train_loss() == 'si-sdr'


@pytest.mark.parametrize('keys,name', [({KEY: True}, KEY), ({KEY: False}, KEY), ({KEY: 1}, KEY), ({KEY: 0.5}, KEY),
                                       ({KEY: 'SI-SDR'}, KEY), ({KEY: 'mse'}, KEY), ({KEY: ''}, KEY),
                                       ({KEY: 'si-sdr', 'FFT_SIZE': 64, 'FFT_STRIDE': 48}, 'FFT_STRIDE'),
                                       ({KEY: 'si-sdr', 'FFT_SIZE': 256, 'FFT_STRIDE': 16}, 'FFT_STRIDE'),
                                       ({KEY: 'si-sdr', 'FFT_SIZE': 2048, 'FFT_STRIDE': 512}, 'FFT_SIZE'),
                                       ({KEY: 'si-sdr', 'FFT_SIZE': 96, 'FFT_STRIDE': 24}, 'FFT_SIZE'),
                                       ({KEY: 'si-sdr', 'MAX_N_SIGNAL': 5}, 'MAX_N_SIGNAL')])
def test_build_raises_and_names_the_offending_key(hp, keys, name):
    from danet_amd.model import Model
    hp.load(keys)
    hp.digest()
    with pytest.raises(ValueError) as e:
        Model('wavloss', device='cuda:0').build()            # raised before anything touches a device
    assert re.search(r'\b%s\b' % name, str(e.value)) and KEY in str(e.value)      # and TRAIN_LOSS as the reason
    if keys.get('FFT_STRIDE') == 48:
        assert 'window edges' in str(e.value) and 'LDS' not in str(e.value)
    if keys.get('FFT_STRIDE') == 16:
        assert 'LDS' in str(e.value) and 'window edges' not in str(e.value)
    if name != KEY:
        # with the key null or "pit-mse" none of them is looked at
        for v in (None, 'pit-mse'):
            hp.load({KEY: v})
            assert Model._check_train_loss() == 'pit-mse'


def test_no_command_line_flag_is_added():
    from danet_amd import cli
    src = open(cli.__file__).read().lower()
    assert 'train_loss' not in src and 'si-sdr' not in src and 'wavloss' not in src


# ----------------------------------------------------------------------------------- the restatement
def _spectra(rng, B, C, T, N, scale=3.0):
    F = N // 2 + 1
    return (rng.standard_normal((B, C, T, F)) + 1j * rng.standard_normal((B, C, T, F))) * scale


def _torch_synth(X, w, S):
    '''the synthesis rule in torch float64 (differentiable): X complex128 [..., T, F] -> [..., (T - 1) * S]'''
    T, F = X.shape[-2:]
    N = 2 * (F - 1)
    # numpy's irfft convention: the imaginary parts of bins 0 and N/2 are ignored
    mask = torch.ones(F, dtype=torch.float64)
    mask[0] = mask[-1] = 0.0
    X = torch.complex(X.real, X.imag * mask)
    f = torch.fft.irfft(X, n=N, dim=-1)
    Ls = (T - 1) * S
    acc = torch.zeros(X.shape[:-2] + (Ls + N,), dtype=torch.float64)
    wsum = torch.zeros(Ls + N, dtype=torch.float64)
    for t in range(T):
        acc[..., t * S:t * S + N] = acc[..., t * S:t * S + N] + w * f[..., t, :]
        wsum[t * S:t * S + N] = wsum[t * S:t * S + N] + w * w
    return acc[..., N // 2:N // 2 + Ls] / wsum[N // 2:N // 2 + Ls]


def _torch_loss(src, est, w, S, fwd):
    '''-SI-SDR in torch float64 under the pairing the restatement found (the search is piecewise constant)'''
    ws = _torch_synth(torch.cat([src, est], dim=1), w, S)
    B, C = src.shape[:2]
    total, n_utt = 0.0, 0
    for b in range(B):
        live = [(int(fwd['pair'][b, j]), j) for j in range(C) if fwd['pair'][b, j] >= 0]
        if not live:
            continue
        n_utt += 1
        u = 0.0
        for i, j in live:
            s, y = ws[b, i], ws[b, C + j]
            # SI-SDR by its definition, 10 log10(|k s|^2 / |y - k s|^2) with k = <s, y> / <s, s>: the same function
            # as the rule's t / (b - t), without the cancellation in b - t (a relative 10^(SDR/10) 2^-53 there)
            k = (s * y).sum() / (s * s).sum()
            res = y - k * s
            u = u + 10.0 * torch.log10((k * k * (s * s).sum()) / (res * res).sum())
        total = total + u / len(live)
    return -(total / n_utt)


@pytest.mark.parametrize('N,S,T', [(64, 16, 9), (64, 24, 7), (64, 32, 3), (256, 64, 6), (128, 32, 21)])
def test_analytic_gradient_matches_float64_autograd_through_the_synthesis(N, S, T):
    rng = np.random.RandomState(N + S + T)
    w = _sqrt_hann(N).astype(np.float64)
    B, C = 4, 2
    src = _spectra(rng, B, C, T, N)
    db = np.array([-5.0, 10.0, 30.0, 50.0])
    est = src[:, ::-1] + 10.0 ** (-db[:, None, None, None] / 20) * _spectra(rng, B, C, T, N)
    f, dX = WR.loss_and_grad(src, est, w, S)
    assert np.array_equal(f['perm_idx'], [1] * B) and f['per_utt'].min() < 0 and f['per_utt'].max() > 40
    e = torch.tensor(est, dtype=torch.complex128, requires_grad=True)
    L = _torch_loss(torch.tensor(src, dtype=torch.complex128), e, torch.tensor(w), S, f)
    L.backward()
    assert abs(float(L.detach()) - f['loss']) <= 1e-10 * max(1.0, abs(f['loss']))
    g = e.grad.numpy().copy()                                        # dL/dRe + i dL/dIm
    g[..., 0] = g[..., 0].real                                        # (the ignored imaginary parts have no gradient)
    g[..., -1] = g[..., -1].real
    err = np.abs(dX - g).max() / np.abs(g).max()
    print('N %d S %d T %d: analytic vs autograd %.3g of the maximum' % (N, S, T, err))
    assert err <= 1e-10
    assert not dX[..., 0].imag.any() and not dX[..., -1].imag.any()


@pytest.mark.parametrize('N,S,T', [(64, 16, 9), (64, 24, 5), (256, 128, 4), (1024, 256, 3)])
def test_adjoint_identity(N, S, T):
    '''<synth(X), g> = Re<X, adj(g)> with adj(g) = adjoint(g / wsum)'''
    rng = np.random.RandomState(N + T)
    w = _sqrt_hann(N).astype(np.float64)
    X = _spectra(rng, 2, 3, T, N)
    X[..., 0] = X[..., 0].real                                        # (the synthesis ignores these two)
    X[..., -1] = X[..., -1].real
    g = rng.standard_normal((2, 3, (T - 1) * S))
    wsum = WR.window_sum(w, S, T)
    lhs = float((MR.synth(X, w, S) * g).sum())
    A = WR.adjoint(g / wsum, w, S, T)
    rhs = float((X.real * A.real + X.imag * A.imag).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.linalg.norm(MR.synth(X, w, S)) * np.linalg.norm(g))


# ----------------------------------------------------------------------------------- known answers
def test_perfect_and_zero_estimates_are_clamped_and_have_no_gradient():
    rng = np.random.RandomState(1)
    N, S, T = 64, 16, 8
    w = _sqrt_hann(N).astype(np.float64)
    src = _spectra(rng, 3, 2, T, N)
    f, dX = WR.loss_and_grad(src, src, w, S)
    assert f['loss'] == -100.0 and np.array_equal(f['per_utt'], [100.0] * 3) and not f['perm_idx'].any()
    assert np.array_equal(f['pair'], [[0, 1]] * 3) and not f['coef'].any() and not dX.any()
    f, dX = WR.loss_and_grad(src, np.zeros_like(src), w, S)
    assert f['loss'] == 100.0 and np.array_equal(f['per_utt'], [-100.0] * 3)
    assert not f['coef'].any() and not dX.any()


def test_swapping_the_sources_flips_the_permutation_and_keeps_the_loss():
    rng = np.random.RandomState(2)
    N, S, T = 64, 16, 8
    w = _sqrt_hann(N).astype(np.float64)
    src = _spectra(rng, 3, 2, T, N)
    est = src + 0.3 * _spectra(rng, 3, 2, T, N)
    f0, d0 = WR.loss_and_grad(src, est, w, S)
    f1, d1 = WR.loss_and_grad(src, est[:, ::-1], w, S)
    assert np.array_equal(f0['perm_idx'], [0] * 3) and np.array_equal(f1['perm_idx'], [1] * 3)
    assert abs(f0['loss'] - f1['loss']) <= 1e-12 and np.array_equal(f1['pair'], [[1, 0]] * 3)
    assert np.abs(d1[:, ::-1] - d0).max() <= 1e-12 * np.abs(d0).max()


def test_a_silent_reference_is_left_out_and_its_partner_gets_no_pair():
    rng = np.random.RandomState(3)
    N, S, T = 64, 16, 8
    w = _sqrt_hann(N).astype(np.float64)
    src = _spectra(rng, 2, 2, T, N)
    src[0, 1] = 0
    src[1] = 0                                                        # an utterance without a live reference
    est = src[:, ::-1] + 0.2 * _spectra(rng, 2, 2, T, N)
    f, dX = WR.loss_and_grad(src, est, w, S)
    assert np.array_equal(f['pair'], [[-1, 0], [-1, -1]]) and f['perm_idx'][0] == 1 and f['perm_idx'][1] == 0
    assert not f['coef'][0, 0].any() and f['coef'][0, 1].all() and not f['coef'][1].any()
    assert not dX[0, 0].any() and dX[0, 1].any() and not dX[1].any()
    assert f['loss'] == -f['per_utt'][0] and f['per_utt'][1] == 0.0
    none, d = WR.loss_and_grad(src[1:], est[1:], w, S)
    assert none['loss'] == 0.0 and not d.any()


def test_scale_invariance_and_its_orthogonality():
    rng = np.random.RandomState(4)
    N, S, T = 256, 64, 7
    w = _sqrt_hann(N).astype(np.float64)
    src = _spectra(rng, 3, 2, T, N)
    est = src + 10.0 ** (-np.array([0.0, 12.0, 28.0])[:, None, None, None] / 20) * _spectra(rng, 3, 2, T, N)
    f, dX = WR.loss_and_grad(src, est, w, S)
    for k in (0.01, 3.0, 1e4):
        assert abs(WR.loss_and_grad(src, k * est, w, S)[0]['loss'] - f['loss']) <= 1e-10
    # the synthesis ignores the imaginary parts of bins 0 and N/2, and dX is 0 there: the inner product is that of
    # the part of X the loss depends on
    for b in range(3):
        for j in range(2):
            dot = float((dX[b, j].real * est[b, j].real + dX[b, j].imag * est[b, j].imag).sum())
            assert abs(dot) <= 1e-12 * np.linalg.norm(dX[b, j]) * np.linalg.norm(est[b, j]), (b, j, dot)


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_loss_is_minus_the_metric(C):
    rng = np.random.RandomState(C)
    B, L = 40, 96
    perms = list(itertools.permutations(range(C)))
    s = rng.standard_normal((B, C, L))
    want = rng.randint(0, len(perms), B)
    e = np.zeros((B, C, L))
    for b in range(B):
        for i in range(C):
            e[b, perms[want[b]][i]] = s[b, i]
    e += 10.0 ** (-rng.uniform(-5, 30, (B, 1, 1)) / 20) * rng.standard_normal((B, C, L))
    s[5] *= 0
    s[6, 0] *= 0
    G = MR.gram(np.concatenate([s, e], axis=1))
    f = WR.fwd(G, C)
    per_utt, perm_idx, mean2 = MR.finalize(G, C)
    assert f['loss'] == -mean2[0] and np.array_equal(f['per_utt'], per_utt[:, 0])
    assert np.array_equal(f['perm_idx'], perm_idx)
    for b in range(B):
        live = [i for i in range(C) if G[b, i, i] != 0]
        assert sorted(int(v) for v in f['pair'][b] if v >= 0) == live
        for i in live:
            assert f['pair'][b, perms[perm_idx[b]][i]] == i
