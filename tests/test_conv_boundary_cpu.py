'''
CPU tests (no GPU) of the conv-bilstm-v1 encoder's boundary: the registry resolves the name, the
extension library libdanet_conv_hip.so loads and exports exactly what include/danet_conv_hip.h
declares, and its host-side checks answer without a GPU.  The core library's ABI is untouched.
'''
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, 'include', 'danet_conv_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(danet_conv_[a-z0-9_]+)\s*\(', txt)))


def test_registry_resolves_conv_bilstm_v1(hp):
    from danet_amd import modules
    hp.load(dict(ENCODER_TYPE='conv-bilstm-v1'))
    assert hp.get_encoder() is modules.ConvBiLstmEncoder
    assert issubclass(modules.ConvBiLstmEncoder, modules.Encoder)


def test_extension_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_conv()
    syms = _header_symbols()
    assert set(_lib.CONV_PROTOTYPES) == set(syms), set(_lib.CONV_PROTOTYPES) ^ set(syms)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.CONV_LIB_PATH], capture_output=True, text=True,
                         check=True)
    exported = sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())
    assert set(exported) == set(syms), set(exported) ^ set(syms)
    assert lib.danet_conv_abi_version() == 1
    # the core table keeps exactly the core header's symbols
    assert not any(k.startswith('danet_conv_') for k in _lib.PROTOTYPES)


def _desc(**kw):
    from danet_amd import ops
    d = ops.conv_encoder_descs(2, 16, 64, 0.3)[1]
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_workspace_query_and_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_conv()
    bad = ctypes.c_size_t(-1).value
    d = _desc()
    n = lib.danet_conv_workspace_bytes(_lib.CONV_WS_BWD_WEIGHT, ctypes.byref(d))
    assert 0 < n < (1 << 32)
    assert n % ((8 * 25 + 1) * 16 * 4) == 0            # whole slabs of (Cin k k + 1) x Cout floats
    assert lib.danet_conv_workspace_bytes(7, ctypes.byref(d)) == bad
    assert b'unknown op' in lib.danet_conv_last_error()
    assert lib.danet_conv_workspace_bytes(_lib.CONV_WS_BWD_WEIGHT, None) == bad
    for k in (1, 2, 4, 7):
        dk = _desc(k=k)
        assert lib.danet_conv_workspace_bytes(_lib.CONV_WS_BWD_WEIGHT, ctypes.byref(dk)) == bad
        assert lib.danet_conv_fwd(None, ctypes.byref(dk), 16, 16, 16, 16, 16) == -1
        assert b'k must be 3 or 5' in lib.danet_conv_last_error()
    # null pointers, flags, bounds: refused before any launch
    assert lib.danet_conv_fwd(None, ctypes.byref(d), None, 16, 16, 16, 16) == -1
    assert lib.danet_conv_fwd(None, ctypes.byref(d), 16, 16, 16, 16, None) == -1      # pool without argmax
    assert b'argmax' in lib.danet_conv_last_error()
    assert lib.danet_conv_bwd_data(None, ctypes.byref(d), 16, None, 16, 16, 16) == -1
    assert lib.danet_conv_bwd_weight(None, ctypes.byref(d), 16, 16, 16, 16, 16, 16, 0, None, 0) == -1
    assert lib.danet_conv_bwd_weight(None, ctypes.byref(d), 16, 16, 16, 16, 16, 16, 0, 16, n - 4) == -4
    for kw in (dict(pool=1, d2s=1), dict(Cout=65), dict(Cin=0), dict(alpha=1.0), dict(d2s=1, pool=0, Cout=6)):
        dd = _desc(**kw)
        assert lib.danet_conv_fwd(None, ctypes.byref(dd), 16, 16, 16, 16, 16) == -1, kw
    assert lib.danet_conv_add(None, 0, 16, 16, 16) == -1
    assert lib.danet_conv_add(None, 4, None, 16, 16) == -1
    with pytest.raises(_lib.DanetHipError, match='k must be 3 or 5'):
        _lib.conv_ws_bytes(_lib.CONV_WS_BWD_WEIGHT, _desc(k=4))


def test_shape_rules_raise_value_error(hp):
    from danet_amd import ops
    ops.conv_encoder_check(128, 256, 129)
    for T, nfft, F in ((126, 256, 129), (5, 64, 33), (128, 60, 31), (128, 8, 5), (128, 256, 128)):
        with pytest.raises(ValueError):
            ops.conv_encoder_check(T, nfft, F)


def test_missing_extension_library_is_a_loud_error(tmp_path):
    import sys
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib\n"
        "_lib.CONV_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_conv()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e))\n"
    ) % (ROOT, str(tmp_path / 'nope.so'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'LOUD: True' in out.stdout, out.stdout + out.stderr
