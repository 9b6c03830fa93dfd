'''
CPU tests (no GPU) of the dropout feature's boundary: the mask generator's known answers, the
threshold / scale derivation, the mask statistics, the extension library libdanet_dropout_hip.so
against its header (exports, prototypes, no environment read, argument errors), the untouched core
ABI, and the Python surface (Model.forward's signature, which encoders look at the argument, where the
Philox key and step come from).
'''
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dropout_ref as D
import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(name, prefix):
    txt = open(os.path.join(ROOT, 'include', name)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, txt)))


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in D.philox4x32_10(ctr, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])


def test_words_follow_the_counter_layout():
    # element e = word (e & 3) of counter (g lo, g hi, stream, step), g = e >> 2
    w = D.words(11, 7, 9, 2, 5)
    for e in (0, 3, 4, 10):
        one = D.philox4x32_10((e >> 2, 0, 2, 5), (7, 9))
        assert int(w[e]) == int(one[e & 3])
    hi = D.philox4x32_10((np.uint64(1) << np.uint64(32) >> np.uint64(32), 1, 2, 5), (7, 9))
    assert hi.shape == (4,)


def test_threshold_and_scale_derivation():
    from danet_amd import ops
    assert ops.dropout_threshold(0.5) == 1 << 31
    assert ops.dropout_threshold(1.0) == 0xffffffff
    assert ops.dropout_threshold(0.8) == 3435973836          # floor(0.8 * 2^32), 0.8 as a double
    assert ops.dropout_threshold(1e-12) == 0
    for keep in (0.5, 0.8, 0.95, 0.1, 0.999999, 1.0, 1. / 3):
        assert ops.dropout_threshold(keep) == D.threshold_of(keep), keep
        s = ops.dropout_scale(keep)
        assert np.float32(s) == s                               # a float32 value
        assert s == float(D.scale_of(keep)), keep
    assert ops.dropout_scale(0.8) == 1.25
    assert ops.dropout_scale(0.95) == float(np.float32(1.0 / 0.95))
    sp = ops.DropoutSpec(0.8, key0=(1 << 32) + 5, key1=1, step=3)
    assert (sp.key0, sp.key1, sp.step, sp.threshold, sp.scale, sp.active) == (5, 1, 3, 3435973836, 1.25, True)
    assert [sp.take(3), sp.take(), sp.take()] == [0, 3, 4]
    assert not ops.DropoutSpec(1.0).active
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ops.DropoutSpec(bad)


@pytest.mark.parametrize('keep', [0.5, 0.8, 0.95])
def test_keep_fraction_at_the_cfg2_layer_shape(keep):
    n = 4096 * 600
    bound = 6 * np.sqrt(keep * (1 - keep) / n)
    for step in range(4):
        frac = float((D.words(n, 1337, 0, 0, step) < np.uint32(D.threshold_of(keep))).mean())
        print('keep %.2f step %d: fraction %.6f (bound +-%.6f)' % (keep, step, frac, bound))
        assert abs(frac - keep) <= bound, (keep, step, frac)


def test_extension_library_exports_exactly_its_header():
    from danet_amd import _lib
    lib = _lib.load_dropout()
    syms = _header_symbols('danet_dropout_hip.h', 'danet_dropout_')
    assert syms == ['danet_dropout_abi_version', 'danet_dropout_apply', 'danet_dropout_last_error']
    assert set(_lib.DROPOUT_PROTOTYPES) == set(syms)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.DROPOUT_LIB_PATH], capture_output=True,
                         text=True, check=True)
    exported = sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())
    assert exported == syms, set(exported) ^ set(syms)
    assert lib.danet_dropout_abi_version() == 1
    # the argument list of the one operator, as the header writes it
    txt = open(os.path.join(ROOT, 'include', 'danet_dropout_hip.h')).read()
    args = re.search(r'int danet_dropout_apply\((.*?)\);', txt, flags=re.S).group(1)
    ctype = {'void*': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'const float*': ctypes.c_void_p,
             'float*': ctypes.c_void_p, 'uint32_t': ctypes.c_uint32, 'float': ctypes.c_float}
    want = [ctype[a.strip().rsplit(' ', 1)[0]] for a in args.replace('\n', ' ').split(',')]
    assert _lib.DROPOUT_PROTOTYPES['danet_dropout_apply'][1] == want


def test_library_does_not_read_the_environment():
    from danet_amd import _lib
    out = subprocess.run(['nm', '-D', _lib.DROPOUT_LIB_PATH], capture_output=True, text=True, check=True)
    assert 'getenv' not in out.stdout
    src = open(os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc', 'dropout', 'dropout.hip')).read()
    src += csrc_scan.shared_code(src, comments=True)
    assert 'ext_core.h' in src and 'getenv' not in src and 'environ' not in src


def test_core_library_abi_is_untouched():
    from danet_amd import _lib
    lib = _lib.load()
    assert lib.danet_abi_version() == 7
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())
    assert len(exported) <= 51
    assert exported == _header_symbols('danet_hip.h', 'danet_')
    assert not any(k.startswith('danet_dropout_') for k in list(_lib.PROTOTYPES) + list(_lib.CONV_PROTOTYPES))


def test_argument_errors_without_gpu():
    from danet_amd import _lib
    lib = _lib.load_dropout()
    ok = dict(stream=None, rows=4, cols=8, x=64, ldx=8, y=1024, ldy=8, threshold=1 << 31, scale=2.0,
              key0=0, key1=0, stream_id=0, step=0)
    cases = [(dict(x=None), b'null'), (dict(y=None), b'null'), (dict(rows=0), b'rows and cols'),
             (dict(cols=-1), b'rows and cols'), (dict(ldx=7), b'>= cols'), (dict(ldy=4), b'>= cols'),
             (dict(x=66), b'4-byte'), (dict(y=1025), b'4-byte'), (dict(threshold=0), b'threshold'),
             (dict(rows=1 << 40, cols=1 << 30, ldx=1 << 30, ldy=1 << 30), b'2^62'),
             (dict(y=64, ldy=12), b'in place'), (dict(scale=float('inf')), b'finite'),
             (dict(scale=float('nan')), b'finite')]
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert lib.danet_dropout_apply(*a.values()) == -1, kw
        assert msg in lib.danet_dropout_last_error(), (kw, lib.danet_dropout_last_error())
    with pytest.raises(_lib.DanetHipError, match='threshold'):
        _lib.dropout_check(lib.danet_dropout_apply(*dict(ok, threshold=0).values()))


def test_missing_extension_library_is_a_loud_error(tmp_path):
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib\n"
        "print('LAZY:', _lib._dropout is None)\n"
        "_lib.DROPOUT_LIB_PATH = %r\n"
        "try:\n"
        "    _lib.load_dropout()\n"
        "except _lib.DanetHipError as e:\n"
        "    print('LOUD:', 'no CPU fallback' in str(e))\n"
    ) % (ROOT, str(tmp_path / 'nope.so'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'LAZY: True' in out.stdout and 'LOUD: True' in out.stdout, out.stdout + out.stderr


def test_model_forward_signature_and_defaults():
    from danet_amd.model import Model
    from danet_amd import modules
    sig = inspect.signature(Model.forward)
    assert list(sig.parameters) == ['self', 's_src_signals', 'with_valid', 'with_train', 'fuse_heads',
                                    's_dropout_keep']
    assert sig.parameters['s_dropout_keep'].default == 1.0
    for cls in (modules.ToyEncoder, modules.LstmEncoder, modules.BiLstmEncoder, modules.ConvBiLstmEncoder):
        p = inspect.signature(cls.__call__).parameters
        assert p['s_dropout_keep'].default == 1., cls
    p = inspect.signature(modules._lyr_bilstm).parameters
    assert list(p)[-1] == 's_dropout_keep_'


class _FakeModel(object):
    '''variables as CPU zeros; records whether an encoder asked for the step's mask source'''

    def __init__(self):
        self.asked = []

    def get_variable(self, name, shape, init):
        return torch.zeros(shape)

    def dropout_spec(self, keep):
        from danet_amd import ops
        self.asked.append(keep)
        return ops.DropoutSpec(keep, 1, 0, 0)


def test_which_encoders_look_at_the_keep_probability(hp, monkeypatch):
    from danet_amd import modules, ops
    hp.load(dict(BATCH_SIZE=2, FFT_SIZE=16, EMBED_SIZE=2, NUM_LSTM_LAYERS=2, LSTM_HDIM=4))
    hp.digest()
    F, E = hp.FEATURE_SIZE, hp.EMBED_SIZE
    seen = []

    class Stub(object):
        @staticmethod
        def apply(x, *a):
            seen.append(ops._dropout_cur[0])
            return torch.zeros(x.shape[0], x.shape[1], F * E)

    monkeypatch.setattr(ops, 'RnnEncoderFn', Stub)
    monkeypatch.setattr(ops, 'lyr_linear', lambda x, W, b=None: torch.zeros(x.shape[:-1] + (W.shape[1],)))
    monkeypatch.setattr(ops, 'relu', lambda x, a=0.: x)
    x = torch.zeros(2, 3, F)
    # lstm-orig and toy: accepted and ignored (the reference's classes never read it)
    m = _FakeModel()
    modules.LstmEncoder(m, 'encoder')(x, 0.8)
    modules.ToyEncoder(m, 'encoder')(x, 0.8)
    assert seen == [None] and m.asked == []
    # bilstm-orig: the step's spec is in scope for the encoder function, and only for keep < 1
    modules.BiLstmEncoder(m, 'encoder')(x, 0.8)
    assert m.asked == [0.8] and seen[1] is not None and seen[1].keep == 0.8
    modules.BiLstmEncoder(m, 'encoder')(x, 1.0)
    modules.BiLstmEncoder(m, 'encoder')(x)
    assert m.asked == [0.8] and seen[2:] == [None, None]
    assert ops._dropout_cur[0] is None


def test_key_and_step_derivation(hp, monkeypatch):
    '''key0 = the model's seed, key1 = the data-parallel rank (ranks draw different masks), step =
    train steps taken, resumed runs included'''
    from danet_amd import dist
    from danet_amd.model import Model
    m = Model('k', device='cpu', seed=(5 << 32) + 1337)
    a = m.dropout_spec(0.8)
    assert (a.key0, a.key1, a.step, a.keep) == (1337, 0, 0, 0.8)
    assert m.dropout_spec(0.8) is a                 # one spec per forward pass: stream ids keep counting
    monkeypatch.setattr(dist, 'rank', lambda: 3)
    m._dropout = None                               # (Model.forward does this at the start of a pass)
    m.step_count, m.step_base = 2, 40
    b = m.dropout_spec(0.8)
    assert (b.key0, b.key1, b.step) == (1337, 3, 42)
    # the two ranks' masks differ, the same rank's repeat
    m0 = D.keep_mask(8, 12, a.threshold, 1337, 0, 0, 42)
    m3 = D.keep_mask(8, 12, b.threshold, b.key0, b.key1, 0, b.step)
    assert (m0 != m3).any()
    assert (m3 == D.keep_mask(8, 12, b.threshold, 1337, 3, 0, 42)).all()
