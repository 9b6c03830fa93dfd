'''
CPU tests (no GPU) of what the five HIP libraries have in common, one case per record of _lib.LIBRARIES:
the binding and the build name the same file, the prototype table is the header's symbol list is the
built file's export list, nothing is mapped by importing the package, a missing file is a loud error
that names it, and <name>_check raises with the library's own error text.
'''
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['', 'conv', 'dropout', 'prep', 'mix']


def _spec(name):
    from danet_amd import _lib
    spec = _lib.LIBRARIES[NAMES.index(name)]
    assert spec.name == name
    return spec


def _public(name, what):
    '''_lib's load / check of the core, load_<name> / <name>_check of an extension'''
    from danet_amd import _lib
    return getattr(_lib, {'load': 'load_' + name, 'check': name + '_check'}[what] if name else what)


# one call per library that fails on a null pointer before anything touches a device
NULL_POINTER_CALL = {
    '': lambda lib: lib.danet_stft(None, 1, 8000, 256, 64, None, None, None),
    'conv': lambda lib: lib.danet_conv_fwd(None, None, 16, 16, 16, 16, 16),
    'dropout': lambda lib: lib.danet_dropout_apply(None, 4, 8, None, 8, 1024, 8, 1 << 31, 2.0, 0, 0, 0, 0),
    'prep': lambda lib: lib.danet_prep_stft_batch(None, 4, None, 100000, 2048, 40, 0, 40, 256, 64, 4096, 8192,
                                                  16384, 129),
    'mix': lambda lib: lib.danet_mix_scale_c64(None, 4, 8, 129, None, 129, 1024),
}


def test_the_records_are_the_five_libraries_in_build_order():
    from danet_amd import _lib
    assert [spec.name for spec in _lib.LIBRARIES] == NAMES
    assert [spec.so for spec in _lib.LIBRARIES] == ['libdanet_hip.so', 'libdanet_conv_hip.so',
                                                    'libdanet_dropout_hip.so', 'libdanet_prep_hip.so',
                                                    'libdanet_mix_hip.so']
    assert len(set(spec.path_var for spec in _lib.LIBRARIES)) == 5
    assert len(set(spec.handle_var for spec in _lib.LIBRARIES)) == 5


@pytest.mark.parametrize('name', NAMES)
def test_binding_and_build_name_the_same_file(name):
    import importlib
    from danet_amd import _lib
    build = importlib.import_module('danet-tensorflow_amd._build')
    spec = _spec(name)
    out = getattr(build, (name.upper() + '_' if name else '') + 'LIB')
    assert out == build.LIBRARIES[NAMES.index(name)].out
    assert os.path.basename(out) == spec.so
    if name or not os.environ.get('DANET_LIB_PATH'):
        assert getattr(_lib, spec.path_var) == out
    assert os.path.dirname(out) == os.path.join(ROOT, 'danet-tensorflow_amd', 'csrc')
    assert os.path.isfile(os.path.join(build.LIBRARIES[NAMES.index(name)].src_dir, 'exports.map'))


@pytest.mark.parametrize('name', NAMES)
def test_table_is_the_header_is_the_export_list(name):
    from danet_amd import _lib
    spec = _spec(name)
    assert spec.prefix == ('danet_%s_' % name if name else 'danet_')
    txt = open(os.path.join(ROOT, 'include', spec.prefix + 'hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % spec.prefix, txt)))
    out = subprocess.run(['nm', '-D', '--defined-only', getattr(_lib, spec.path_var)], capture_output=True,
                         text=True, check=True)
    exported = sorted(l.split()[-1] for l in out.stdout.splitlines() if l.strip())
    assert sorted(spec.prototypes) == declared == exported
    assert spec.prefix + 'abi_version' in spec.prototypes and spec.prefix + 'last_error' in spec.prototypes
    assert spec.prototypes is getattr(_lib, (name.upper() + '_' if name else '') + 'PROTOTYPES')
    assert '#define DANET_%sABI_VERSION %d' % (name.upper() + '_' if name else '', spec.abi) in txt
    assert getattr(_public(name, 'load')(), spec.prefix + 'abi_version')() == spec.abi


@pytest.fixture(scope='module')
def fresh_process(tmp_path_factory):
    '''what ONE fresh interpreter sees, per library: the handle after importing the package, then the
    error of a load with the path global pointed at a file that does not exist'''
    nope = str(tmp_path_factory.mktemp('libraries') / 'nope.so')
    code = (
        "import json, sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib, ops, model\n"
        "res = {}\n"
        "for spec in _lib.LIBRARIES:\n"
        "    r = res[spec.name] = {'handle_is_none': getattr(_lib, spec.handle_var) is None}\n"
        "    setattr(_lib, spec.path_var, %r)\n"
        "    try:\n"
        "        getattr(_lib, 'load_' + spec.name if spec.name else 'load')()\n"
        "        r['error'] = None\n"
        "    except _lib.DanetHipError as e:\n"
        "        r['error'] = str(e)\n"
        "    r['handle_is_none_after'] = getattr(_lib, spec.handle_var) is None\n"
        "res['mapped'] = 'libdanet_' in open('/proc/self/maps').read()\n"
        "print('RESULT ' + json.dumps(res))\n"
    ) % (ROOT, nope)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    lines = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')]
    assert lines, out.stdout + out.stderr
    return nope, json.loads(lines[-1][len('RESULT '):])


@pytest.mark.parametrize('name', NAMES)
def test_import_maps_nothing_and_a_missing_file_is_a_loud_error(fresh_process, name):
    nope, res = fresh_process
    spec = _spec(name)
    assert res[name]['handle_is_none'] is True
    err = res[name]['error']
    assert err is not None, 'load of a missing file did not raise'
    assert spec.so in err and nope in err and 'no CPU fallback' in err and 'g.build()' in err
    assert res[name]['handle_is_none_after'] is True
    assert res['mapped'] is False               # neither the import nor a refused load mapped a library


@pytest.mark.parametrize('name', NAMES)
def test_check_raises_with_the_librarys_own_message(name):
    from danet_amd import _lib
    spec = _spec(name)
    lib, check = _public(name, 'load')(), _public(name, 'check')
    assert lib is getattr(_lib, spec.handle_var) is _public(name, 'load')()
    assert check(0) is None
    assert NULL_POINTER_CALL[name](lib) == -1
    text = getattr(lib, spec.prefix + 'last_error')().decode()
    assert 'null' in text
    with pytest.raises(_lib.DanetHipError) as e:
        check(-1)
    assert str(e.value) == '%s error -1: %s' % (spec.so[:-len('.so')], text)
