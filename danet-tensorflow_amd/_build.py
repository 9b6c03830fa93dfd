'''
Builds libdanet_hip.so (gfx950 only) in-tree with hipcc.

    python danet-tensorflow_amd/_build.py [--force]

One object per .hip/.cpp under csrc/, compiled in parallel, linked into
csrc/libdanet_hip.so.  The extension library of the conv-bilstm-v1 encoder
(csrc/conv/*.hip -> csrc/libdanet_conv_hip.so, include/danet_conv_hip.h) is
built by the same call, and so is the dropout extension (csrc/dropout/*.hip ->
csrc/libdanet_dropout_hip.so, include/danet_dropout_hip.h), the dataset front-end extension
(csrc/prep/*.hip -> csrc/libdanet_prep_hip.so, include/danet_prep_hip.h) and the mixture level
extension (csrc/mix/*.hip -> csrc/libdanet_mix_hip.so, include/danet_mix_hip.h).  Objects are rebuilt only when their
source (or a shared header) is newer.  No torch headers are involved: the library is a plain C ABI
(include/danet_hip.h).
'''
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
INCLUDE = os.path.join(os.path.dirname(HERE), 'include')
BUILD = os.path.join(CSRC, 'build')
LIB = os.path.join(CSRC, 'libdanet_hip.so')
CONV_CSRC = os.path.join(CSRC, 'conv')
CONV_BUILD = os.path.join(CONV_CSRC, 'build')
CONV_LIB = os.path.join(CSRC, 'libdanet_conv_hip.so')
DROPOUT_CSRC = os.path.join(CSRC, 'dropout')
DROPOUT_BUILD = os.path.join(DROPOUT_CSRC, 'build')
DROPOUT_LIB = os.path.join(CSRC, 'libdanet_dropout_hip.so')
PREP_CSRC = os.path.join(CSRC, 'prep')
PREP_BUILD = os.path.join(PREP_CSRC, 'build')
PREP_LIB = os.path.join(CSRC, 'libdanet_prep_hip.so')
MIX_CSRC = os.path.join(CSRC, 'mix')
MIX_BUILD = os.path.join(MIX_CSRC, 'build')
MIX_LIB = os.path.join(CSRC, 'libdanet_mix_hip.so')
ARCH = 'gfx950'
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# -fvisibility=hidden: only what include/danet_hip.h declares (inside its visibility pragma) is exported
FLAGS = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-I' + INCLUDE,
         '-I' + CSRC, '-Wno-unused-result']
# extra -D switches for A/B builds, e.g. DANET_BUILD_DEFS='-DBK=32' (use --force)
FLAGS += os.environ.get('DANET_BUILD_DEFS', '').split()


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(('.hip', '.cpp')))


def _headers_mtime():
    m = 0.0
    for d in (CSRC, INCLUDE):
        for f in os.listdir(d):
            if f.endswith('.h'):
                m = max(m, os.path.getmtime(os.path.join(d, f)))
    return m


def _compile(src, force, hdr_m, bdir=BUILD, defs=(), src_dir=CSRC):
    obj = os.path.join(bdir, os.path.splitext(src)[0] + '.o')
    sp = os.path.join(src_dir, src)
    if (not force and os.path.exists(obj)
            and os.path.getmtime(obj) > max(os.path.getmtime(sp), hdr_m)):
        return obj, False
    cmd = [HIPCC] + FLAGS + list(defs) + ['-c', sp, '-o', obj]
    if src.endswith('.hip'):
        cmd[1:1] = ['-x', 'hip']
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed for %s:\n%s\n%s' % (src, r.stdout, r.stderr))
    return obj, True


def _link(objs, out, exports=os.path.join(CSRC, 'exports.map')):
    cmd = [HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC',
           '-Wl,--version-script=' + exports, '-o', out] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('link failed:\n%s\n%s' % (r.stdout, r.stderr))


def build(force=False, verbose=True):
    os.makedirs(BUILD, exist_ok=True)
    hdr_m = _headers_mtime()
    srcs = _sources()
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        res = list(ex.map(lambda s: _compile(s, force, hdr_m), srcs))
    objs = [o for o, _ in res]
    rebuilt = any(r for _, r in res)
    if rebuilt or not os.path.exists(LIB):
        _link(objs, LIB)
    if verbose:
        print('libdanet_hip.so: %s (%d objects, %s)' % (
            LIB, len(objs), 'rebuilt' if rebuilt else 'up to date'))
    build_conv(force=force, verbose=verbose)
    build_dropout(force=force, verbose=verbose)
    build_prep(force=force, verbose=verbose)
    build_mix(force=force, verbose=verbose)
    return LIB


def build_conv(force=False, verbose=True):
    '''csrc/conv/*.hip -> csrc/libdanet_conv_hip.so (objects under csrc/conv/build/)'''
    os.makedirs(CONV_BUILD, exist_ok=True)
    hdr_m = max([os.path.getmtime(os.path.join(INCLUDE, 'danet_conv_hip.h'))] +
                [os.path.getmtime(os.path.join(CONV_CSRC, f)) for f in os.listdir(CONV_CSRC) if f.endswith('.h')])
    srcs = sorted(f for f in os.listdir(CONV_CSRC) if f.endswith('.hip'))
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        res = list(ex.map(lambda s: _compile(s, force, hdr_m, CONV_BUILD, src_dir=CONV_CSRC), srcs))
    objs = [o for o, _ in res]
    rebuilt = any(r for _, r in res)
    if rebuilt or not os.path.exists(CONV_LIB):
        _link(objs, CONV_LIB, exports=os.path.join(CONV_CSRC, 'exports.map'))
    if verbose:
        print('libdanet_conv_hip.so: %s (%d objects, %s)' % (
            CONV_LIB, len(objs), 'rebuilt' if rebuilt else 'up to date'))
    return CONV_LIB


def build_dropout(force=False, verbose=True):
    '''csrc/dropout/*.hip -> csrc/libdanet_dropout_hip.so (objects under csrc/dropout/build/)'''
    os.makedirs(DROPOUT_BUILD, exist_ok=True)
    hdr_m = os.path.getmtime(os.path.join(INCLUDE, 'danet_dropout_hip.h'))
    srcs = sorted(f for f in os.listdir(DROPOUT_CSRC) if f.endswith('.hip'))
    res = [_compile(s, force, hdr_m, DROPOUT_BUILD, src_dir=DROPOUT_CSRC) for s in srcs]
    objs = [o for o, _ in res]
    rebuilt = any(r for _, r in res)
    if rebuilt or not os.path.exists(DROPOUT_LIB):
        _link(objs, DROPOUT_LIB, exports=os.path.join(DROPOUT_CSRC, 'exports.map'))
    if verbose:
        print('libdanet_dropout_hip.so: %s (%d objects, %s)' % (
            DROPOUT_LIB, len(objs), 'rebuilt' if rebuilt else 'up to date'))
    return DROPOUT_LIB


def build_prep(force=False, verbose=True):
    '''csrc/prep/*.hip -> csrc/libdanet_prep_hip.so (objects under csrc/prep/build/)'''
    os.makedirs(PREP_BUILD, exist_ok=True)
    hdr_m = os.path.getmtime(os.path.join(INCLUDE, 'danet_prep_hip.h'))
    srcs = sorted(f for f in os.listdir(PREP_CSRC) if f.endswith('.hip'))
    res = [_compile(s, force, hdr_m, PREP_BUILD, src_dir=PREP_CSRC) for s in srcs]
    objs = [o for o, _ in res]
    rebuilt = any(r for _, r in res)
    if rebuilt or not os.path.exists(PREP_LIB):
        _link(objs, PREP_LIB, exports=os.path.join(PREP_CSRC, 'exports.map'))
    if verbose:
        print('libdanet_prep_hip.so: %s (%d objects, %s)' % (
            PREP_LIB, len(objs), 'rebuilt' if rebuilt else 'up to date'))
    return PREP_LIB


def build_mix(force=False, verbose=True):
    '''csrc/mix/*.hip -> csrc/libdanet_mix_hip.so (objects under csrc/mix/build/)'''
    os.makedirs(MIX_BUILD, exist_ok=True)
    hdr_m = os.path.getmtime(os.path.join(INCLUDE, 'danet_mix_hip.h'))
    srcs = sorted(f for f in os.listdir(MIX_CSRC) if f.endswith('.hip'))
    res = [_compile(s, force, hdr_m, MIX_BUILD, src_dir=MIX_CSRC) for s in srcs]
    objs = [o for o, _ in res]
    rebuilt = any(r for _, r in res)
    if rebuilt or not os.path.exists(MIX_LIB):
        _link(objs, MIX_LIB, exports=os.path.join(MIX_CSRC, 'exports.map'))
    if verbose:
        print('libdanet_mix_hip.so: %s (%d objects, %s)' % (
            MIX_LIB, len(objs), 'rebuilt' if rebuilt else 'up to date'))
    return MIX_LIB


def build_variant(name, defs):
    '''A/B variant csrc/libdanet_hip_<name>.so compiled with extra -D switches (e.g.
    name='accmath', defs=['-DDANET_LSTM_ACCURATE_MATH']; name='trace',
    defs=['-DDANET_LSTM_TRACE']: the persistent LSTM kernels time-stamp every step,
    tools/trace_lstm.py); loaded instead of the product library when DANET_LIB_PATH points at it
    (tests / tools only).  Objects under csrc/build_<name>/.'''
    out = os.path.join(CSRC, 'libdanet_hip_%s.so' % name)
    bdir = os.path.join(CSRC, 'build_' + name)
    os.makedirs(bdir, exist_ok=True)
    srcs = _sources()
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        res = list(ex.map(lambda s: _compile(s, True, 0.0, bdir, defs), srcs))
    _link([o for o, _ in res], out)
    return out


def build_trace():
    return build_variant('trace', ['-DDANET_LSTM_TRACE'])


if __name__ == '__main__':
    if '--trace' in sys.argv:
        print(build_trace())
    elif '--variant' in sys.argv:
        i = sys.argv.index('--variant')
        print(build_variant(sys.argv[i + 1], sys.argv[i + 2:]))
    else:
        build(force='--force' in sys.argv)
