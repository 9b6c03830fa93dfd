'''
Builds the twenty-one HIP libraries (gfx950 only) in-tree with hipcc.

    python danet-tensorflow_amd/_build.py [--force]

    library (under csrc/)         sources                  rebuilt when one of these headers is newer
    libdanet_hip.so               csrc/*.hip, csrc/*.cpp   csrc/*.h, include/*.h
    libdanet_conv_hip.so          csrc/conv/*.hip          include/danet_conv_hip.h, csrc/conv/*.h, csrc/ext_core.h
    libdanet_dropout_hip.so       csrc/dropout/*.hip       include/danet_dropout_hip.h, csrc/ext_core.h
    libdanet_prep_hip.so          csrc/prep/*.hip          include/danet_prep_hip.h, csrc/ext_core.h
    libdanet_mix_hip.so           csrc/mix/*.hip           include/danet_mix_hip.h,
                                                           csrc/{ext_core,ragged_rows,sumsq_f64}.h
    libdanet_speed_hip.so         csrc/speed/*.hip         include/danet_speed_hip.h, csrc/{ext_core,ragged_rows}.h
    libdanet_reverb_hip.so        csrc/reverb/*.hip        include/danet_reverb_hip.h, csrc/{ext_core,ragged_rows}.h
    libdanet_metric_hip.so        csrc/metric/*.hip        include/danet_metric_hip.h, csrc/{wave_metric,ext_core}.h
    libdanet_noise_hip.so         csrc/noise/*.hip         include/danet_noise_hip.h, csrc/ext_core.h
    libdanet_level_hip.so         csrc/level/*.hip         include/danet_level_hip.h, csrc/{ext_core,ragged_rows}.h
    libdanet_wavloss_hip.so       csrc/wavloss/*.hip       include/danet_wavloss_hip.h, csrc/{wave_metric,ext_core}.h
    libdanet_gclip_hip.so         csrc/gclip/*.hip         include/danet_gclip_hip.h,
                                                           csrc/{ext_core,adam_one,sumsq_f64}.h
    libdanet_dpcl_hip.so          csrc/dpcl/*.hip          include/danet_dpcl_hip.h, csrc/ext_core.h
    libdanet_neval_hip.so         csrc/neval/*.hip         include/danet_neval_hip.h, csrc/{wave_metric,ext_core}.h
    libdanet_stitch_hip.so        csrc/stitch/*.hip        include/danet_stitch_hip.h, csrc/ext_core.h
    libdanet_bss_hip.so           csrc/bss/*.hip           include/danet_bss_hip.h, csrc/ext_core.h
    libdanet_stoi_hip.so          csrc/stoi/*.hip          include/danet_stoi_hip.h, csrc/ext_core.h
    libdanet_phase_hip.so         csrc/phase/*.hip         include/danet_phase_hip.h, csrc/{ext_core,wave_metric}.h
    libdanet_online_hip.so        csrc/online/*.hip        include/danet_online_hip.h, csrc/ext_core.h
    libdanet_causal_hip.so        csrc/causal/*.hip        include/danet_causal_hip.h, csrc/ext_core.h
    libdanet_tonline_hip.so       csrc/tonline/*.hip       include/danet_tonline_hip.h, csrc/ext_core.h

One object per source under <source directory>/build/, compiled in parallel and linked with the
exports.map of the source directory; an object is rebuilt only when its source or one of its library's
headers is newer.  No torch headers are involved: every library is a plain C ABI (include/*.h).
'''
import collections
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
INCLUDE = os.path.join(os.path.dirname(HERE), 'include')
ARCH = 'gfx950'
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# -fvisibility=hidden: only what the library's header declares (inside its visibility pragma) is exported
FLAGS = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-I' + INCLUDE,
         '-I' + CSRC, '-Wno-unused-result']
# extra -D switches for A/B builds, e.g. DANET_BUILD_DEFS='-DBK=32' (use --force)
FLAGS += os.environ.get('DANET_BUILD_DEFS', '').split()

# out: the shared object; src_dir: its sources, its exports.map and (under build/) its objects;
# headers: glob patterns of the headers whose change rebuilds every object of the library
Library = collections.namedtuple('Library', 'out src_dir headers')


def _extension(name, *more_headers):
    src_dir = os.path.join(CSRC, name)
    return Library(os.path.join(CSRC, 'libdanet_%s_hip.so' % name), src_dir,
                   (os.path.join(INCLUDE, 'danet_%s_hip.h' % name),) + more_headers)


def _shared(*names):
    return tuple(os.path.join(CSRC, n + '.h') for n in names)


CORE = Library(os.path.join(CSRC, 'libdanet_hip.so'), CSRC, (os.path.join(CSRC, '*.h'), os.path.join(INCLUDE, '*.h')))
CONV = _extension('conv', os.path.join(CSRC, 'conv', '*.h'), *_shared('ext_core'))
DROPOUT = _extension('dropout', *_shared('ext_core'))
PREP = _extension('prep', *_shared('ext_core'))
MIX = _extension('mix', *_shared('ext_core', 'ragged_rows', 'sumsq_f64'))
SPEED = _extension('speed', *_shared('ext_core', 'ragged_rows'))
# build() builds them in this order; a new record is APPENDED (the first five are indexed by position)
LIBRARIES = (CORE, CONV, DROPOUT, PREP, MIX, SPEED)
LIB, CONV_LIB, DROPOUT_LIB, PREP_LIB, MIX_LIB, SPEED_LIB = (spec.out for spec in LIBRARIES)
# LIBRARIES stays the six records above; every library added after them goes HERE, appended, and build() runs
# over LIBRARIES + LATER_LIBRARIES
REVERB = _extension('reverb', *_shared('ext_core', 'ragged_rows'))
LATER_LIBRARIES = (REVERB,)
REVERB_LIB = REVERB.out
# build() stays the seven libraries above.  Every library after them goes HERE, appended: build_all() runs
# build() and then over EXTENSIONS, and nothing pins the length of this tuple
METRIC = _extension('metric', *_shared('wave_metric', 'ext_core'))
NOISE = _extension('noise', *_shared('ext_core'))
LEVEL = _extension('level', *_shared('ext_core', 'ragged_rows'))
WAVLOSS = _extension('wavloss', *_shared('wave_metric', 'ext_core'))
GCLIP = _extension('gclip', *_shared('ext_core', 'adam_one', 'sumsq_f64'))
DPCL = _extension('dpcl', *_shared('ext_core'))
NEVAL = _extension('neval', *_shared('wave_metric', 'ext_core'))
EXTENSIONS = (METRIC, NOISE, LEVEL, WAVLOSS, GCLIP, DPCL, NEVAL)
# EXTENSIONS stays the seven records above (tests/test_neval_cpu.py pins it).  Every library after them goes HERE,
# appended: build_all() runs over MORE_EXTENSIONS after EXTENSIONS
STITCH = _extension('stitch', *_shared('ext_core'))
BSS = _extension('bss', *_shared('ext_core'))
STOI = _extension('stoi', *_shared('ext_core'))
PHASE = _extension('phase', *_shared('ext_core', 'wave_metric'))
ONLINE = _extension('online', *_shared('ext_core'))
CAUSAL = _extension('causal', *_shared('ext_core'))
TONLINE = _extension('tonline', *_shared('ext_core'))
MORE_EXTENSIONS = (STITCH, BSS, STOI, PHASE, ONLINE, CAUSAL, TONLINE)
METRIC_LIB = METRIC.out
NOISE_LIB = NOISE.out
LEVEL_LIB = LEVEL.out
WAVLOSS_LIB = WAVLOSS.out
GCLIP_LIB = GCLIP.out
DPCL_LIB = DPCL.out
NEVAL_LIB = NEVAL.out
STITCH_LIB = STITCH.out
BSS_LIB = BSS.out
STOI_LIB = STOI.out
PHASE_LIB = PHASE.out
ONLINE_LIB = ONLINE.out
CAUSAL_LIB = CAUSAL.out
TONLINE_LIB = TONLINE.out


def _sources(src_dir):
    return sorted(f for f in os.listdir(src_dir) if f.endswith(('.hip', '.cpp')))


def _compile(src_dir, src, bdir, force, hdr_m, defs=()):
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


def _compile_all(src_dir, bdir, force, hdr_m, defs=()):
    '''-> [(object, rebuilt)] of every source of src_dir, in sorted order'''
    os.makedirs(bdir, exist_ok=True)
    srcs = _sources(src_dir)
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        return list(ex.map(lambda s: _compile(src_dir, s, bdir, force, hdr_m, defs), srcs))


def _link(objs, out, src_dir):
    cmd = [HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC',
           '-Wl,--version-script=' + os.path.join(src_dir, 'exports.map'), '-o', out] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('link failed:\n%s\n%s' % (r.stdout, r.stderr))


def _build_spec(spec, force, verbose):
    hdr_m = max((os.path.getmtime(h) for pattern in spec.headers for h in glob.glob(pattern)), default=0.0)
    res = _compile_all(spec.src_dir, os.path.join(spec.src_dir, 'build'), force, hdr_m)
    objs = [o for o, _ in res]
    rebuilt = any(r for _, r in res)
    if rebuilt or not os.path.exists(spec.out):
        _link(objs, spec.out, spec.src_dir)
    if verbose:
        print('%s: %s (%d objects, %s)' % (
            os.path.basename(spec.out), spec.out, len(objs), 'rebuilt' if rebuilt else 'up to date'))
    return spec.out


def _build_library(spec, force, verbose):
    return _build_spec(spec, force, verbose)


def build(force=False, verbose=True):
    '''the seven libraries of LIBRARIES + LATER_LIBRARIES (build_all: every library)'''
    for spec in LIBRARIES + LATER_LIBRARIES:
        _build_library(spec, force, verbose)
    return LIB


def build_all(force=False, verbose=True):
    '''build(), then every record of EXTENSIONS and MORE_EXTENSIONS -> [every shared object built, in order]'''
    build(force, verbose)
    for spec in EXTENSIONS + MORE_EXTENSIONS:
        _build_spec(spec, force, verbose)
    return [spec.out for spec in LIBRARIES + LATER_LIBRARIES + EXTENSIONS + MORE_EXTENSIONS]


def build_conv(force=False, verbose=True):
    return _build_library(CONV, force, verbose)


def build_dropout(force=False, verbose=True):
    return _build_library(DROPOUT, force, verbose)


def build_prep(force=False, verbose=True):
    return _build_library(PREP, force, verbose)


def build_mix(force=False, verbose=True):
    return _build_library(MIX, force, verbose)


def build_speed(force=False, verbose=True):
    return _build_library(SPEED, force, verbose)


def build_reverb(force=False, verbose=True):
    return _build_library(REVERB, force, verbose)


def build_metric(force=False, verbose=True):
    return _build_spec(METRIC, force, verbose)


def build_noise(force=False, verbose=True):
    return _build_spec(NOISE, force, verbose)


def build_level(force=False, verbose=True):
    return _build_spec(LEVEL, force, verbose)


def build_wavloss(force=False, verbose=True):
    return _build_spec(WAVLOSS, force, verbose)


def build_gclip(force=False, verbose=True):
    return _build_spec(GCLIP, force, verbose)


def build_dpcl(force=False, verbose=True):
    return _build_spec(DPCL, force, verbose)


def build_neval(force=False, verbose=True):
    return _build_spec(NEVAL, force, verbose)


def build_stitch(force=False, verbose=True):
    return _build_spec(STITCH, force, verbose)


def build_bss(force=False, verbose=True):
    return _build_spec(BSS, force, verbose)


def build_stoi(force=False, verbose=True):
    return _build_spec(STOI, force, verbose)


def build_phase(force=False, verbose=True):
    return _build_spec(PHASE, force, verbose)


def build_online(force=False, verbose=True):
    return _build_spec(ONLINE, force, verbose)


def build_causal(force=False, verbose=True):
    return _build_spec(CAUSAL, force, verbose)


def build_tonline(force=False, verbose=True):
    return _build_spec(TONLINE, force, verbose)


def build_variant(name, defs):
    '''A/B variant csrc/libdanet_hip_<name>.so compiled with extra -D switches (e.g.
    name='accmath', defs=['-DDANET_LSTM_ACCURATE_MATH']; name='trace',
    defs=['-DDANET_LSTM_TRACE']: the persistent LSTM kernels time-stamp every step,
    tools/trace_lstm.py); loaded instead of the product library when DANET_LIB_PATH points at it
    (tests / tools only).  Objects under csrc/build_<name>/.'''
    out = os.path.join(CSRC, 'libdanet_hip_%s.so' % name)
    res = _compile_all(CSRC, os.path.join(CSRC, 'build_' + name), True, 0.0, defs)
    _link([o for o, _ in res], out, CSRC)
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
        build_all(force='--force' in sys.argv)
