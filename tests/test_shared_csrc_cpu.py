'''
CPU tests (no GPU) of what the thirteen extension libraries share under danet-tensorflow_amd/csrc/: every shared part
is defined once and in its header, every extension source includes the host core, and the build record of every user
of a shared header lists it.  Source text and the build records only; no library is loaded.
'''
import glob
import importlib
import os
import re

import csrc_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = csrc_scan.CSRC
# extension library -> its one source
SOURCES = {n: os.path.join(CSRC, n, (n if n != 'prep' else 'stft_batch') + '.hip')
           for n in ('conv', 'dropout', 'prep', 'mix', 'speed', 'reverb', 'metric', 'noise', 'level', 'wavloss', 'gclip',
                     'dpcl', 'neval')}
LAUNCH_FAILED = '"kernel launch failed: %s (%s:%d)"'


def _code():
    files = [f for pattern in ('*.h', '*.hip', '*.cpp', os.path.join('*', '*.hip'))
             for f in glob.glob(os.path.join(CSRC, pattern))]
    assert set(SOURCES.values()) < set(files) and len(files) == len(set(files))
    return {os.path.relpath(f, CSRC): csrc_scan.strip_comments(open(f).read()) for f in files}


def _definitions(code, name):
    # a definition: the name after a type, its parameter list, then a body
    define = re.compile(r'[\w>&*]\s+%s\s*\([^;{}()]*\)\s*\{' % name)
    return {f: len(define.findall(txt)) for f, txt in code.items() if define.search(txt)}


def test_every_shared_part_is_defined_once_and_in_its_header():
    code = _code()
    for name, header in (('clamp_row', 'ragged_rows.h'), ('cut_span', 'ragged_rows.h'), ('sq', 'sumsq_f64.h'),
                         ('sq4', 'sumsq_f64.h'), ('slice_sumsq', 'sumsq_f64.h'), ('wave_sums', 'sumsq_f64.h'),
                         ('adam_one', 'adam_one.h'), ('set_error', 'ext_core.h'),
                         (r'DANET_EXT_CAT\(danet_, DANET_EXT, _last_error\)', 'ext_core.h'),
                         (r'DANET_EXT_CAT\(danet_, DANET_EXT, _abi_version\)', 'ext_core.h')):
        assert _definitions(code, name) == {header: 1}, name
    # the named exception: the core library's own error path, csrc/error.cpp behind csrc/common.h
    assert _definitions(code, r'\w+_set_error') == {'error.cpp': 1}
    assert _definitions(code, r'danet_\w*(last_error|abi_version)') == {'error.cpp': 2}
    for text, where in ((LAUNCH_FAILED, {'ext_core.h': 1}), ('failed: %s (%s:%d)', {'ext_core.h': 1, 'common.h': 1}),
                        ('thread_local char', {'ext_core.h': 1, 'error.cpp': 1}),
                        ('typedef float f32x4 ', {'ext_core.h': 1, 'common.h': 1}),
                        ('define CHECK_ARG(', {'ext_core.h': 1}), ('define CHECK_LAUNCH(', {'ext_core.h': 1})):
        assert {f: txt.count(text) for f, txt in code.items() if text in txt} == where, text
    # the butterfly over the wave of the sum of squares (wave_metric.h keeps its own tree, block_sum_f64, pinned)
    assert [f for f, txt in code.items() if '__shfl_xor(acc, m, 64)' in txt] == ['sumsq_f64.h']


def test_every_extension_source_includes_the_host_core_after_naming_its_prefix():
    code = _code()
    for name, path in SOURCES.items():
        txt = code[os.path.relpath(path, CSRC)]
        want = ('#include "danet_%s_hip.h"\n#define DANET_EXT %s\n#define DANET_EXT_UPPER %s\n#include "ext_core.h"\n'
                % (name, name, name.upper()))
        assert txt.count(want) == 1, name
        assert not re.search(r'\b%s_set_error\b|\b%s_CHECK_(ARG|LAUNCH)\b' % (name, name.upper()), txt), name
        assert 'CHECK_LAUNCH();' in txt and 'CHECK_ARG(' in txt, name          # dropout, speed and reverb too
        assert '= hipGetLastError()' not in txt and 'g_err' not in txt, name       # no launch check by hand
    for name in ('common.h', 'pointwise.hip'):
        assert 'ext_core.h' not in code[name], name                            # the core library keeps its own
    assert '#include "adam_one.h"' in code['pointwise.hip'] and code['pointwise.hip'].count('adam_one(') == 2
    assert '#include "adam_one.h"' in code[os.path.join('gclip', 'gclip.hip')]
    for f in ('mix/mix.hip', 'level/level.hip'):
        assert re.search(r'struct \w+Args : RowTable \{', code[f]) and 'clamp_row(a, u, off, len);' in code[f], f
    assert code['speed/speed.hip'].count('cut_span(') == 2 and code['reverb/reverb.hip'].count('cut_span(') == 1
    for f in ('mix/mix.hip', 'gclip/gclip.hip'):
        assert code[f].count('slice_sumsq(') == 1 and code[f].count('four_waves(part)') == 1, f


def test_the_build_record_of_every_user_of_a_shared_header_lists_it():
    build = importlib.import_module('danet-tensorflow_amd._build')
    for name, path in SOURCES.items():
        spec = getattr(build, name.upper())
        assert spec.headers[0] == os.path.join(ROOT, 'include', 'danet_%s_hip.h' % name), name
        used = csrc_scan.shared_headers(open(path).read())
        assert os.path.join(CSRC, 'ext_core.h') in used, name
        assert set(used) <= set(spec.headers), (name, used)
        # and no record names a shared header its source does not include
        assert {h for h in spec.headers if os.path.dirname(h) == CSRC} == set(used), name
    # the core library picks up csrc/*.h, adam_one.h among them
    assert os.path.join(CSRC, '*.h') in build.CORE.headers
