'''
CPU side of tests/test_gpu_lstm_fwd_fx_parts.py: the FX_STEP_PATH parts of lstm_fwd_fx_kernel change no entry point,
so the dynamic symbol table of the core library is the one recorded with the golden hashes
(tests/golden/lstm_fwd_fx_parent.json), and that file covers exactly the GPU file's case table.
'''
import json
import os
import subprocess

import lstm_layer as ll

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'lstm_fwd_fx_parent.json')


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_core_library_exports_are_unchanged():
    from danet_amd import _lib
    _lib.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exports = sorted(' '.join(l.split()[-2:]) for l in out.stdout.splitlines() if l.strip())
    want = _golden()['core_library_exports']
    assert exports == want, sorted(set(exports) ^ set(want))


def test_golden_file_covers_the_case_table():
    import test_gpu_lstm_fwd_fx_parts as tp
    cases = _golden()['cases']
    assert sorted(cases) == sorted(c.name for c, _ in tp.CASES)
    kernels = set()
    for c, kernel in tp.CASES:
        g = cases[c.name]
        assert g['dims'] == [c.B, c.T, c.D, c.H, c.ndir] and g['seed'] == c.seed and g['kernel'] == kernel
        assert ll.fx_plan(c.B, c.H, c.ndir, c.D, c.opts)['kernel'] == kernel
        for name, width in (('y', c.H), ('gates', 4 * c.H), ('cell', c.H)):
            assert [d['shape'] for d in g[name]] == [[c.T, c.B, width]] * c.ndir
            assert all(len(d['sha256']) == 64 for d in g[name])
        kernels.add(kernel)
    assert kernels == {'fx<2,1>', 'fx<4,2>', 'fx<8,3>', 'fx<8,4>'}
    # the table of the GPU file's docstring
    assert {c.T for c, _ in tp.CASES} >= {1, 2, 3, 5} and {c.B for c, _ in tp.CASES} == {17, 32}
    assert {c.H for c, _ in tp.CASES} == {20, 300, 320} and {c.D for c, _ in tp.CASES} == {20, 176, 600, 640}
    assert {c.ndir for c, _ in tp.CASES} == {1, 2} and any(c.sat and c.H == 300 for c, _ in tp.CASES)
