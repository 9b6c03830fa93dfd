'''
GPU tests of lstm_fwd_fx_kernel (csrc/lstm.hip) for the parts built behind FX_STEP_PATH: FETCH (recurrent weight
fragments straight from global memory, no LDS staging; the default), and the two that were measured with it and
removed again, ONEBAR (double-buffered `red`, one barrier per step) and HALFBLK (the half-empty last recurrent
k-block splits only its real group) -- their shapes stay, they cost a few milliseconds and pin the same kernel.
danet_lstm_fwd_fused is called directly with lstm_fwd_fused forced on, through the guarded launches of
tests/lstm_layer.py: padded leading dimensions with NaN in the gaps, sentinel guards around outputs and
workspace, status word 0.

Two checks per case:
* y, gates and cell against the float64 scan at the envelope suite's bar (1e-5 of each output's maximum, the
  float32 restatement below 1e-6);
* y, gates and cell bit for bit what the kernel BEFORE the three parts computed: their sha256 were recorded from
  that commit's library for the same seeded inputs (tests/golden/lstm_fwd_fx_parent.json: hashes and shapes
  only).  None of the parts changes a value or the order of a sum, and the kernel is bit-reproducible, so
  "results stay what they were" is an equality.

Shapes, each the smallest that can break the part named:
  T = 1, 2, 3, 5      `red`'s second buffer is first reused at the third step; an odd count ends on the other one
  B = 17, 32          ragged second row cluster | two full ones
  ndir = 1, 2
  H = 20              ragged unit group (3 workgroups, the last with 4 units); waves 2 and 3 see only padding
                      k-groups, wave 1 a group that ends at k = 20 inside it
  H = 300             odd fifth k-group; wave 3's fifth group all padding; wave 2's ends at 300 inside a group
  H = 320             nothing ragged
  D = 20, 176, 600, 640   fx<2,1> (fp32 input half), fx<4,2>, fx<8,3>, fx<8,4>
  saturated gates     one H = 300 case with pre-activations at +-20 (and beyond) through the last k-block
'''
import hashlib
import json
import os

import numpy as np
import pytest

import lstm_layer as ll
from lstm_layer import Case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lstm_fwd_fx_parent.json')
FX1 = {'lstm_fwd_fused': 1}
PAD = (8, 4, 12, 8)        # ldw, ldy, lddy, ldx beyond the row
WIDE = 0.2                 # x of the wide-input cases (see tests/test_gpu_lstm_envelope.py)

#         name                          B   T   D    H  ndir
CASES = [
    (Case('t1-h20-d20',                17,  1,  20,  20, 2, FX1, pad=PAD), 'fx<2,1>'),
    (Case('t2-h20-d20',                17,  2,  20,  20, 2, FX1), 'fx<2,1>'),
    (Case('t3-h20-d20',                17,  3,  20,  20, 2, FX1, pad=PAD), 'fx<2,1>'),
    (Case('t5-h20-d20',                17,  5,  20,  20, 2, FX1), 'fx<2,1>'),
    (Case('h20-d176-b32',              32,  3, 176,  20, 1, FX1, scale=0.5), 'fx<4,2>'),
    (Case('h20-d600',                  17,  2, 600,  20, 2, FX1, pad=PAD, scale=WIDE), 'fx<8,3>'),
    (Case('h20-d640',                  17,  3, 640,  20, 2, FX1, scale=WIDE), 'fx<8,4>'),
    (Case('h300-d20-t5',               17,  5,  20, 300, 1, FX1, pad=PAD), 'fx<2,1>'),
    (Case('h300-d176',                 17,  3, 176, 300, 2, FX1, scale=0.5), 'fx<4,2>'),
    (Case('h300-d600-b32-cfg2',        32,  3, 600, 300, 2, FX1, pad=PAD, scale=WIDE), 'fx<8,3>'),
    (Case('h300-d640-t2',              32,  2, 640, 300, 1, FX1, scale=WIDE), 'fx<8,4>'),
    (Case('h320-d176-b32',             32,  2, 176, 320, 2, FX1, pad=PAD, scale=0.5), 'fx<4,2>'),
    (Case('h320-d640',                 17,  3, 640, 320, 1, FX1, scale=WIDE), 'fx<8,4>'),
    (Case('h320-d20-t5',               17,  5,  20, 320, 2, FX1), 'fx<2,1>'),
    (Case('h300-saturated',            17,  3,  20, 300, 2, FX1, sat=True), 'fx<2,1>'),
]


def digests(case, out):
    '''{output: [per direction {shape, sha256}]} of a forward launch's CPU arrays'''
    d = {}
    for name in ('y', 'gates', 'cell'):
        d[name] = []
        for a in out[name]:
            a = np.ascontiguousarray(a, dtype=np.float32)
            d[name].append(dict(shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest()))
    return d


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('case,kernel', CASES, ids=[c[0].name for c in CASES])
def test_fused_forward_parts(case, kernel, golden):
    from danet_amd import _lib
    assert ll.fx_plan(case.B, case.H, case.ndir, case.D, case.opts)['kernel'] == kernel
    with ll.set_options(case.opts):
        assert _lib.load().danet_lstm_fwd_fused_supported(case.T, case.B, case.H, case.ndir, case.D) == 1
    if case.sat:
        gx = ll.inputs(case)['gx']
        assert float(gx[0].abs().max()) > 20 and all(bool(np.isfinite(t.numpy()).all()) for t in gx)
    out, k, f = ll.check_forward(case, fused=True)
    got, want = digests(case, out), golden[case.name]
    assert want['dims'] == [case.B, case.T, case.D, case.H, case.ndir] and want['seed'] == case.seed
    for name in ('y', 'gates', 'cell'):
        for d in range(case.ndir):
            assert got[name][d]['shape'] == want[name][d]['shape'], (name, d)
            assert got[name][d]['sha256'] == want[name][d]['sha256'], \
                '%s[%d] is not bit for bit what the kernel before FX_STEP_PATH computed\n%s' % (name, d, case.describe())
