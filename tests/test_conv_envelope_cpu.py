'''
CPU checks (no GPU) of the case tables of tests/test_gpu_conv_envelope.py: the instantiation
matrix runs every <KS, NT> kernel include/danet_conv_hip.h's library compiles, pool at every NT,
depth-to-space at every NT with both k, and channel counts that make both K walks wrap; the slab
cases get the slab counts their comments promise (danet_conv_workspace_bytes answers without a
GPU).  A later edit of the tables cannot silently drop coverage.
'''
import numpy as np

import test_gpu_conv_envelope as env

ALL = {(k, nt) for k in (3, 5) for nt in (1, 2, 4)}
CHANNELS = {1, 2, 3, 5, 7, 12, 16, 17, 20, 31, 32, 33, 48, 63, 64}


def ntiles(n):
    '''csrc/conv/conv.hip: the N tiles of 16 a kernel is compiled for'''
    return 1 if n <= 16 else (2 if n <= 32 else 4)


def test_matrix_runs_every_instantiation():
    M = env.MATRIX
    assert all(mode in ('plain', 'pool', 'd2s') and k in (3, 5) for _, _, k, mode in M)
    assert all(ci in CHANNELS and co in CHANNELS for ci, co, _, _ in M)
    fwd = {(k, ntiles(co)) for ci, co, k, mode in M}           # wgrad: the same <k, ntiles(Cout)>
    dgrad = {(k, ntiles(ci)) for ci, co, k, mode in M}
    assert fwd == ALL, ALL - fwd
    assert dgrad == ALL, ALL - dgrad
    pool = {ntiles(co) for ci, co, k, mode in M if mode == 'pool'}
    assert pool == {1, 2, 4}, pool
    d2s = {(k, ntiles(co)) for ci, co, k, mode in M if mode == 'd2s'}
    assert d2s == ALL, ALL - d2s
    assert all(co % 4 == 0 for ci, co, k, mode in M if mode == 'd2s')


def test_matrix_walks_k_with_wrapping_channel_counts():
    '''the fwd walk steps ci by 4 over Cin, the dgrad walk co by 4 over Cout: a count that is not a
    multiple of 4 changes tap mid-step, one below 4 wraps more than once in a step'''
    M = env.MATRIX
    for pick in (lambda c: c[0], lambda c: c[1]):
        assert {c[2] for c in M if pick(c) % 4} == {3, 5}
        assert {c[2] for c in M if pick(c) < 4} == {3, 5}
    assert any(ci == 64 and k == 5 for ci, co, k, mode in M)  # the deepest K


def test_slab_cases_get_their_slab_counts():
    from danet_amd import _lib
    short_last = []
    for Cin, Cout, k, mode, B, T, F, nslab in env.SLABS:
        d = env.desc(B, Cin, Cout, T, F, k, mode)
        Mtot = Cin * k * k + 1
        assert _lib.conv_ws_bytes(_lib.CONV_WS_BWD_WEIGHT, d) == nslab * Mtot * Cout * 4
        # wgrad_plan restated: the last slab holds fewer rows when rows_per_slab does not divide R
        R, nmt = B * T, (Mtot + 15) // 16
        rps = -(-R // max(1, 4096 // nmt))
        assert -(-R // rps) == nslab
        if nslab > 16 and nslab % 16 and R % rps:
            short_last.append((Cin, k))
    counts = [c[-1] for c in env.SLABS]
    assert 1 in counts and 16 in counts
    assert (1, 3) in short_last and (64, 5) in short_last     # nmt = 1 and nmt = 101


def test_sentinel_is_nan_poison():
    assert np.isnan(np.array(env.SENT, np.int32).view(np.float32))
