'''
Ops of the DANet hot path, MI355X-native: thin tensor-level wrappers over the
C ABI (include/danet_hip.h) plus the `torch.autograd.Function`s that let
PyTorch-ROCm drive backward.  Mirrors the roles of the reference's
`app/ops.py` (lyr_linear, lyr_lstm_flat, combinations, pit_mse_loss,
batch_snr) and of `Model.lyr_lstm` (main.py:76-132); names and argument meaning
follow the reference where a counterpart exists.

Everything here requires the HIP library and a GPU; nothing falls back to CPU.
'''
import ctypes
import itertools
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr, check


def _L():
    return _lib.load()


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32, (t.device, t.dtype)
    return t


def _ws(nbytes, dev):
    w = _lib.workspace(nbytes, dev)
    return w, w.numel()


def _ptrs(ts):
    '''the C array of the tensors' device pointers'''
    return (_lib.c_p * len(ts))(*[ptr(t) for t in ts])


# ---------------------------------------------------------------------------
# raw wrappers (no autograd)
# ---------------------------------------------------------------------------
# stream-K schedule (danet_gemm_f32_streamk*: persistent workgroups, whole tiles data-parallel,
# the ragged last round cut along K, deterministic in-kernel fix-up) for single products on the
# critical path -- bit mask: 1 = dYc / unidirectional dX, 2 = output projection, 4 = the
# K-concatenated dX of a BiLSTM layer.  Default 5.  Round 3, in-step at cfg 2 (us per launch /
# ms per step): dX 133 -> 117 (3.273 -> 3.241), dYc 142 -> 125 (-> 3.265), both 3.228; the
# output projection (672 tiles, K = 600) LOSES on it (126 -> 132: two workgroups per CU instead
# of three, and 160 of its tiles need a fix-up) and stays on the tile kernel.
STREAMK = _lib.expert('streamk', 5)


def gemm(A, B, C, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None, beta=0.0,
         max_workgroups=0, streamk=False, tag=None, stop_event=None):
    '''C[M,N] = op(A) op(B) (+bias) (+beta*C) on the fp32 matrix cores.
    A, B, C are tensors whose data_ptr() is element (0,0); ld* in elements.
    max_workgroups > 0 caps the launch (persistent workgroups); streamk selects the
    stream-K schedule (for a product that has the GPU to itself).'''
    L = _L()
    if streamk:
        need = _lib.ws_bytes(_lib.WS_GEMM_STREAMK, M, N, K)
        # dedicated (zero-initialised, never shared) scratch: it holds the stream-K
        # hand-off flags, which must only ever contain earlier launch sequence numbers
        w = _lib.workspace(need, C.device, tag='gemm_sk')
        with _lib.timed('gemm_f32', tag):
            if stop_event is not None:
                stop_event.arm()
            check(L.danet_gemm_f32_streamk(_lib.stream(), int(transA), int(transB), M, N, K,
                                           ptr(_f32(A)), lda, ptr(_f32(B)), ldb, ptr(_f32(C)), ldc,
                                           ptr(bias), float(beta), ptr(w), w.numel()))
            if stop_event is not None:
                stop_event.attached = True
        return C
    need = _lib.ws_bytes(_lib.WS_GEMM, M, N, K)
    w, wn = _ws(need, C.device)
    with _lib.timed('gemm_f32', tag):
        check(L.danet_gemm_f32(_lib.stream(), int(transA), int(transB), M, N, K,
                                  ptr(_f32(A)), lda, ptr(_f32(B)), ldb, ptr(_f32(C)), ldc,
                                  ptr(bias), float(beta), ptr(w), wn, int(max_workgroups)))
    return C


def gemm_kcat(A1, lda1, B1, ldb1, K1, A2, lda2, B2, ldb2, K2, C, M, N, ldc,
              transA=False, transB=False, bias=None, beta=0.0, tag=None, streamk=False,
              stop_event=None):
    '''C[M,N] = op(A1) op(B1) + op(A2) op(B2) (+bias) (+beta*C) in one launch.
    streamk: the hybrid stream-K schedule (no slabs / reduce kernel; K1 % 16 == 0)
    stop_event: a ForkEvent that completes with this launch (stream-K path only)'''
    L = _L()
    if streamk and K1 % 16 == 0:
        w = _lib.workspace(_lib.ws_bytes(_lib.WS_GEMM_STREAMK, M, N, K1 + K2), C.device,
                           tag='gemm_sk')
        with _lib.timed('gemm_f32', tag):
            if stop_event is not None:
                stop_event.arm()
            check(L.danet_gemm_f32_streamk_kcat(_lib.stream(), int(transA), int(transB), M, N,
                                                K1, ptr(_f32(A1)), lda1, ptr(_f32(B1)), ldb1,
                                                K2, ptr(_f32(A2)), lda2, ptr(_f32(B2)), ldb2,
                                                ptr(_f32(C)), ldc, ptr(bias), float(beta),
                                                ptr(w), w.numel()))
            if stop_event is not None:
                stop_event.attached = True
        return C
    # (no stream-K: two accumulating products on the tile kernel)
    gemm(A1, B1, C, M, N, K1, lda1, ldb1, ldc, transA=transA, transB=transB, bias=bias, beta=beta,
         tag=tag)
    gemm(A2, B2, C, M, N, K2, lda2, ldb2, ldc, transA=transA, transB=transB, beta=1.0, tag=tag)
    return C


# fp32 products on the bf16 matrix cores for products whose B operand is a weight (the output
# projection, dYc, dX; csrc/gemm_x6.hip): the weight is split into three bf16 pieces and laid out in
# the matrix instruction's operand order ONCE per optimizer step (`repack_weights`), the activation
# is split inside the kernel.  Same accuracy as the exact-fp32 kernels (six of the nine piece
# products), 1.6-1.8 x their speed at cfg 2.  DANET_GEMM_X6=0: the exact-fp32 kernels everywhere.
GEMM_X6 = int(__import__('os').environ.get('DANET_GEMM_X6', '3'))    # bit 0: weight products, bit 1: weight gradients


class _PackedWeight(object):
    __slots__ = ('W', 'N', 'K', 'sn', 'sk', 'lo', 'hi', 'out', 'stale', 'version', 'unused')

    def __init__(self, W, N, K, sn, sk):
        self.W, self.N, self.K, self.sn, self.sk = W, N, K, sn, sk
        self.lo = W.data_ptr()
        self.hi = self.lo + 4 * ((N - 1) * sn + (K - 1) * sk + 1)
        self.out = torch.empty(_lib.ws_bytes(_lib.WS_GEMM_PACK, N, K), dtype=torch.uint8,
                               device=W.device)
        self.stale, self.version, self.unused = True, -1, 0


_packs = {}      # device -> {(ptr, N, K, sn, sk): _PackedWeight}


def _pack_now(pws):
    arr = (_lib.GemmPack * len(pws))()
    for i, pw in enumerate(pws):
        arr[i].src, arr[i].stride_n, arr[i].stride_k = pw.W.data_ptr(), pw.sn, pw.sk
        arr[i].N, arr[i].K = pw.N, pw.K
        arr[i].out, arr[i].out_bytes = pw.out.data_ptr(), pw.out.numel()
    check(_L().danet_gemm_pack_weights(_lib.stream(), len(pws), arr))
    for pw in pws:
        pw.stale, pw.version = False, pw.W._version


def packed_weight(W, N, K, sn, sk):
    '''the operand-layout copy of the weight B(n, k) = W.flat[n * sn + k * sk] (W: a tensor whose
    data_ptr() is B(0, 0)), packed now if the weight has changed since its last pack'''
    reg = _packs.setdefault(_dev_key(W.device), {})
    key = (W.data_ptr(), N, K, sn, sk)
    pw = reg.get(key)
    if pw is None:
        pw = reg[key] = _PackedWeight(W, N, K, sn, sk)
    pw.unused = 0
    if pw.stale or pw.version != W._version:
        _pack_now([pw])
    return pw.out


def weights_written(t):
    '''a kernel of this library has written the parameter range `t` (torch's version counter
    does not see such writes): packs that overlap it are stale'''
    reg = _packs.get(_dev_key(t.device))
    if reg:
        lo = t.data_ptr()
        hi = lo + 4 * t.numel()
        for pw in reg.values():
            if pw.lo < hi and lo < pw.hi:
                pw.stale = True


def repack_weights(dev):
    '''re-pack every stale registered weight of the device in ONE launch on the current stream
    (the end of an optimizer step); packs nobody has asked for in 8 rounds are dropped'''
    reg = _packs.get(_dev_key(dev))
    if not reg:
        return
    todo = []
    for key in list(reg):
        pw = reg[key]
        pw.unused += 1
        if pw.unused > 8:
            del reg[key]
        elif pw.stale or pw.version != pw.W._version:
            todo.append(pw)
    if todo:
        _pack_now(todo)


def drop_packs(dev):
    '''forget every packed weight of the device (its parameters have moved)'''
    _packs.pop(_dev_key(dev), None)


def _x6_ok(M, N, *pairs):
    if not (GEMM_X6 & 1):
        return False
    for A, lda, K in pairs:
        if K % 4 or lda % 4 or lda < K or A.data_ptr() % 16 or M * lda >= (1 << 29):
            return False
    return True


def _x6_tn_ok(problems, K):
    if not (GEMM_X6 & 2) or len(problems) > 6:
        return False
    for pr in problems:
        A, lda, B, ldb = pr[:4]
        if len(pr) > 9 and pr[9] is not None:
            return False
        if lda % 4 or ldb % 4 or A.data_ptr() % 16 or B.data_ptr() % 16 or \
                K * max(lda, ldb) >= (1 << 29):
            return False
    return True


def gemm_w(A, lda, W, sn, sk, C, M, N, K, ldc, tag=None, stop_event=None,
           A2=None, lda2=0, W2=None, K2=0, sn2=None, sk2=None, bias=None):
    '''C[M,N] = A B^T (+ A2 B2^T) with B(n, k) = W.flat[n * sn + k * sk] a (packed) weight, on the
    bf16 matrix cores with fp32 accuracy (B2 with strides sn2 / sk2, default: B's).  The caller
    has checked `_x6_ok`.'''
    L = _L()
    p1 = packed_weight(W, N, K, sn, sk)
    p2 = packed_weight(W2, N, K2, sn if sn2 is None else sn2, sk if sk2 is None else sk2) if K2 else None
    need = _lib.ws_bytes(_lib.WS_GEMM_X6, M, N, K, K2)
    # dedicated (zero-initialised, never shared) scratch: its first 16 KB are the K-slice tickets
    w = _lib.workspace(need, C.device, tag='gemm_x6')
    wn = w.numel()
    with _lib.timed('gemm_x6', tag):
        if stop_event is not None:
            stop_event.arm()
        check(L.danet_gemm_x6(_lib.stream(), M, N, K, ptr(_f32(A)), lda, ptr(p1),
                              K2, ptr(_f32(A2)) if K2 else None, lda2, ptr(p2) if K2 else None,
                              ptr(_f32(C)), ldc, ptr(bias), ptr(w), wn))
        if stop_event is not None:
            stop_event.attached = True
    return C


def _x6_tn_tiles(M, N):
    '''128 x 128 tiles of one product of danet_gemm_x6_tn_grouped (include/danet_hip.h): 1..4 rows
    beyond a multiple of 128 are tail rows, not a tile row (N a multiple of 4)'''
    tail = M % 128
    rows = M - tail if (M > 128 and 1 <= tail <= 4 and N % 4 == 0) else M
    return ((rows + 127) // 128) * ((N + 127) // 128)


def gemm_group(problems, K, transA=False, transB=False, max_workgroups=0):
    '''up to 6 products sharing K and the transpose flags as ONE stream-K launch.
    problems: list of (A, lda, B, ldb, C, ldc, M, N, beta) with tensors whose data_ptr()
    is element (0,0); an optional 10th entry is the bias vector.'''
    L = _L()
    x6 = transA and not transB and _x6_tn_ok(problems, K)
    arr = (_lib.GemmProblem * len(problems))()
    keep = []
    for i, pr in enumerate(problems):
        A, lda, B, ldb, C, ldc, M, N, beta = pr[:9]
        bias = pr[9] if len(pr) > 9 else None
        A, B, C = _f32(A), _f32(B), _f32(C)
        keep += [A, B, C, bias]
        arr[i].A, arr[i].lda, arr[i].B, arr[i].ldb = ptr(A), lda, ptr(B), ldb
        arr[i].C, arr[i].ldc, arr[i].M, arr[i].N = ptr(C), ldc, M, N
        arr[i].bias, arr[i].beta = ptr(bias), float(beta)
    dev = problems[0][4].device
    if x6:
        # both operands split inside the kernel (csrc/gemm_x6.hip, TN section); not persistent:
        # `max_workgroups` does not apply
        need = _lib.ws_bytes(_lib.WS_GEMM_X6_TN, sum(pr[6] * pr[7] for pr in problems),
                             sum(_x6_tn_tiles(pr[6], pr[7]) for pr in problems), K)
        w = _lib.workspace(need, dev, tag='gemm_x6_tn') if need else None
        with _lib.timed('gemm_x6_tn_group'):
            check(L.danet_gemm_x6_tn_grouped(_lib.stream(), K, len(problems), arr, ptr(w),
                                             w.numel() if w is not None else 0))
        return
    w = _lib.workspace(_lib.ws_bytes(_lib.WS_GEMM_STREAMK, 0, 0, K), dev, tag='gemm_sk')
    with _lib.timed('gemm_f32_group'):
        check(L.danet_gemm_f32_streamk_grouped(_lib.stream(), int(transA), int(transB), K,
                                               len(problems), arr, int(max_workgroups),
                                               ptr(w), w.numel()))


# weight gradients of a BiLSTM layer as one grouped stream-K launch (DANET_EXPERT grouped_dw=0:
# four split-K launches + reduce kernels)
GROUPED_DW = _lib.expert('grouped_dw', 1)
GROUPED_DW_WGS = _lib.expert('grouped_dw_wgs', 256)
GROUPED_GX = _lib.expert('grouped_gx', 512)   # grid of the grouped gx launch (0: two launches on two streams)


def colsum(A, M, N, lda, out, beta=0.0):
    L = _L()
    w, wn = _ws(_lib.ws_bytes(_lib.WS_COLSUM, M, N), out.device)
    check(L.danet_colsum_f32(_lib.stream(), M, N, ptr(_f32(A)), lda, ptr(out), float(beta),
                             ptr(w), wn))
    return out


def center(x, B, T, D, in_layout, ld_in, out, out_layout, ld_out):
    '''out[b] = x[b] - mean(x[b]) with an optional layout switch; returns means [B]'''
    L = _L()
    scratch = torch.empty(_lib.ws_bytes(_lib.WS_CENTER_MEAN, B) // 4, dtype=torch.float32, device=x.device)
    check(L.danet_center(_lib.stream(), B, T, D, ptr(_f32(x)), in_layout, ld_in,
                         ptr(out), out_layout, ld_out, ptr(scratch)))
    return scratch[:B]


def frontend(src, want_phase=False, want_mix=False):
    '''main.py:233-240.  src complex64 [B,C,T,F] ->
    dict(src_pwr [B,C,T,F], mix_pwr, mix_log [B,T,F], phasor [B,T,F,2], ...)'''
    assert src.is_cuda and src.dtype == torch.complex64
    src = src.contiguous()
    B, C, T, F = src.shape
    N = T * F
    dev = src.device
    out = dict(
        src_pwr=torch.empty(B, C, T, F, device=dev),
        mix_pwr=torch.empty(B, T, F, device=dev),
        mix_log=torch.empty(B, T, F, device=dev),
        phasor=torch.empty(B, T, F, 2, device=dev))
    phase = torch.empty(B, T, F, device=dev) if want_phase else None
    mix = torch.empty(B, T, F, dtype=torch.complex64, device=dev) if want_mix else None
    check(_L().danet_frontend_fwd(
        _lib.stream(), B, C, N, ptr(torch.view_as_real(src)), ptr(out['mix_pwr']),
        ptr(out['mix_log']), ptr(out['phasor']), ptr(phase), ptr(out['src_pwr']),
        ptr(torch.view_as_real(mix)) if mix is not None else None))
    if want_phase:
        out['phase'] = phase
    if want_mix:
        out['mix'] = mix
    return out


def noise_frontend(src, noise, gain=None, want_mix=False):
    '''ops.frontend over the mixture of the C sources and one more component that is not a target
    (danet_noise_frontend_fwd, include/danet_noise_hip.h): mixture = sum of the sources + fl(gain[b] * noise),
    ONE launch.  src complex64 [B,C,T,F], noise complex64 [B,T,F], gain float32 [B] or None (= 1), all contiguous
    on one device -> the dict of ops.frontend: src_pwr [B,C,T,F] (the clean sources'), mix_pwr, mix_log [B,T,F],
    phasor [B,T,F,2], and mix complex64 [B,T,F] when asked.  On the extension library libdanet_noise_hip.so,
    mapped at the first call: a run with NOISE_DIR null never gets here.'''
    assert src.is_cuda and src.dtype == torch.complex64 and src.dim() == 4 and src.is_contiguous(), \
        (src.device, src.dtype, src.shape)
    B, C, T, F = src.shape
    assert noise.dtype == torch.complex64 and noise.device == src.device and tuple(noise.shape) == (B, T, F) \
        and noise.is_contiguous(), (noise.device, noise.dtype, noise.shape)
    if gain is not None:
        assert gain.dtype == torch.float32 and gain.device == src.device and tuple(gain.shape) == (B,) \
            and gain.is_contiguous(), (gain.device, gain.dtype, gain.shape)
    dev = src.device
    out = dict(
        src_pwr=torch.empty(B, C, T, F, device=dev),
        mix_pwr=torch.empty(B, T, F, device=dev),
        mix_log=torch.empty(B, T, F, device=dev),
        phasor=torch.empty(B, T, F, 2, device=dev))
    mix = torch.empty(B, T, F, dtype=torch.complex64, device=dev) if want_mix else None
    with _lib.timed('noise_frontend'):
        _lib.noise_check(_lib.load_noise().danet_noise_frontend_fwd(
            _lib.stream(), B, C, T * F, ptr(torch.view_as_real(src)), ptr(torch.view_as_real(noise)), ptr(gain),
            ptr(out['mix_pwr']), ptr(out['mix_log']), ptr(out['phasor']), ptr(out['src_pwr']),
            ptr(torch.view_as_real(mix)) if mix is not None else None))
    if want_mix:
        out['mix'] = mix
    return out


def reattach_phase(sep_pwr, phasor, perm_idx=None):
    '''main.py:281-284 / :330-335 (with the permutation gather of :293-306)'''
    B, C, T, F = sep_pwr.shape
    out = torch.empty(B, C, T, F, dtype=torch.complex64, device=sep_pwr.device)
    check(_L().danet_reattach_phase(
        _lib.stream(), B, C, T * F, ptr(_f32(sep_pwr.contiguous())), ptr(phasor),
        ptr(perm_idx), ptr(torch.view_as_real(out))))
    return out


def combinations(s_data, subset_size, total_size=None, name=None):
    '''reference app/ops.py:273-292: gather rows by itertools.combinations'''
    if total_size is None:
        total_size = s_data.shape[0]
    combs = torch.tensor(list(itertools.combinations(range(total_size), subset_size)),
                         device=s_data.device)
    return s_data[combs]


def stft(x, window, fft_size, fft_stride):
    '''x float32 [n_sig, Ls] (or [Ls]) -> complex64 [n_sig, T, F]
    (app/utils.py:117-122).  Raises ValueError when Ls < fft_size like scipy.'''
    squeeze = x.dim() == 1
    if squeeze:
        x = x[None]
    x = _f32(x.contiguous())
    n_sig, Ls = x.shape
    L = _L()
    T = L.danet_stft_num_frames(Ls, fft_size, fft_stride)
    if T < 0:
        raise ValueError('window is longer than input signal')
    F = fft_size // 2 + 1
    out = torch.empty(n_sig, T, F, dtype=torch.complex64, device=x.device)
    check(L.danet_stft(_lib.stream(), n_sig, Ls, fft_size, fft_stride, ptr(x),
                       ptr(_f32(window)), ptr(torch.view_as_real(out))))
    return out[0] if squeeze else out


def istft(X, stride, window):
    '''utils.istft (app/utils.py:53-75).  X complex64 [n_sig, T, F] or [T, F]
    -> float64 [n_sig, T*stride]'''
    squeeze = X.dim() == 2
    if squeeze:
        X = X[None]
    assert X.dtype == torch.complex64 and X.is_cuda
    X = X.contiguous()
    n_sig, T, F = X.shape
    N = (F - 1) * 2
    L = _L()
    out = torch.empty(n_sig, T * stride, dtype=torch.float64, device=X.device)
    w, wn = _ws(_lib.ws_bytes(_lib.WS_ISTFT, n_sig, T, N, stride), X.device)
    check(L.danet_istft(_lib.stream(), n_sig, T, N, stride, ptr(torch.view_as_real(X)),
                        ptr(_f32(window)), ptr(out), ptr(w), wn))
    return out[0] if squeeze else out


# ---- the wrappers of the extension libraries: what they share ------------------------------------------
# A new library's wrapper checks every tensor it hands to the library with _chk (or takes its `out` from _out, which
# allocates or checks), and a chain that keeps intermediates between launches gets them from _scratch: it lists its
# parts as [(name, shape, dtype)] in the order of the header's layout, names the library's *_workspace_bytes, and keeps
# a dict of its own as the per-shape cache.  Nothing else carves a buffer or keys a cache by (device, stream).
def _dev_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _stride(fft_stride):
    '''the hop of the STFT: hparams.FFT_STRIDE unless given'''
    from .hparams import hparams
    return int(hparams.FFT_STRIDE if fft_stride is None else fft_stride)


def _chk(name, t, dtype, shape=None, numel=None, dim=None, dev=None, contiguous=True, cuda=True, optional=False):
    '''t, an argument called `name`, is a tensor of `dtype` and, where asked, of this exact shape, numel, dim and
    device; contiguous and on a GPU unless the call says otherwise; None only where `optional` -> t, else an
    AssertionError naming the argument, what was wanted and what was got'''
    if t is None and optional:
        return t
    if not (torch.is_tensor(t) and t.dtype == dtype and (t.is_cuda or not cuda)
            and (shape is None or tuple(t.shape) == tuple(shape)) and (numel is None or t.numel() == numel)
            and (dim is None or t.dim() == dim) and (dev is None or t.device == dev)
            and (not contiguous or t.is_contiguous())):
        want = [str(dtype)] + ['%s %s' % kv for kv in (('shape', shape if shape is None else tuple(shape)),
                                                       ('numel', numel), ('dim', dim), ('on', dev)) if kv[1] is not None]
        got = '%s %s, strides %s, on %s' % (t.dtype, tuple(t.shape), t.stride(), t.device) if torch.is_tensor(t) else repr(t)
        raise AssertionError('%s: want %s%s%s, got %s' % (name, ', '.join(want), ', contiguous' if contiguous else '',
                                                          ', on a GPU' if cuda else '', got))
    return t


def _out(name, out, shape, dtype, dev):
    '''`out`, checked to be of this shape and dtype on `dev`, or a fresh tensor when it is None'''
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    return _chk(name, out, dtype, shape, dev=dev)


def _result(B, k, dev, flags=False, count=False):
    '''the tensors a finalize launch writes for a batch of B utterances and k figures: (per_utt float64 [B, k],
    perm_idx int32 [B], [flags int32 [B],] means float64 [k], [count int32 [1]])'''
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    return (torch.empty(B, k, dtype=torch.float64, device=dev), i32(B)) + ((i32(B),) if flags else ()) \
        + (torch.empty(k, dtype=torch.float64, device=dev),) + ((i32(1),) if count else ())


def _check_result(per_utt, perm_idx, flags, means, k):
    '''the (per_utt, perm_idx, flags, means) of a batch of any size, as _result lays them out -> its rows B_all'''
    B_all = per_utt.shape[0]
    _chk('per_utt', per_utt, torch.float64, (B_all, k), cuda=False)
    _chk('perm_idx', perm_idx, torch.int32, (B_all,), cuda=False)
    _chk('flags', flags, torch.int32, (B_all,), cuda=False)
    _chk('means', means, torch.float64, numel=k, cuda=False)
    return B_all


def _group(B, limit, bytes_of):
    '''the most utterances, at most B and limit // bytes_of(1) and at least one, whose scratch bytes_of(g) stays within
    `limit`'''
    g = max(1, min(int(B), limit // bytes_of(1)))
    while g > 1 and bytes_of(g) > limit:
        g -= 1
    return g


def _carve(buf, parts):
    '''({name: view}, end): the parts [(name, shape, dtype)] laid into the uint8 buffer `buf` in their order, each at
    the next multiple of 256 bytes, and the offset behind the last one, rounded up likewise.  buf None: no views, only
    the end.  Works on any device.'''
    views, off = {}, 0
    for name, shape, dtype in parts:
        n = int(np.prod(shape)) * dtype.itemsize
        if buf is not None:
            views[name] = buf[off:off + n].view(dtype).view(shape)
        off += (n + 255) & ~255
    return views, off


def _scratch(tag, cache, dims, parts, nbytes, dev, flat=False):
    '''(buffer, {name: view}), or with `flat` (buffer, view, view, ...): the parts() one shape `dims` cuts out of the
    grow-only scratch `tag` of this (device, stream), cached in `cache` per (device, stream, shape); a hit returns the
    cached tuple itself.  A hit counts only while its buffer is still the one _lib.workspace holds: a larger shape may
    have replaced it.  nbytes(): the library's size of the layout, which the carve must end at; None where the layout
    is the caller's own and the carve's end is the size.'''
    key = (_dev_index(dev), torch.cuda.current_stream().cuda_stream) + tuple(dims)
    hit = cache.get(key)
    if hit is not None and _lib._ws.get(key[:2] + (tag,)) is hit[0]:
        return hit
    want = None if nbytes is None else nbytes()            # first: the library refuses a shape outside its envelope
    parts = parts()
    end = _carve(None, parts)[1]
    assert want is None or end == want, (tag, end, want)
    buf = _lib.workspace(end, dev, tag)
    if len(cache) >= 64:
        cache.clear()
    views = _carve(buf, parts)[0]
    hit = cache[key] = (buf,) + tuple(views.values()) if flat else (buf, views)
    return hit


# ---- ragged-batch STFT of the wavdir dataset (include/danet_prep_hip.h) ----------------------------
# On the extension library libdanet_prep_hip.so, mapped at the first call.  ops.stft above stays the
# front-end of every other path.
PREP_DESC_DTYPE = np.dtype([('offset', '<i8'), ('length', '<i8'), ('pad_left', '<i4'), ('reserved', '<i4')])
_prep_plans = {}         # (device index, N, window bytes) -> plan tensor
_prep_plans_fast = {}    # (device index, N, window data_ptr, window version) -> (window, plan)


def _desc_table(who, dtype_name, desc, validate, device):
    '''the descriptor table of `who` -> (device tensor, rows): a record array of the dtype named `dtype_name` goes
    through validate(desc) and is uploaded; a device tensor of rows of that size is the caller's to have validated'''
    dtype = globals()[dtype_name]
    if not torch.is_tensor(desc):
        desc = np.asarray(desc)
        if desc.dtype != dtype:
            raise TypeError('%s: desc must be a %s record array or a device tensor' % (who, dtype_name))
        validate(desc)
        desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8).copy()).to(device)
    row = dtype.itemsize
    assert desc.is_cuda and desc.is_contiguous() and (desc.numel() * desc.element_size()) % row == 0
    return desc, desc.numel() * desc.element_size() // row


def _c64_row_pitch(t, F):
    '''the row pitch, in complex elements, of a complex64 [n_utt, t_count, >= F] view whose last dimension is
    contiguous and whose utterances lie t_count rows apart'''
    n_utt, t_count = t.shape[:2]
    ld = t.stride(1) if t_count > 1 else max(t.stride(1), F)
    assert t.stride(2) == 1 and (n_utt == 1 or t.stride(0) == t_count * ld), t.stride()
    return ld


def _row_tables(who, pool, offsets, lengths, max_len):
    '''the (offsets, lengths, max_len) of the rows of `pool` as `who` launches them: host sequences are validated
    (a row outside the pool is a ValueError) and uploaded, max_len taken from them when not given; device tensors
    are the caller's to have validated and need max_len'''
    if not torch.is_tensor(offsets):
        offsets, lengths = np.asarray(offsets, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
        if offsets.shape != lengths.shape or offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError('%s: offsets and lengths must be two vectors of one length >= 1' % who)
        _check_source_spans(who, offsets, lengths, pool.numel(), 0)
        if max_len is None:
            max_len = int(lengths.max())
        offsets, lengths = torch.from_numpy(offsets).to(pool.device), torch.from_numpy(lengths).to(pool.device)
    if max_len is None:
        raise ValueError('%s: device tables need max_len' % who)
    return offsets, lengths, max_len


def _check_source_spans(who, so, sl, src_len, min_len=1):
    '''ValueError naming the first row [so, so + sl) that is shorter than min_len or outside a pool of src_len'''
    bad = np.nonzero((so < 0) | (sl < min_len) | (so + sl > src_len))[0]
    if len(bad):
        u = int(bad[0])
        raise ValueError('%s: utterance %d [%d, %d) is outside the pool of %d samples'
                         % (who, u, so[u], so[u] + sl[u], src_len))


def _spans_apart(lo, hi):
    '''no two of the spans [lo, hi) share a sample'''
    order = np.argsort(lo, kind='stable')
    return not np.any(lo[order][1:] < hi[order][:-1])


def prep_num_frames(n_samples, fft_size, fft_stride):
    '''frames of an n_samples waveform (danet_prep_num_frames); ValueError when it is shorter than the window'''
    T = _lib.load_prep().danet_prep_num_frames(int(n_samples), fft_size, fft_stride)
    if T < 0:
        raise ValueError('window is longer than input signal')
    return T


def prep_desc(offsets, lengths, pad_left, T_out, pool_len, fft_size, fft_stride, out=None):
    '''the validated descriptor table of one ragged batch as a numpy record array (PREP_DESC_DTYPE; into
    `out` when given).  Everything the kernel would have to clamp is a ValueError HERE, before any
    upload or launch: an utterance outside the pool, shorter than the window, or placed beyond T_out.'''
    n = len(offsets)
    d = np.zeros(n, PREP_DESC_DTYPE) if out is None else out
    assert d.dtype == PREP_DESC_DTYPE and d.shape == (n,)
    for u in range(n):
        o, l, p = int(offsets[u]), int(lengths[u]), int(pad_left[u])
        if o < 0 or l < 0 or o + l > pool_len:
            raise ValueError('stft_batch: utterance %d [%d, %d) is outside the pool of %d samples' % (u, o, o + l, pool_len))
        T_u = prep_num_frames(l, fft_size, fft_stride)
        if p < 0 or p + T_u > T_out:
            raise ValueError('stft_batch: utterance %d: pad_left %d + %d frames exceeds T_out = %d' % (u, p, T_u, T_out))
        d[u] = (o, l, p, 0)
    return d


def _prep_plan(window, fft_size):
    '''the (device, N, window) plan: twiddles + 1/sum(window), built once by danet_prep_stft_plan'''
    dev = _dev_index(window.device)
    fast = (dev, fft_size, window.data_ptr(), window._version)
    hit = _prep_plans_fast.get(fast)
    if hit is not None:
        return hit[1]
    key = (dev, fft_size, window.detach().cpu().numpy().tobytes())
    plan = _prep_plans.get(key)
    if plan is None:
        L = _lib.load_prep()
        nbytes = _lib.bytes_or_raise(L.danet_prep_workspace_bytes(fft_size), _lib.prep_check)
        plan = torch.zeros(nbytes, dtype=torch.uint8, device=window.device)
        _lib.prep_check(L.danet_prep_stft_plan(_lib.stream(), fft_size, ptr(window), ptr(plan), nbytes))
        _prep_plans[key] = plan
    if len(_prep_plans_fast) >= 64:
        _prep_plans_fast.clear()
    _prep_plans_fast[fast] = (window, plan)      # the reference keeps data_ptr from being reused
    return plan


def stft_batch(pool, desc, T_out, window, fft_size, fft_stride, t_begin=0, t_count=None, out=None):
    '''frames [t_begin, t_begin + t_count) of the zero-padded batch of the utterances `desc` describes
    -> complex64 [n_utt, t_count, F], ONE launch (danet_prep_stft_batch).
    pool: float32 device vector of waveforms laid back to back.  desc: the table of ops.prep_desc --
    a numpy record array (validated again and uploaded here) or a device uint8 / int64 tensor of 24-byte
    rows the caller has validated and uploaded.  window: float32 device vector.  out: optional
    complex64 [n_utt, t_count, >= F] view whose last dimension is contiguous (its row pitch is used).'''
    _chk('pool', pool, torch.float32, dim=1)
    _chk('window', window, torch.float32, numel=fft_size, dev=pool.device, contiguous=False)
    if t_count is None:
        t_count = T_out - t_begin
    F = fft_size // 2 + 1
    desc, n_utt = _desc_table('stft_batch', 'PREP_DESC_DTYPE', desc, lambda d: prep_desc(
        d['offset'], d['length'], d['pad_left'], T_out, pool.numel(), fft_size, fft_stride), pool.device)
    if out is None:
        out = torch.empty(n_utt, t_count, F, dtype=torch.complex64, device=pool.device)
    _chk('out', out, torch.complex64, (n_utt, t_count, F), contiguous=False)
    ld = _c64_row_pitch(out, F)
    plan = _prep_plan(window, fft_size)
    with _lib.timed('stft_batch'):
        _lib.prep_check(_lib.load_prep().danet_prep_stft_batch(
            _lib.stream(), n_utt, ptr(pool), pool.numel(), ptr(desc), T_out, t_begin, t_count, fft_size,
            fft_stride, ptr(window), ptr(plan), ptr(torch.view_as_real(out)), ld))
    return out


# ---- mixture level control of the wavdir dataset (include/danet_mix_hip.h) --------------------------
# On the extension library libdanet_mix_hip.so, mapped at the first call: a wavdir run with
# MIX_SNR_RANGE and MIX_LEVEL_RANGE null never gets here.
def mix_power(pool, offsets, lengths, max_len=None):
    '''sum of squares of every row [offset, offset + length) of the float32 device vector `pool`
    -> float64 DEVICE vector [n] (danet_mix_power: float64 accumulation, a fixed reduction tree).
    offsets, lengths: host integer sequences (validated here: a row outside the pool is a ValueError
    before any upload or launch) or int64 device tensors the caller has validated (the kernel clamps,
    and `max_len`, an upper bound of the lengths, must then be given).'''
    _chk('pool', pool, torch.float32, dim=1)
    offsets, lengths, max_len = _row_tables('mix_power', pool, offsets, lengths, max_len)
    n = _chk('offsets', offsets, torch.int64, dim=1).numel()
    _chk('lengths', lengths, torch.int64, numel=n, dim=1)
    L = _lib.load_mix()
    nbytes = _lib.bytes_or_raise(L.danet_mix_workspace_bytes(n, int(max_len)), _lib.mix_check)
    ws = _lib.workspace(nbytes, pool.device, 'mix') if nbytes else None
    out = torch.empty(n, dtype=torch.float64, device=pool.device)
    with _lib.timed('mix_power'):
        _lib.mix_check(L.danet_mix_power(_lib.stream(), n, ptr(pool), pool.numel(), ptr(offsets), ptr(lengths),
                                         int(max_len), ptr(out), ptr(ws), nbytes))
    return out


def mix_scale_(batch, gains):
    '''batch[u] *= gains[u] in place, ONE launch (danet_mix_scale_c64): complex64 device tensor
    [n_utt, t_count, F] whose last dimension is contiguous (its row pitch is used; the gaps are never
    touched), float32 device vector [n_utt].  Every part becomes the single rounding fl(g * x).'''
    _chk('batch', batch, torch.complex64, dim=3, contiguous=False)
    n_utt, t_count, F = batch.shape
    _chk('gains', gains, torch.float32, (n_utt,), dev=batch.device)
    ld = _c64_row_pitch(batch, F)
    with _lib.timed('mix_scale'):
        _lib.mix_check(_lib.load_mix().danet_mix_scale_c64(
            _lib.stream(), n_utt, t_count, F, ptr(torch.view_as_real(batch)), ld, ptr(gains)))
    return batch


# ---- active speech level of the wavdir dataset (include/danet_level_hip.h) ---------------------------
# On the extension library libdanet_level_hip.so, mapped at the first call: a wavdir run with
# MIX_LEVEL_MEASURE null never gets here.
LEVEL_THRESHOLDS, LEVEL_TILE = 16, 1024              # DANET_LEVEL_THRESHOLDS, DANET_LEVEL_TILE
LEVEL_MAX_LEN, LEVEL_MAX_HANG = 1 << 31, 1 << 40


def level_activity(pool, offsets, lengths, thresholds, g, hang, max_len=None):
    '''P.56 activity counts of every row [offset, offset + length) of the float32 device vector `pool`
    -> int64 DEVICE tensor [n, 16] (danet_level_activity: float64 envelope with the smoothing coefficient `g`,
    `hang` samples of hangover, counts[u][j] against thresholds[u][j]).
    offsets, lengths: host integer sequences (validated here: a row outside the pool is a ValueError
    before any upload or launch) or int64 device tensors the caller has validated (the kernel clamps,
    and `max_len`, an upper bound of the lengths, must then be given).  thresholds: float64 [n, 16], a host
    array or a device tensor.  Every violation the host can see is a ValueError raised before any launch.'''
    _chk('pool', pool, torch.float32, dim=1)
    g, hang = float(g), int(hang)
    if not 0.0 < g < 1.0:
        raise ValueError('level_activity: g must be inside (0, 1), got %r' % (g,))
    if not 0 <= hang <= LEVEL_MAX_HANG:
        raise ValueError('level_activity: hang must be in [0, 2^40] samples, got %r' % (hang,))
    offsets, lengths, max_len = _row_tables('level_activity', pool, offsets, lengths, max_len)
    max_len = int(max_len)
    n = _chk('offsets', offsets, torch.int64, dim=1).numel()
    _chk('lengths', lengths, torch.int64, dim=1)
    if n < 1 or lengths.numel() != n:
        raise ValueError('level_activity: offsets and lengths must be two vectors of one length >= 1')
    if not torch.is_tensor(thresholds):
        thresholds = torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float64)).to(pool.device)
    if thresholds.dtype != torch.float64 or tuple(thresholds.shape) != (n, LEVEL_THRESHOLDS):
        raise ValueError('level_activity: thresholds must be float64 [%d, %d], got %s %s'
                         % (n, LEVEL_THRESHOLDS, thresholds.dtype, tuple(thresholds.shape)))
    assert thresholds.is_cuda and thresholds.is_contiguous()
    tiles = max(1, -(-max_len // LEVEL_TILE))
    if not 0 <= max_len <= LEVEL_MAX_LEN or n * tiles >= 1 << 31:
        raise ValueError('level_activity: need 0 <= max_len <= 2^31 and rows * tiles per row < 2^31 (got max_len %d, '
                         '%d rows)' % (max_len, n))
    L = _lib.load_level()
    nbytes = _lib.bytes_or_raise(L.danet_level_workspace_bytes(n, max_len), _lib.level_check)
    # once per pool and as large as a fifth of it: a buffer of the call's own, not the grow-only scratch
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=pool.device)
    out = torch.empty(n, LEVEL_THRESHOLDS, dtype=torch.int64, device=pool.device)
    with _lib.timed('level_activity'):
        _lib.level_check(L.danet_level_activity(_lib.stream(), n, ptr(pool), pool.numel(), ptr(offsets), ptr(lengths),
                                                max_len, g, hang, ptr(thresholds), ptr(out), ptr(ws), nbytes))
    return out


# ---- speed perturbation of the wavdir dataset (include/danet_speed_hip.h) ----------------------------
# On the extension library libdanet_speed_hip.so, mapped at the first call: a wavdir run with
# SPEED_PERTURB_RANGE null never gets here.
SPEED_PHASES, SPEED_TAPS = 512, 32                   # Q, 2Z (DANET_SPEED_PHASES, DANET_SPEED_TAPS)
SPEED_P_MIN, SPEED_P_MAX = SPEED_PHASES - SPEED_PHASES // 4, SPEED_PHASES + SPEED_PHASES // 4
SPEED_DESC_DTYPE = np.dtype([('src_offset', '<i8'), ('src_length', '<i8'), ('dst_offset', '<i8'),
                             ('dst_length', '<i8'), ('p', '<i4'), ('reserved', '<i4')])


def speed_table(P):
    '''the float32 [Q][2Z] filter table of SPEED_PERTURB_RANGE = P (the rule of include/danet_speed_hip.h):
    float64 numpy, rounded once.  Host only, no library involved.'''
    Q, Z = SPEED_PHASES, SPEED_TAPS // 2
    fc = 1.0 / (1.0 + float(P))
    t = (np.arange(2 * Z, dtype=np.float64)[None, :] - (Z - 1)) - np.arange(Q, dtype=np.float64)[:, None] / Q
    a = fc * t
    k = np.rint(a)                                       # sin(pi a) = (-1)^k sin(pi (a - k)): exactly 0 at an integer a
    s = np.where(k % 2 == 0, 1.0, -1.0) * np.sin(np.pi * (a - k))
    sinc = np.where(a == 0, 1.0, s / np.where(a == 0, 1.0, np.pi * a))
    h = fc * sinc * 0.5 * (1.0 + np.cos(np.pi * t / Z))
    return (np.where(np.abs(t) < Z, h, 0.0) + 0.0).astype(np.float32)       # + 0.0: a zero tap is +0


def speed_out_len(L, p):
    '''L' = floor((L - 1) * Q / p) + 1 for an array of lengths and of speed numerators (int64 numpy; the rule
    danet_speed_out_len applies).  Host only, no library involved.'''
    L, p = np.asarray(L, dtype=np.int64), np.asarray(p, dtype=np.int64)
    return (L - 1) * SPEED_PHASES // p + 1


def speed_desc(src_offsets, src_lengths, dst_offsets, dst_lengths, p, src_len, dst_len, out=None):
    '''the validated descriptor table of one launch as a numpy record array (SPEED_DESC_DTYPE; into `out`
    when given).  Everything the kernel would have to clamp is a ValueError HERE, before any upload or
    launch: a source span outside the pool, a destination span outside the buffer or across another, a p
    outside [SPEED_P_MIN, SPEED_P_MAX].'''
    n = len(src_offsets)
    d = np.zeros(n, SPEED_DESC_DTYPE) if out is None else out
    assert d.dtype == SPEED_DESC_DTYPE and d.shape == (n,)
    d['src_offset'], d['src_length'], d['dst_offset'], d['dst_length'] = src_offsets, src_lengths, dst_offsets, dst_lengths
    d['p'], d['reserved'] = p, 0
    so, sl, do, dl, pp = (d[k].astype(np.int64) for k in ('src_offset', 'src_length', 'dst_offset', 'dst_length', 'p'))
    _check_source_spans('speed_resample', so, sl, src_len)
    bad = np.nonzero((pp < SPEED_P_MIN) | (pp > SPEED_P_MAX))[0]
    if len(bad):
        raise ValueError('speed_resample: utterance %d: p = %d is outside [%d, %d]'
                         % (bad[0], pp[bad[0]], SPEED_P_MIN, SPEED_P_MAX))
    bad = np.nonzero((do < 0) | (dl < 0) | (do + dl > dst_len))[0]
    if len(bad) or not _spans_apart(do, do + dl):
        raise ValueError('speed_resample: the destination spans must lie inside the buffer of %d samples and '
                         'apart from each other' % dst_len)
    return d


def speed_resample(pool, desc, table, out):
    '''every utterance `desc` describes resampled from the float32 device vector `pool` into the float32
    device vector `out`, ONE launch (danet_speed_resample); nothing of `out` outside the destination spans
    is touched.  desc: the table of ops.speed_desc -- a numpy record array (validated again and uploaded
    here) or a device uint8 / int64 tensor of 40-byte rows the caller has validated and uploaded.
    table: ops.speed_table(P) on the device, float32 [512, 32].  There is no CPU fallback.'''
    _chk('pool', pool, torch.float32, dim=1)
    _chk('out', out, torch.float32, dim=1, dev=pool.device)
    _chk('table', table, torch.float32, (SPEED_PHASES, SPEED_TAPS), dev=pool.device)
    desc, n_utt = _desc_table('speed_resample', 'SPEED_DESC_DTYPE', desc, lambda d: speed_desc(
        d['src_offset'], d['src_length'], d['dst_offset'], d['dst_length'], d['p'], pool.numel(), out.numel()),
        pool.device)
    with _lib.timed('speed_resample'):
        _lib.speed_check(_lib.load_speed().danet_speed_resample(
            _lib.stream(), n_utt, ptr(pool), pool.numel(), ptr(desc), ptr(table), ptr(out), out.numel()))
    return out


# ---- reverberation of the wavdir dataset (include/danet_reverb_hip.h) -----------------------------------
# On the extension library libdanet_reverb_hip.so, mapped at the first call: a wavdir run with
# REVERB_RT60_MAX null never gets here.
REVERB_ROWS, REVERB_MIN_TAPS, REVERB_MAX_TAPS = 32, 4, 8192     # NB (DANET_REVERB_ROWS), DANET_REVERB_MIN_TAPS / _MAX_TAPS
REVERB_DESC_DTYPE = np.dtype([('src_offset', '<i8'), ('src_length', '<i8'), ('dst_offset', '<i8'),
                              ('out_begin', '<i8'), ('out_count', '<i8'), ('row', '<i4'), ('reserved', '<i4')])


def reverb_taps(R, smprate):
    '''K = 4 * ceil(R * smprate / 4), at least REVERB_MIN_TAPS (the rule of include/danet_reverb_hip.h); one
    above REVERB_MAX_TAPS is the caller's to refuse.  Host only, no library involved.'''
    return max(REVERB_MIN_TAPS, 4 * int(np.ceil(float(R) * float(smprate) / 4.0)))


def reverb_bank(R, smprate):
    '''the float32 [NB][K] bank of room responses of REVERB_RT60_MAX = R at `smprate` (the rule of
    include/danet_reverb_hip.h): float64 numpy, rounded once, checked to be finite.  Host only, no library
    involved.'''
    NB, K = REVERB_ROWS, reverb_taps(R, smprate)
    if K > REVERB_MAX_TAPS:
        raise ValueError('reverb_bank: REVERB_RT60_MAX = %r at SMPRATE = %r needs %d taps, more than the %d of '
                         'include/danet_reverb_hip.h' % (R, smprate, K, REVERB_MAX_TAPS))
    bank = np.zeros((NB, K), dtype=np.float64)
    bank[:, 0] = 1.0
    n = np.arange(K, dtype=np.float64)
    for k in range(1, NB):
        rt60 = float(R) * k / (NB - 1)
        if rt60 <= 0:
            continue                                                  # R = 0: no tail, the unit impulse
        g = np.random.RandomState([1337, 2, k]).standard_normal(K)
        t = g * np.exp(-3.0 * np.log(10.0) * n / (rt60 * float(smprate)))
        t[0] = 0.0
        e = float(np.sum(t * t))
        if e > 0:
            t *= np.sqrt(10.0 ** (-(10.0 - 10.0 * k / (NB - 1)) / 10.0) / e)
        e = float(np.sum(t * t))
        t[0] = 1.0
        bank[k] = t / np.sqrt(1.0 + e)
    bank = bank.astype(np.float32)
    if not np.isfinite(bank).all():
        raise ValueError('reverb_bank: the bank of REVERB_RT60_MAX = %r is not finite' % (R,))
    return bank


def reverb_desc(src_offsets, src_lengths, dst_offsets, out_begin, out_count, rows, src_len, dst_len, out=None):
    '''the validated descriptor table of one launch as a numpy record array (REVERB_DESC_DTYPE; into `out`
    when given).  Everything the kernel would have to clamp is a ValueError HERE, before any upload or
    launch: a source span outside the pool, a span outside [0, length), a written span outside the buffer or
    across another, a row outside [0, REVERB_ROWS).'''
    n = len(src_offsets)
    d = np.zeros(n, REVERB_DESC_DTYPE) if out is None else out
    assert d.dtype == REVERB_DESC_DTYPE and d.shape == (n,)
    d['src_offset'], d['src_length'], d['dst_offset'] = src_offsets, src_lengths, dst_offsets
    d['out_begin'], d['out_count'], d['row'], d['reserved'] = out_begin, out_count, rows, 0
    so, sl, do, ob, oc, rw = (d[k].astype(np.int64) for k in ('src_offset', 'src_length', 'dst_offset', 'out_begin',
                                                              'out_count', 'row'))
    _check_source_spans('reverb_apply', so, sl, src_len)
    bad = np.nonzero((rw < 0) | (rw >= REVERB_ROWS))[0]
    if len(bad):
        raise ValueError('reverb_apply: utterance %d: row = %d is outside [0, %d)' % (bad[0], rw[bad[0]], REVERB_ROWS))
    bad = np.nonzero((ob < 0) | (oc < 0) | (ob + oc > sl))[0]
    if len(bad):
        u = int(bad[0])
        raise ValueError('reverb_apply: utterance %d: the span [%d, %d) is outside its %d samples'
                         % (u, ob[u], ob[u] + oc[u], sl[u]))
    lo, hi = do + ob, do + ob + oc
    if np.any(lo < 0) or np.any(hi > dst_len) or not _spans_apart(lo, hi):
        raise ValueError('reverb_apply: the written spans must lie inside the buffer of %d samples and '
                         'apart from each other' % dst_len)
    return d


def reverb_apply(src, desc, bank, n_taps, out):
    '''every utterance `desc` describes convolved with its row of `bank` from the float32 device vector `src`
    into the float32 device vector `out`, ONE launch (danet_reverb_apply); nothing of `out` outside the asked
    spans is touched.  desc: the table of ops.reverb_desc -- a numpy record array (validated again and uploaded
    here) or a device uint8 / int64 tensor of 48-byte rows the caller has validated and uploaded.
    bank: ops.reverb_bank(R, smprate) on the device, float32 [32, n_taps].  There is no CPU fallback.'''
    _chk('src', src, torch.float32, dim=1)
    _chk('out', out, torch.float32, dim=1, dev=src.device)
    _chk('bank', bank, torch.float32, (REVERB_ROWS, n_taps), dev=src.device)
    assert src.data_ptr() != out.data_ptr()
    desc, n_utt = _desc_table('reverb_apply', 'REVERB_DESC_DTYPE', desc, lambda d: reverb_desc(
        d['src_offset'], d['src_length'], d['dst_offset'], d['out_begin'], d['out_count'], d['row'], src.numel(),
        out.numel()), src.device)
    with _lib.timed('reverb_apply'):
        _lib.reverb_check(_lib.load_reverb().danet_reverb_apply(
            _lib.stream(), n_utt, ptr(src), src.numel(), ptr(desc), ptr(bank), int(n_taps), ptr(out), out.numel()))
    return out


# ---- waveform metric of valid / test (include/danet_metric_hip.h) -------------------------------------
# On the extension library libdanet_metric_hip.so, mapped at the first call: a run with EVAL_SI_SDR null never
# gets here.  Three launches: spectra -> waveforms -> Gram matrices -> decibels.
METRIC_MAX_C = 4                                     # DANET_METRIC_MAX_C
_metric_ws = {}          # (device index, stream, B, C, T, N, S) -> (scratch, wav, G, per_utt, mean2, perm_idx): a cache of _scratch
_metric_windows = {}     # (device index, window bytes) -> float32 device vector


def _metric_window(dev):
    '''hparams.FFT_WND as a float32 device vector, uploaded once per (device, window)'''
    from .hparams import hparams
    w = np.ascontiguousarray(np.asarray(hparams.FFT_WND, dtype=np.float32))
    key = (_dev_index(dev), w.tobytes())
    t = _metric_windows.get(key)
    if t is None:
        t = _metric_windows[key] = torch.from_numpy(w.copy()).to(dev)
    return t


_WAVE = {'metric': (_lib.load_metric, _lib.metric_check), 'neval': (_lib.load_neval, _lib.neval_check)}


def _wave_fn(tag, name):
    '''(danet_<tag>_<name> of the library of that tag (metric or neval), that library's check)'''
    load, check_ = _WAVE[tag]
    return getattr(load(), 'danet_%s_%s' % (tag, name)), check_


def _wave_call(tag, name, *args):
    '''danet_<tag>_<name>(*args), its status checked'''
    fn, check_ = _wave_fn(tag, name)
    check_(fn(*args))


def _wave_parts(rows, outs, B, T, S):
    '''[(name, shape, dtype)] of the parts of the buffer of danet_<tag>_workspace_bytes, in its order: `rows` signals
    and `outs` figures per utterance'''
    f64 = torch.float64
    return [('wav', (B, rows, (T - 1) * S), torch.float32), ('G', (B, rows, rows), f64), ('per_utt', (B, outs), f64),
            ('means', (outs,), f64), ('perm_idx', (B,), torch.int32)]


def _wave_workspace(tag, cache, rows, outs, B, C, T, N, S, dev):
    '''(buffer, wav, G, per_utt, means, perm_idx): the views one shape cuts out of the grow-only scratch `tag` of this
    (device, stream), in the layout of danet_<tag>_workspace_bytes; cached per shape in `cache`'''
    def nbytes():
        fn, check_ = _wave_fn(tag, 'workspace_bytes')
        return _lib.bytes_or_raise(fn(B, C, T, N, S), check_)
    return _scratch(tag, cache, (B, C, T, N, S), lambda: _wave_parts(rows, outs, B, T, S), nbytes, dev, flat=True)


def _wave_gram(tag, wav, out):
    _chk('wav', wav, torch.float32, dim=3)
    B, M, Ls = wav.shape
    out = _out('out', out, (B, M, M), torch.float64, wav.device)
    with _lib.timed(tag + '_gram'):
        _wave_call(tag, 'gram', _lib.stream(), B, M, Ls, ptr(wav), ptr(out))
    return out


def _wave_finalize(tag, outs, G, out):
    '''G [B, M, M], M = 2C + outs - 2 -> (means [outs], per_utt [B, outs], perm_idx int32 [B])'''
    _chk('G', G, torch.float64, dim=3)
    B, M = G.shape[0], G.shape[1]
    assert M == G.shape[2] and M % 2 == outs - 2, G.shape
    per_utt, perm_idx, means = _result(B, outs, G.device) if out is None else out
    with _lib.timed(tag + '_si_sdr'):
        _wave_call(tag, 'si_sdr', _lib.stream(), B, M // 2, ptr(G), ptr(per_utt), ptr(perm_idx), ptr(means))
    return means, per_utt, perm_idx


def metric_synth(src, est, fft_stride, window=None, out=None):
    '''references and UNPERMUTED estimates, complex64 [B, C, T, F] -> float32 waveforms [B, 2C, (T - 1) * S],
    references first, ONE launch (danet_metric_synth: overlap-add with an exact window-sum division).
    window: float32 device vector [N] (default hparams.FFT_WND, uploaded once).'''
    _chk('src', src, torch.complex64, dim=4, contiguous=False)
    _chk('est', est, torch.complex64, src.shape, dev=src.device, contiguous=False)
    src, est = src.contiguous(), est.contiguous()
    B, C, T, F = src.shape
    N = 2 * (F - 1)
    window = _metric_window(src.device) if window is None else _f32(window).contiguous()
    _chk('window', window, torch.float32, numel=N, dev=src.device)
    assert T >= 1, T
    out = _out('out', out, (B, 2 * C, (T - 1) * fft_stride), torch.float32, src.device)
    with _lib.timed('metric_synth'):
        _lib.metric_check(_lib.load_metric().danet_metric_synth(
            _lib.stream(), B, C, T, N, fft_stride, ptr(torch.view_as_real(src)), ptr(torch.view_as_real(est)),
            ptr(window), ptr(out)))
    return out


def metric_gram(wav, out=None):
    '''float32 [B, M, Ls] -> float64 Gram matrices [B, M, M], ONE launch (danet_metric_gram: float64 products
    and sums over a fixed tree; symmetric bit for bit)'''
    return _wave_gram('metric', wav, out)


def metric_finalize(G, out=None):
    '''float64 Gram matrices [B, 2C, 2C] -> (mean2 [2], per_utt [B, 2], perm_idx int32 [B]), ONE launch
    (danet_metric_si_sdr); out: optional (per_utt, perm_idx, mean2) to write into'''
    return _wave_finalize('metric', 2, G, out)


def si_sdr(src, est, fft_stride=None):
    '''SI-SDR and SI-SDRi (dB) of the waveforms of the UNPERMUTED estimates `est` against the references
    `src`, both complex64 [B, C, T, F] -> (si_sdr, si_sdri, per_utt [B, 2], perm_idx [B]): float64 / int32 device
    tensors of the caller's own (allocated here, written by the finalize kernel; the waveforms and Gram
    matrices live in a scratch cached per shape).  Three launches and nothing else on the device, no host
    synchronisation.'''
    return si_sdr_wav(src, est, fft_stride)[:4]


def si_sdr_wav(src, est, fft_stride=None):
    '''si_sdr, and as a fifth result the waveforms it synthesised: float32 [B, 2C, (T - 1) * S], a VIEW of the cached
    scratch that the next call of this shape on this stream overwrites (ops.bss_eval reads it in the same step)'''
    S = _stride(fft_stride)
    B, C, T, F = src.shape
    ws = _wave_workspace('metric', _metric_ws, 2 * C, 2, B, C, T, 2 * (F - 1), S, src.device)
    wav, G = ws[1], ws[2]
    metric_synth(src, est, S, out=wav)
    metric_gram(wav, out=G)
    mean2, per_utt, perm_idx = metric_finalize(G, out=_result(B, 2, src.device))
    return mean2[0], mean2[1], per_utt, perm_idx, wav


def synth_wav(src, est, fft_stride=None):
    '''the float32 waveforms [B, 2C, (T - 1) * S] of the references and the UNPERMUTED estimates, synthesised into the
    metric's cached scratch (a VIEW the next call of this shape on this stream overwrites): what ops.bss_eval and
    ops.stoi_eval synthesise for themselves when no `wav` is given, once for both'''
    S = _stride(fft_stride)
    B, C, T, F = src.shape
    wav = _wave_workspace('metric', _metric_ws, 2 * C, 2, B, C, T, 2 * (F - 1), S, src.device)[1]
    return metric_synth(src, est, S, out=wav)


# ---- MISI phase refinement of the separated spectra (include/danet_phase_hip.h) ---------------------------
# On the extension library libdanet_phase_hip.so, mapped at the first call: a run with PHASE_REFINE_ITERS null never
# gets here.  init (two launches), then per iteration: waveforms of the iterate -> projection onto the magnitudes.
PHASE_MAX_C = 4                                      # DANET_PHASE_MAX_C
_phase_ws = {}           # (device index, stream, B, C, T, N, S) -> (scratch, views)


def phase_workspace_bytes(B, C, T, N, S):
    '''danet_phase_workspace_bytes'''
    return _lib.bytes_or_raise(_lib.load_phase().danet_phase_workspace_bytes(int(B), int(C), int(T), int(N), int(S)),
                               _lib.phase_check)


def phase_parts(ws, B, C, T, N, S):
    '''(A float32 [B, C, T, F], mix complex64 [B, T, F], wav float32 [B, C + 1, Ls]): views of the three parts of a
    workspace buffer (uint8, at least phase_workspace_bytes long) in the header's layout'''
    return tuple(_carve(ws, _phase_layout(B, C, T, N, S))[0].values())


def _phase_layout(B, C, T, N, S):
    '''[(name, shape, dtype)] of the parts of the buffer of danet_phase_workspace_bytes, in its order'''
    F = N // 2 + 1
    return [('A', (B, C, T, F), torch.float32), ('mix', (B, T, F), torch.complex64),
            ('wav', (B, C + 1, (T - 1) * S), torch.float32)]


def _phase_workspace(B, C, T, N, S, dev):
    '''the grow-only scratch 'phase' of this (device, stream), at least one workspace of this shape long; its size
    is asked of the library once per shape'''
    return _scratch('phase', _phase_ws, (B, C, T, N, S), lambda: _phase_layout(B, C, T, N, S),
                    lambda: phase_workspace_bytes(B, C, T, N, S), dev)[0]


def _phase_args(x, window, ws, fft_stride):
    _chk('x', x, torch.complex64, dim=4)
    B, C, T, F = x.shape
    N = 2 * (F - 1)
    _chk('window', window, torch.float32, numel=N, dev=x.device)
    _chk('ws', ws, torch.uint8, dev=x.device)
    S = int(fft_stride)
    assert ws.numel() >= phase_workspace_bytes(B, C, T, N, S), ws.numel()
    return B, C, T, N, S


def phase_init(est0, mixrows, window, ws, fft_stride, x=None):
    '''danet_phase_init, TWO launches: A = |est0|, the mixture sum of mixrows [B, Cm, T, F] and y = synth(mixture) into
    the workspace `ws`, and x = est0 (a fresh tensor unless given; x may be est0) -> x'''
    if x is None:
        x = torch.empty_like(est0)
    B, C, T, N, S = _phase_args(x, window, ws, fft_stride)
    _chk('est0', est0, torch.complex64, x.shape, dev=x.device)
    _chk('mixrows', mixrows, torch.complex64, dim=4, dev=x.device)
    assert (mixrows.shape[0],) + tuple(mixrows.shape[2:]) == (B, T, N // 2 + 1), mixrows.shape
    with _lib.timed('phase_init'):
        _lib.phase_check(_lib.load_phase().danet_phase_init(
            _lib.stream(), B, C, mixrows.shape[1], T, N, S, ptr(torch.view_as_real(est0)),
            ptr(torch.view_as_real(mixrows)), ptr(window), ptr(ws), ptr(torch.view_as_real(x))))
    return x


def phase_synth(x, window, ws, fft_stride):
    '''danet_phase_synth, ONE launch: the waveforms of the C rows of every utterance of x into the workspace'''
    B, C, T, N, S = _phase_args(x, window, ws, fft_stride)
    with _lib.timed('phase_synth'):
        _lib.phase_check(_lib.load_phase().danet_phase_synth(
            _lib.stream(), B, C, T, N, S, ptr(torch.view_as_real(x)), ptr(window), ptr(ws)))


def phase_project(x, window, ws, fft_stride, z_out=None):
    '''danet_phase_project, ONE launch: redistribution, analysis and projection onto the magnitudes, x updated IN
    PLACE; z_out (complex64, the shape of x) receives the analysis Z when given -> x'''
    B, C, T, N, S = _phase_args(x, window, ws, fft_stride)
    if z_out is not None:
        assert _chk('z_out', z_out, torch.complex64, x.shape, dev=x.device).data_ptr() != x.data_ptr()
    with _lib.timed('phase_project'):
        _lib.phase_check(_lib.load_phase().danet_phase_project(
            _lib.stream(), B, C, T, N, S, ptr(window), ptr(ws), ptr(torch.view_as_real(x)),
            ptr(torch.view_as_real(z_out)) if z_out is not None else None))
    return x


def phase_refine(est0, mixrows, K, fft_stride=None, window=None):
    '''K iterations of MISI on est0 complex64 [B, C, T, F] against the mixture that is the sum of mixrows complex64
    [B, Cm, T, F] -> complex64 [B, C, T, F], a FRESH tensor with the magnitudes of est0 (K = 0: est0 bit for bit).
    The workspace is a scratch cached per shape; 2 + 2K launches and nothing else on the device, no host
    synchronisation.  window: float32 device vector [N] (default hparams.FFT_WND, uploaded once).'''
    S = _stride(fft_stride)
    K = int(K)
    assert K >= 0, K
    _chk('est0', est0, torch.complex64, dim=4, contiguous=False)
    est0, mixrows = est0.contiguous(), mixrows.contiguous()
    B, C, T, F = est0.shape
    dev = est0.device
    window = _metric_window(dev) if window is None else _f32(window).contiguous()
    ws = _phase_workspace(B, C, T, 2 * (F - 1), S, dev)
    x = phase_init(est0, mixrows, window, ws, S)
    for _ in range(K):
        phase_synth(x, window, ws, S)
        phase_project(x, window, ws, S)
    return x


# ---- the online attractor estimator (include/danet_online_hip.h) ----------------------------------------------
# On the extension library libdanet_online_hip.so, mapped at the first call: a run with another inference estimator
# never gets here.  init (one launch) -> scan (one launch, one workgroup per utterance) -> separate (one launch).
ONLINE_MAX_C = 4                                     # DANET_ONLINE_MAX_C
ONLINE_MAX_E = 64                                    # DANET_ONLINE_MAX_E
ONLINE_MAX_F = 1025                                  # DANET_ONLINE_MAX_F
ONLINE_MAX_T = 65536                                 # DANET_ONLINE_MAX_T


def online_state_bytes(C, E):
    '''danet_online_state_bytes: the bytes of ONE utterance's state, float64 S [C][E], n [C], A [C][E]'''
    return _lib.bytes_or_raise(_lib.load_online().danet_online_state_bytes(int(C), int(E)), _lib.online_check)


def online_state_parts(state, C, E):
    '''(S [B, C, E], n [B, C], A [B, C, E]): views of a state tensor float64 [B, 2 C E + C] in the header's layout'''
    B, CE = state.shape[0], C * E
    _chk('state', state, torch.float64, (B, 2 * CE + C), contiguous=False, cuda=False)
    return state[:, :CE].view(B, C, E), state[:, CE:CE + C], state[:, CE + C:].view(B, C, E)


def online_init(a0, state=None):
    '''danet_online_init, ONE launch: a0 float32 [B, C, E] -> state float64 [B, 2 C E + C] with S = 0, n = 0, A = a0'''
    assert a0.dim() == 3, a0.shape
    a0 = _f32(a0.contiguous())
    B, C, E = a0.shape
    if state is None:
        state = torch.empty(B, online_state_bytes(C, E) // 8, dtype=torch.float64, device=a0.device)
    _chk('state', state, torch.float64, (B, 2 * C * E + C), dev=a0.device)
    with _lib.timed('online_init'):
        _lib.online_check(_lib.load_online().danet_online_init(_lib.stream(), B, C, E, ptr(a0), ptr(state)))
    return state


def online_scan(embed, w, state, act, lam, T0, eps, t_first=0, attr=None):
    '''danet_online_scan, ONE launch: the frames t_first .. t_first + T - 1 of embed float32 [B, T, F, E] with the
    weights w float32 [B, T, F], from `state` (float64 [B, 2 C E + C], updated IN PLACE) -> the trajectory attr float32
    [B, T, C, E]'''
    B, T, F, E = _chk('embed', embed, torch.float32, dim=4).shape
    _chk('w', w, torch.float32, (B, T, F), dev=embed.device)
    _chk('state', state, torch.float64, dim=2, dev=embed.device)
    assert state.shape[0] == B and (state.shape[1] % (2 * E + 1)) == 0, state.shape
    C = state.shape[1] // (2 * E + 1)
    attr = _out('attr', attr, (B, T, C, E), torch.float32, embed.device)
    with _lib.timed('online_scan'):
        _lib.online_check(_lib.load_online().danet_online_scan(
            _lib.stream(), B, C, T, F, E, int(act), float(lam), int(T0), int(t_first), float(eps), ptr(embed), ptr(w),
            ptr(state), ptr(attr)))
    return attr


def online_separate(w, attr, embed, act, out=None):
    '''danet_online_separate, ONE launch: out[b][c][t][f] = w[b][t][f] * act(embed[b][t][f] . attr[b][t][c]) with
    w float32 [B, T, F], attr float32 [B, T, C, E], embed float32 [B, T, F, E] (or flat [B, T F, E]) -> [B, C, T, F]'''
    w, attr, embed = _f32(w.contiguous()), _f32(attr.contiguous()), _f32(embed.contiguous())
    B, T, F = w.shape
    assert attr.dim() == 4 and tuple(attr.shape[:2]) == (B, T), (attr.shape, w.shape)
    C, E = attr.shape[2], attr.shape[3]
    assert embed.numel() == B * T * F * E and embed.shape[0] == B and embed.shape[-1] == E, (embed.shape, w.shape)
    out = _out('out', out, (B, C, T, F), torch.float32, w.device)
    with _lib.timed('online_separate'):
        _lib.online_check(_lib.load_online().danet_online_separate(
            _lib.stream(), int(act), B, C, T, F, E, ptr(w), ptr(attr), ptr(embed), ptr(out)))
    return out


def online_attractors(embed, w, a0, act, lam, T0, eps):
    '''init plus one scan: the trajectory attr float32 [B, T, C, E] of embed [B, T, F, E] with the weights w [B, T, F]
    from the initial attractors a0 [B, C, E]; lam the forgetting factor, T0 the hold length in frames'''
    return online_scan(embed.contiguous(), w.contiguous(), online_init(a0), act, lam, T0, eps)


# ---- the truth-online estimator and the trajectory separator's backward (include/danet_tonline_hip.h) -----------
# On the extension library libdanet_tonline_hip.so, mapped at the first call: only the train branch of a model built
# with TRAIN_ESTIMATOR_METHOD = "truth-online" gets here.  Forward: frame_sums -> scan (-> online_separate); backward:
# separate_bwd, scan_bwd -> sums_bwd.  Five launches beside the one of danet_online_separate.
_tonline_ws = {}         # (device index, stream, B, T, C, E) -> (scratch, {s, q, r}): a cache of _scratch


def _tonline_scratch(B, T, C, E, dev):
    '''the intermediates that live between two launches: the frame sums s, q of the forward and R of the backward'''
    return _scratch('tonline', _tonline_ws, (B, T, C, E),
                    lambda: [('s', (B, T, C, E), torch.float32), ('q', (B, T, C), torch.float32),
                             ('r', (B, T, C, E), torch.float32)], None, dev)[1]


def tonline_frame_sums(embed, src_pwr, w, out=None):
    '''danet_tonline_frame_sums, ONE launch: embed float32 [B, T, F, E], src_pwr float32 [B, C, T, F], w float32
    [B, T, F] -> (s float32 [B, T, C, E], q float32 [B, T, C]), the W-weighted sums of every frame under the ideal
    assignment'''
    B, T, F, E = _chk('embed', embed, torch.float32, dim=4).shape
    C = _chk('src_pwr', src_pwr, torch.float32, dim=4, dev=embed.device).shape[1]
    _chk('src_pwr', src_pwr, torch.float32, (B, C, T, F))
    _chk('w', w, torch.float32, (B, T, F), dev=embed.device)
    out = out or (None, None)
    s = _out('s', out[0], (B, T, C, E), torch.float32, embed.device)
    q = _out('q', out[1], (B, T, C), torch.float32, embed.device)
    with _lib.timed('tonline_frame_sums'):
        _lib.tonline_check(_lib.load_tonline().danet_tonline_frame_sums(
            _lib.stream(), B, C, T, F, E, ptr(embed), ptr(src_pwr), ptr(w), ptr(s), ptr(q)))
    return s, q


def tonline_scan(s, q, lam, T0, eps, out=None):
    '''danet_tonline_scan, ONE launch: the frame sums s [B, T, C, E], q [B, T, C] -> (attr float32 [B, T, C, E], den
    float64 [B, T, C]): the trajectory and the denominators n + eps the backward divides by'''
    B, T, C, E = _chk('s', s, torch.float32, dim=4).shape
    _chk('q', q, torch.float32, (B, T, C), dev=s.device)
    out = out or (None, None)
    attr = _out('attr', out[0], (B, T, C, E), torch.float32, s.device)
    den = _out('den', out[1], (B, T, C), torch.float64, s.device)
    with _lib.timed('tonline_scan'):
        _lib.tonline_check(_lib.load_tonline().danet_tonline_scan(
            _lib.stream(), B, C, T, E, float(lam), int(T0), float(eps), ptr(s), ptr(q), ptr(attr), ptr(den)))
    return attr, den


def tonline_scan_bwd(dattr, den, lam, T0, out=None):
    '''danet_tonline_scan_bwd, ONE launch: dattr float32 [B, T, C, E] and the saved den float64 [B, T, C] -> r float32
    [B, T, C, E], the gradient with respect to the frame sums of every frame'''
    B, T, C, E = _chk('dattr', dattr, torch.float32, dim=4).shape
    _chk('den', den, torch.float64, (B, T, C), dev=dattr.device)
    r = _out('r', out, (B, T, C, E), torch.float32, dattr.device)
    with _lib.timed('tonline_scan_bwd'):
        _lib.tonline_check(_lib.load_tonline().danet_tonline_scan_bwd(
            _lib.stream(), B, C, T, E, float(lam), int(T0), ptr(dattr), ptr(den), ptr(r)))
    return r


def tonline_sums_bwd(src_pwr, w, r, out=None):
    '''danet_tonline_sums_bwd, ONE launch: dembed[b][t][f] = w[b][t][f] * r[b][t][label of the bin] -> float32
    [B, T, F, E]'''
    B, C, T, F = _chk('src_pwr', src_pwr, torch.float32, dim=4).shape
    _chk('w', w, torch.float32, (B, T, F), dev=src_pwr.device)
    E = _chk('r', r, torch.float32, dim=4, dev=src_pwr.device).shape[3]
    _chk('r', r, torch.float32, (B, T, C, E))
    dembed = _out('dembed', out, (B, T, F, E), torch.float32, src_pwr.device)
    with _lib.timed('tonline_sums_bwd'):
        _lib.tonline_check(_lib.load_tonline().danet_tonline_sums_bwd(
            _lib.stream(), B, C, T, F, E, ptr(src_pwr), ptr(w), ptr(r), ptr(dembed)))
    return dembed


def tonline_separate_bwd(w, attr, embed, dout, act, out=None):
    '''danet_tonline_separate_bwd, ONE launch: the backward of online_separate.  w [B, T, F], attr [B, T, C, E], embed
    [B, T, F, E], dout [B, C, T, F], all float32 -> (dembed float32 [B, T, F, E], dattr float32 [B, T, C, E])'''
    B, T, F, E = _chk('embed', embed, torch.float32, dim=4).shape
    dev = embed.device
    C = _chk('attr', attr, torch.float32, dim=4, dev=dev).shape[2]
    _chk('attr', attr, torch.float32, (B, T, C, E))
    _chk('w', w, torch.float32, (B, T, F), dev=dev)
    _chk('dout', dout, torch.float32, (B, C, T, F), dev=dev)
    out = out or (None, None)
    dembed = _out('dembed', out[0], (B, T, F, E), torch.float32, dev)
    dattr = _out('dattr', out[1], (B, T, C, E), torch.float32, dev)
    with _lib.timed('tonline_separate_bwd'):
        _lib.tonline_check(_lib.load_tonline().danet_tonline_separate_bwd(
            _lib.stream(), int(act), B, C, T, F, E, ptr(w), ptr(attr), ptr(embed), ptr(dout), ptr(dembed), ptr(dattr)))
    return dembed, dattr


class TruthOnlineAttractorFn(torch.autograd.Function):
    '''THE RULE of include/danet_tonline_hip.h: (embed [B, T, F, E], src_pwr [B, C, T, F], mix_pwr [B, T, F]) -> the
    trajectory attr [B, T, C, E] of the running, forgetting-weighted means under the ideal assignment.  The gradient
    goes to embed alone and is returned as an ordinary tensor: autograd adds it to the separator's.'''

    @staticmethod
    def forward(ctx, embed, src_pwr, mix_pwr, lam, T0, eps):
        embed, src_pwr, mix_pwr = _f32(embed.contiguous()), _f32(src_pwr.contiguous()), _f32(mix_pwr.contiguous())
        B, T, F, E = embed.shape
        ws = _tonline_scratch(B, T, src_pwr.shape[1], E, embed.device)
        s, q = tonline_frame_sums(embed, src_pwr, mix_pwr, out=(ws['s'], ws['q']))
        attr, den = tonline_scan(s, q, lam, T0, eps)
        ctx.save_for_backward(src_pwr, mix_pwr, den)
        ctx.args = (lam, T0)
        return attr

    @staticmethod
    def backward(ctx, dattr):
        src_pwr, mix_pwr, den = ctx.saved_tensors
        lam, T0 = ctx.args
        B, T, C = den.shape
        dattr = _f32(dattr.contiguous())
        r = tonline_scan_bwd(dattr, den, lam, T0, out=_tonline_scratch(B, T, C, dattr.shape[3], dattr.device)['r'])
        return tonline_sums_bwd(src_pwr, mix_pwr, r), None, None, None, None, None


class OnlineSeparateFn(torch.autograd.Function):
    '''online_separate with a backward: (mix_pwr [B, T, F], attr [B, T, C, E], embed_flat [B, T F, E] or [B, T, F, E],
    act) -> sep [B, C, T, F].  Both gradients are returned as ordinary tensors.'''

    @staticmethod
    def forward(ctx, mix_pwr, attr, embed_flat, act):
        mix_pwr, attr = _f32(mix_pwr.contiguous()), _f32(attr.contiguous())
        B, T, F = mix_pwr.shape
        embed = _f32(embed_flat.contiguous()).view(B, T, F, attr.shape[3])
        out = online_separate(mix_pwr, attr, embed, act)
        ctx.save_for_backward(mix_pwr, attr, embed)
        ctx.args = (int(act), embed_flat.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        mix_pwr, attr, embed = ctx.saved_tensors
        act, shape = ctx.args
        dembed, dattr = tonline_separate_bwd(mix_pwr, attr, embed, _f32(dout.contiguous()), act)
        return None, dattr, dembed.view(shape), None


# ---- the causal encoder and block-wise streaming (include/danet_causal_hip.h) -----------------------------------
# On the extension library libdanet_causal_hip.so, mapped at the first call: a run with another encoder and no stream
# session never gets here.
CAUSAL_MAX_B = 16                                    # DANET_CAUSAL_MAX_B
CAUSAL_MAX_TB = 64                                   # DANET_CAUSAL_MAX_TB
CAUSAL_MAX_H = 608                                   # DANET_CAUSAL_MAX_H
CAUSAL_MAX_D0 = 1028                                 # DANET_CAUSAL_MAX_D0
CAUSAL_MAX_L = 8                                     # DANET_CAUSAL_MAX_L
CAUSAL_MAX_M = 1024                                  # DANET_CAUSAL_MAX_M


def causal_center_state(B, dev):
    '''the state of a fresh utterance: float64 [B, 2] = (S, n), zeros'''
    return torch.zeros(B, 2, dtype=torch.float64, device=dev)


def causal_center_fwd(x, B, T, D, in_layout, ld_in, out, out_layout, ld_out, state):
    '''danet_causal_center_fwd, ONE launch: out[t] = x[t] - the mean of everything up to and including frame t, from
    `state` (float64 [B, 2], updated IN PLACE); layouts as for `center`'''
    _chk('state', state, torch.float64, (B, 2))
    with _lib.timed('causal_center'):
        _lib.causal_check(_lib.load_causal().danet_causal_center_fwd(
            _lib.stream(), B, T, D, ptr(_f32(x)), in_layout, ld_in, ptr(_f32(out)), out_layout, ld_out, ptr(state)))
    return out


def causal_center_bwd(dout, B, T, D, dout_layout, ld_dout, din, din_layout, ld_din):
    '''danet_causal_center_bwd, ONE launch: the adjoint of causal_center_fwd over a whole utterance from a zero state'''
    with _lib.timed('causal_center_bwd'):
        _lib.causal_check(_lib.load_causal().danet_causal_center_bwd(
            _lib.stream(), B, T, D, ptr(_f32(dout)), dout_layout, ld_dout, ptr(_f32(din)), din_layout, ld_din))
    return din


def causal_lstm_ws_bytes(L, B, Tb, H):
    '''danet_causal_lstm_ws_bytes: the bytes of the per-layer block buffers'''
    return _lib.bytes_or_raise(_lib.load_causal().danet_causal_lstm_ws_bytes(int(L), int(B), int(Tb), int(H)),
                               _lib.causal_check)


def causal_lstm_block(x, ldx, D0, Ws, bs, h, c, y=None, ldy=None, ws=None):
    '''danet_causal_lstm_block: the Tb frames x float32 [Tb, B, ldx] (D0 valid columns) through the L = len(Ws)
    stacked layers FROM the carried state h, c float32 [L, B, H] (both updated IN PLACE) -> y float32 [Tb, B, ldy], the
    top layer's output; Tb + L launches'''
    L = len(Ws)
    Tb, B = x.shape[0], x.shape[1]
    H = h.shape[2]
    dev = x.device
    assert tuple(h.shape) == (L, B, H) == tuple(c.shape) and h.is_contiguous() and c.is_contiguous(), (h.shape, c.shape)
    assert x.is_contiguous() and x.shape[2] == ldx, (x.shape, ldx)
    D = D0
    for W, b in zip(Ws, bs):
        assert tuple(W.shape) == (D + H, 4 * H) and W.is_contiguous() and tuple(b.shape) == (4 * H,), (W.shape, b.shape)
        _f32(W), _f32(b)
        D = H
    if y is None:
        ldy = H
        y = torch.empty(Tb, B, H, device=dev)
    nbytes = causal_lstm_ws_bytes(L, B, Tb, H)
    if ws is None:
        ws = torch.empty(nbytes // 4, device=dev)
    with _lib.timed('causal_lstm_block'):
        _lib.causal_check(_lib.load_causal().danet_causal_lstm_block(
            _lib.stream(), L, B, Tb, D0, H, ptr(_f32(x)), ldx, _ptrs(Ws), _ptrs(bs), ptr(_f32(h)), ptr(_f32(c)),
            ptr(_f32(y)), ldy, ptr(ws), ws.numel() * ws.element_size()))
    return y


def causal_project(A, M, K, N, lda, W, ldw, out=None, ldo=None):
    '''danet_causal_project, ONE launch: out[M, N] = A[M, K] W[K, N] in the fixed-order arithmetic of the LSTM step;
    row r of the result does not depend on M'''
    if out is None:
        ldo = N
        out = torch.empty(M, N, device=A.device)
    with _lib.timed('causal_project'):
        _lib.causal_check(_lib.load_causal().danet_causal_project(
            _lib.stream(), M, K, N, ptr(_f32(A)), lda, ptr(_f32(W)), ldw, ptr(_f32(out)), ldo))
    return out


# ---- BSS-eval figures of valid / test (include/danet_bss_hip.h) ----------------------------------------
# On the extension library libdanet_bss_hip.so, mapped at the first call: a run with EVAL_BSS_SDR null never gets
# here.  waveforms (ops.metric_synth) -> lagged correlations -> block-Toeplitz systems -> two batched Cholesky
# solves -> decibels, the utterances of a batch in groups whose scratch stays under BSS_SCRATCH_BYTES.
BSS_MAX_C = 4                                        # DANET_BSS_MAX_C
BSS_MAX_L = 512                                      # DANET_BSS_MAX_L
BSS_SCRATCH_BYTES = 256 << 20
_bss_ws = {}             # (device index, stream, g, C, L) -> (scratch, views)


def bss_workspace_bytes(B, C, L):
    '''danet_bss_workspace_bytes'''
    return _lib.bytes_or_raise(_lib.load_bss().danet_bss_workspace_bytes(int(B), int(C), int(L)), _lib.bss_check)


def bss_parts(B, C, L):
    '''[(name, shape, dtype)] of the parts of the buffer of danet_bss_workspace_bytes, in its order'''
    n, f64, i32 = C * L, torch.float64, torch.int32
    return [('R', (B, C, C, 2 * L - 1), f64), ('D', (B, C, C, L), f64), ('ee', (B, C), f64), ('G', (B, n, n), f64),
            ('Gs', (B, C, L, L), f64), ('Xg', (B, C, n), f64), ('Xs', (B, C, C + 1, L), f64), ('fg', (B,), i32),
            ('fs', (B, C), i32), ('per_utt', (B, 4), f64), ('perm_idx', (B,), i32), ('flags', (B,), i32),
            ('mean4', (4,), f64)]


def _bss_workspace(g, C, L, dev):
    '''the views a group of g utterances cuts out of the grow-only scratch 'bss' of this (device, stream): a dict by
    the names of bss_parts; cached per shape'''
    return _scratch('bss', _bss_ws, (g, C, L), lambda: bss_parts(g, C, L), lambda: bss_workspace_bytes(g, C, L), dev)[1]


def bss_xcorr(wav, filter_len, out=None):
    '''float32 waveforms [B, 2C, Ls] (references first) -> (R [B, C, C, 2L - 1], D [B, C, C, L], ee [B, C]), float64,
    ONE launch (danet_bss_xcorr); out: optional (R, D, ee) to write into'''
    B, M, Ls = _chk('wav', wav, torch.float32, dim=3).shape
    assert M % 2 == 0, M
    C, L, dev = M // 2, int(filter_len), wav.device
    out = out or (None, None, None)
    R = _out('R', out[0], (B, C, C, 2 * L - 1), torch.float64, dev)
    D = _out('D', out[1], (B, C, C, L), torch.float64, dev)
    ee = _out('ee', out[2], (B, C), torch.float64, dev)
    with _lib.timed('bss_xcorr'):
        _lib.bss_check(_lib.load_bss().danet_bss_xcorr(_lib.stream(), B, C, Ls, L, ptr(wav), ptr(R), ptr(D), ptr(ee)))
    return R, D, ee


def bss_systems(R, D, out=None):
    '''R [B, C, C, 2L - 1], D [B, C, C, L] -> (G [B, CL, CL], Gs [B, C, L, L], Xg [B, C, CL], Xs [B, C, C + 1, L]),
    ONE launch (danet_bss_systems); out: optional tuple of the four to write into'''
    B, C, L, dev = _chk('R', R, torch.float64, dim=4).shape[0], R.shape[1], D.shape[3], R.device
    _chk('R', R, torch.float64, (B, C, C, 2 * L - 1))
    _chk('D', D, torch.float64, (B, C, C, L), dev=dev)
    out = out or (None,) * 4
    G = _out('G', out[0], (B, C * L, C * L), torch.float64, dev)
    Gs = _out('Gs', out[1], (B, C, L, L), torch.float64, dev)
    Xg = _out('Xg', out[2], (B, C, C * L), torch.float64, dev)
    Xs = _out('Xs', out[3], (B, C, C + 1, L), torch.float64, dev)
    with _lib.timed('bss_systems'):
        _lib.bss_check(_lib.load_bss().danet_bss_systems(_lib.stream(), B, C, L, ptr(R), ptr(D), ptr(G), ptr(Gs),
                                                         ptr(Xg), ptr(Xs)))
    return G, Gs, Xg, Xs


def bss_chol_solve(A, X, flags=None):
    '''IN PLACE: A float64 [nmat, n, n] symmetric positive definite -> its Cholesky factor, X float64 [nmat, nrhs, n]
    (one right-hand side per row) -> the solutions; -> flags int32 [nmat], 1 where a pivot failed
    (danet_bss_chol_solve: blocked, the trailing updates of the whole batch on f64 MFMA)'''
    nmat, n = _chk('A', A, torch.float64, dim=3).shape[:2]
    _chk('X', X, torch.float64, dim=3, dev=A.device)
    assert A.shape[2] == n and X.shape[0] == nmat and X.shape[2] == n, (A.shape, X.shape)
    flags = _out('flags', flags, (nmat,), torch.int32, A.device)
    with _lib.timed('bss_chol_solve'):
        _lib.bss_check(_lib.load_bss().danet_bss_chol_solve(_lib.stream(), nmat, n, X.shape[1], ptr(A), ptr(X),
                                                            ptr(flags)))
    return flags


def bss_finalize(R, D, ee, Xg, Xs, fg, fs, b0=0, out=None):
    '''the correlations, right-hand sides, solutions and factorisation flags of B utterances -> (mean4 [4],
    per_utt [B_all, 4], perm_idx int32 [B_all], flags int32 [B_all]), ONE launch (danet_bss_finalize): rows b0 ..
    b0 + B - 1 are written, and mean4 from all rows when b0 + B = B_all.  out: optional (per_utt, perm_idx, flags,
    mean4) of a batch of B_all utterances to write into (default B_all = B)'''
    B, C, L, dev = R.shape[0], R.shape[1], D.shape[3], R.device
    for name, t, shape, dtype in (('R', R, (B, C, C, 2 * L - 1), torch.float64), ('D', D, (B, C, C, L), torch.float64),
                                  ('ee', ee, (B, C), torch.float64), ('Xg', Xg, (B, C, C * L), torch.float64),
                                  ('Xs', Xs, (B, C, C + 1, L), torch.float64), ('fg', fg, (B,), torch.int32),
                                  ('fs', fs, (B, C), torch.int32)):
        _chk(name, t, dtype, shape, dev=dev)
    per_utt, perm_idx, flags, mean4 = _result(B, 4, dev, flags=True) if out is None else out
    B_all = _check_result(per_utt, perm_idx, flags, mean4, 4)
    with _lib.timed('bss_finalize'):
        _lib.bss_check(_lib.load_bss().danet_bss_finalize(
            _lib.stream(), B, C, L, ptr(R), ptr(D), ptr(ee), ptr(Xg), ptr(Xs), ptr(fg), ptr(fs), int(b0), B_all,
            ptr(per_utt), ptr(perm_idx), ptr(flags), ptr(mean4)))
    return mean4, per_utt, perm_idx, flags


def bss_group(B, C, L):
    '''the utterances ops.bss_eval takes at a time: the most whose scratch stays under BSS_SCRATCH_BYTES (one at least)'''
    return _group(B, BSS_SCRATCH_BYTES, lambda g: bss_workspace_bytes(g, C, L))


def bss_eval(src, est, filter_len=None, fft_stride=None, wav=None, group=None):
    '''BSS-eval SDR, SIR, SAR and SDRi (dB; the rule of include/danet_bss_hip.h) of the waveforms of the UNPERMUTED
    estimates `est` against the references `src`, both complex64 [B, C, T, F] -> (sdr, sir, sar, sdri,
    per_utt [B, 4], perm_idx [B], flags [B]): float64 / int32 device tensors of the caller's own.  wav: the float32
    waveforms [B, 2C, (T - 1) * S] when they exist already (ops.si_sdr_wav), else they are synthesised here
    (ops.metric_synth, into the metric's cached scratch).  filter_len: L (default hparams.EVAL_BSS_FILTER_LEN, 512
    when that is null).  The utterances go through the stages in groups of `group` (default ops.bss_group: the scratch
    stays under BSS_SCRATCH_BYTES); the batch means are formed on the device over all groups by the last group's
    finalize launch, so they do not depend on the grouping.  No host synchronisation.'''
    from .hparams import hparams
    if filter_len is None:
        filter_len = getattr(hparams, 'EVAL_BSS_FILTER_LEN', None) or BSS_MAX_L
    L = int(filter_len)
    B, C, T, F = src.shape
    dev = src.device
    if wav is None:
        wav = synth_wav(src, est, fft_stride)
    assert tuple(_chk('wav', wav, torch.float32).shape[:2]) == (B, 2 * C), wav.shape
    g = bss_group(B, C, L) if group is None else max(1, min(int(group), B))
    out = _result(B, 4, dev, flags=True)
    for b0 in range(0, B, g):
        nb = min(g, B - b0)
        w = _bss_workspace(nb, C, L, dev)
        bss_xcorr(wav[b0:b0 + nb], L, out=(w['R'], w['D'], w['ee']))
        bss_systems(w['R'], w['D'], out=(w['G'], w['Gs'], w['Xg'], w['Xs']))
        bss_chol_solve(w['G'], w['Xg'], w['fg'])
        bss_chol_solve(w['Gs'].view(nb * C, L, L), w['Xs'].view(nb * C, C + 1, L), w['fs'].view(nb * C))
        bss_finalize(w['R'], w['D'], w['ee'], w['Xg'], w['Xs'], w['fg'], w['fs'], b0=b0, out=out)
    per_utt, perm_idx, flags, mean4 = out
    return mean4[0], mean4[1], mean4[2], mean4[3], per_utt, perm_idx, flags


# ---- STOI / ESTOI of valid / test (include/danet_stoi_hip.h) -------------------------------------------
# On the extension library libdanet_stoi_hip.so, mapped at the first call: a run with EVAL_STOI null never gets
# here.  waveforms (ops.metric_synth) -> 10 kHz rows with the mixture -> silent frames of every reference -> band
# magnitudes of the compacted frames -> segment correlations -> permutation search and batch means.
STOI_MAX_C = 4                                       # DANET_STOI_MAX_C
STOI_MAX_TABLE = 16384                               # DANET_STOI_MAX_TABLE
STOI_FS = 10000
STOI_MIN_RATE = 8000
STOI_SCRATCH_BYTES = 256 << 20
_stoi_ws = {}            # (device index, stream, g, C, Ls, U, D) -> (scratch, views)
_stoi_tables = {}        # (device index, SMPRATE) -> dict(U, D, H, h, w, tw, bins, bands)


def stoi_rate(smprate):
    '''SMPRATE -> (U, D, H) of the resampling to 10 kHz (H = 0: the stage is a copy); ValueError naming EVAL_STOI and
    SMPRATE where the table of 2H + 1 entries would not fit or the rate is below 8 kHz'''
    if isinstance(smprate, bool) or not isinstance(smprate, (int, np.integer)) or smprate < STOI_MIN_RATE:
        raise ValueError('EVAL_STOI needs SMPRATE to be an integer >= %d: the fifteen bands reach 4.3 kHz (got '
                         'SMPRATE = %r)' % (STOI_MIN_RATE, smprate))
    g = math.gcd(STOI_FS, int(smprate))
    U, D = STOI_FS // g, int(smprate) // g
    H = 0 if U == D == 1 else 10 * max(U, D)
    if 2 * H + 1 > STOI_MAX_TABLE:
        raise ValueError('EVAL_STOI needs an SMPRATE whose resampling table to 10 kHz has at most %d entries (SMPRATE '
                         '= %d gives U / D = %d / %d and %d entries)' % (STOI_MAX_TABLE, smprate, U, D, 2 * H + 1))
    return U, D, H


def stoi_tables(smprate, dev):
    '''the inputs the library computes nothing of, uploaded once per (device, SMPRATE): h (float32 [2H + 1]), the
    window w (float32 [256]), the twiddle factors tw (float64 [256, 2]) and the band bins (a HOST int32 [15][2])'''
    key = (_dev_index(dev), int(smprate))
    t = _stoi_tables.get(key)
    if t is not None:
        return t
    U, D, H = stoi_rate(smprate)
    if H:
        import scipy.signal
        h = U * scipy.signal.firwin(2 * H + 1, 1.0 / max(U, D), window=('kaiser', 5.0))
    else:
        h = np.ones(1)
    grid = np.arange(257) * (STOI_FS / 512.0)
    edge = lambda e: int(np.argmin(np.abs(grid - 150.0 * 2.0 ** (e / 6.0))))
    bins = tuple((edge(2 * b - 1), edge(2 * b + 1)) for b in range(15))
    ang = -2.0 * np.pi * np.arange(256) / 512.0
    t = dict(U=U, D=D, H=H, bins=bins, bands=(ctypes.c_int32 * 30)(*[v for lo_hi in bins for v in lo_hi]),
             h=torch.from_numpy(h.astype(np.float32)).to(dev),
             w=torch.from_numpy(np.hanning(258)[1:-1].astype(np.float32)).to(dev),
             tw=torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], axis=1)).to(dev))
    _stoi_tables[key] = t
    return t


def _stoi_smprate(smprate):
    from .hparams import hparams
    return int(hparams.SMPRATE if smprate is None else smprate)


def stoi_lengths(Ls, U, D):
    '''(L10, nf): samples of a 10 kHz row and its frames of 256 at hop 128'''
    L10 = -(-int(Ls) * U // D)
    return L10, ((L10 - 256) // 128 + 1 if L10 >= 256 else 0)


def stoi_workspace_bytes(B, C, Ls, U, D):
    '''danet_stoi_workspace_bytes'''
    return _lib.bytes_or_raise(_lib.load_stoi().danet_stoi_workspace_bytes(int(B), int(C), int(Ls), int(U), int(D)),
                               _lib.stoi_check)


def stoi_parts(B, C, Ls, U, D):
    '''[(name, shape, dtype)] of the parts of the buffer of danet_stoi_workspace_bytes, in its order'''
    L10, nf = stoi_lengths(Ls, U, D)
    n, f32, f64, i32 = max(nf, 1), torch.float32, torch.float64, torch.int32
    return [('sig', (B, 2 * C + 1, L10), f32), ('E', (B, C, n), f64), ('mask', (B, C, n), i32),
            ('kidx', (B, C, n), i32), ('M', (B, C), i32), ('Emax', (B, C), f64), ('T', (B, C, C + 2, 15, n), f64),
            ('d', (B, C, C + 1, 2), f64), ('per_utt', (B, 4), f64), ('perm_idx', (B,), i32), ('flags', (B,), i32),
            ('mean4', (4,), f64), ('count', (1,), i32)]


def _stoi_workspace(g, C, Ls, U, D, dev):
    '''the views a group of g utterances cuts out of the grow-only scratch 'stoi' of this (device, stream): a dict by
    the names of stoi_parts; cached per shape'''
    return _scratch('stoi', _stoi_ws, (g, C, Ls, U, D), lambda: stoi_parts(g, C, Ls, U, D),
                    lambda: stoi_workspace_bytes(g, C, Ls, U, D), dev)[1]


def stoi_resample(wav, smprate=None, out=None):
    '''float32 waveforms [B, 2C, Ls] (references first) -> the 10 kHz rows float32 [B, 2C + 1, L10], the last one the
    mixture of the references, ONE launch (danet_stoi_resample); out: optional tensor to write into'''
    B, R, Ls = _chk('wav', wav, torch.float32, dim=3, contiguous=False).shape
    # the strides themselves, not is_contiguous(), which lets any stride pass on a dimension of one element
    assert R % 2 == 0 and wav.stride() == (R * Ls, Ls, 1), (wav.shape, wav.stride())
    t = stoi_tables(_stoi_smprate(smprate), wav.device)
    sig = _out('out', out, (B, R + 1, stoi_lengths(Ls, t['U'], t['D'])[0]), torch.float32, wav.device)
    with _lib.timed('stoi_resample'):
        _lib.stoi_check(_lib.load_stoi().danet_stoi_resample(_lib.stream(), B, R // 2, Ls, t['U'], t['D'], ptr(wav),
                                                             ptr(t['h']), ptr(sig)))
    return sig


def _stoi_sig(sig):
    '''the 10 kHz rows float32 [B, 2C + 1, L10], checked -> (B, C, L10, n = max(nf, 1), device)'''
    B, R, L10 = _chk('sig', sig, torch.float32, dim=3).shape
    assert R % 2, R
    return B, R // 2, L10, max((L10 - 256) // 128 + 1 if L10 >= 256 else 0, 1), sig.device


def stoi_frames(sig, smprate=None, out=None):
    '''the 10 kHz rows [B, 2C + 1, L10] -> (E [B, C, n], mask [B, C, n], kidx [B, C, n], M [B, C], Emax [B, C]) of
    the C references, n = max(nf, 1), ONE launch (danet_stoi_frames); out: optional tuple of the five'''
    B, C, L10, n, dev = _stoi_sig(sig)
    out = out or (None,) * 5
    E = _out('E', out[0], (B, C, n), torch.float64, dev)
    mask = _out('mask', out[1], (B, C, n), torch.int32, dev)
    kidx = _out('kidx', out[2], (B, C, n), torch.int32, dev)
    M = _out('M', out[3], (B, C), torch.int32, dev)
    Emax = _out('Emax', out[4], (B, C), torch.float64, dev)
    t = stoi_tables(_stoi_smprate(smprate), dev)
    with _lib.timed('stoi_frames'):
        _lib.stoi_check(_lib.load_stoi().danet_stoi_frames(_lib.stream(), B, C, L10, ptr(sig), ptr(t['w']), ptr(E),
                                                           ptr(mask), ptr(kidx), ptr(M), ptr(Emax)))
    return E, mask, kidx, M, Emax


def stoi_bands(sig, kidx, M, smprate=None, out=None):
    '''the 10 kHz rows, k(.) and M of the references -> the band magnitudes T float64 [B, C, C + 2, 15, n] of the
    compacted frames of every (reference, paired signal), ONE launch (danet_stoi_bands; none when L10 < 256)'''
    B, C, L10, n, dev = _stoi_sig(sig)
    _chk('kidx', kidx, torch.int32, (B, C, n), dev=dev)
    _chk('M', M, torch.int32, (B, C), dev=dev)
    T = _out('out', out, (B, C, C + 2, 15, n), torch.float64, dev)
    t = stoi_tables(_stoi_smprate(smprate), dev)
    with _lib.timed('stoi_bands'):
        _lib.stoi_check(_lib.load_stoi().danet_stoi_bands(_lib.stream(), B, C, L10, ptr(sig), ptr(t['w']), ptr(t['tw']),
                                                          ctypes.addressof(t['bands']), ptr(kidx), ptr(M), ptr(T)))
    return T


def stoi_segments(T, M, nf, out=None):
    '''T [B, C, C + 2, 15, max(nf, 1)] and M [B, C] -> d float64 [B, C, C + 1, 2]: (STOI, ESTOI) of every reference
    against every estimate and the mixture, ONE launch (danet_stoi_segments)'''
    B, C, dev = _chk('T', T, torch.float64, dim=5).shape[0], T.shape[1], T.device
    assert tuple(T.shape) == (B, C, C + 2, 15, max(int(nf), 1)), (T.shape, nf)
    _chk('M', M, torch.int32, (B, C), dev=dev)
    d = _out('out', out, (B, C, C + 1, 2), torch.float64, dev)
    with _lib.timed('stoi_segments'):
        _lib.stoi_check(_lib.load_stoi().danet_stoi_segments(_lib.stream(), B, C, int(nf), ptr(T), ptr(M), ptr(d)))
    return d


def stoi_finalize(d, M, Emax, nf, b0=0, out=None):
    '''d, M and Emax of B utterances -> (mean4 [4], per_utt [B_all, 4], perm_idx int32 [B_all], flags int32 [B_all],
    count int32 [1]), ONE launch (danet_stoi_finalize): rows b0 .. b0 + B - 1 are written, and mean4 and count from
    all rows when b0 + B = B_all.  out: optional (per_utt, perm_idx, flags, mean4, count) of a batch of B_all
    utterances to write into (default B_all = B)'''
    B, C, dev = d.shape[0], d.shape[1], d.device
    _chk('d', d, torch.float64, (B, C, C + 1, 2), dev=dev)
    _chk('M', M, torch.int32, (B, C), dev=dev)
    _chk('Emax', Emax, torch.float64, (B, C), dev=dev)
    per_utt, perm_idx, flags, mean4, count = _result(B, 4, dev, flags=True, count=True) if out is None else out
    B_all = _check_result(per_utt, perm_idx, flags, mean4, 4)
    _chk('count', count, torch.int32, numel=1, contiguous=False, cuda=False)
    with _lib.timed('stoi_finalize'):
        _lib.stoi_check(_lib.load_stoi().danet_stoi_finalize(
            _lib.stream(), B, C, int(nf), ptr(d), ptr(M), ptr(Emax), int(b0), B_all, ptr(per_utt), ptr(perm_idx),
            ptr(flags), ptr(mean4), ptr(count)))
    return mean4, per_utt, perm_idx, flags, count


def stoi_group(B, C, Ls, U, D):
    '''the utterances ops.stoi_eval takes at a time: the most whose scratch stays under STOI_SCRATCH_BYTES (one at
    least)'''
    return _group(B, STOI_SCRATCH_BYTES, lambda g: stoi_workspace_bytes(g, C, Ls, U, D))


def stoi_eval(src, est, fft_stride=None, wav=None, smprate=None, group=None, with_count=False):
    '''STOI, ESTOI and their improvements over the mixture (the rule of include/danet_stoi_hip.h) of the waveforms of
    the UNPERMUTED estimates `est` against the references `src`, both complex64 [B, C, T, F] -> (stoi, estoi, stoii,
    estoii, per_utt [B, 4], perm_idx [B], flags [B]): float64 / int32 device tensors of the caller's own; with_count:
    an eighth, the int32 [1] count of the utterances behind the means.  wav: the float32 waveforms
    [B, 2C, (T - 1) * S] when they exist already (ops.si_sdr_wav), else they are synthesised here (ops.metric_synth,
    into the metric's cached scratch).  smprate: default hparams.SMPRATE.  The utterances go through the stages in
    groups of `group` (default ops.stoi_group); the batch means are formed on the device over all groups by the last
    group's finalize launch, so they do not depend on the grouping.  Six launches a group, no host synchronisation.'''
    B, C, T, F = src.shape
    dev = src.device
    if wav is None:
        wav = synth_wav(src, est, fft_stride)
    assert tuple(_chk('wav', wav, torch.float32).shape[:2]) == (B, 2 * C), wav.shape
    smprate = _stoi_smprate(smprate)
    t = stoi_tables(smprate, dev)
    U, D, Ls = t['U'], t['D'], wav.shape[2]
    nf = stoi_lengths(Ls, U, D)[1]
    g = stoi_group(B, C, Ls, U, D) if group is None else max(1, min(int(group), B))
    out = _result(B, 4, dev, flags=True, count=True)
    for b0 in range(0, B, g):
        nb = min(g, B - b0)
        w = _stoi_workspace(nb, C, Ls, U, D, dev)
        stoi_resample(wav[b0:b0 + nb], smprate, out=w['sig'])
        stoi_frames(w['sig'], smprate, out=(w['E'], w['mask'], w['kidx'], w['M'], w['Emax']))
        stoi_bands(w['sig'], w['kidx'], w['M'], smprate, out=w['T'])
        stoi_segments(w['T'], w['M'], nf, out=w['d'])
        stoi_finalize(w['d'], w['M'], w['Emax'], nf, b0=b0, out=out)
    per_utt, perm_idx, flags, mean4, count = out
    res = (mean4[0], mean4[1], mean4[2], mean4[3], per_utt, perm_idx, flags)
    return res + (count,) if with_count else res


# ---- waveform metric of a noisy valid / test sweep (include/danet_neval_hip.h) -------------------------
# On the extension library libdanet_neval_hip.so, mapped at the first call: a run with NOISE_EVAL_DIR or EVAL_SI_SDR
# null never gets here.  Three launches: spectra (+ the scaled noise) -> waveforms -> Gram matrices -> decibels; the
# baseline of SI-SDRi is the mixture the model was given, sources + noise.
NEVAL_MAX_C = 4                                      # DANET_NEVAL_MAX_C
_neval_ws = {}           # (device index, stream, B, C, T, N, S) -> (scratch, wav, G, per_utt, mean3, perm_idx)


def neval_synth(src, est, noise, gain, fft_stride, window=None, out=None):
    '''references and UNPERMUTED estimates, complex64 [B, C, T, F], noise complex64 [B, T, F], gain float32 [B] or
    None (= 1) -> float32 waveforms [B, 2C + 1, (T - 1) * S]: references, estimates, then the synthesis of
    fl(gain * noise), ONE launch (danet_neval_synth).  window: float32 device vector [N] (default hparams.FFT_WND).'''
    _chk('src', src, torch.complex64, dim=4, contiguous=False)
    _chk('est', est, torch.complex64, src.shape, dev=src.device, contiguous=False)
    B, C, T, F = src.shape
    _chk('noise', noise, torch.complex64, (B, T, F), dev=src.device, contiguous=False)
    _chk('gain', gain, torch.float32, (B,), dev=src.device, optional=True)
    src, est, noise = src.contiguous(), est.contiguous(), noise.contiguous()
    N = 2 * (F - 1)
    window = _metric_window(src.device) if window is None else _f32(window).contiguous()
    _chk('window', window, torch.float32, numel=N, dev=src.device)
    assert T >= 1, T
    out = _out('out', out, (B, 2 * C + 1, (T - 1) * fft_stride), torch.float32, src.device)
    with _lib.timed('neval_synth'):
        _lib.neval_check(_lib.load_neval().danet_neval_synth(
            _lib.stream(), B, C, T, N, fft_stride, ptr(torch.view_as_real(src)), ptr(torch.view_as_real(est)),
            ptr(torch.view_as_real(noise)), ptr(gain), ptr(window), ptr(out)))
    return out


def neval_gram(wav, out=None):
    '''float32 [B, M, Ls], M <= 9 -> float64 Gram matrices [B, M, M], ONE launch (danet_neval_gram: the tree of
    danet_metric_gram; symmetric bit for bit)'''
    return _wave_gram('neval', wav, out)


def neval_finalize(G, out=None):
    '''float64 Gram matrices [B, 2C + 1, 2C + 1] -> (mean3 [3], per_utt [B, 3], perm_idx int32 [B]): SI-SDR, SI-SDRi
    against the noisy mixture, nSNR; ONE launch (danet_neval_si_sdr); out: optional (per_utt, perm_idx, mean3)'''
    return _wave_finalize('neval', 3, G, out)


def si_sdr_noisy(src, est, noise, gain=None, fft_stride=None):
    '''SI-SDR, SI-SDRi and nSNR (dB) of the waveforms of the UNPERMUTED estimates `est` against the clean references
    `src`, both complex64 [B, C, T, F], for a mixture that held fl(gain * noise) as well (noise complex64 [B, T, F],
    gain float32 [B] or None = 1): the baseline of SI-SDRi is that noisy mixture, nSNR the ratio of the summed
    sources to the noise -> (si_sdr, si_sdri, nsnr, per_utt [B, 3], perm_idx [B]): float64 / int32 device tensors
    of the caller's own (allocated here; the waveforms and Gram matrices live in a scratch cached per shape).  Three
    launches and nothing else on the device, no host synchronisation.'''
    S = _stride(fft_stride)
    B, C, T, F = src.shape
    ws = _wave_workspace('neval', _neval_ws, 2 * C + 1, 3, B, C, T, 2 * (F - 1), S, src.device)
    wav, G = ws[1], ws[2]
    neval_synth(src, est, noise, gain, S, out=wav)
    neval_gram(wav, out=G)
    mean3, per_utt, perm_idx = neval_finalize(G, out=_result(B, 3, src.device))
    return mean3[0], mean3[1], mean3[2], per_utt, perm_idx


# ---- waveform training loss (include/danet_wavloss_hip.h) ---------------------------------------------
# On the extension library libdanet_wavloss_hip.so, mapped at the first call: a run with TRAIN_LOSS null or
# "pit-mse" never gets here.  Forward: reattach_phase -> metric_synth -> metric_gram (libdanet_metric_hip.so) ->
# wavloss_fwd; backward: ONE launch, wavloss_bwd.
WAVLOSS_MAX_C = 4                                    # DANET_WAVLOSS_MAX_C


def wavloss_tile_frames(N):
    '''DANET_WAVLOSS_TILE_FRAMES(N): the frames one workgroup of danet_wavloss_bwd takes'''
    return min(32, (16384 - 3 * N // 2) // (3 * N // 2))


def wavloss_fwd(G, out=None):
    '''float64 Gram matrices [B, 2C, 2C] -> (loss_f64 [1], loss_f32 [1], per_utt [B], perm_idx int32 [B],
    pair int32 [B, C], coef float64 [B, C, 2]), ONE launch (danet_wavloss_fwd); out: optional tuple of the six to
    write into'''
    B, M = _chk('G', G, torch.float64, dim=3).shape[:2]
    assert M == G.shape[2] and M % 2 == 0, G.shape
    C, dev = M // 2, G.device
    if out is None:
        out = (torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, C, dtype=torch.int32, device=dev), torch.empty(B, C, 2, dtype=torch.float64, device=dev))
    loss64, loss32, per_utt, perm_idx, pair, coef = out
    with _lib.timed('wavloss_fwd'):
        _lib.wavloss_check(_lib.load_wavloss().danet_wavloss_fwd(
            _lib.stream(), B, C, ptr(G), ptr(loss64), ptr(loss32), ptr(per_utt), ptr(perm_idx), ptr(pair), ptr(coef)))
    return out


def wavloss_bwd(wav, pair, coef, fft_size, fft_stride, window=None, dloss=None, phasor=None, out=None):
    '''the gradient of the waveform loss with respect to the estimates' spectra, ONE launch (danet_wavloss_bwd):
    wav float32 [B, 2C, (T - 1) * S] (ops.metric_synth), pair int32 [B, C] and coef float64 [B, C, 2]
    (ops.wavloss_fwd) -> complex64 dX [B, C, T, F], or with phasor float32 [B, T, F, 2] the real float32
    dsep [B, C, T, F].  dloss: float32 device scalar or None (= 1); window: float32 device vector [N] (default
    hparams.FFT_WND, uploaded once).'''
    B, M, Ls = _chk('wav', wav, torch.float32, dim=3).shape
    N, S = int(fft_size), int(fft_stride)
    assert M % 2 == 0 and S >= 1 and Ls % S == 0, (M, Ls, S)
    C, T, F, dev = M // 2, Ls // S + 1, N // 2 + 1, wav.device
    _chk('pair', pair, torch.int32, (B, C), dev=dev)
    _chk('coef', coef, torch.float64, (B, C, 2), dev=dev)
    window = _metric_window(dev) if window is None else _f32(window).contiguous()
    _chk('window', window, torch.float32, numel=N, dev=dev)
    _chk('dloss', dloss, torch.float32, numel=1, dev=dev, contiguous=False, optional=True)
    _chk('phasor', phasor, torch.float32, (B, T, F, 2), dev=dev, optional=True)
    out = _out('out', out, (B, C, T, F), torch.complex64 if phasor is None else torch.float32, dev)
    with _lib.timed('wavloss_bwd'):
        _lib.wavloss_check(_lib.load_wavloss().danet_wavloss_bwd(
            _lib.stream(), B, C, T, N, S, ptr(wav), ptr(pair), ptr(coef), ptr(window), ptr(dloss), ptr(phasor),
            ptr(torch.view_as_real(out)) if phasor is None else ptr(out)))
    return out


class SiSdrLossFn(torch.autograd.Function):
    '''-SI-SDR (dB) of the separated waveforms under the metric's permutation rule (include/danet_wavloss_hip.h):
    (src complex64 [B,C,T,F], sep_pwr [B,C,T,F], phasor [B,T,F,2]) -> (loss, perm_idx).  Shaped like PitMseFn: the
    gradient goes to sep_pwr only, backward is ONE launch.  The waveforms must survive until backward, so they
    are a tensor of this call's own, not the cached scratch ops.si_sdr shares with valid_step.'''

    @staticmethod
    def forward(ctx, src, sep_pwr, phasor):
        from .hparams import hparams
        assert src.dtype == torch.complex64
        B, C, T, F = sep_pwr.shape
        S = int(hparams.FFT_STRIDE)
        sep_pwr = _f32(sep_pwr.contiguous())
        phasor = _f32(phasor.contiguous())
        est = reattach_phase(sep_pwr, phasor)                  # unpermuted: the loss does its own search
        wav = metric_synth(src, est, S)
        loss64, loss, _per_utt, perm_idx, pair, coef = wavloss_fwd(metric_gram(wav))
        ctx.save_for_backward(wav, pair, coef, phasor)
        ctx.args = (2 * (F - 1), S)
        ctx.mark_non_differentiable(perm_idx)
        ctx.set_materialize_grads(False)
        return loss.view(()), perm_idx

    @staticmethod
    def backward(ctx, dloss, _dperm):
        if dloss is None:
            return None, None, None
        wav, pair, coef, phasor = ctx.saved_tensors
        N, S = ctx.args
        # dloss is a device scalar: the kernel reads it (no host sync, no extra pass)
        dsep = wavloss_bwd(wav, pair, coef, N, S, dloss=_f32(dloss.contiguous()), phasor=phasor)
        return None, dsep, None


def si_sdr_loss(s_x, s_y_pwr, phasor):
    '''(loss, loss_perm_idx): minus the SI-SDR in dB of the waveforms of the separated magnitudes `s_y_pwr` with
    the mixture phase against the references `s_x`, a float32 device scalar, and the index of every utterance's
    permutation in itertools.permutations order'''
    return SiSdrLossFn.apply(s_x, s_y_pwr, phasor)


# ---- deep-clustering auxiliary loss (include/danet_dpcl_hip.h) -----------------------------------------
# On the extension library libdanet_dpcl_hip.so, mapped at the first call: a run with DPCL_WEIGHT null never gets
# here.  Forward: dpcl_stats -> dpcl_finalize (which also adds the main loss); backward: ONE launch, dpcl_bwd.
DPCL_MAX_E = 64                                      # DANET_DPCL_MAX_E
DPCL_MAX_C = 4                                       # DANET_DPCL_MAX_C


def dpcl_workspace_bytes(B, N, E, C):
    '''danet_dpcl_workspace_bytes(B, N, E, C): the bytes dpcl_stats writes and dpcl_finalize reads'''
    return _lib.bytes_or_raise(_lib.load_dpcl().danet_dpcl_workspace_bytes(int(B), int(N), int(E), int(C)),
                               _lib.dpcl_check)


def _dpcl_shapes(embed, src_pwr):
    B, N, E = _chk('embed', embed, torch.float32, dim=3).shape
    _chk('src_pwr', src_pwr, torch.float32, dim=3, dev=embed.device)
    assert src_pwr.shape[0] == B and src_pwr.shape[2] == N, (src_pwr.shape, embed.shape)
    return B, N, E, src_pwr.shape[1]


def dpcl_stats(embed, src_pwr, ws=None):
    '''embed float32 [B, N, E], src_pwr float32 [B, C, N] -> the per-chunk partial sums, a uint8 workspace of
    dpcl_workspace_bytes(B, N, E, C) bytes (ws: one to write into), ONE launch (danet_dpcl_stats)'''
    B, N, E, C = _dpcl_shapes(embed, src_pwr)
    if ws is None:
        ws = torch.empty(dpcl_workspace_bytes(B, N, E, C), dtype=torch.uint8, device=embed.device)
    _chk('ws', ws, torch.uint8, dev=embed.device)
    with _lib.timed('dpcl_stats'):
        _lib.dpcl_check(_lib.load_dpcl().danet_dpcl_stats(_lib.stream(), B, N, E, C, ptr(embed), ptr(src_pwr), ptr(ws),
                                                          ws.numel()))
    return ws


def dpcl_finalize(ws, B, N, E, C, alpha, main=None, out=None):
    '''the workspace of dpcl_stats -> (per_utt float64 [B], dpcl float32 [1], total float32 [1] = main + alpha * dpcl,
    tables float32 [B, E, E + C], cs float32 [B, C + 1]), ONE launch (danet_dpcl_finalize).  main: float32 device
    scalar or None (= 0); alpha: a host number; out: optional tuple of the five to write into'''
    dev = _chk('ws', ws, torch.uint8).device
    _chk('main', main, torch.float32, numel=1, dev=dev, contiguous=False, optional=True)
    if out is None:
        out = (torch.empty(B, dtype=torch.float64, device=dev), torch.empty(1, device=dev), torch.empty(1, device=dev),
               torch.empty(B, E, E + C, device=dev), torch.empty(B, C + 1, device=dev))
    per_utt, dpcl, total, tables, cs = out
    _chk('per_utt', per_utt, torch.float64, numel=B, cuda=False)
    for name, t, n in (('dpcl', dpcl, 1), ('total', total, 1), ('tables', tables, B * E * (E + C)), ('cs', cs, B * (C + 1))):
        _chk(name, t, torch.float32, numel=n, dev=dev)
    with _lib.timed('dpcl_finalize'):
        _lib.dpcl_check(_lib.load_dpcl().danet_dpcl_finalize(
            _lib.stream(), B, N, E, C, ptr(ws), ws.numel(), ptr(main), float(alpha), ptr(per_utt), ptr(dpcl),
            ptr(total), ptr(tables), ptr(cs)))
    return out


def dpcl_bwd(embed, src_pwr, tables, cs, scale, dloss=None, out=None):
    '''the gradient of alpha * dpcl with respect to the embedding, ONE launch (danet_dpcl_bwd): tables, cs as
    dpcl_finalize wrote them, scale = alpha / B (a host number), dloss float32 device scalar or None (= 1)
    -> dembed float32 [B, N, E]'''
    B, N, E, C = _dpcl_shapes(embed, src_pwr)
    dev = embed.device
    _chk('tables', tables, torch.float32, (B, E, E + C), dev=dev)
    _chk('cs', cs, torch.float32, (B, C + 1), dev=dev)
    _chk('dloss', dloss, torch.float32, numel=1, dev=dev, contiguous=False, optional=True)
    out = _out('out', out, (B, N, E), torch.float32, dev)
    with _lib.timed('dpcl_bwd'):
        _lib.dpcl_check(_lib.load_dpcl().danet_dpcl_bwd(_lib.stream(), B, N, E, C, ptr(embed), ptr(src_pwr),
                                                        ptr(tables), ptr(cs), ptr(dloss), float(scale), ptr(out)))
    return out


class DpclLossFn(torch.autograd.Function):
    '''main + alpha * (deep-clustering affinity loss of the embedding against the ideal binary mask of src_pwr)
    (include/danet_dpcl_hip.h): (embed [B,N,E], src_pwr [B,C,N], main scalar, alpha) -> (total, dpcl).  The sum with
    `main` happens in the finalize kernel; backward is ONE launch and hands `main` the incoming gradient as it is.'''

    @staticmethod
    def forward(ctx, embed, src_pwr, main, alpha):
        embed = _f32(embed.contiguous())
        src_pwr = _f32(src_pwr.contiguous())
        B, N, E, C = _dpcl_shapes(embed, src_pwr)
        if _chain():
            # `main` may still be queued for the side stream (SeparatePitFn's finalize): it has to exist before the
            # kernel that adds to it, and the tables have to exist before this Function's backward
            _flush_lazy(embed.device)
        ws = dpcl_stats(embed, src_pwr)
        _per_utt, dpcl, total, tables, cs = dpcl_finalize(ws, B, N, E, C, alpha, main=_f32(main))
        ctx.save_for_backward(embed, src_pwr, tables, cs)
        ctx.scale = float(alpha) / B
        total, dpcl = total.view(()), dpcl.view(())
        ctx.mark_non_differentiable(dpcl)
        ctx.set_materialize_grads(False)
        return total, dpcl

    @staticmethod
    def backward(ctx, dtotal, _ddpcl):
        if dtotal is None:
            return None, None, None, None
        embed, src_pwr, tables, cs = ctx.saved_tensors
        dembed = None
        if ctx.needs_input_grad[0]:
            # dtotal is a device scalar: the kernel reads it (no host sync, no extra pass)
            dembed = dpcl_bwd(embed, src_pwr, tables, cs, ctx.scale, dloss=_f32(dtotal.contiguous()))
        return dembed, None, dtotal, None


def dpcl_loss(s_embed_flat, s_src_pwr, main, alpha):
    '''(total, dpcl): total = main + alpha * dpcl as a float32 device scalar, differentiable in the embedding
    [B, N, E] and in `main`; dpcl = the mean deep-clustering affinity loss, not differentiable.  s_src_pwr [B, C, T, F]
    or [B, C, N]: the clean sources' magnitudes'''
    B, N = s_embed_flat.shape[0], s_embed_flat.shape[1]
    return DpclLossFn.apply(s_embed_flat, s_src_pwr.reshape(B, -1, N), main, alpha)


# ---- stitching of chunked inference (include/danet_stitch_hip.h) ---------------------------------------
# On the extension library libdanet_stitch_hip.so, mapped at the first call: a run with INFER_CHUNK_LEN null, and an
# input of at most one chunk, never gets here.  Three launches: overlap affinities -> permutation chain -> merge.
STITCH_MAX_C = 4                                     # DANET_STITCH_MAX_C
_stitch_ws = {}          # (device index, stream, n, C, L, F, V, T) -> (scratch, views)
_stitch_fades = {}       # (device index, V) -> float32 device vector [V]


def stitch_chunks(T, L, V):
    '''n of the plan of include/danet_stitch_hip.h (1 when T <= L): danet_stitch_chunks, a pure host function'''
    n = _lib.load_stitch().danet_stitch_chunks(int(T), int(L), int(V))
    if n < 0:
        _lib.stitch_check(n)
    return n


def stitch_plan(T, L, V):
    '''the chunk starts [s_0, ..., s_{n-1}] of the plan: s_i = i * (L - V), the last chunk slid back to end at T'''
    n = stitch_chunks(T, L, V)
    if n == 1:
        return [0]
    return [i * (L - V) for i in range(n - 1)] + [T - L]


def stitch_workspace_bytes(T, L, V, C, F):
    '''danet_stitch_workspace_bytes: the bytes stitch_affinity writes and stitch_assign reads'''
    return _lib.bytes_or_raise(_lib.load_stitch().danet_stitch_workspace_bytes(int(T), int(L), int(V), int(C), int(F)),
                               _lib.stitch_check)


def stitch_fade(V, dev):
    '''w_k = (k + 1) / (V + 1), k < V: computed in float64, rounded once to float32, uploaded once per (device, V)'''
    key = (_dev_index(dev), int(V))
    t = _stitch_fades.get(key)
    if t is None:
        w = ((np.arange(V, dtype=np.float64) + 1.0) / (V + 1.0)).astype(np.float32)
        t = _stitch_fades[key] = torch.from_numpy(w).to(dev)
    return t


def _stitch_shapes(mags, T, V):
    n, C, L, F = _chk('mags', mags, torch.float32, dim=4).shape
    assert n == stitch_chunks(T, L, V), (n, T, L, V)
    return n, C, L, F


def stitch_affinity(mags, T, V, ws=None):
    '''mags float32 [n, C, L, F] -> the per-pair, per-tile float64 partials of S, a uint8 workspace of
    stitch_workspace_bytes(T, L, V, C, F) bytes (ws: one to write into), ONE launch (danet_stitch_affinity)'''
    n, C, L, F = _stitch_shapes(mags, T, V)
    if ws is None:
        ws = torch.empty(stitch_workspace_bytes(T, L, V, C, F), dtype=torch.uint8, device=mags.device)
    _chk('ws', ws, torch.uint8, dev=mags.device)
    with _lib.timed('stitch_affinity'):
        _lib.stitch_check(_lib.load_stitch().danet_stitch_affinity(_lib.stream(), T, L, V, C, F, ptr(mags), ptr(ws),
                                                                   ws.numel()))
    return ws


def stitch_assign(ws, T, L, V, C, F, out=None):
    '''the workspace of stitch_affinity -> (S float64 [n - 1, C, C], perm int32 [n, C]), ONE launch of one workgroup
    (danet_stitch_assign): perm[i][c] is the channel of chunk i that is output channel c.  out: optional (S, perm)'''
    _chk('ws', ws, torch.uint8)
    n = stitch_chunks(T, L, V)
    if out is None:
        out = (torch.empty(max(n - 1, 0), C, C, dtype=torch.float64, device=ws.device),
               torch.empty(n, C, dtype=torch.int32, device=ws.device))
    S, perm = out
    _chk('S', S, torch.float64, numel=(n - 1) * C * C, dev=ws.device)
    _chk('perm', perm, torch.int32, numel=n * C, dev=ws.device)
    with _lib.timed('stitch_assign'):
        _lib.stitch_check(_lib.load_stitch().danet_stitch_assign(_lib.stream(), T, L, V, C, F, ptr(ws), ws.numel(),
                                                                 ptr(S), ptr(perm)))
    return S, perm


def stitch_merge(mags, phasor, perm, T, V, fade=None, out=None):
    '''mags float32 [n, C, L, F], phasor float32 [n, L, F, 2], perm int32 [n, C] -> complex64 [C, T, F]: the owner
    chunk's magnitudes (cross-faded with the next chunk's on the last V frames of every chunk but the last) times
    the mixture phasor, ONE launch (danet_stitch_merge).  fade: float32 device vector [V] (default stitch_fade)'''
    n, C, L, F = _stitch_shapes(mags, T, V)
    dev = mags.device
    _chk('phasor', phasor, torch.float32, (n, L, F, 2), dev=dev)
    _chk('perm', perm, torch.int32, (n, C), dev=dev)
    fade = stitch_fade(V, dev) if fade is None else fade
    _chk('fade', fade, torch.float32, numel=V, dev=dev)
    out = _out('out', out, (C, T, F), torch.complex64, dev)
    with _lib.timed('stitch_merge'):
        _lib.stitch_check(_lib.load_stitch().danet_stitch_merge(
            _lib.stream(), T, L, V, C, F, ptr(mags), ptr(phasor), ptr(fade), ptr(perm), ptr(torch.view_as_real(out))))
    return out


def _stitch_parts(n, C, L, F, T, V):
    '''[(name, shape, dtype)] of the scratch of ops.stitch: the library's workspace, then S and perm, its own'''
    return [('partials', (stitch_workspace_bytes(T, L, V, C, F),), torch.uint8), ('S', (n - 1, C, C), torch.float64),
            ('perm', (n, C), torch.int32)]


def _stitch_workspace(n, C, L, F, T, V, dev):
    '''(buffer, partials, S, perm): the views one shape cuts out of the grow-only scratch 'stitch' of this (device,
    stream), each at a multiple of 256 bytes; cached per shape'''
    buf, v = _scratch('stitch', _stitch_ws, (n, C, L, F, V, T), lambda: _stitch_parts(n, C, L, F, T, V), None, dev)
    return buf, v['partials'], v['S'], v['perm']


def stitch(mags, phasor, T, V):
    '''the separated chunks of one recording -> its separated spectra: mags float32 [n, C, L, F] (the separator's
    output per chunk, channels in each chunk's own order), phasor float32 [n, L, F, 2], the plan (T, L, V) of
    include/danet_stitch_hip.h -> complex64 [C, T, F], output channel c following one speaker across the chunks.
    Three launches and nothing else on the device, no host synchronisation; the partials, S and the permutation chain
    live in a scratch cached per shape, the result is the caller's own.'''
    n, C, L, F = _stitch_shapes(mags, T, V)
    _buf, part, S, perm = _stitch_workspace(n, C, L, F, T, V, mags.device)
    stitch_affinity(mags, T, V, ws=part)
    stitch_assign(part, T, L, V, C, F, out=(S, perm))
    return stitch_merge(mags, phasor, perm, T, V)


# ---------------------------------------------------------------------------
# LSTM layer (both directions), raw forward / backward on time-major tensors
# ---------------------------------------------------------------------------
class _LayerCtx(object):
    __slots__ = ('x', 'ldx', 'D', 'T', 'B', 'H', 'ndir', 'ypad', 'gates', 'cells',
                 'Ws', 'bs')


# ---- inverted dropout behind the BiLSTM layers (app/modules.py:137) ------------------------------
# On the extension library libdanet_dropout_hip.so (include/danet_dropout_hip.h).  The mask is never
# stored: it is a pure function of (key0, key1, stream_id, step, logical element index), so the
# backward pass -- and a float64 restatement on another machine -- regenerate it.
def dropout_threshold(keep):
    '''keep probability -> the 32-bit threshold an element's Philox word is compared with'''
    return min(0xffffffff, int(float(keep) * 4294967296.0))


def dropout_scale(keep):
    '''float32(1 / keep): one double division, rounded once'''
    return ctypes.c_float(1.0 / float(keep)).value


class DropoutSpec(object):
    '''What one model step's dropout masks are drawn from: keep probability, Philox key
    (key0 = the model's seed, key1 = the data-parallel rank), `step` (the train step's index) --
    and a counter that hands out stream ids, one per BiLSTM layer in creation order, so a layer
    draws the same stream in its forward and its backward pass.'''
    __slots__ = ('keep', 'key0', 'key1', 'step', 'threshold', 'scale', '_next')

    def __init__(self, keep, key0=0, key1=0, step=0):
        keep = float(keep)
        if not 0.0 < keep <= 1.0:
            raise ValueError('dropout keep probability must lie in (0, 1], got %r' % keep)
        self.keep = keep
        self.key0, self.key1, self.step = int(key0) & 0xffffffff, int(key1) & 0xffffffff, int(step) & 0xffffffff
        self.threshold, self.scale = dropout_threshold(keep), dropout_scale(keep)
        self._next = 0

    @property
    def active(self):
        return self.keep < 1.0

    def take(self, n=1):
        '''the first of `n` consecutive fresh stream ids'''
        first = self._next
        self._next += n
        return first


def dropout_apply(x, y, rows, cols, ldx, ldy, spec, stream_id):
    '''y[r][c] = x[r][c] * scale where the (spec, stream_id) mask keeps logical element r * cols + c,
    else 0 (danet_dropout_apply; y may be x).  Forward and backward are this same call.'''
    with _lib.timed('dropout'):
        _lib.dropout_check(_lib.load_dropout().danet_dropout_apply(
            _lib.stream(), rows, cols, ptr(_f32(x)), ldx, ptr(_f32(y)), ldy, spec.threshold, spec.scale,
            spec.key0, spec.key1, stream_id, spec.step))
    return y


_dropout_cur = [None]


class dropout_scope(object):
    '''with ops.dropout_scope(spec): the BiLSTM layers applied inside (LstmLayerFn with two directions,
    RnnEncoderFn with ndir == 2, ConvBiLstmEncoderFn) drop their outputs by `spec`; None or
    keep == 1: today's path, no launch, no allocation, the extension library stays unloaded.'''

    def __init__(self, spec):
        self.spec = spec if (spec is not None and spec.active) else None

    def __enter__(self):
        self.prev, _dropout_cur[0] = _dropout_cur[0], self.spec
        return self.spec

    def __exit__(self, *exc):
        _dropout_cur[0] = self.prev
        return False


# ---- hand-off status of the persistent kernels + bounded host run-ahead -------
# ONE sticky 4-byte word per device (include/danet_hip.h: `status` of danet_lstm_fwd/bwd):
# the kernels store DANET_STATUS_TIMEOUT (the bit pattern of 1.0f) into it when a bounded
# inter-workgroup wait times out.  Where it lives:
#   * single process: in PINNED, device-mapped host memory -- the kernels write it across
#     the bus (only on a timeout; they read it once per 256 failed polls), the host reads
#     it directly once a step's event has completed.  No copy, no extra launch.
#   * data parallel: Model points it at the 4 spare floats behind its flat gradient bucket,
#     so the word rides in the step's gradient all-reduce (SUM of 1.0f per timed-out rank):
#     after the reduction every rank holds the same value and they all raise at the same
#     step instead of one rank leaving the others hanging in the next collective.  The
#     reduced word is copied to pinned memory asynchronously once per step.
# `StepFence` bounds how far the host may run ahead of the GPU: Model.train_step /
# valid_step / infer record an event when a step has been enqueued and wait for the event
# of the step MAX_STEPS_IN_FLIGHT back before enqueuing the next.  A step whose event has
# completed is "retired": its status is inspected then, so a timeout raises DanetHipError
# at most MAX_STEPS_IN_FLIGHT steps later (round 2 polled every 16 calls).  Bounding the
# run-ahead also keeps the host from ever sitting 8-9 steps (30 ms of queued kernels)
# ahead of the GPU -- the situation in which the one-off 13-19 ms recurrent-kernel stall
# of DESIGN.md 5 was observed.
import collections as _collections
import os as _os

MAX_STEPS_IN_FLIGHT = int(_os.environ.get('DANET_MAX_STEPS_IN_FLIGHT', '4'))
STATUS_HOST = _os.environ.get('DANET_STATUS_HOST', '1') == '1'
TIMEOUT_MSG = ('persistent LSTM kernel: an inter-workgroup hand-off timed out -- the outputs of '
               'that launch (and everything computed from them) are invalid')


class _DeviceStatus(object):
    __slots__ = ('dev', 'word', 'own', 'host_mapped', 'slots', 'queue', 'n', 'retired', 'events')

    def __init__(self, dev):
        self.dev = dev
        if STATUS_HOST:
            self.own = torch.zeros(4, dtype=torch.int32).pin_memory()
        else:
            self.own = torch.zeros(4, dtype=torch.int32, device=dev)
        self.word, self.host_mapped = self.own, STATUS_HOST
        self.slots = torch.zeros(MAX_STEPS_IN_FLIGHT + 2, 4, dtype=torch.int32).pin_memory()
        self.queue = _collections.deque()     # (event, slot or -1, may_raise)
        self.n = 0
        self.retired = 0
        self.events = []                      # ring of re-recorded step events (created once)


_status = {}


def _dev_status(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _status.get(key)
    if st is None:
        st = _status[key] = _DeviceStatus(torch.device('cuda', key))
    return st


def status_word(dev):
    '''the device's sticky 4 x int32 status tensor (element 0 = LSTM hand-off) that the
    launches are given; pinned host memory or device memory (see above)'''
    return _dev_status(dev).word


def set_status_word(dev, word=None):
    '''point the device's status word at caller-owned DEVICE memory (an int32 view of 4
    elements; Model uses the tail of its gradient bucket under data parallelism); None
    restores the process-owned word'''
    st = _dev_status(dev)
    torch.cuda.synchronize(st.dev)
    st.queue.clear()
    if word is None:
        st.word, st.host_mapped = st.own, STATUS_HOST
    else:
        assert word.is_cuda and word.dtype == torch.int32 and word.numel() == 4
        st.word, st.host_mapped = word, False


def _word_flag(st):
    '''current value of word 0 (caller has synchronised what it needs)'''
    return int(st.word[0].item())


def _raise_timeout(st):
    torch.cuda.synchronize(st.dev)
    st.word.zero_()              # so the caller may restore parameters and go on
    st.queue.clear()
    raise _lib.DanetHipError(TIMEOUT_MSG)


def _retire(st, block):
    ev, slot, may_raise = st.queue[0]
    if block:
        ev.synchronize()
    elif not ev.query():
        return False
    st.queue.popleft()
    st.retired += 1
    flag = int(st.slots[slot, 0]) if slot >= 0 else int(st.word[0])
    if flag != 0 and may_raise:
        _raise_timeout(st)
    return True


def _collective():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


def poll_status(dev):
    '''admission of a new step (called first by Model.train_step / valid_step / infer):
    retire every completed step, wait until fewer than MAX_STEPS_IN_FLIGHT are in flight;
    raises DanetHipError when a retired step recorded a hand-off timeout.

    Under torch.distributed the retirement is DETERMINISTIC: at the admission of step n a rank
    retires exactly step n - MAX_STEPS_IN_FLIGHT (blocking on its event) and nothing else -- no
    opportunistic `query()` path, whose outcome depends on how far each rank's GPU happens to
    be.  Every rank issues the same sequence of steps and the flag of step k is the same on
    every rank (it rides in that step's gradient all-reduce), so all ranks raise at the
    admission of the SAME step, with the same collectives enqueued behind it
    (test_handoff_timeout_raises_at_the_same_step_on_every_rank_gloo_world2).'''
    st = _dev_status(dev)
    if not _collective():
        while st.queue and _retire(st, block=False):
            pass
    while len(st.queue) >= max(MAX_STEPS_IN_FLIGHT, 1):
        _retire(st, block=True)


def _record_event(st):
    '''the event of the step just enqueued, from a ring of MAX_STEPS_IN_FLIGHT + 2 events that
    are created once and re-recorded: an entry is reused only after the step it stood for has
    been retired (the queue never holds more than MAX_STEPS_IN_FLIGHT entries)'''
    ring = getattr(st, 'events', None)
    if ring is None:                          # (tests build the record by hand)
        ring = st.events = []
    n = max(MAX_STEPS_IN_FLIGHT, 1) + 2
    if len(ring) < n:
        ring.append(torch.cuda.Event())
        ev = ring[-1]
    else:
        ev = ring[st.n % n]
    ev.record()
    return ev


def step_done(dev, collective_consistent=True):
    '''a step has been enqueued on the current stream: record its event (and, for a
    device-resident word, an asynchronous 16-byte snapshot into pinned memory).
    collective_consistent=False (data parallel, a step without a gradient all-reduce): the
    word is rank-local, so retiring the step does not raise -- `check_status` does, on
    every rank together.'''
    st = _dev_status(dev)
    slot = -1
    if not st.host_mapped:
        slot = st.n % st.slots.shape[0]
        st.slots[slot].copy_(st.word, non_blocking=True)
    st.n += 1
    st.queue.append((_record_event(st), slot, collective_consistent))


def check_status(dev=None):
    '''blocking check (end of an epoch / a sweep, before results are written, tests);
    raises DanetHipError on a recorded timeout.  Under torch.distributed the flag is
    MAX-reduced first, so every rank raises (or none does).'''
    for st in ([_dev_status(dev)] if dev is not None else list(_status.values())):
        torch.cuda.synchronize(st.dev)
        st.queue.clear()
        flag = 1 if _word_flag(st) != 0 else 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            t = torch.tensor([flag], dtype=torch.int32, device=st.dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            flag = int(t.item())
        if flag != 0:
            _raise_timeout(st)


def lstm_status_ok():
    '''True when no persistent-LSTM launch since the last call reported an
    inter-workgroup timeout (clears the word).  Synchronises.'''
    ok = True
    for st in _status.values():
        torch.cuda.synchronize(st.dev)
        st.queue.clear()
        if _word_flag(st) != 0:
            ok = False
            st.word.zero_()
    return ok


def _lstm_ws(T, B, H, ndir, dev):
    n = _lib.ws_bytes(_lib.WS_LSTM, T, B, H, ndir)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


# ---- concurrent chains on side HIP streams ---------------------------------
# The GEMMs of the two scan directions (and dWx / dWh / dX in backward) are
# independent and individually too small to fill 256 CUs evenly (e.g. 320 tiles);
# issued on separate streams their tiles co-schedule.  All tensors are allocated
# on the main stream and the main stream joins the side streams before anything
# is returned, so the caching allocator never recycles memory still in use.
_side = {}
SIDE_STREAMS = int(__import__('os').environ.get('DANET_SIDE_STREAMS', '1'))
# persistent-workgroup cap for GEMMs that run under a BPTT kernel (per chain; 0 = off).
# Measured at cfg 2: caps of 32..96 all LOSE (5.4-7.1 ms/step vs 5.2 uncapped): the
# interference is fabric contention on the exchange hops, not CU placement.
OVERLAP_GEMM_WGS = _lib.expert('overlap_gemm_wgs', 0)


def _side_streams(dev, n):
    # (stream priorities were measured in round 6 -- side streams at priority 1 / -1 against the main
    # stream's 0: 2.402 / 2.399 against 2.401 ms per cfg-2 step, BPTT 316.0 / 315.6 against 315.6 us: the
    # weight-gradient group's cost to the BPTT kernel is not a matter of dispatch priority)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    pool = _side.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:n]


_copy = {}
# which stream uploads ride on (feed.BatchFeed): 'side' = the first side stream, 'own' = a stream
# of their own.  HIP maps streams onto a handful of hardware queues; a third busy stream lands on
# the main or the side stream's queue depending on creation order and the kernels of the two then
# serialise: the same loop measured 3.14 or 4.2 ms per cfg-2 step from one stream object to the
# next (tools/feed_probe.py, profiles/r04_feed_probe.txt).  The side stream exists anyway and is
# idle at the step boundary, where the feed issues the upload of the next batch.
COPY_STREAM = _lib.expert('copy_stream', 'side')


def copy_stream(dev):
    '''the upload stream of a device (created once per process)'''
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _copy.get(key)
    if st is None:
        sides = _side_streams(dev, max(SIDE_STREAMS, 1))
        st = _copy[key] = sides[0] if (COPY_STREAM == 'side' and SIDE_STREAMS > 0) else \
            torch.cuda.Stream(device=dev)
    return st


def prepare_streams(dev):
    '''Create the process's HIP context and the side streams NOW.  Must run before an
    RCCL communicator is created: a group initialised first takes the hardware queues the
    side streams would get, the chains then share a queue with the main stream and the
    train step is 0.6 ms (16 %) slower (tools/dist_order_probe.py: 4.32 vs 3.72 ms).'''
    torch.zeros(1, device=dev)
    _side_streams(dev, max(SIDE_STREAMS, 1))
    copy_stream(dev)
    torch.cuda.synchronize(dev)


# An event that rides on a stream-K launch's own dispatch packet (danet_next_launch_events)
# instead of a hipEventRecord behind it: the record costs the launching stream ~4.4 us before its
# next kernel, the attached event ~1.1 us, and the side chain starts ~3.7 us earlier
# (tools/csrc/event_gap.hip).  Raw events from a small rotating pool per device (a slot is reused
# dozens of launches later; the host keeps at most MAX_STEPS_IN_FLIGHT steps queued).
FORK_ATTACH = _lib.expert('fork_attach', True)
_fork_event_pool = {}


class ForkEvent(object):
    __slots__ = ('handle', 'attached')

    def __init__(self, handle):
        self.handle, self.attached = handle, False

    def arm(self):
        '''the NEXT stream-K launch of this host thread completes the event; `attached` is set
        by the caller once that launch has been accepted (a rejected launch consumes the armed
        event inside the library and nothing may wait for it)'''
        check(_L().danet_next_launch_events(None, self.handle))


def fork_event(dev):
    '''the next ForkEvent of the device's pool, or None when attaching is switched off'''
    if not FORK_ATTACH or SIDE_STREAMS <= 0:
        return None
    pool = _fork_event_pool.setdefault(str(dev), {'i': 0, 'ev': []})
    if len(pool['ev']) < 32:
        h = _lib.c_p()
        check(_L().danet_event_create(__import__('ctypes').byref(h)))
        pool['ev'].append(h.value)
        return ForkEvent(h.value)
    pool['i'] = (pool['i'] + 1) % 32
    return ForkEvent(pool['ev'][pool['i']])


# A deferred side chain (a weight-gradient group) and the main stream's next kernel (the next layer's
# persistent BPTT kernel) become runnable at the same instant: when the launch the fork event rides on
# completes.  Nothing orders the two dispatches, and in ~4 % of the launches the group got its 480
# workgroups onto the CUs first: the BPTT kernel, whose workgroups exchange partials every time step,
# then starts piecemeal and takes 470-500 us instead of 360 (tools/bptt_hist.sh).  One tiny kernel
# in front of the group on the SIDE stream (a few microseconds of dispatch + run) lets the BPTT
# kernel's workgroups go first; it costs the main stream nothing.  DANET_EXPERT fork_spacer=0 switches it off.
FORK_SPACER = _lib.expert('fork_spacer', True)
_spacer_buf = {}


def _spacer(dev):
    '''one tiny kernel of THIS library on the current (side) stream -- danet_leaky_relu over 64
    floats, in place; until round 5 a `tensor.zero_()`, the only torch kernel left in a train step'''
    t = _spacer_buf.get(_dev_key(dev))
    if t is None:
        t = _spacer_buf[_dev_key(dev)] = torch.zeros(64, device=dev)
    check(_L().danet_leaky_relu(_lib.stream(), 64, ptr(t), None, 0.0, ptr(t)))


class _Fork(object):
    '''with _Fork(dev, n) as f:  f.run(i, fn)  -> fn runs on chain i
    (chain 0 = the current stream, chain i>0 = side stream i-1); join on exit.'''

    def __init__(self, dev, nchains, defer=False, keep=(), lazy=False, event=None, spacer=False):
        '''defer=True: do not join on exit -- the side chains keep running under
        whatever the main stream does next (e.g. weight-gradient GEMMs under the
        next layer's latency-bound BPTT kernel, which leaves most CUs idle);
        `join_deferred()` joins them.  `keep` = tensors the chains read that the
        caller is about to drop (kept alive until the join).
        lazy=True: the fork event is recorded when the first side chain is issued instead of
        on entry -- a fork that ends up with no side work then costs the main stream nothing
        (an event record is a ~7 us bubble in front of the next kernel); only for forks whose
        main-stream work comes AFTER their side chains.
        event: a ForkEvent already attached to the last launch the side chains have to wait for
        (then no event is recorded at all).
        spacer: put the spacer kernel in front of a deferred side chain that forks on a RECORDED event
        as well (an attached event always gets one).'''
        self.main = torch.cuda.current_stream(dev)
        n = min(nchains - 1, SIDE_STREAMS)
        self.sides = _side_streams(dev, n) if n > 0 else []
        self.used = set()
        self.defer, self.keep = defer, keep
        self.lazy, self.forked = lazy, False
        self.event = event if (event is not None and event.attached) else None
        self.spacer = spacer

    def _fork_now(self):
        if self.sides and not self.forked:
            if self.event is not None:
                for s in self.sides:
                    check(_L().danet_stream_wait_event(s.cuda_stream, self.event.handle))
            else:
                ev = self.main.record_event()
                for s in self.sides:
                    s.wait_event(ev)
        self.forked = True

    def __enter__(self):
        if not self.lazy:
            self._fork_now()
        return self

    def run(self, chain, fn):
        if not self.sides or chain == 0:
            return fn()
        self._fork_now()
        s = self.sides[(chain - 1) % len(self.sides)]
        self.used.add(s)
        with torch.cuda.stream(s):
            q = _lazy.get(_dev_key(s.device))
            if q:
                self.keep = tuple(self.keep) + tuple(k for _f, k in q)
                _flush_lazy(s.device)  # queued small kernels ride on this fork's event
            elif self.defer and (self.event is not None or self.spacer) and FORK_SPACER:
                _spacer(s.device)
            return fn()

    def after_all(self, fn, wait_main=False):
        '''run fn() on one of the used side streams once ALL side chains of this
        fork have been issued (that stream first waits for the others) -- the
        place to launch work that consumes everything the chains produce, e.g. a
        gradient-bucket all-reduce.  wait_main: part of that work was issued on the
        main stream (chain 0), so the side stream waits for the main stream's
        current position too.  With no side stream in use, fn runs in place.'''
        used = list(self.used)
        if not used:
            return fn()
        first = used[0]
        for s in used[1:]:
            first.wait_stream(s)
        if wait_main:
            first.wait_stream(self.main)
        with torch.cuda.stream(first):
            return fn()

    def __exit__(self, *exc):
        if self.defer and self.used:
            _deferred.append((self.main, tuple(self.used), self.keep))
        else:
            for s in self.used:
                self.main.wait_stream(s)
        return False


_deferred = []

# Called as hook(tag, params) when the gradients of `params` have been fully
# issued (on the stream that is current during the call); tag = ('layer', l) /
# ('out',).  Model uses it to launch per-bucket gradient all-reduces that overlap
# the rest of backward (dist.GradBuckets).
# ('rest', ) additionally fires on a side stream that has waited for the main stream right
# after the BOTTOM layer's BPTT kernel of an encoder was issued: from then on every gradient
# except the bottom layer's own is final (dist.TailOverlap reduces them under the bottom
# layer's weight-gradient GEMMs).  Entries are weak references to bound methods (a
# disposed Model drops out by itself).
GRAD_READY_HOOKS = []


def add_grad_ready_hook(bound_method):
    import weakref
    GRAD_READY_HOOKS.append(weakref.WeakMethod(bound_method))


def _live_hooks():
    live = [(r, r()) for r in GRAD_READY_HOOKS]
    if any(h is None for _, h in live):
        GRAD_READY_HOOKS[:] = [r for r, h in live if h is not None]
    return [h for _, h in live if h is not None]


def _fire_grad_ready(tag, params):
    for h in _live_hooks():
        h(tag, params)


# Fast backward (scoped: only inside `with ops.fast_backward():`, which Model.train_step
# enters).  (1) kernels ADD the parameter gradients straight into an existing dense
# `param.grad` (a view of Model's flat all-reduce bucket) and hand autograd None -- one
# elementwise accumulate kernel less per parameter; outside the scope every backward returns
# ordinary gradient tensors, so torch.autograd.grad / double backward / foreign optimisers see
# standard autograd behaviour.  (2) the gradient-ready hooks above fire.
DIRECT_GRADS = _lib.expert('direct_grads', True)
_fast_depth = [0]


class fast_backward(object):
    def __enter__(self):
        _fast_depth[0] += 1
        return self

    def __exit__(self, *exc):
        _fast_depth[0] -= 1
        return False


def _fast():
    return _fast_depth[0] > 0


def _grad_target(param, shape, dev):
    """(tensor to accumulate the gradient of `param` into, is_direct).  Direct =
    inside `fast_backward()` and the parameter already owns a dense .grad (e.g. a
    view of Model's flat gradient bucket): kernels add into it (beta=1) and
    autograd is handed None."""
    g = param.grad if (DIRECT_GRADS and _fast() and torch.is_tensor(param)) else None
    if g is not None and g.is_contiguous() and tuple(g.shape) == tuple(shape):
        return g, True
    return torch.empty(*shape, device=dev), False


def join_deferred():
    '''main stream waits for every deferred side chain -- ONE wait per distinct side stream
    (each wait is an event record + a barrier packet: four of them in a row put a 17 us bubble
    in front of the optimiser kernel)'''
    _flush_lazy()                      # nothing forked since they were queued: run them here
    waits = {}
    while _deferred:
        main, used, _keep = _deferred.pop()
        for s in used:
            waits.setdefault((main.cuda_stream, s.cuda_stream), (main, s))
    for main, s in waits.values():
        main.wait_stream(s)


def lstm_prefill_fwd(T, B, ldy, ypads, wss):
    '''ONE fill launch for the output buffers (+ workspaces) of several forward launches'''
    check(_L().danet_lstm_fwd_prefill(_lib.stream(), T, B, ldy, len(ypads), _ptrs(ypads), _ptrs(wss)))


# the input's centring and the recurrent launches' prefill in one launch (danet_encoder_prologue)
ENC_PROLOGUE = _lib.expert('enc_prologue', True)


def encoder_prologue(x, B, T, F, xc, Fp, H, ndir, ypads, fwd_wss, bwd_wss):
    '''xc[T, B, Fp] = x[B, T, F] - mean_{t,f}(x) (time-major, zero pad) AND the prefill of the n recurrent
    launches' buffers (bwd_wss: + the BPTT rings), one launch; False: the rings were NOT prefilled'''
    bp = _ptrs(bwd_wss) if bwd_wss is not None else None
    scratch = torch.empty(_lib.ws_bytes(_lib.WS_CENTER_MEAN, B) // 4, dtype=torch.float32, device=x.device)
    args = (_lib.stream(), B, T, F, ptr(_f32(x)), 0, F, ptr(xc), 1, Fp, ptr(scratch), H, ndir, ndir * H, len(ypads),
            _ptrs(ypads), _ptrs(fwd_wss))
    rc = _L().danet_encoder_prologue(*args, bp)
    if rc == -3 and bp is not None:      # BPTT geometry outside the reduce-scatter kernel: it prefills itself
        check(_L().danet_encoder_prologue(*args, None))
        return False
    check(rc)
    return True


def lstm_prefill_train(T, B, H, ndir, ypads, fwd_wss, bwd_wss):
    '''ONE fill launch for the forward launches' buffers AND the partial-dh rings of the BPTT launches
    that will follow; False (nothing launched) when the shape takes the all-gather BPTT kernel, which
    prefills its own exchange medium'''
    return _L().danet_lstm_train_prefill(_lib.stream(), T, B, H, ndir, ndir * H, len(ypads), _ptrs(ypads),
                                         _ptrs(fwd_wss), _ptrs(bwd_wss)) == 0


def _stack_buffers(train, n, T, B, H, ndir, dev):
    '''(ypads, wss, bwss) of n recurrent launches: their output buffers and workspaces, and on a train step whose
    shape the reduce-scatter BPTT kernel covers the workspaces of the BPTT launches (their rings), else None'''
    ypads = [torch.empty(T + 2, B, ndir * H, device=dev) for _ in range(n)]
    wss = [_lstm_ws(T, B, H, ndir, dev)[0] for _ in range(n)]
    bwss = None
    if train and BWD_DB and _L().danet_lstm_bwd_db_supported(T, B, H, ndir) == 1:
        bwss = [_lstm_ws(T, B, H, ndir, dev)[0] for _ in range(n)]
    return ypads, wss, bwss


def _stack_prefill(T, B, H, ndir, ypads, wss, bwss):
    '''ONE fill launch for the buffers of `_stack_buffers`: the train prefill, or the forward prefill where there
    are no rings or the train prefill declines the shape; returns bwss, None if the rings were NOT prefilled'''
    if bwss is None or not lstm_prefill_train(T, B, H, ndir, ypads, wss, bwss):
        bwss = None
        lstm_prefill_fwd(T, B, ndir * H, ypads, wss)
    return bwss


def lstm_layer_fwd(x, ldx, D, T, B, H, Ws, bs, x_pad_zero=False, ypad=None, ws=None):
    '''x: time-major [T*B rows, ldx] tensor (data_ptr = row 0), D valid columns.
    Ws[d]: [D+H, 4H] (reference layout, rows 0..D-1 input, D.. recurrent),
    bs[d]: [4H].  Returns ctx with ypad [T+2, B, ndir*H].
    x_pad_zero: the caller guarantees that columns D..ldx-1 of x hold finite values (zeros).
    The fused-input kernel loads whole float4 groups of a row and masks only W for k >= D,
    so with D % 4 != 0 a non-finite pad value would poison the gates (0 * NaN); without the
    guarantee such inputs take the hoisted GEMM path, which never reads the pad.'''
    ndir = len(Ws)
    dev = x.device
    L = _L()
    gates = [torch.empty(T * B, 4 * H, device=dev) for _ in range(ndir)]
    cells = [torch.empty(T * B, H, device=dev) for _ in range(ndir)]
    flags = 0
    if ypad is None:
        ypad = torch.empty(T + 2, B, ndir * H, device=dev)
        ws, wn = _lstm_ws(T, B, H, ndir, dev)
    else:                    # allocated and prefilled by the caller (lstm_prefill_fwd)
        wn = ws.numel()
        flags = 1            # DANET_LSTM_PREFILLED
    fused = (ldx % 4 == 0 and x.data_ptr() % 16 == 0 and (D % 4 == 0 or x_pad_zero) and
             all(W.stride(0) == 4 * H and W.stride(1) == 1 for W in Ws) and
             L.danet_lstm_fwd_fused_supported(T, B, H, ndir, D) == 1)
    if fused:
        # the whole cell [x_t, h_{t-1}] W + b (app/ops.py:139-147) in ONE launch: the input
        # half runs on the matrix cores inside the per-step exchange wait (csrc/lstm.hip)
        with _lib.timed('lstm_fwd'):
            check(L.danet_lstm_fwd_fused(
                _lib.stream(), T, B, H, ndir, ptr(_f32(x)), ldx, D,
                ptr(Ws[0]), ptr(Ws[-1]), 4 * H, ptr(bs[0]), ptr(bs[-1]), ptr(ypad), ndir * H,
                ptr(gates[0]), ptr(gates[-1]), ptr(cells[0]), ptr(cells[-1]), ptr(ws), wn,
                ptr(status_word(dev)), flags))
    else:
        if _x6_ok(T * B, 4 * H, (x, ldx, D)):
            # hoisted input half [x]Wx + b (app/ops.py:139-142) on the packed weight, one launch per
            # direction; `gates[d]` is later overwritten in place by g,i,f,o
            for d in range(ndir):
                gemm_w(x, ldx, Ws[d], 1, 4 * H, gates[d], T * B, 4 * H, D, 4 * H, tag='gx', bias=bs[d])
        elif GROUPED_GX and ndir == 2:
            # hoisted input half of ops.lyr_lstm_flat's [x,h]W+b (app/ops.py:139-142) of both
            # directions as one grouped stream-K launch (nothing else runs at this point of the
            # forward pass: 2 x 320 tiles fill 512 workgroups evenly; -1.5% per step vs two
            # launches on two streams); `gates[d]` is later overwritten in place by g,i,f,o
            gemm_group([(x, ldx, Ws[d], 4 * H, gates[d], 4 * H, T * B, 4 * H, 0.0, bs[d])
                        for d in range(ndir)], D, max_workgroups=GROUPED_GX)
        else:
            with _Fork(dev, ndir) as f:
                for d in range(ndir):
                    f.run(d, lambda d=d: gemm(x, Ws[d], gates[d], T * B, 4 * H, D, ldx, 4 * H,
                                              4 * H, bias=bs[d], tag='gx'))
        Whs = [W[D:] for W in Ws]
        with _lib.timed('lstm_fwd'):
            check(L.danet_lstm_fwd(
                _lib.stream(), T, B, H, ndir, ptr(gates[0]), ptr(gates[-1]),
                ptr(Whs[0]), ptr(Whs[-1]), 4 * H, ptr(ypad), ndir * H,
                ptr(gates[0]), ptr(gates[-1]), ptr(cells[0]), ptr(cells[-1]), ptr(ws), wn,
                ptr(status_word(dev)), flags))
    c = _LayerCtx()
    c.x, c.ldx, c.D, c.T, c.B, c.H, c.ndir = x, ldx, D, T, B, H, ndir
    c.ypad, c.gates, c.cells, c.Ws, c.bs = ypad, gates, cells, Ws, bs
    return c


# Do the weight-gradient groups run UNDER the next BPTT kernel (side stream) or serially on the
# main stream?  Under: the group is hidden but the BPTT kernel beside it slows down for as long as
# the overlap lasts.  Measured: H = 300 (cfg 2 / cfg 4) 3.61 / 5.13 ms per step overlapped vs
# 3.90 / 5.62 serial; H = 600 (cfg 4 as written) 14.3 overlapped vs 13.7 serial (the group lasts
# 0.9-1.3 ms there and costs the BPTT kernel 0.7 ms).  'auto' = overlap up to H = 384 with the
# exact-fp32 groups, always with the groups on the bf16 matrix cores (round 4).
DW_OVERLAP = _lib.expert('dw_overlap', 'auto')


def _overlap_dw(H, tn_ok=True):
    '''tn_ok: this group's products will actually take the bf16-matrix-core TN kernel
    (`_x6_tn_ok`); a group that falls back to the exact-fp32 stream-K kernels is overlapped only
    up to H = 384 (the combination measured slower above that)'''
    if DW_OVERLAP in ('0', '1'):
        return DW_OVERLAP == '1'
    # (with the groups on the bf16 matrix cores the overlap wins at H = 600 as well: cfg 4 as
    # written 9.66 overlapped vs 9.86 serial on the same box, BPTT 674 vs 575 us)
    return H <= 384 or (bool(GEMM_X6 & 2) and tn_ok)


# experiment: fork the weight-gradient group BEFORE dX (the two GEMMs share the GPU, the next
# BPTT kernel then has the group beside it for a shorter time)
DW_FORK_EARLY = _lib.expert('dw_fork_early', False)
# bias gradients summed inside the (unfused) BPTT kernel instead of by column-sum launches
BWD_DB = _lib.expert('lstm_bwd_db', True)
DB_DEFER = _lib.expert('lstm_db_defer', True)


def lstm_layer_bwd(c, dy, need_dx, layer_tag=None, is_top=False, ws_prefilled=None, dx_drop=None):
    '''dy: [T, B, ndir*H] contiguous.  Returns (dx [T*B, D] or None, dWs, dbs).
    ws_prefilled: a workspace whose ring the caller prefilled (lstm_prefill_train).
    dx_drop: (DropoutSpec, stream_id) of the dropout that sits on this layer's INPUT (the output of
    the BiLSTM layer below): dx is masked in place right behind the dX product, and the weight-
    gradient side chain is forked behind THAT launch by a recorded event (+ the spacer) instead of
    by the event attached to dX -- with the attached event the chain would become runnable one
    mask launch before the next BPTT kernel and could take the CUs first ("who goes first",
    DESIGN 3.1).'''
    T, B, H, D, ndir = c.T, c.B, c.H, c.D, c.ndir
    dev = dy.device
    das = [torch.empty(T * B, 4 * H, device=dev) for _ in range(ndir)]
    L = _L()
    ldy = ndir * H
    # gradients accumulate straight into the parameters' .grad (the model's flat
    # all-reduce bucket) when there is one; autograd then gets None for them
    dWs, dbs, direct = [], [], []
    for d in range(ndir):
        gW, okW = _grad_target(c.Ws[d], (D + H, 4 * H), dev)
        gb, okb = _grad_target(c.bs[d], (4 * H,), dev)
        dWs.append(gW); dbs.append(gb); direct.append((okW, okb))
    dx = torch.empty(T * B, D, device=dev) if need_dx else None
    if ws_prefilled is not None:
        ws, wn = ws_prefilled, ws_prefilled.numel()
    else:
        ws, wn = _lstm_ws(T, B, H, ndir, dev)
    Whs = [W[D:] for W in c.Ws]
    b_direct = [okb for _, okb in direct]
    # bias gradients summed inside the BPTT kernel (no column-sum launches) where the
    # reduce-scatter kernel covers the shape
    db_in_kernel = (BWD_DB and (all(b_direct) or not any(b_direct)) and
                    all(t.data_ptr() % 16 == 0 for t in dbs) and
                    L.danet_lstm_bwd_db_supported(T, B, H, ndir) == 1)
    # the 6-us sum of the kernel's per-cluster bias partials leaves the critical path (BPTT ->
    # dX -> next BPTT) when a side chain is forked behind this launch anyway
    # (not for the bottom layer: its weight-gradient group takes every CU on the main stream
    # and the side chain's reduce would sit behind it for the group's whole duration)
    def hprev_of(d):
        # Hprev(t) = ypad block t (fwd) / block t+2 (bwd)
        return c.ypad.view(-1)[(0 if d == 0 else 2 * B * ldy + H):]

    def group_problems():
        # dWx = X^T da and dWh = Hprev^T da of every direction
        probs = []
        for d in range(ndir):
            bW = 1.0 if direct[d][0] else 0.0
            probs.append((c.x, c.ldx, das[d], 4 * H, dWs[d], 4 * H, D, 4 * H, bW))
            probs.append((hprev_of(d), ldy, das[d], 4 * H, dWs[d][D:], 4 * H, H, 4 * H, bW))
        return probs
    overlap = _overlap_dw(H, _x6_tn_ok(group_problems(), T * B))
    db_deferred = (db_in_kernel and DB_DEFER and GROUPED_DW and SIDE_STREAMS > 0 and
                   need_dx and overlap)
    with _lib.timed('lstm_bwd'):
        check(L.danet_lstm_bwd(
            _lib.stream(), T, B, H, ndir, ptr(_f32(dy)), ndir * H,
            ptr(Whs[0]), ptr(Whs[-1]), 4 * H, ptr(c.gates[0]), ptr(c.gates[-1]),
            ptr(c.cells[0]), ptr(c.cells[-1]), ptr(das[0]), ptr(das[-1]),
            ptr(dbs[0]) if db_in_kernel else None, ptr(dbs[-1]) if db_in_kernel else None,
            1.0 if all(b_direct) else 0.0, ptr(ws), wn, ptr(status_word(dev)),
            ((1 if ws_prefilled is not None else 0) | (2 if db_deferred else 0))
            if db_in_kernel else 0))

    # the weight-gradient products overlap the NEXT layer's BPTT kernel (152 of
    # 256 CUs at cfg 2): cap each chain so both together stay on the idle CUs
    cap = OVERLAP_GEMM_WGS if need_dx else 0

    def weight_grads(d):
        bW, bb = (1.0 if direct[d][0] else 0.0), (1.0 if direct[d][1] else 0.0)
        # dWx = X^T da
        gemm(c.x, das[d], dWs[d], D, 4 * H, T * B, c.ldx, 4 * H, 4 * H, transA=True, beta=bW,
             max_workgroups=cap)
        # dWh = Hprev^T da
        gemm(hprev_of(d), das[d], dWs[d][D:], H, 4 * H, T * B, ldy, 4 * H, 4 * H, transA=True, beta=bW,
             max_workgroups=cap)
        if not db_in_kernel:
            colsum(das[d], T * B, 4 * H, 4 * H, dbs[d], beta=bb)

    def weight_grads_grouped(wgs=GROUPED_DW_WGS, with_bias=True):
        # dWx = X^T da and dWh = Hprev^T da of every direction: one launch
        gemm_group(group_problems(), T * B, transA=True, max_workgroups=wgs)
        # (the bias gradients as M = 1 members of the group were measured slower than
        # the two column-sum kernels: +25 us on the group for 128-row tiles with one row)
        if with_bias:
            bias_grads()

    def bias_grads():
        if db_deferred:
            check(L.danet_lstm_bwd_db_reduce(_lib.stream(), T, B, H, ndir, ptr(dbs[0]), ptr(dbs[-1]),
                                             1.0 if direct[0][1] else 0.0, ptr(ws), wn))
            return
        if db_in_kernel:
            return
        for d in range(ndir):
            colsum(das[d], T * B, 4 * H, 4 * H, dbs[d], beta=1.0 if direct[d][1] else 0.0)

    fork_ev = [None]

    def input_grad(attach=False):
        if ndir == 2:
            # dX = da_f Wx_f^T + da_b Wx_b^T: one K-concatenated launch (the fork event of the
            # weight-gradient chain rides on it: see ForkEvent)
            sk = (STREAMK & 4) != 0 and (4 * H) % 16 == 0
            if _x6_ok(T * B, D, (das[0], 4 * H, 4 * H), (das[1], 4 * H, 4 * H)):
                if attach:
                    fork_ev[0] = fork_event(dev)
                gemm_w(das[0], 4 * H, c.Ws[0], 4 * H, 1, dx, T * B, D, 4 * H, D, tag='dX',
                       stop_event=fork_ev[0], A2=das[1], lda2=4 * H, W2=c.Ws[1], K2=4 * H)
                return
            if attach and sk:
                fork_ev[0] = fork_event(dev)
            gemm_kcat(das[0], 4 * H, c.Ws[0], 4 * H, 4 * H, das[1], 4 * H, c.Ws[1], 4 * H, 4 * H,
                      dx, T * B, D, D, transB=True, tag='dX', streamk=(STREAMK & 4) != 0,
                      stop_event=fork_ev[0])
            return
        for d in range(ndir):
            # dX += da Wx^T
            gemm(das[d], c.Ws[d], dx, T * B, D, 4 * H, 4 * H, 4 * H, D, transB=True,
                 beta=0.0 if d == 0 else 1.0, streamk=(STREAMK & 1) != 0, tag='dX')

    # dX is what the next layer's BPTT waits for: it is issued first, alone, on
    # the main stream.  The weight-gradient chains fork AFTER it (the fork event
    # is recorded behind dX), so they do not compete with dX for CUs but overlap
    # the next layer's latency-bound BPTT kernel instead; the caller joins them
    # (`join_deferred`).
    fork_early = DW_FORK_EARLY and need_dx and GROUPED_DW
    def drop_dx():
        dropout_apply(dx, dx, T * B, D, D, D, dx_drop[0], dx_drop[1])

    if need_dx and not fork_early:
        input_grad(attach=GROUPED_DW and overlap and dx_drop is None)
        if dx_drop is not None:
            drop_dx()
    hooks = bool(GRAD_READY_HOOKS) and _fast() and layer_tag is not None and \
        all(a and b for a, b in direct)
    if hooks and not need_dx:
        # bottom layer of an encoder: its BPTT kernel is on the main stream, the weight-
        # gradient chains of every layer above are on the side streams -- a stream that has
        # waited for all of them sees every gradient except this layer's in its final state
        sides = _side_streams(dev, max(SIDE_STREAMS, 1))
        main = torch.cuda.current_stream(dev)
        for sd in sides[1:]:
            sides[0].wait_stream(sd)
        sides[0].wait_stream(main)
        with torch.cuda.stream(sides[0]):
            _fire_grad_ready(('rest',), list(c.Ws) + list(c.bs))
    with _Fork(dev, ndir + 1, defer=True, keep=(das, c.x, c.ypad, dy, ws), lazy=True,
               event=fork_ev[0], spacer=dx_drop is not None) as f:
        on_main = False
        if GROUPED_DW and not need_dx:
            # bottom layer: no BPTT kernel follows, so the group takes the whole GPU on
            # the main stream while the column sums (if any) run beside it
            if not db_in_kernel:
                f.run(1, bias_grads)
            weight_grads_grouped(wgs=512, with_bias=False)
            on_main = True
        elif GROUPED_DW and not overlap:
            weight_grads_grouped(wgs=512)      # serial: alone on the main stream, whole GPU
            on_main = True
        elif GROUPED_DW:
            f.run(1, weight_grads_grouped)
            if fork_early:
                input_grad()          # beside the group, both behind this layer's BPTT kernel
                if dx_drop is not None:
                    drop_dx()
        else:
            for d in range(ndir):
                f.run(d + 1, lambda d=d: weight_grads(d))
        if hooks:
            # (wait_main: the bottom layer's group GEMM ran on the main stream)
            f.after_all(lambda: _fire_grad_ready(('layer', layer_tag), list(c.Ws) + list(c.bs)),
                        wait_main=on_main)
    dWs = [None if direct[d][0] else dWs[d] for d in range(ndir)]
    dbs = [None if direct[d][1] else dbs[d] for d in range(ndir)]
    return dx, dWs, dbs


class LstmLayerFn(torch.autograd.Function):
    '''One (bi)LSTM layer on batch-major input: Model.lyr_lstm / _lyr_bilstm
    (main.py:76-132, app/modules.py:120-137).  x [B,T,D] -> [B,T,ndir*H].
    Inside an active `dropout_scope` a bidirectional layer's output is dropped (app/modules.py:137);
    a single direction (Model.lyr_lstm) has no dropout in the reference and none here.'''

    @staticmethod
    def forward(ctx, x, H, *params):
        ndir = len(params) // 2
        Ws, bs = list(params[0::2]), list(params[1::2])
        B, T, D = x.shape
        xt = x.transpose(0, 1).contiguous()         # tf.transpose, main.py:98-104
        c = lstm_layer_fwd(xt, D, D, T, B, H, Ws, bs)
        ctx.c = c
        ctx.xt = xt
        spec = _dropout_cur[0] if ndir == 2 else None
        ctx.drop = None
        if spec is not None:                        # tf.nn.dropout, app/modules.py:137
            ctx.drop = (spec, spec.take())
            yd = torch.empty(T, B, 2 * H, device=x.device)
            dropout_apply(c.ypad[1:], yd, T * B, 2 * H, 2 * H, 2 * H, *ctx.drop)
            return yd.transpose(0, 1).contiguous()
        return c.ypad[1:T + 1].transpose(0, 1).contiguous()

    @staticmethod
    def backward(ctx, dy):
        c = ctx.c
        dyt = dy.transpose(0, 1).contiguous()
        if ctx.drop is not None:
            # (out of place: .contiguous() may have handed back the caller's own tensor)
            W = c.ndir * c.H
            dyt = dropout_apply(dyt, torch.empty(c.T, c.B, W, device=dy.device), c.T * c.B, W, W, W, *ctx.drop)
        dx, dWs, dbs = lstm_layer_bwd(c, dyt, ctx.needs_input_grad[0])
        join_deferred()
        out = [None, None]
        if dx is not None:
            out[0] = dx.view(c.T, c.B, c.D).transpose(0, 1).contiguous()
        for dW, db in zip(dWs, dbs):
            out += [dW, db]
        return tuple(out)


def _project_fwd(rows, K, W, B, T, streamk):
    '''the encoders' bias-free projection embed [B, T, O] = rows [B*T, K] W [K, O]; streamk: the schedule of the
    product where it does not run on the packed weight'''
    O = W.shape[1]
    embed = torch.empty(B, T, O, device=rows.device)
    if _x6_ok(B * T, O, (rows, K, K)):
        gemm_w(rows, K, W, 1, O, embed, B * T, O, K, O, tag='proj')
    else:
        gemm(rows, W, embed, B * T, O, K, K, O, O, tag='proj', streamk=streamk)
    return embed


def _encoder_center(causal, x, B, T, D, in_layout, ld_in, out, out_layout, ld_out):
    '''an encoder's centring: x minus its whole-utterance mean, or (causal) minus its running mean from a zero state'''
    if causal:
        return causal_center_fwd(x, B, T, D, in_layout, ld_in, out, out_layout, ld_out,
                                 causal_center_state(B, x.device))
    return center(x, B, T, D, in_layout, ld_in, out, out_layout, ld_out)


def _rnn_encoder_fwd(ctx, causal, x, H, L, ndir, params):
    '''centre -> L stacked (bi)LSTM layers -> centre -> bias-free projection: the forward of RnnEncoderFn and
    (causal) of CausalRnnEncoderFn, which differ in the centrings only'''
    x = _f32(x.contiguous())
    B, T, F = x.shape
    dev = x.device
    Wout = params[-1]
    Fp = (F + 3) // 4 * 4
    # x - its mean, switched to time-major, zero-padded to a float4 row                modules.py:209-210
    xc = torch.empty(T, B, Fp, device=dev)
    ctxs = []
    cur, ld, D = xc, Fp, F
    # output buffers + workspaces of ALL layers (a train step: + the BPTT launches' rings), prefilled
    # by ONE fill -- which rides in the whole-utterance centring launch (danet_encoder_prologue)
    ypads, wss, bwss = _stack_buffers(any(ctx.needs_input_grad), L, T, B, H, ndir, dev)
    if causal or not ENC_PROLOGUE:
        _encoder_center(causal, x, B, T, F, 0, F, xc, 1, Fp)
        bwss = _stack_prefill(T, B, H, ndir, ypads, wss, bwss)
    elif not encoder_prologue(x, B, T, F, xc, Fp, H, ndir, ypads, wss, bwss):
        bwss = None
    ctx.bwss = bwss
    spec = _dropout_cur[0] if ndir == 2 else None
    ctx.drop = (spec, spec.take(L)) if spec is not None else None
    for l in range(L):                                    # modules.py:223-242
        Ws = [params[(l * ndir + d) * 2] for d in range(ndir)]
        bs = [params[(l * ndir + d) * 2 + 1] for d in range(ndir)]
        # (the centre kernel zero-fills the float4 pad of layer 0's rows; deeper layers
        # read ypad, whose row length is a multiple of 4)
        c = lstm_layer_fwd(cur, ld, D, T, B, H, Ws, bs, x_pad_zero=True, ypad=ypads[l],
                           ws=wss[l])
        ctxs.append(c)
        cur, ld, D = c.ypad[1:], ndir * H, ndir * H
        if spec is not None:                              # modules.py:137
            cur = dropout_apply(cur, torch.empty(T, B, D, device=dev), T * B, D, D, D, spec,
                                ctx.drop[1] + l)
    # y - its mean, back to batch-major                     modules.py:244-245
    yc = torch.empty(B, T, D, device=dev)
    _encoder_center(causal, cur, B, T, D, 1, D, yc, 0, D)
    O = Wout.shape[1]
    # (hybrid stream-K pays for the projection only with >= 4 tiles per CU: cfg 4, 1312 tiles,
    # 248 -> 238 us; cfg 2, 672 tiles, 126 -> 132 us)
    big = ((B * T + 127) // 128) * ((O + 127) // 128) >= 1024
    embed = _project_fwd(yc, D, Wout, B, T, (STREAMK & 2) != 0 or (big and STREAMK != 0))     # modules.py:249-255
    ctx.ctxs, ctx.yc, ctx.Wout = ctxs, yc, Wout
    ctx.dims = (B, T, F, H, L, ndir, D, O)
    ctx.causal = causal
    return embed


def _rnn_encoder_bwd(ctx, dembed):
    '''the backward of `_rnn_encoder_fwd`: the gradients of its params, in their order (None: accumulated
    straight into .grad)'''
    B, T, F, H, L, ndir, D, O = ctx.dims
    dembed = _f32(dembed.contiguous())
    dev = dembed.device
    dWout, direct_out = _grad_target(ctx.Wout, (D, O), dev)
    dyc = torch.empty(B, T, D, device=dev)
    x6 = _x6_ok(B * T, D, (dembed, O, O))
    ev = fork_event(dev) if ((STREAMK & 1) != 0 or x6) else None
    if x6:                                                # critical path first
        gemm_w(dembed, O, ctx.Wout, O, 1, dyc, B * T, D, O, D, tag='dYc', stop_event=ev)
    else:
        gemm(dembed, ctx.Wout, dyc, B * T, D, O, O, O, D, transB=True, streamk=(STREAMK & 1) != 0,
             tag='dYc', stop_event=ev)
    with _Fork(dev, 2, defer=True, keep=(dembed, ctx.yc), lazy=True, event=ev) as f:
        if GROUPED_DW:    # alone on its stream under the top layer's BPTT kernel (or serial)
            ov = _overlap_dw(H, _x6_tn_ok([(ctx.yc, D, dembed, O, dWout, O, D, O, 0.0)], B * T))
            f.run(1 if ov else 0, lambda: gemm_group(
                [(ctx.yc, D, dembed, O, dWout, O, D, O, 1.0 if direct_out else 0.0)], B * T,
                transA=True, max_workgroups=GROUPED_DW_WGS if ov else 512))
        else:
            f.run(1, lambda: gemm(ctx.yc, dembed, dWout, D, O, B * T, D, O, O, transA=True,
                                  beta=1.0 if direct_out else 0.0,
                                  max_workgroups=2 * OVERLAP_GEMM_WGS, tag='dWout'))
        if GRAD_READY_HOOKS and _fast() and direct_out:
            f.after_all(lambda: _fire_grad_ready(('out',), [ctx.Wout]))
    dy = torch.empty(T, B, D, device=dev)
    if ctx.causal:
        causal_center_bwd(dyc, B, T, D, 0, D, dy, 1, D)      # the running mean is not self-adjoint
    else:
        center(dyc, B, T, D, 0, D, dy, 1, D)                 # centre is self-adjoint
    drop = ctx.drop
    if drop is not None:                                 # the top layer's mask (dy is ours: in place)
        dropout_apply(dy, dy, T * B, D, D, D, drop[0], drop[1] + L - 1)
    grads = [None] * (2 * L * ndir)
    # partial-dh rings of all layers' BPTT launches: prefilled by the forward pass's fill launch
    bwss = ctx.bwss if ctx.bwss is not None else [None] * L
    ctx.bwss = None
    for l in reversed(range(L)):
        dx, dWs, dbs = lstm_layer_bwd(ctx.ctxs[l], dy, need_dx=(l > 0), layer_tag=l,
                                      is_top=(l == L - 1), ws_prefilled=bwss[l],
                                      dx_drop=(drop[0], drop[1] + l - 1) if (drop is not None and l > 0)
                                      else None)
        for d in range(ndir):
            grads[(l * ndir + d) * 2] = dWs[d]
            grads[(l * ndir + d) * 2 + 1] = dbs[d]
        dy = dx
    join_deferred()
    ctx.ctxs = None
    return tuple(grads) + (None if direct_out else dWout,)


class RnnEncoderFn(torch.autograd.Function):
    '''Whole `bilstm-orig` / `lstm-orig` encoder (app/modules.py:148-260):
    mean-centre -> L stacked (bi)LSTM layers -> mean-centre -> bias-free output
    projection.  x [B,T,F] -> embed [B,T,F*E].
    params = (W_0f, b_0f, [W_0b, b_0b], W_1f, ..., W_out)
    Inside an active `dropout_scope`, `bilstm-orig` (ndir == 2) drops every layer's output the way
    `_lyr_bilstm` does (app/modules.py:137): the dropped copy of ypad[1:] goes to a buffer of its own,
    which is the next layer's input (and its dWx operand) or the centring's; ypad stays intact as
    the recurrent exchange medium and dWh operand.  Stream id = layer index.  `lstm-orig`
    (ndir == 1) calls model.lyr_lstm directly in the reference (app/modules.py:164-179), which has
    no dropout: it stays as it is.'''

    @staticmethod
    def forward(ctx, x, H, L, ndir, *params):
        return _rnn_encoder_fwd(ctx, False, x, H, L, ndir, params)

    @staticmethod
    def backward(ctx, dembed):
        return (None, None, None, None) + _rnn_encoder_bwd(ctx, dembed)


class CausalRnnEncoderFn(torch.autograd.Function):
    '''Whole `lstm-causal` encoder: RnnEncoderFn with ndir = 1 (the `lstm-orig` stack, on the same recurrent kernels
    and the same projection) with both whole-utterance centrings replaced by the causal running mean of
    include/danet_causal_hip.h from a zero state -- the embedding of frame t depends on frames <= t only.
    x [B,T,F] -> embed [B,T,F*E].  params = (W_0, b_0, W_1, ..., W_out).  No dropout, as `lstm-orig`.'''

    @staticmethod
    def forward(ctx, x, H, L, *params):
        return _rnn_encoder_fwd(ctx, True, x, H, L, 1, params)

    @staticmethod
    def backward(ctx, dembed):
        return (None, None, None) + _rnn_encoder_bwd(ctx, dembed)


# ---------------------------------------------------------------------------
# conv-bilstm-v1 encoder (app/modules.py:263-379) on the extension library libdanet_conv_hip.so
# ---------------------------------------------------------------------------
def _conv_desc(B, Cin, Cout, T, F, k, alpha, xs, ys, pool=False, d2s=False):
    d = _lib.ConvDesc()
    d.B, d.Cin, d.Cout, d.T, d.F, d.k = B, Cin, Cout, T, F, k
    d.pool, d.d2s, d.alpha = int(pool), int(d2s), float(alpha)
    for a in range(4):
        d.x_stride[a], d.y_stride[a] = int(xs[a]), int(ys[a])
    return d


def conv_fwd(d, x, w, b, y, argmax=None):
    '''y = lrelu(conv(x, w) + b) (+ pool -> argmax | depth-to-space), layouts by d's strides'''
    with _lib.timed('conv_fwd'):
        _lib.conv_check(_lib.load_conv().danet_conv_fwd(_lib.stream(), ctypes.byref(d), ptr(_f32(x)), ptr(_f32(w)),
                                                        ptr(_f32(b)), ptr(_f32(y)), ptr(argmax)))
    return y


def conv_bwd_data(d, dy, y, argmax, w, dx):
    '''dx = dgrad of layer d from dy (at y's layout), lrelu' from the saved y, pool via argmax'''
    with _lib.timed('conv_dgrad'):
        _lib.conv_check(_lib.load_conv().danet_conv_bwd_data(_lib.stream(), ctypes.byref(d), ptr(_f32(dy)),
                                                             ptr(_f32(y)), ptr(argmax), ptr(_f32(w)), ptr(_f32(dx))))
    return dx


def conv_bwd_weight(d, x, dy, y, argmax, dw, db, accumulate=False):
    '''dw, db of layer d (accumulate: += into them); deterministic two-pass slab reduction'''
    need = _lib.conv_ws_bytes(_lib.CONV_WS_BWD_WEIGHT, d)
    w, wn = _ws(need, dy.device)
    with _lib.timed('conv_wgrad'):
        _lib.conv_check(_lib.load_conv().danet_conv_bwd_weight(
            _lib.stream(), ctypes.byref(d), ptr(_f32(x)), ptr(_f32(dy)), ptr(_f32(y)), ptr(argmax),
            ptr(_f32(dw)), ptr(_f32(db)), int(bool(accumulate)), ptr(w), wn))


def conv_add(a, b, out):
    '''out = a + b over out.numel() elements (all three dense)'''
    _lib.conv_check(_lib.load_conv().danet_conv_add(_lib.stream(), out.numel(), ptr(_f32(a)), ptr(_f32(b)),
                                                    ptr(_f32(out))))
    return out


def conv_encoder_check(T, nfft, F):
    '''the shapes conv-bilstm-v1 is defined for (ValueError before any launch)'''
    if nfft % 8 or nfft < 16:
        raise ValueError('conv-bilstm-v1: FFT_SIZE must be a multiple of 8 and >= 16 (got %d)' % nfft)
    if F != nfft // 2 + 1:
        raise ValueError('conv-bilstm-v1: %d bins, FFT_SIZE %d needs %d' % (F, nfft, nfft // 2 + 1))
    if T % 4:
        raise ValueError('conv-bilstm-v1: the number of frames must be a multiple of 4 (LENGTH_ALIGN), '
                         'got %d' % T)


# conv layers of the encoder, in creation order: (Cin, Cout, k, pool, depth-to-space)
CONV_LAYERS = ((1, 8, 5, False, False), (8, 16, 5, True, False), (16, 32, 3, False, False),
               (32, 16, 3, True, False), (16, 32, 3, False, False), (32, 64, 3, False, True),
               (16, 16, 5, False, False), (16, 8, 5, False, False))


def conv_encoder_descs(B, T, nfft, alpha):
    '''the 8 layer descriptors, with the layouts that chain them without copies:
    x [B][T][F] (mix_log) -> a0 [B][8][T][F] -> pool -> p1 [B][16][T/2][nfft/4] -> a2 [B][32][T/2][nfft/4]
    -> pool -> p3 time-major [T/4][B][16 * nfft/8] (the LSTM's input rows; conv_act and lstm_act alike)
    lstm_act -> a4 [B][32][T/4][nfft/8] -> depth-to-space -> mid4 [B][16][T/2][nfft/4]
    -> a6 [B][16][T/2][nfft/4] -> rows [B][T/2][8][nfft/4], which is the dense layer's [B*T][nfft]'''
    F = nfft // 2 + 1
    T2, T4, N4, N8 = T // 2, T // 4, nfft // 4, nfft // 8
    D = 2 * nfft
    X0 = (T * F, T * F, F, 1)
    A0 = (8 * T * F, T * F, F, 1)
    P1 = (16 * T2 * N4, T2 * N4, N4, 1)
    A2 = (32 * T2 * N4, T2 * N4, N4, 1)
    TM = (D, N8, B * D, 1)
    A4 = (32 * T4 * N8, T4 * N8, N8, 1)
    M4 = (16 * T2 * N4, T2 * N4, N4, 1)
    RW = (T2 * 8 * N4, N4, 8 * N4, 1)
    geo = ((T, F, X0, A0), (T, F, A0, P1), (T2, N4, P1, A2), (T2, N4, A2, TM),
           (T4, N8, TM, A4), (T4, N8, A4, M4), (T2, N4, M4, M4), (T2, N4, M4, RW))
    return [_conv_desc(B, ci, co, t, f, k, alpha, xs, ys, pool=pool, d2s=d2s)
            for (ci, co, k, pool, d2s), (t, f, xs, ys) in zip(CONV_LAYERS, geo)]


class ConvBiLstmEncoderFn(torch.autograd.Function):
    '''Whole `conv-bilstm-v1` encoder (app/modules.py:263-379): conv2d .. conv2d_3 (two fused 2x2
    max-pools) -> centre (conv_act) -> 2 BiLSTM layers of width nfft -> + conv_act -> centre
    (lstm_act) -> conv2d_4, conv2d_5 (+ depth-to-space), conv2d_6, conv2d_7 -> bias-free dense.
    x [B,T,F] (T % 4 == 0) -> embed [B,T,O].  Every step is a library kernel; the layers hand
    each other their layouts through strides (conv_encoder_descs), so there are no copies.
    params = (w0, b0, .., w3, b3, W_0f, b_0f, W_0b, b_0b, W_1f, b_1f, W_1b, b_1b, w4, b4, .., w7, b7,
    W_dense).  debug: None or a dict that receives conv_act, lstm_act (time-major [T/4][B][2 nfft])
    and mid4 ([B][16][T/2][nfft/4]).  Inside an active `dropout_scope` both BiLSTM layers drop their
    outputs as in RnnEncoderFn; the residual add sees the dropped lstm1 output.'''

    @staticmethod
    def forward(ctx, x, nfft, alpha, debug, *params):
        x = _f32(x.contiguous())
        B, T, F = x.shape
        conv_encoder_check(T, nfft, F)
        dev = x.device
        T2, T4, N4, N8 = T // 2, T // 4, nfft // 4, nfft // 8
        H, D = nfft, 2 * nfft
        ds = conv_encoder_descs(B, T, nfft, alpha)
        cw = [(params[2 * l], params[2 * l + 1]) for l in range(4)] + \
             [(params[16 + 2 * l], params[17 + 2 * l]) for l in range(4)]
        lp = params[8:16]
        Wd = params[24]
        O = Wd.shape[1]
        # output buffers + workspaces of both recurrent launches (a train step: + the BPTT rings), ONE fill
        ypads, wss, bwss = _stack_buffers(any(ctx.needs_input_grad), 2, T4, B, H, 2, dev)
        bwss = _stack_prefill(T4, B, H, 2, ypads, wss, bwss)
        u8 = torch.uint8
        a0 = conv_fwd(ds[0], x, *cw[0], torch.empty(B, 8, T, F, device=dev))            # modules.py:290-293
        am1 = torch.empty(B, 16, T2, N4, dtype=u8, device=dev)
        p1 = conv_fwd(ds[1], a0, *cw[1], torch.empty(B, 16, T2, N4, device=dev), am1)    # :294-300
        a2 = conv_fwd(ds[2], p1, *cw[2], torch.empty(B, 32, T2, N4, device=dev))         # :302-305
        am3 = torch.empty(B, 16, T4, N8, dtype=u8, device=dev)
        p3 = conv_fwd(ds[3], a2, *cw[3], torch.empty(T4, B, D, device=dev), am3)         # :306-311
        conv_act = torch.empty(T4, B, D, device=dev)
        center(p3, B, T4, D, 1, D, conv_act, 1, D)                                       # :313
        c0 = lstm_layer_fwd(conv_act, D, D, T4, B, H, list(lp[0:4:2]), list(lp[1:4:2]),  # :315-324
                            ypad=ypads[0], ws=wss[0])
        spec = _dropout_cur[0]
        ctx.drop = (spec, spec.take(2)) if spec is not None else None
        y0 = c0.ypad[1:]
        if spec is not None:                         # _lyr_bilstm's dropout (modules.py:137), stream id = layer
            y0 = dropout_apply(y0, torch.empty(T4, B, D, device=dev), T4 * B, D, D, D, spec, ctx.drop[1])
        c1 = lstm_layer_fwd(y0, D, D, T4, B, H, list(lp[4:8:2]), list(lp[5:8:2]),           # :325-329
                            ypad=ypads[1], ws=wss[1])
        y1 = c1.ypad[1:T4 + 1]
        if spec is not None:                         # the residual add sees the dropped lstm1 output
            y1 = dropout_apply(y1, torch.empty(T4, B, D, device=dev), T4 * B, D, D, D, spec, ctx.drop[1] + 1)
        s = conv_add(y1, conv_act, torch.empty(T4, B, D, device=dev))                    # :333
        lstm_act = torch.empty(T4, B, D, device=dev)
        center(s, B, T4, D, 1, D, lstm_act, 1, D)                                        # :334
        a4 = conv_fwd(ds[4], lstm_act, *cw[4], torch.empty(B, 32, T4, N8, device=dev))   # :339-343
        mid4 = conv_fwd(ds[5], a4, *cw[5], torch.empty(B, 16, T2, N4, device=dev))       # :344-353
        a6 = conv_fwd(ds[6], mid4, *cw[6], torch.empty(B, 16, T2, N4, device=dev))       # :355-358
        rows = conv_fwd(ds[7], a6, *cw[7], torch.empty(B * T, nfft, device=dev))         # :359-366
        embed = _project_fwd(rows, nfft, Wd, B, T, False)                                # :369-371
        if debug is not None:
            debug.update(conv_act=conv_act, lstm_act=lstm_act, mid4=mid4)
        ctx.bwss = bwss
        ctx.ds, ctx.cw, ctx.Wd = ds, cw, Wd
        ctx.acts = (x, a0, p1, am1, a2, p3, am3, lstm_act, a4, mid4, a6, rows)
        ctx.lstm = (c0, c1)
        ctx.dims = (B, T, F, nfft, O)
        return embed

    @staticmethod
    def backward(ctx, dembed):
        B, T, F, nfft, O = ctx.dims
        T4, D = T // 4, 2 * nfft
        dembed = _f32(dembed.contiguous())
        dev = dembed.device
        ds, cw, Wd = ctx.ds, ctx.cw, ctx.Wd
        x, a0, p1, am1, a2, p3, am3, lstm_act, a4, mid4, a6, rows = ctx.acts
        grads = [None] * 25

        def conv_bwd(l, xin, y, am, dy, dx):
            w, b = cw[l]
            if dx is not None:                       # the critical path first
                conv_bwd_data(ds[l], dy, y, am, w, dx)
            gw, okw = _grad_target(w, tuple(w.shape), dev)
            gb, okb = _grad_target(b, tuple(b.shape), dev)
            direct = okw and okb
            if not direct:
                gw, gb = torch.empty(*w.shape, device=dev), torch.empty(*b.shape, device=dev)
                i = 2 * l if l < 4 else 16 + 2 * (l - 4)
                grads[i], grads[i + 1] = gw, gb
            conv_bwd_weight(ds[l], xin, dy, y, am, gw, gb, accumulate=direct)
            return dx

        # dense (modules.py:369-371): drows = dembed Wd^T, dWd = rows^T dembed
        drows = torch.empty(B * T, nfft, device=dev)
        if _x6_ok(B * T, nfft, (dembed, O, O)):
            gemm_w(dembed, O, Wd, O, 1, drows, B * T, nfft, O, nfft, tag='dYc')
        else:
            gemm(dembed, Wd, drows, B * T, nfft, O, O, O, nfft, transB=True, tag='dYc')
        dWd, okd = _grad_target(Wd, (nfft, O), dev)
        gemm(rows, dembed, dWd, nfft, O, B * T, nfft, O, O, transA=True, beta=1.0 if okd else 0.0, tag='dWout')
        grads[24] = None if okd else dWd
        da6 = conv_bwd(7, a6, rows, None, drows, torch.empty(a6.shape, device=dev))
        dmid4 = conv_bwd(6, mid4, a6, None, da6, torch.empty(a6.shape, device=dev))
        da4 = conv_bwd(5, a4, mid4, None, dmid4, torch.empty(a4.shape, device=dev))
        dla = conv_bwd(4, lstm_act, a4, None, da4, torch.empty(T4, B, D, device=dev))
        # lstm_act = centre(y1 + conv_act): both branches get centre(dla) (centring is self-adjoint)
        g = torch.empty(T4, B, D, device=dev)
        center(dla, B, T4, D, 1, D, g, 1, D)
        bwss = ctx.bwss if ctx.bwss is not None else [None, None]
        ctx.bwss = None
        c0, c1 = ctx.lstm
        dy = g
        drop = ctx.drop
        if drop is not None:       # lstm1's mask; out of place: the residual branch keeps the unmasked g
            dy = dropout_apply(g, torch.empty(T4, B, D, device=dev), T4 * B, D, D, D, drop[0], drop[1] + 1)
        for l, c in ((1, c1), (0, c0)):
            dx, dWs, dbs = lstm_layer_bwd(c, dy, need_dx=True, is_top=(l == 1), ws_prefilled=bwss[l],
                                          dx_drop=(drop[0], drop[1]) if (drop is not None and l == 1) else None)
            for d in range(2):
                grads[8 + 4 * l + 2 * d], grads[9 + 4 * l + 2 * d] = dWs[d], dbs[d]
            dy = dx
        # conv_act feeds lstm0 and the residual: its gradient is the sum, then centring's backward
        dca = conv_add(dy, g, torch.empty(T4, B, D, device=dev))
        dp3 = torch.empty(T4, B, D, device=dev)
        center(dca, B, T4, D, 1, D, dp3, 1, D)
        da2 = conv_bwd(3, a2, p3, am3, dp3, torch.empty(a2.shape, device=dev))
        dp1 = conv_bwd(2, p1, a2, None, da2, torch.empty(p1.shape, device=dev))
        da0 = conv_bwd(1, a0, p1, am1, dp1, torch.empty(a0.shape, device=dev))
        conv_bwd(0, x, a0, None, da0, None)
        join_deferred()
        ctx.acts = ctx.lstm = None
        return (None, None, None, None) + tuple(grads)


class LinearFn(torch.autograd.Function):
    '''ops.lyr_linear on the last axis (app/ops.py:72-78,81-89)'''

    @staticmethod
    def forward(ctx, x, W, b):
        shp = x.shape
        x2 = _f32(x.contiguous()).view(-1, shp[-1])
        M, K = x2.shape
        N = W.shape[1]
        y = torch.empty(M, N, device=x.device)
        gemm(x2, W, y, M, N, K, K, N, N, bias=b)
        ctx.save_for_backward(x2, W)
        ctx.has_b = b is not None
        ctx.shp = shp
        return y.view(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, W = ctx.saved_tensors
        M, K = x2.shape
        N = W.shape[1]
        dy2 = _f32(dy.contiguous()).view(M, N)
        dW = torch.empty(K, N, device=dy.device)
        gemm(x2, dy2, dW, K, N, M, K, N, N, transA=True)
        db = None
        if ctx.has_b:
            db = torch.empty(N, device=dy.device)
            colsum(dy2, M, N, N, db)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, device=dy.device)
            gemm(dy2, W, dx, M, K, N, N, N, K, transB=True)
            dx = dx.view(ctx.shp)
        return dx, dW, db


def lyr_linear(x, W, b=None):
    return LinearFn.apply(x, W, b)


class LeakyReluFn(torch.autograd.Function):
    '''ops.relu (app/ops.py:93-107) as a HIP kernel pair'''

    @staticmethod
    def forward(ctx, x, alpha):
        x = _f32(x.contiguous())
        y = torch.empty_like(x)
        check(_L().danet_leaky_relu(_lib.stream(), x.numel(), ptr(x), None, float(alpha), ptr(y)))
        ctx.save_for_backward(x)
        ctx.alpha = float(alpha)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dx = torch.empty_like(x)
        check(_L().danet_leaky_relu(_lib.stream(), x.numel(), ptr(x), ptr(_f32(dy.contiguous())),
                                    ctx.alpha, ptr(dx)))
        return dx, None


def relu(s_x, alpha=0.):
    '''app/ops.py:93-107 (toy encoder)'''
    return LeakyReluFn.apply(s_x, alpha)


# ---------------------------------------------------------------------------
# estimators / separators / loss
# ---------------------------------------------------------------------------
TRUTH_MODES = {'truth': 0, 'truth-threshold': 1, 'truth-weighted': 2}


# The embedding feeds both the estimator and the separator; autograd would materialise
# the two gradient contributions (42 MB each at cfg 2) and add them.  The separator's
# backward runs first (it consumes the attractors): it leaves its dembed here and the
# estimator's backward -- whose kernels accumulate (`dembed += ...`) -- adds into that
# buffer in place and returns no gradient of its own.  DANET_FUSE_DEMBED=0 disables.
FUSE_DEMBED = _lib.expert('fuse_dembed', 1)
# Inside Model.train_step (heads chain) with the anchor estimator: the fused separator + loss
# backward produces only dattr and the estimator's backward forms the WHOLE embedding gradient in
# one pass (danet_attractor_anchor_bwd_embed_sep) -- the separator's term is not written to HBM
# and read back.  DANET_HEADS_RECOMPUTE=0: the two-pass accumulate-in-place form.
HEADS_RECOMPUTE = _lib.expert('heads_recompute', 1)
# ... and, where the library offers it (C == 2), the fused separator + loss FORWARD already leaves the
# attractor-gradient partials of every permutation behind: its backward then launches nothing at all -- the
# estimator's backward derives the permutation from the records, adds up that permutation's partials and
# uses them as dattr (round 6: one read of the embedding, danet_separate_pit_bwd and its chunk sum gone from
# the train step).  DANET_EXPERT heads_gradfwd=0: the round-5 form.
HEADS_GRADFWD = _lib.expert('heads_gradfwd', 1)


# "Heads chain" scope (entered by Model.train_step around forward + backward): inside it the two
# reductions nobody on the critical path waits for are issued on the side stream --
#   * the loss / SNR / permutation finalize of SeparatePitFn (the backward kernel derives the
#     permutation from the chunk records itself), and
#   * the anchors' gradient finalize of AnchorAttractorFn (only the optimiser reads it)
# -- and joined by `join_deferred()` (RnnEncoderFn.backward ends with it; train_step calls it
# again before the optimiser).  Outside the scope both run in stream order, so a caller that
# reads `loss` right after forward needs no join.
_chain_depth = [0]


class heads_chain(object):
    def __enter__(self):
        _chain_depth[0] += 1
        return self

    def __exit__(self, *exc):
        _chain_depth[0] -= 1
        return False


def _chain():
    return _chain_depth[0] > 0 and SIDE_STREAMS > 0


_lazy = {}          # device index -> [(fn, keep)]


def _dev_key(dev):
    if dev is not None and dev.type != 'cuda':
        return dev.type                    # (host tensors: the data-parallel CPU tests)
    return dev.index if (dev is not None and dev.index is not None) else torch.cuda.current_device()


def _on_side(dev, fn, keep=()):
    '''fn() runs on the side stream at the NEXT fork of the backward pass (behind that fork's
    event, i.e. behind everything issued on the main stream so far), ahead of the fork's own
    work; the main stream joins it at the next join_deferred().  No fork of its own: recording
    an event on the main stream costs it ~8 us (the following kernel cannot overlap the
    previous one's tail), more than the small kernels moved here take.  Without any fork before
    the join, fn() runs in stream order at the join.'''
    _lazy.setdefault(_dev_key(dev), []).append((fn, keep))


def _flush_lazy(dev=None):
    '''run the queued closures of `dev` (default: the current device) on the current stream; a
    closure that raises leaves nothing queued behind it'''
    q = _lazy.get(_dev_key(dev))
    try:
        while q:
            fn, _keep = q.pop(0)
            fn()
    finally:
        if q:
            del q[:]


def drop_lazy(dev=None):
    '''forget the queued side-stream closures of `dev` (Model.train_step: forward raised, the
    finalizers of that step must not run inside the next step's first fork)'''
    q = _lazy.get(_dev_key(dev))
    if q:
        del q[:]


class _DembedToken(object):
    '''links an estimator's autograd node to the separator node that consumes its
    attractors: created in the estimator's forward, carried on the attractor tensor
    (`attr._danet_dembed_token`; lost -- and the fusion with it -- if the caller
    transforms the attractors in between), picked up by SeparateFn.forward.  No global
    state, so several models / re-entrant backward passes cannot alias each other.'''
    __slots__ = ('dembed', 'kind', 'recipe', 'inputs', 'share')

    def __init__(self):
        self.dembed = None
        self.share = True         # False: the separator's dembed is NOT handed over (unshare_dembed)
        self.kind = None          # 'anchor': the estimator's backward can recompute the separator's term
        self.recipe = None        # set by SeparatePitFn.backward when it left that term to the estimator
        self.inputs = None        # (embed ptr, numel, mix_pwr ptr or None) the estimator saw

    def same_inputs(self, embed_flat, mix_pwr):
        '''the recompute kernels form the separator's term from the ESTIMATOR's saved embedding
        (and, for the truth family, are handed the separator's mix_pwr where the estimator's own
        is expected): only valid when both modules were given the same tensors'''
        if self.inputs is None:
            return False
        e_ptr, e_n, m_ptr = self.inputs
        return (embed_flat.data_ptr() == e_ptr and embed_flat.numel() == e_n and
                (m_ptr is None or mix_pwr.data_ptr() == m_ptr))


def _new_token(attr):
    if not FUSE_DEMBED:
        return None
    tok = _DembedToken()
    attr._danet_dembed_token = tok
    return tok


def unshare_dembed(attr):
    """the embedding behind the attractors `attr` has a consumer besides the estimator and the separator (the
    deep-clustering loss): the separator's backward must not hand its dembed to the estimator to add into in place.
    That hand-over relies on the separator's gradient being the tensor autograd keeps for the embedding, which holds
    only while it is the FIRST gradient to arrive; a consumer created after the heads runs its backward before them.
    Both modules then return ordinary gradients and autograd adds them.  (The recompute path of the fused heads hands
    over a recipe, not a buffer, and is not affected.)"""
    tok = getattr(attr, '_danet_dembed_token', None)
    if tok is not None:
        tok.share = False


def _take_dembed(tok, numel):
    if tok is None:
        return None
    t, tok.dembed = tok.dembed, None
    if t is not None and t.numel() == numel:
        return t
    return None


class TruthAttractorFn(torch.autograd.Function):
    '''app/modules.py:382-487'''

    @staticmethod
    def forward(ctx, embed, src_pwr, mix_pwr, mode, eps):
        B, T, F, E = embed.shape
        C = src_pwr.shape[1]
        N = T * F
        dev = embed.device
        embed = _f32(embed.contiguous())
        src_pwr = _f32(src_pwr.contiguous())
        mix_pwr = _f32(mix_pwr.contiguous())
        attr = torch.empty(B, C, E, device=dev)
        denom = torch.empty(B, C, device=dev)
        L = _L()
        w, wn = _ws(_lib.ws_bytes(_lib.WS_ATTRACTOR_TRUTH, B, C, N, E), dev)
        check(L.danet_attractor_truth_fwd(_lib.stream(), mode, B, C, N, E, ptr(embed),
                                          ptr(src_pwr), ptr(mix_pwr), eps, ptr(attr),
                                          ptr(denom), ptr(w), wn))
        ctx.save_for_backward(src_pwr, mix_pwr, denom, embed, attr)
        ctx.args = (mode, eps, B, C, N, E, T, F)
        ctx.token = _new_token(attr)
        if ctx.token is not None:
            ctx.token.kind = 'truth'
            ctx.token.inputs = (embed.data_ptr(), embed.numel(), mix_pwr.data_ptr())
        return attr

    @staticmethod
    def backward(ctx, dattr):
        src_pwr, mix_pwr, denom, embed, attr = ctx.saved_tensors
        mode, eps, B, C, N, E, T, F = ctx.args
        recipe = None
        if ctx.token is not None:
            recipe, ctx.token.recipe = ctx.token.recipe, None
        if recipe is not None:
            # the separator's embedding-gradient term is recomputed here (one pass, one store)
            act, lmode, s_mix, src, phasor, records, dl, gpart = recipe
            dembed = torch.empty(B, T, F, E, device=dattr.device)
            # (gpart: dattr is formed by the kernel from the forward's partials; the tensor autograd
            # handed over is a placeholder)
            check(_L().danet_attractor_truth_bwd_sep(
                _lib.stream(), mode, B, C, N, E, None if gpart is not None else ptr(_f32(dattr.contiguous())),
                ptr(src_pwr), ptr(s_mix), ptr(denom), eps, ptr(embed), ptr(attr), act, lmode,
                ptr(torch.view_as_real(src)), ptr(phasor), None, ptr(records), 1.0, ptr(dl),
                ptr(dembed), ptr(gpart)))
            return dembed, None, None, None, None
        shared = _take_dembed(ctx.token, B * T * F * E)
        dembed = shared if shared is not None else torch.zeros(B, T, F, E, device=dattr.device)
        check(_L().danet_attractor_truth_bwd(
            _lib.stream(), mode, B, C, N, E, ptr(_f32(dattr.contiguous())), ptr(src_pwr),
            ptr(mix_pwr), ptr(denom), eps, ptr(dembed)))
        return (None if shared is not None else dembed), None, None, None, None


class AnchorAttractorFn(torch.autograd.Function):
    '''app/modules.py:490-545.  Returns (attr, asets, subset_choice)'''

    @staticmethod
    def forward(ctx, embed, anchors, C):
        B, T, F, E = embed.shape
        A = anchors.shape[0]
        N = T * F
        dev = embed.device
        embed = _f32(embed.contiguous())
        anchors_in = anchors
        anchors = _f32(anchors.contiguous())
        P = math.comb(A, C)
        attr = torch.empty(B, C, E, device=dev)
        asets = torch.empty(B, P, C, E, device=dev)
        asum = torch.empty(B, P, C, device=dev)
        choice = torch.empty(B, dtype=torch.int32, device=dev)
        L = _L()
        w, wn = _ws(_lib.ws_bytes(_lib.WS_ATTRACTOR_ANCHOR, B, C, N, E, A), dev)
        check(L.danet_attractor_anchor_fwd(_lib.stream(), B, C, N, E, A, ptr(embed),
                                           ptr(anchors), ptr(attr), ptr(asets), ptr(asum),
                                           ptr(choice), ptr(w), wn))
        ctx.save_for_backward(embed, anchors, attr, asum, choice)
        ctx.anchors_param = anchors_in      # the parameter object (owner of .grad), not a copy
        ctx.args = (B, C, N, E, A, T, F)
        ctx.mark_non_differentiable(asets, choice)
        ctx.set_materialize_grads(False)
        ctx.token = _new_token(attr)
        if ctx.token is not None:
            ctx.token.kind = 'anchor'
            ctx.token.inputs = (embed.data_ptr(), embed.numel(), None)
        return attr, asets, choice

    @staticmethod
    def backward(ctx, dattr, _dasets, _dchoice):
        if dattr is None:
            return None, None, None
        embed, anchors, attr, asum, choice = ctx.saved_tensors
        B, C, N, E, A, T, F = ctx.args
        dev = dattr.device
        recipe = None
        if ctx.token is not None:
            recipe, ctx.token.recipe = ctx.token.recipe, None
        shared = None if recipe is not None else _take_dembed(ctx.token, B * T * F * E)
        if recipe is not None:
            dembed = torch.empty(B, T, F, E, device=dev)       # written whole by the kernel
        else:
            dembed = shared if shared is not None else torch.zeros(B, T, F, E, device=dev)
        # fast backward: add straight into the parameter's .grad (no autograd accumulate kernel)
        danchors, direct = _grad_target(ctx.anchors_param, (A, E), dev)
        L = _L()
        nbytes = _lib.ws_bytes(_lib.WS_ATTRACTOR_ANCHOR, B, C, N, E, A)
        dattr = _f32(dattr.contiguous())
        if recipe is not None:
            # the separator's embedding-gradient term is recomputed here (one pass, one store)
            act, mode, mix_pwr, src, phasor, records, dl, gpart = recipe
            w = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(L.danet_attractor_anchor_bwd_embed_sep(
                _lib.stream(), B, C, N, E, A, None if gpart is not None else ptr(dattr), ptr(embed),
                ptr(anchors), ptr(attr), ptr(asum), ptr(choice), act, mode, ptr(mix_pwr),
                ptr(torch.view_as_real(src)), ptr(phasor), None, ptr(records), 1.0, ptr(dl), ptr(dembed),
                ptr(w), nbytes, ptr(gpart)))
            _on_side(dev, lambda: check(L.danet_attractor_anchor_bwd_anchors(
                _lib.stream(), B, C, N, E, A, ptr(choice), ptr(danchors), ptr(w), nbytes,
                1.0 if direct else 0.0)), keep=(w, choice, danchors))
        elif _chain():
            # part 1 (dembed) on this stream; part 2 (danchors, from the chunk partials) on the
            # side stream: its own scratch, kept alive until the join
            w = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(L.danet_attractor_anchor_bwd_embed(
                _lib.stream(), B, C, N, E, A, ptr(dattr), ptr(embed), ptr(anchors), ptr(attr),
                ptr(asum), ptr(choice), ptr(dembed), ptr(w), nbytes))
            _on_side(dev, lambda: check(L.danet_attractor_anchor_bwd_anchors(
                _lib.stream(), B, C, N, E, A, ptr(choice), ptr(danchors), ptr(w), nbytes,
                1.0 if direct else 0.0)), keep=(w, choice, danchors))
        else:
            w, wn = _ws(nbytes, dev)
            check(L.danet_attractor_anchor_bwd_embed(
                _lib.stream(), B, C, N, E, A, ptr(dattr), ptr(embed), ptr(anchors), ptr(attr),
                ptr(asum), ptr(choice), ptr(dembed), ptr(w), wn))
            check(L.danet_attractor_anchor_bwd_anchors(
                _lib.stream(), B, C, N, E, A, ptr(choice), ptr(danchors), ptr(w), wn,
                1.0 if direct else 0.0))
        return (None if shared is not None else dembed), (None if direct else danchors), None


class SeparateFn(torch.autograd.Function):
    '''app/modules.py:548-603.  act 0 softmax / 1 sigmoid.
    (mix_pwr [B,T,F], attr [B,C,E], embed_flat [B,N,E]) -> (sep [B,C,T,F], masks)'''

    @staticmethod
    def forward(ctx, mix_pwr, attr, embed_flat, act, want_masks):
        B, T, F = mix_pwr.shape
        C, E = attr.shape[1], attr.shape[2]
        N = T * F
        dev = mix_pwr.device
        mix_pwr = _f32(mix_pwr.contiguous())
        attr = _f32(attr.contiguous())
        embed_flat = _f32(embed_flat.contiguous())
        out = torch.empty(B, C, T, F, device=dev)
        masks = torch.empty(B, T, F, C, device=dev) if want_masks else None
        check(_L().danet_separate_fwd(_lib.stream(), act, B, C, N, E, ptr(mix_pwr), ptr(attr),
                                      ptr(embed_flat), ptr(out), ptr(masks)))
        ctx.save_for_backward(mix_pwr, attr, embed_flat)
        ctx.args = (act, B, C, N, E)
        ctx.token = getattr(attr, '_danet_dembed_token', None)
        if masks is None:
            masks = torch.empty(0, device=dev)
        ctx.mark_non_differentiable(masks)
        ctx.set_materialize_grads(False)
        return out, masks

    @staticmethod
    def backward(ctx, dout, _dmasks):
        if dout is None:
            return None, None, None, None, None
        mix_pwr, attr, embed_flat = ctx.saved_tensors
        act, B, C, N, E = ctx.args
        dev = dout.device
        dembed = torch.empty(B, N, E, device=dev)
        dattr = torch.empty(B, C, E, device=dev)
        L = _L()
        w, wn = _ws(_lib.ws_bytes(_lib.WS_SEPARATE_BWD, B, C, N, E), dev)
        check(L.danet_separate_bwd(_lib.stream(), act, B, C, N, E, ptr(mix_pwr), ptr(attr),
                                   ptr(embed_flat), ptr(_f32(dout.contiguous())), ptr(dembed),
                                   ptr(dattr), ptr(w), wn))
        if ctx.token is not None and ctx.token.share and ctx.needs_input_grad[1]:
            # the estimator that made `attr` runs its backward next and adds into `dembed`
            ctx.token.dembed = dembed
        return None, dattr, dembed, None, None


class PitMseFn(torch.autograd.Function):
    '''ops.pit_mse_loss (app/ops.py:374-431) fused with the phase re-attach
    (main.py:281-284) and batch_snr (app/ops.py:191-222).
    mode 0: complex MSE (train, main.py:289-290); mode 1: magnitude MSE
    (valid, main.py:312-313).  Returns (loss, snr, perm_idx)'''

    @staticmethod
    def forward(ctx, src, sep_pwr, phasor, mode, eps):
        assert src.dtype == torch.complex64
        B, C, T, F = sep_pwr.shape
        N = T * F
        dev = sep_pwr.device
        src = src.contiguous()
        sep_pwr = _f32(sep_pwr.contiguous())
        phasor = _f32(phasor.contiguous())
        loss, snr = torch.empty((), device=dev), torch.empty((), device=dev)
        perm_idx = torch.empty(B, dtype=torch.int32, device=dev)
        L = _L()
        w, wn = _ws(_lib.ws_bytes(_lib.WS_PIT_MSE, B, C, N), dev)
        check(L.danet_pit_mse_fwd(_lib.stream(), mode, B, C, N, ptr(torch.view_as_real(src)),
                                  ptr(sep_pwr), ptr(phasor), eps, ptr(loss), ptr(snr),
                                  ptr(perm_idx), ptr(w), wn))
        ctx.save_for_backward(src, sep_pwr, phasor, perm_idx)
        ctx.args = (mode, B, C, N)
        ctx.mark_non_differentiable(snr, perm_idx)
        ctx.set_materialize_grads(False)
        return loss, snr, perm_idx

    @staticmethod
    def backward(ctx, dloss, _dsnr, _dperm):
        src, sep_pwr, phasor, perm_idx = ctx.saved_tensors
        mode, B, C, N = ctx.args
        if dloss is None:
            return None, None, None, None, None
        dsep = torch.empty_like(sep_pwr)
        # dloss is a device scalar: the kernel reads it (no host sync, no extra pass)
        check(_L().danet_pit_mse_bwd(_lib.stream(), mode, B, C, N,
                                     ptr(torch.view_as_real(src)), ptr(sep_pwr), ptr(phasor),
                                     ptr(perm_idx), 1.0, ptr(_f32(dloss.contiguous())), ptr(dsep)))
        return None, dsep, None, None, None


class SeparatePitFn(torch.autograd.Function):
    '''Separator + phase re-attach + PIT-MSE + SNR in ONE pass over the embedding and ONE
    pass back (danet_separate_pit_fwd_records + _final / _bwd): the training path of app/modules.py:548-603 ->
    main.py:281-290, 308-309 -> app/ops.py:374-431.  Same arithmetic as SeparateFn followed by
    PitMseFn; the masks, the separated magnitudes and dL/dsep never touch HBM.
    (mix_pwr [B,T,F], attr [B,C,E], embed_flat [B,N,E], src complex64 [B,C,T,F],
    phasor [B,T,F,2]) -> (loss, snr, perm_idx)'''

    @staticmethod
    def forward(ctx, mix_pwr, attr, embed_flat, src, phasor, act, mode, eps):
        assert src.dtype == torch.complex64
        B, T, F = mix_pwr.shape
        C, E = attr.shape[1], attr.shape[2]
        N = T * F
        dev = mix_pwr.device
        mix_pwr = _f32(mix_pwr.contiguous())
        attr_c = _f32(attr.contiguous())
        embed_flat = _f32(embed_flat.contiguous())
        src = src.contiguous()
        phasor = _f32(phasor.contiguous())
        loss, snr = torch.empty((), device=dev), torch.empty((), device=dev)
        perm_idx = torch.empty(B, dtype=torch.int32, device=dev)
        L = _L()
        records = torch.empty(_lib.ws_bytes(_lib.WS_SEPARATE_PIT_RECORDS, B, N) // 4, device=dev)
        # the backward's attractor-gradient partials already here?  Only where the backward will be able
        # to leave everything to the estimator's backward (the conditions of `defer` below, as far as
        # they are known now) and the library offers it for the shape
        tok = getattr(attr, '_danet_dembed_token', None)
        gpart = None
        if (HEADS_GRADFWD and HEADS_RECOMPUTE and _chain() and tok is not None and
                tok.kind in ('anchor', 'truth') and ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and
                tok.same_inputs(embed_flat, mix_pwr)):
            nb = _lib.ws_bytes(_lib.WS_SEPARATE_PIT_GRAD, B, C, N, E)
            if nb:
                gpart = torch.empty(nb // 4, device=dev)
        check(L.danet_separate_pit_fwd_records(
            _lib.stream(), act, mode, B, C, N, E, ptr(mix_pwr), ptr(attr_c), ptr(embed_flat),
            ptr(torch.view_as_real(src)), ptr(phasor), None, ptr(records), ptr(gpart)))
        ctx.gpart = gpart

        def final():
            check(L.danet_separate_pit_final(_lib.stream(), B, C, N, eps, ptr(records), ptr(loss),
                                             ptr(snr), ptr(perm_idx)))
        if _chain():
            _on_side(dev, final, keep=(records, loss, snr, perm_idx))   # the backward does not wait for it
        else:
            final()
        ctx.records = records
        ctx.save_for_backward(mix_pwr, attr_c, embed_flat, src, phasor, perm_idx)
        ctx.args = (act, mode, B, C, N, E)
        ctx.token = getattr(attr, '_danet_dembed_token', None)
        ctx.mark_non_differentiable(snr, perm_idx)
        ctx.set_materialize_grads(False)
        return loss, snr, perm_idx

    @staticmethod
    def backward(ctx, dloss, _dsnr, _dperm):
        if dloss is None:
            return (None,) * 8
        mix_pwr, attr, embed_flat, src, phasor, perm_idx = ctx.saved_tensors
        act, mode, B, C, N, E = ctx.args
        records, ctx.records = ctx.records, None
        gpart, ctx.gpart = ctx.gpart, None
        dev = dloss.device
        tok = ctx.token
        defer = (HEADS_RECOMPUTE and _chain() and tok is not None and tok.kind in ('anchor', 'truth') and
                 ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and
                 tok.same_inputs(embed_flat, mix_pwr))
        dembed = None if defer else torch.empty(B, N, E, device=dev)
        dattr = torch.empty(B, C, E, device=dev)
        dl = _f32(dloss.contiguous())
        L = _L()
        if defer and gpart is not None:
            # nothing to launch: the estimator's backward (next node) forms dattr from the forward's
            # partials and the whole embedding gradient; `dattr` is a placeholder that only keeps
            # autograd walking to that node
            tok.recipe = (act, mode, mix_pwr, src, phasor, records, dl, gpart)
            return None, dattr, None, None, None, None, None, None
        w, wn = _ws(_lib.ws_bytes(_lib.WS_SEPARATE_PIT, B, C, N, E), dev)
        # dloss is a device scalar: the kernel reads it (no host sync, no extra pass)
        check(L.danet_separate_pit_bwd(_lib.stream(), act, mode, B, C, N, E, ptr(mix_pwr),
                                       ptr(attr), ptr(embed_flat), ptr(torch.view_as_real(src)),
                                       ptr(phasor), None, ptr(records), 1.0,
                                       ptr(dl), ptr(dembed), ptr(dattr), ptr(w), wn))
        if defer:
            # the estimator's backward (next node) recomputes this kernel's dembed term
            # and returns the whole embedding gradient
            tok.recipe = (act, mode, mix_pwr, src, phasor, records, dl, None)
            return None, dattr, None, None, None, None, None, None
        if ctx.token is not None and ctx.token.share and ctx.needs_input_grad[1]:
            # the estimator that made `attr` runs its backward next and adds into `dembed`
            ctx.token.dembed = dembed
        return None, dattr, dembed, None, None, None, None, None


def separate_pit_loss(s_mix_pwr, s_attractors, s_embed_flat, s_x, phasor, act, mode=0, eps=1e-7):
    '''fused separator + pit_mse_loss; returns (s_loss, v_perms, s_loss_sets_idx, snr) like
    pit_mse_loss'''
    C = s_attractors.shape[1]
    loss, snr, idx = SeparatePitFn.apply(s_mix_pwr, s_attractors, s_embed_flat, s_x, phasor,
                                         act, mode, eps)
    v_perms = torch.tensor(list(itertools.permutations(range(C))), dtype=torch.int32)
    return loss, v_perms, idx, snr


def pit_mse_loss(s_x, s_y_pwr, phasor, mode=0, eps=1e-7):
    '''returns (s_loss, v_perms, s_loss_sets_idx, snr) like app/ops.py:374-431'''
    C = s_y_pwr.shape[1]
    loss, snr, idx = PitMseFn.apply(s_x, s_y_pwr, phasor, mode, eps)
    v_perms = torch.tensor(list(itertools.permutations(range(C))), dtype=torch.int32)
    return loss, v_perms, idx, snr


def adam_clip_step(theta, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, clip=100.0,
                   grad_scale=1.0, zero_grad=False):
    '''flat fp32 buffers; tf.train.AdamOptimizer + clip_by_value
    (main.py:359-363, app/ozers.py:15-18)'''
    check(_L().danet_adam_clip_step(_lib.stream(), theta.numel(), ptr(_f32(theta)),
                                    ptr(_f32(grad)), ptr(_f32(m)), ptr(_f32(v)), lr_t, beta1,
                                    beta2, eps, clip if clip else 0.0, grad_scale,
                                    int(bool(zero_grad))))
    weights_written(theta)


def gclip_partials(n):
    '''danet_gclip_partials(n): the float64 partials of the sum of squares of n gradient values'''
    p = _lib.load_gclip().danet_gclip_partials(int(n))
    if p <= 0:
        _lib.gclip_check(-1)
    return p


def grad_sumsq(grad, partials=None):
    '''the sum of squares of the flat fp32 gradient as float64 per-workgroup partials (include/danet_gclip_hip.h);
    partials: the buffer of a previous call with the same length (None: a new one) -> partials'''
    n = grad.numel()
    if partials is None:
        partials = torch.empty(gclip_partials(n), dtype=torch.float64, device=grad.device)
    assert partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous(), partials.dtype
    _lib.gclip_check(_lib.load_gclip().danet_gclip_sumsq(_lib.stream(), n, ptr(_f32(grad)), ptr(partials),
                                                         partials.numel()))
    return partials


def adam_gclip_step(theta, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, clip=100.0,
                    grad_scale=1.0, zero_grad=False, max_norm=None, partials=None, norm_out=None):
    '''adam_clip_step with the gradient scaled by grad_scale * coef, coef the global-norm clip coefficient formed
    on the device from `partials` (grad_sumsq of the same gradient) and `max_norm`; norm_out: float64 [2] that
    receives (norm, coef)'''
    assert norm_out.is_cuda and norm_out.dtype == torch.float64 and norm_out.numel() == 2
    assert partials.is_cuda and partials.dtype == torch.float64
    _lib.gclip_check(_lib.load_gclip().danet_gclip_adam_step(
        _lib.stream(), theta.numel(), ptr(_f32(theta)), ptr(_f32(grad)), ptr(_f32(m)), ptr(_f32(v)), lr_t, beta1,
        beta2, eps, clip if clip else 0.0, grad_scale, int(bool(zero_grad)), float(max_norm), ptr(partials),
        partials.numel(), ptr(norm_out)))
    weights_written(theta)
