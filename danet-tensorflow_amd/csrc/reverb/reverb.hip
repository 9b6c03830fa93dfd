/*
 * libdanet_reverb_hip.so (include/danet_reverb_hip.h): every utterance of a ragged batch convolved with
 * one row of a bank of room responses of up to 8192 taps.  gfx950, wave64.  The VECTOR form: fused
 * multiply-adds on the VALU, one chain per output, j ascending -- the summation order the header fixes.
 *
 * One persistent launch: min(4 * compute units, an upper bound of the tiles) workgroups of 128 threads.
 * A workgroup walks the descriptor rows in order with a running tile count -- every workgroup reads every
 * row, 48 bytes of uniform loads each -- and takes the tiles whose running index is its own modulo the
 * grid: no list is built, no atomic is used, the split is a pure function of the table.
 *
 * A tile is the part of a row's span inside one BLOCK of 1024 outputs; blocks are counted from output
 * sample 0, not from the span's first sample, so which chain a sample gets is a function of the sample
 * alone.  Lane l owns the eight consecutive outputs nb + 8 l + r, r < 8, of block nb in registers.  The
 * taps the block needs, j < Kt = min(K, ceil4(min(nb + 1024, L))), are walked in chunks of at most 1024:
 * the chunk h[jc .. jc + kc) and the samples x[nb - jc - kc .. nb - jc + 1024) it meets are staged in
 * LDS; per four taps a lane loads ONE new 16-byte vector of x (its window of twelve samples slides down
 * by four: the other two vectors stay in registers) and one 16-byte vector of h that every lane reads at
 * the same address (a broadcast), and issues 32 fused multiply-adds.  The accumulators stay in registers
 * across the chunks.  Everything written goes through ordinary vector stores.
 */
#include <hip/hip_runtime.h>

#include "danet_reverb_hip.h"
#define DANET_EXT reverb
#define DANET_EXT_UPPER REVERB
#include "ext_core.h"
#include "ragged_rows.h"

static const int kThreads = 128;
static const int kPerLane = 8;                    /* consecutive outputs of a lane           */
static const int kTile = kThreads * kPerLane;     /* outputs of a block                      */
static const int kChunk = 1024;                   /* taps staged at a time                   */
static const int kBlocksPerCu = 4;
static const int64_t kMaxLen = kMaxSpan;          /* 2^40: what cut_span cuts to */

static_assert(kTile == 1024, "the header's rule names the block of 1024 outputs");
static_assert(kChunk % 4 == 0 && kTile % 4 == 0 && DANET_REVERB_MAX_TAPS % 4 == 0, "16-byte vectors");
static_assert(sizeof(danet_reverb_utt_t) == 48, "descriptor row");

struct ReverbArgs {
  const float* src;
  int64_t src_len;
  const danet_reverb_utt_t* desc;
  const float* bank;
  float* dst;
  int64_t dst_len;
  int n_utt;
  int n_taps;
};

/* a row as the kernel uses it: sample i of the utterance is src[so + i] for lo <= i < hi and zero
 * elsewhere; it has L samples; output n is written to dst[dof + n] for nlo <= n < nhi */
struct Row {
  int64_t so, lo, hi, L, dof, nlo, nhi;
  int row;
};

__device__ __forceinline__ Row load_row(const ReverbArgs& a, int u) {
  const danet_reverb_utt_t d = a.desc[u];
  Row r;
  r.so = d.src_offset;
  r.dof = d.dst_offset;
  r.row = d.row < 0 ? 0 : (d.row >= DANET_REVERB_ROWS ? DANET_REVERB_ROWS - 1 : d.row);
  int64_t L = d.src_length;
  if (L < 0) L = 0;
  if (L > kMaxLen) L = kMaxLen;
  r.L = L;
  int64_t lo, hi;                                   /* [0, L) cut to the samples i with 0 <= so + i < src_len */
  cut_span(r.so, L, a.src_len, lo, hi);
  r.lo = lo;
  r.hi = hi;
  /* the span [out_begin, out_begin + out_count) cut to [0, L) ... */
  int64_t ob = d.out_begin, oc = d.out_count;
  if (oc < 0) oc = 0;
  if (oc > kMaxLen) oc = kMaxLen;
  if (ob < 0) {
    oc = ob < -kMaxLen ? 0 : (oc + ob > 0 ? oc + ob : 0);
    ob = 0;
  }
  if (ob > L) ob = L;
  r.nlo = ob;
  r.nhi = ob + oc < L ? ob + oc : L;                /* ob, oc <= 2^40 */
  /* ... and to the outputs n with 0 <= dof + n < dst_len */
  if (r.dof >= a.dst_len || r.dof < -kMaxLen) {
    r.nlo = r.nhi = 0;
  } else {
    if (r.nlo < -r.dof) r.nlo = -r.dof;
    if (r.nhi > a.dst_len - r.dof) r.nhi = a.dst_len - r.dof;
    if (r.nhi < r.nlo) r.nhi = r.nlo;
  }
  return r;
}

/* four taps c[0..3] = h[j .. j + 3] against the window w0 | w1 | w2 = x[q - 4 .. q + 8), q = n0 - j:
 * output r meets tap j + k at x[n0 + r - j - k] = window[4 + r - k]; k ascending keeps the chain's order */
__device__ __forceinline__ void four_taps(float (&acc)[kPerLane], const f32x4 c, const f32x4 w0, const f32x4 w1,
                                          const f32x4 w2) {
  const float w[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) acc[r] = __builtin_fmaf(c[k], w[4 + r - k], acc[r]);
  }
}

__global__ __launch_bounds__(kThreads) void reverb_apply_kernel(ReverbArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[kTile + kChunk];
  __shared__ __attribute__((aligned(16))) float hs[kChunk];
  const int tid = threadIdx.x;
  const int64_t G = gridDim.x, b = blockIdx.x;
  const int K = a.n_taps;
  int64_t g0 = 0;                                     /* tiles of the rows in front of row u */
  for (int u = 0; u < a.n_utt; ++u) {
    const Row r = load_row(a, u);
    const int64_t t_first = r.nlo / kTile;
    const int64_t nt = r.nhi > r.nlo ? (r.nhi - 1) / kTile - t_first + 1 : 0;
    const float* h = a.bank + (int64_t)r.row * K;
    for (int64_t t = (b + G - g0 % G) % G; t < nt; t += G) {
      const int64_t nb = (t_first + t) * kTile;       /* first output of the block */
      const int64_t tlo = nb > r.nlo ? nb : r.nlo;    /* the tile: [tlo, thi) */
      const int64_t thi = nb + kTile < r.nhi ? nb + kTile : r.nhi;
      const int64_t xend = nb + kTile < r.L ? nb + kTile : r.L;        /* > nb >= 0 */
      const int Kt = (int)(((xend + 3) & ~(int64_t)3) < K ? ((xend + 3) & ~(int64_t)3) : K);
      const int64_t n0 = nb + kPerLane * tid;
      const bool active = n0 + kPerLane > tlo && n0 < thi;
      float acc[kPerLane];
#pragma unroll
      for (int q = 0; q < kPerLane; ++q) acc[q] = 0.0f;
      for (int jc = 0; jc < Kt; jc += kChunk) {
        const int kc = Kt - jc < kChunk ? Kt - jc : kChunk;            /* a multiple of 4 */
        const int64_t xb = nb - jc - kc;              /* xs[i] is sample xb + i; xb is a multiple of 4 */
        __syncthreads();                              /* the chunk before is read */
        for (int v = tid; v < kc / 4; v += kThreads)
          *reinterpret_cast<f32x4*>(hs + 4 * v) = *reinterpret_cast<const f32x4*>(h + jc + 4 * v);
        for (int v = tid; v < (kTile + kc) / 4; v += kThreads) {
          const int64_t i = xb + 4 * (int64_t)v;
          f32x4 x;
          /* (the 16-byte load needs the address, not the sample index, to be a multiple of 4 floats) */
          if (i >= r.lo && i + 4 <= r.hi && ((((uintptr_t)a.src >> 2) + (uint64_t)r.so + (uint64_t)i) & 3) == 0) {
            x = *reinterpret_cast<const f32x4*>(a.src + r.so + i);
          } else {
            for (int k = 0; k < 4; ++k) x[k] = (i + k >= r.lo && i + k < r.hi) ? a.src[r.so + i + k] : 0.0f;
          }
          *reinterpret_cast<f32x4*>(xs + 4 * v) = x;
        }
        __syncthreads();
        if (active) {
          /* tap jc + jj meets output n0 + r at xs[p - jj + r], p = 8 tid + kc */
          const float* xp = xs + kPerLane * tid + kc;
          f32x4 w1 = *reinterpret_cast<const f32x4*>(xp);
          f32x4 w2 = *reinterpret_cast<const f32x4*>(xp + 4);
#pragma unroll 3
          for (int jj = 0; jj < kc; jj += 4) {
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(xp - 4 - jj);
            const f32x4 c = *reinterpret_cast<const f32x4*>(hs + jj);
            four_taps(acc, c, w0, w1, w2);
            w2 = w1;
            w1 = w0;
          }
        }
      }
      if (active) {
#pragma unroll
        for (int q = 0; q < kPerLane; ++q) {
          const int64_t n = n0 + q;
          if (n >= tlo && n < thi) a.dst[r.dof + n] = acc[q];
        }
      }
    }
    g0 += nt;
  }
}

/* compute units of the current device, asked once per device and thread */
static int compute_units(void) {
  static thread_local int cached_dev = -1, cached_cus = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev != cached_dev) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cached_dev = dev;
    cached_cus = cus;
  }
  return cached_cus;
}

extern "C" int danet_reverb_apply(void* stream, int n_utt, const float* src, int64_t src_len,
                                  const danet_reverb_utt_t* desc, const float* bank, int n_taps, float* dst,
                                  int64_t dst_len) {
  CHECK_ARG(n_utt >= 1, "apply: n_utt must be >= 1 (got %d)", n_utt);
  CHECK_ARG(src && desc && bank && dst, "apply: null pointer");
  CHECK_ARG(n_taps >= DANET_REVERB_MIN_TAPS && n_taps <= DANET_REVERB_MAX_TAPS && n_taps % 4 == 0,
            "apply: n_taps must be a multiple of 4 in [%d, %d] (got %d)", DANET_REVERB_MIN_TAPS,
            DANET_REVERB_MAX_TAPS, n_taps);
  CHECK_ARG(src_len >= 0 && src_len <= kMaxLen && dst_len >= 0 && dst_len <= kMaxLen,
            "apply: src_len and dst_len must be in [0, 2^40] (got %lld, %lld)", (long long)src_len,
            (long long)dst_len);
  CHECK_ARG(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)desc & 7) == 0 &&
                ((uintptr_t)bank & 15) == 0,
            "apply: misaligned pointer (src, dst 4-byte; desc 8-byte; bank 16-byte)");
  const int cus = compute_units();
  if (cus < 1) {
    set_error("apply: no device (%s:%d)", __FILE__, __LINE__);
    return DANET_REVERB_ERR_LAUNCH;
  }
  /* a row's span of c outputs inside dst meets at most c / 1024 + 2 blocks: with disjoint spans this bounds
   * the sum (the bound only sizes the grid: the walk covers every tile whatever the grid) */
  const int64_t bound = dst_len / kTile + 2 * (int64_t)n_utt;
  const int64_t most = (int64_t)kBlocksPerCu * cus;
  ReverbArgs a;
  a.src = src; a.src_len = src_len; a.desc = desc; a.bank = bank; a.dst = dst; a.dst_len = dst_len;
  a.n_utt = n_utt; a.n_taps = n_taps;
  reverb_apply_kernel<<<dim3((unsigned)(bound < most ? bound : most)), kThreads, 0, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_REVERB_OK;
}
