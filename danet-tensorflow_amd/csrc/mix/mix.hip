/*
 * libdanet_mix_hip.so (include/danet_mix_hip.h): the power of every utterance of a ragged pool, and a
 * per-utterance gain on the complex64 batch of the ragged-batch STFT.  gfx950, wave64.
 *
 * danet_mix_power.  One workgroup of 256 threads per (row, slice); a slice is
 * max(65536, ceil4(max_len / 256)) samples, so a row of millions of samples is spread over up to 256
 * workgroups while a short row costs one, and thousands of rows go in ONE launch (grid = rows x
 * slices; a workgroup whose slice starts beyond its row returns before it loads anything).  The row
 * is clamped by clamp_row of csrc/ragged_rows.h; a slice's sum is that of csrc/sumsq_f64.h, which
 * describes it: slice_sumsq per thread, wave_sums, and thread 0 adds the four wave sums as
 * (w0 + w1) + (w2 + w3).  Longest chain of additions: slice / 1024 + 2 (thread) + 2 (head,
 * tail) + 8 (workgroup) + slices (second launch) <= 2^21 + 268 at max_len = 2^39.  With one slice
 * per row the workgroup writes the result itself; otherwise it writes ws[row][slice] and a second
 * launch, one thread per row, adds the row's slices in index order.  No read-modify-write on
 * memory anywhere, so the result is a pure function of the arguments.
 *
 * danet_mix_scale_c64.  Element-wise, in place.  With ld == F an utterance is one contiguous span
 * of t_count * F complex elements: workgroups take 4096-element pieces of it as 16-byte loads and
 * stores (an 8-byte access at a piece's misaligned head or odd tail; F is odd).  With ld > F a
 * workgroup takes max(1, 4096 / F) rows of one utterance, each row a span of its own, so the pitch
 * gaps are never loaded into a store.
 */
#include <hip/hip_runtime.h>

#include "danet_mix_hip.h"
#define DANET_EXT mix
#define DANET_EXT_UPPER MIX
#include "ext_core.h"
#include "ragged_rows.h"
#include "sumsq_f64.h"

static const int64_t kMinSlice = 65536;
static const int kMaxSlices = 256;
static const int64_t kMaxLen = (int64_t)1 << 39;

/* ---------------------------------------------------------------------------------- power */
struct Slicing {
  int64_t slice;   /* samples per slice, a multiple of 4 */
  int n_slices;    /* slices of a max_len row, >= 1      */
};

static Slicing slicing_of(int64_t max_len) {
  Slicing g;
  g.slice = (((max_len + kMaxSlices - 1) / kMaxSlices) + 3) & ~(int64_t)3;
  if (g.slice < kMinSlice) g.slice = kMinSlice;
  g.n_slices = (int)((max_len + g.slice - 1) / g.slice);
  if (g.n_slices < 1) g.n_slices = 1;
  return g;
}

extern "C" size_t danet_mix_workspace_bytes(int n_utt, int64_t max_len) {
  if (n_utt < 1 || max_len < 0 || max_len > kMaxLen) {
    set_error("workspace_bytes: need n_utt >= 1 and 0 <= max_len <= 2^39 (got %d, %lld)", n_utt,
              (long long)max_len);
    return (size_t)-1;
  }
  const Slicing g = slicing_of(max_len);
  return g.n_slices == 1 ? 0 : (size_t)n_utt * (size_t)g.n_slices * sizeof(double);
}

struct PowerArgs : RowTable {
  int64_t slice;
  int n_slices;
  double* out;
  double* ws;      /* [n_utt][n_slices] when n_slices > 1 */
};

__global__ __launch_bounds__(kThreads) void mix_power_kernel(PowerArgs a) {
  __shared__ double part[kWaves];
  const int tid = threadIdx.x;
  const int u = (int)(blockIdx.x / (unsigned)a.n_slices);
  const int s = (int)(blockIdx.x - (unsigned)u * (unsigned)a.n_slices);
  int64_t off, len;
  clamp_row(a, u, off, len);
  const int64_t b = (int64_t)s * a.slice;
  if (b >= len) {                                 /* (uniform) nothing of this row here */
    if (a.n_slices == 1 && tid == 0) a.out[u] = 0.0;
    return;
  }
  const int64_t n = min(a.slice, len - b);
  const float* x = a.pool + off + b;
  wave_sums(slice_sumsq(x, n), part);
  if (tid == 0) {
    const double r = four_waves(part);
    if (a.n_slices == 1) a.out[u] = r;
    else a.ws[(int64_t)u * a.n_slices + s] = r;
  }
}

__global__ __launch_bounds__(kThreads) void mix_power_rows_kernel(PowerArgs a, int n_utt) {
  const int u = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
  if (u >= n_utt) return;
  int64_t off, len;
  clamp_row(a, u, off, len);
  const int np = (int)((len + a.slice - 1) / a.slice);     /* the slices phase one wrote */
  const double* p = a.ws + (int64_t)u * a.n_slices;
  double acc = 0.0;
  for (int k = 0; k < np; ++k) acc += p[k];
  a.out[u] = acc;
}

extern "C" int danet_mix_power(void* stream, int n_utt, const float* pool, int64_t pool_len,
                               const int64_t* offsets, const int64_t* lengths, int64_t max_len, double* out_f64,
                               void* ws, size_t ws_bytes) {
  CHECK_ARG(n_utt >= 1, "power: n_utt must be >= 1 (got %d)", n_utt);
  CHECK_ARG(pool_len >= 0, "power: pool_len must be >= 0");
  CHECK_ARG(max_len >= 0 && max_len <= kMaxLen, "power: max_len must be in [0, 2^39] (got %lld)",
            (long long)max_len);
  CHECK_ARG(pool && offsets && lengths && out_f64, "power: null pointer");
  CHECK_ARG(((uintptr_t)pool & 3) == 0 && ((uintptr_t)offsets & 7) == 0 && ((uintptr_t)lengths & 7) == 0 &&
                ((uintptr_t)out_f64 & 7) == 0 && ((uintptr_t)ws & 7) == 0,
            "power: misaligned pointer (pool 4-byte; offsets, lengths, out, ws 8-byte)");
  const Slicing g = slicing_of(max_len);
  CHECK_ARG((int64_t)n_utt * g.n_slices < ((int64_t)1 << 31), "power: n_utt * slices per row must be < 2^31");
  const size_t need = danet_mix_workspace_bytes(n_utt, max_len);
  CHECK_ARG(need == 0 || ws != nullptr, "power: null pointer (ws, %zu bytes needed)", need);
  CHECK_ARG(ws_bytes >= need, "power: workspace too small (%zu < %zu)", ws_bytes, need);
  PowerArgs a;
  a.pool = pool; a.pool_len = pool_len; a.offsets = offsets; a.lengths = lengths; a.max_len = max_len;
  a.slice = g.slice; a.n_slices = g.n_slices; a.out = out_f64; a.ws = (double*)ws;
  mix_power_kernel<<<dim3((unsigned)((int64_t)n_utt * g.n_slices)), kThreads, 0, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  if (g.n_slices > 1) {
    mix_power_rows_kernel<<<dim3((unsigned)((n_utt + kThreads - 1) / kThreads)), kThreads, 0,
                            (hipStream_t)stream>>>(a, n_utt);
    CHECK_LAUNCH();
  }
  return DANET_MIX_OK;
}

/* ---------------------------------------------------------------------------------- scale */
static const int kPiece = 4096;      /* complex elements per workgroup (even: a piece keeps its span's parity) */

struct ScaleArgs {
  float2* buf;
  const float* gains;
  int64_t ld;
  int64_t span;        /* dense: t_count * F */
  int t_count, F;
  int n_chunks;        /* workgroups per utterance */
  int rows;            /* pitched: rows per workgroup */
  int dense;
};

/* p[0..n) *= g, p 8-byte aligned: 16-byte accesses over the 16-byte aligned middle */
__device__ __forceinline__ void scale_span(float2* __restrict__ p, int n, float g) {
  const int head = (int)(((uintptr_t)p >> 3) & 1);
  const int npair = (n - head) >> 1;
  f32x4* pv = reinterpret_cast<f32x4*>(p + head);
  for (int k = threadIdx.x; k < npair; k += kThreads) {
    f32x4 v = pv[k];
    v[0] *= g; v[1] *= g; v[2] *= g; v[3] *= g;
    pv[k] = v;
  }
  if (threadIdx.x == kThreads - 1) {
    if (head) { float2 v = p[0]; v.x *= g; v.y *= g; p[0] = v; }
    if ((n - head) & 1) { float2 v = p[n - 1]; v.x *= g; v.y *= g; p[n - 1] = v; }
  }
}

__global__ __launch_bounds__(kThreads) void mix_scale_kernel(ScaleArgs a) {
  const int u = (int)(blockIdx.x / (unsigned)a.n_chunks);
  const int c = (int)(blockIdx.x - (unsigned)u * (unsigned)a.n_chunks);
  const float g = a.gains[u];
  if (a.dense) {
    const int64_t b = (int64_t)c * kPiece;
    scale_span(a.buf + (int64_t)u * a.span + b, (int)min((int64_t)kPiece, a.span - b), g);
  } else {
    const int r1 = min(a.t_count, (c + 1) * a.rows);
    for (int r = c * a.rows; r < r1; ++r) scale_span(a.buf + ((int64_t)u * a.t_count + r) * a.ld, a.F, g);
  }
}

extern "C" int danet_mix_scale_c64(void* stream, int n_utt, int t_count, int F, float* buf_c64, int64_t ld,
                                   const float* gains) {
  CHECK_ARG(n_utt >= 1 && t_count >= 1 && F >= 1, "scale_c64: n_utt, t_count and F must be >= 1 (got %d, %d, %d)",
            n_utt, t_count, F);
  CHECK_ARG(buf_c64 && gains, "scale_c64: null pointer");
  CHECK_ARG(ld >= F, "scale_c64: ld must be >= F (%lld < %d)", (long long)ld, F);
  CHECK_ARG(ld < ((int64_t)1 << 40), "scale_c64: ld too large");
  CHECK_ARG(((uintptr_t)buf_c64 & 7) == 0 && ((uintptr_t)gains & 3) == 0,
            "scale_c64: misaligned pointer (buf 8-byte, gains 4-byte)");
  ScaleArgs a;
  a.buf = (float2*)buf_c64; a.gains = gains; a.ld = ld; a.t_count = t_count; a.F = F;
  a.dense = (ld == F) ? 1 : 0;
  a.span = (int64_t)t_count * F;
  a.rows = F >= kPiece ? 1 : kPiece / F;
  const int64_t n_chunks = a.dense ? (a.span + kPiece - 1) / kPiece : ((int64_t)t_count + a.rows - 1) / a.rows;
  CHECK_ARG(n_chunks * n_utt < ((int64_t)1 << 31), "scale_c64: n_utt * workgroups per utterance must be < 2^31");
  a.n_chunks = (int)n_chunks;
  mix_scale_kernel<<<dim3((unsigned)(n_chunks * n_utt)), kThreads, 0, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_MIX_OK;
}
