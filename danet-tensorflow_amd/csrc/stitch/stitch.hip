/*
 * libdanet_stitch_hip.so (include/danet_stitch_hip.h): speaker-continuity stitching of chunked inference.  gfx950,
 * wave64.
 *
 * danet_stitch_affinity.  One workgroup per (tile, pair): both factors of an overlap are contiguous runs, so a thread
 * loads four consecutive floats of each of the 2C runs and adds the C x C products in float64; the workgroup sum is a
 * fixed butterfly over the wave and (w0 + w1) + (w2 + w3) over the four waves.
 *
 * danet_stitch_assign.  One workgroup: a thread per pair adds the tiles in order, searches the permutations and
 * leaves its local permutation in the pair's row of perm_out; one thread then composes the chain in place.
 *
 * danet_stitch_merge.  Gather: two consecutive flat (t, f) elements of one channel per thread.
 *
 * The extension libraries share csrc/ext_core.h and nothing with the core library.
 */
#include <hip/hip_runtime.h>

#include "danet_stitch_hip.h"
#define DANET_EXT stitch
#define DANET_EXT_UPPER STITCH
#include "ext_core.h"

static const int kThreads = 256;
static const int kTile = DANET_STITCH_TILE;
static const int kMaxC = DANET_STITCH_MAX_C;

/* n of THE RULE for a plan inside the envelope of danet_stitch_chunks (T > L) */
static int64_t chunks_of(int64_t T, int64_t L, int64_t V) {
  const int64_t H = L - V;
  return 1 + (T - L + H - 1) / H;
}

static bool plan_ok(const char* who, int T, int L, int V) {
  if (T < 1 || L < 2 || V < 1 || V > L / 2) {
    set_error("%s: need T >= 1, L >= 2 and 1 <= V <= L / 2 (got T=%d L=%d V=%d)", who, T, L, V);
    return false;
  }
  return true;
}

static bool envelope_ok(const char* who, int T, int L, int V, int C, int F) {
  if (!plan_ok(who, T, L, V)) return false;
  if (T <= L) {
    set_error("%s: need T > L, one chunk is not stitched (got T=%d L=%d)", who, T, L);
    return false;
  }
  if (C < 1 || C > kMaxC || F < 1) {
    set_error("%s: need 1 <= C <= %d and F >= 1 (got C=%d F=%d)", who, kMaxC, C, F);
    return false;
  }
  if (chunks_of(T, L, V) > DANET_STITCH_MAX_CHUNKS) {
    set_error("%s: need at most %d chunks (got %lld at T=%d L=%d V=%d)", who, DANET_STITCH_MAX_CHUNKS,
              (long long)chunks_of(T, L, V), T, L, V);
    return false;
  }
  if ((int64_t)L * F >= ((int64_t)1 << 31) || (int64_t)T * F >= ((int64_t)1 << 40)) {
    set_error("%s: need L * F < 2^31 and T * F < 2^40 (got T=%d L=%d F=%d)", who, T, L, F);
    return false;
  }
  return true;
}

static int tiles_of(int L, int F) { return (int)(((int64_t)L * F + kTile - 1) / kTile); }

static size_t ws_bytes_of(int T, int L, int V, int C, int F) {
  return (size_t)(chunks_of(T, L, V) - 1) * (size_t)tiles_of(L, F) * (size_t)(C * C) * sizeof(double);
}

static bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int danet_stitch_chunks(int T, int L, int V) {
  if (!plan_ok("chunks", T, L, V)) return -1;
  if (T <= L) return 1;
  const int64_t n = chunks_of(T, L, V);
  if (n > 0x7fffffff) {
    set_error("chunks: the count does not fit an int (T=%d L=%d V=%d)", T, L, V);
    return -1;
  }
  return (int)n;
}

extern "C" size_t danet_stitch_workspace_bytes(int T, int L, int V, int C, int F) {
  if (!envelope_ok("workspace_bytes", T, L, V, C, F)) return (size_t)-1;
  return ws_bytes_of(T, L, V, C, F);
}

/* start of chunk i of a plan of n chunks */
__device__ __forceinline__ int chunk_start(int i, int n, int T, int L, int H) { return i < n - 1 ? i * H : T - L; }

/* --------------------------------------------------------------------------------------- affinity */
template <int C>
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t stride, bool vec, float (&x)[C][4]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* q = p + c * stride;
    if (vec) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(q);
      x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
    } else {
      x[c][0] = q[0]; x[c][1] = q[1]; x[c][2] = q[2]; x[c][3] = q[3];
    }
  }
}

template <int C>
__global__ __launch_bounds__(kThreads) void stitch_affinity_kernel(int T, int L, int V, int F, int n, int base16,
                                                                   const float* __restrict__ mags,
                                                                   double* __restrict__ part) {
  __shared__ double red[4][kMaxC * kMaxC];
  const int tid = threadIdx.x;
  const int pair = blockIdx.y, tile = blockIdx.x, nt = gridDim.x;
  const int H = L - V;
  const int hop = chunk_start(pair + 1, n, T, L, H) - chunk_start(pair, n, T, L, H);
  const int64_t LF = (int64_t)L * F;
  const int64_t run = (int64_t)(L - hop) * F;                 /* |O_i| * F floats, < LF */
  const float* a0 = mags + (int64_t)pair * C * LF + (int64_t)hop * F;       /* m_i[0]: rows hop .. L - 1 */
  const float* b0 = mags + (int64_t)(pair + 1) * C * LF;                    /* m_{i+1}[0]: rows 0 .. */
  const bool vec_b = base16 && (LF & 3) == 0;
  const bool vec_a = vec_b && (((int64_t)hop * F) & 3) == 0;
  const int64_t k0 = (int64_t)tile * kTile;
  const int64_t k1 = min(run, k0 + kTile);

  double acc[C][C];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int d = 0; d < C; ++d) acc[c][d] = 0.0;

  for (int64_t k = k0 + 4 * tid; k < k1; k += 4 * kThreads) {
    if (k + 4 <= k1) {
      float a[C][4], b[C][4];
      load4<C>(a0 + k, LF, vec_a, a);
      load4<C>(b0 + k, LF, vec_b, b);
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int d = 0; d < C; ++d)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[c][d] += (double)a[c][j] * (double)b[d][j];
    } else {
      for (int64_t kk = k; kk < k1; ++kk)
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int d = 0; d < C; ++d) acc[c][d] += (double)a0[c * LF + kk] * (double)b0[d * LF + kk];
    }
  }

  /* the wave: a fixed butterfly; the four waves: (w0 + w1) + (w2 + w3) */
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int d = 0; d < C; ++d) {
      double v = acc[c][d];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
      if ((tid & 63) == 0) red[tid >> 6][c * C + d] = v;
    }
  __syncthreads();
  if (tid < C * C)
    part[((int64_t)pair * nt + tile) * (C * C) + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

extern "C" int danet_stitch_affinity(void* stream, int T, int L, int V, int C, int F, const float* mags, void* ws,
                                     size_t ws_bytes) {
  if (!envelope_ok("affinity", T, L, V, C, F)) return DANET_STITCH_ERR_ARG;
  CHECK_ARG(mags && ws, "affinity: null pointer");
  CHECK_ARG(aligned(mags, 4) && aligned(ws, 8), "affinity: misaligned pointer (mags 4, ws 8 bytes)");
  CHECK_ARG(ws_bytes >= ws_bytes_of(T, L, V, C, F), "affinity: workspace too small (%zu bytes, need %zu)", ws_bytes,
            ws_bytes_of(T, L, V, C, F));
  const int n = (int)chunks_of(T, L, V);
  const dim3 grid(tiles_of(L, F), n - 1);
  const int base16 = aligned(mags, 16) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  switch (C) {
    case 1: stitch_affinity_kernel<1><<<grid, kThreads, 0, st>>>(T, L, V, F, n, base16, mags, part); break;
    case 2: stitch_affinity_kernel<2><<<grid, kThreads, 0, st>>>(T, L, V, F, n, base16, mags, part); break;
    case 3: stitch_affinity_kernel<3><<<grid, kThreads, 0, st>>>(T, L, V, F, n, base16, mags, part); break;
    default: stitch_affinity_kernel<4><<<grid, kThreads, 0, st>>>(T, L, V, F, n, base16, mags, part); break;
  }
  CHECK_LAUNCH();
  return DANET_STITCH_OK;
}

/* ----------------------------------------------------------------------------------------- assign */
/* permutation `idx` of range(C) in itertools.permutations (lexicographic) order, channel c in bits 2c, 2c + 1 */
__device__ __forceinline__ int packed_permutation(int C, int idx) {
  int avail = 0xe4;                        /* the digits 0, 1, 2, 3 not yet taken, lowest first, two bits each */
  int fact = C == 4 ? 6 : C == 3 ? 2 : 1;  /* (C - 1)! */
  int packed = 0;
  for (int pos = 0; pos < C; ++pos) {
    const int d = idx / fact;
    idx -= d * fact;
    packed |= ((avail >> (2 * d)) & 3) << (2 * pos);
    const int low = avail & ((1 << (2 * d)) - 1);
    avail = low | ((avail >> (2 * d + 2)) << (2 * d));      /* drop digit d */
    if (C - 1 - pos > 1) fact /= (C - 1 - pos);
  }
  return packed;
}

__device__ __forceinline__ int pack4(const int32_t* __restrict__ row, int C) {
  int packed = 0;
  for (int c = 0; c < C; ++c) packed |= (row[c] & 3) << (2 * c);
  return packed;
}

__global__ __launch_bounds__(kThreads) void stitch_assign_kernel(int n, int C, int nt, const double* __restrict__ part,
                                                                 double* __restrict__ S_out, int32_t* perm_out) {
  const int tid = threadIdx.x;
  const int CC = C * C;
  const int nperm = C == 4 ? 24 : C == 3 ? 6 : C;
  for (int pair = tid; pair < n - 1; pair += kThreads) {
    double S[kMaxC * kMaxC];
#pragma unroll
    for (int e = 0; e < kMaxC * kMaxC; ++e) {
      double s = 0.0;
      if (e < CC) {
        for (int tile = 0; tile < nt; ++tile) s += part[((int64_t)pair * nt + tile) * CC + e];
        S_out[(int64_t)pair * CC + e] = s;
      }
      S[e] = s;
    }
    int best = 0xe4;                       /* the identity: permutation 0 */
    double best_total = 0.0;
    for (int p = 0; p < nperm; ++p) {
      const int packed = packed_permutation(C, p);
      double total = 0.0;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < C) {
          const int e = c * C + ((packed >> (2 * c)) & 3);
          double v = 0.0;
#pragma unroll
          for (int q = 0; q < kMaxC * kMaxC; ++q) v = (q == e) ? S[q] : v;       /* S stays in registers */
          total += v;
        }
      }
      if (p == 0 || total > best_total) {  /* strictly greater: the first permutation wins a tie */
        best = packed;
        best_total = total;
      }
    }
    for (int c = 0; c < C; ++c) perm_out[(int64_t)(pair + 1) * C + c] = (best >> (2 * c)) & 3;      /* pi_i, for now */
  }
  __syncthreads();
  if (tid == 0) {
    int P = 0xe4;
    for (int c = 0; c < C; ++c) perm_out[c] = c;
    for (int i0 = 0; i0 < n - 1; i0 += 8) {
      int pi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pi[j] = i0 + j < n - 1 ? pack4(perm_out + (int64_t)(i0 + j + 1) * C, C) : 0xe4;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (i0 + j < n - 1) {
          int next = 0;
          for (int c = 0; c < C; ++c) next |= ((pi[j] >> (2 * ((P >> (2 * c)) & 3))) & 3) << (2 * c);
          P = next;
          for (int c = 0; c < C; ++c) perm_out[(int64_t)(i0 + j + 1) * C + c] = (P >> (2 * c)) & 3;
        }
      }
    }
  }
}

extern "C" int danet_stitch_assign(void* stream, int T, int L, int V, int C, int F, const void* ws, size_t ws_bytes,
                                   double* S_out, int32_t* perm_out) {
  if (!envelope_ok("assign", T, L, V, C, F)) return DANET_STITCH_ERR_ARG;
  CHECK_ARG(ws && S_out && perm_out, "assign: null pointer");
  CHECK_ARG(aligned(ws, 8) && aligned(S_out, 8) && aligned(perm_out, 4),
            "assign: misaligned pointer (ws, S_out 8, perm_out 4 bytes)");
  CHECK_ARG(ws_bytes >= ws_bytes_of(T, L, V, C, F), "assign: workspace too small (%zu bytes, need %zu)", ws_bytes,
            ws_bytes_of(T, L, V, C, F));
  const int n = (int)chunks_of(T, L, V);
  stitch_assign_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(n, C, tiles_of(L, F), (const double*)ws, S_out,
                                                                perm_out);
  CHECK_LAUNCH();
  return DANET_STITCH_OK;
}

/* ------------------------------------------------------------------------------------------ merge */
struct MergeArgs {
  int T, L, V, C, F, n;
  const float* mags;
  const float2* phasor;
  const float* fade;
  const int32_t* perm;
};

__device__ __forceinline__ int clamped(const int32_t* __restrict__ perm, int i, int C, int c) {
  return min(max(perm[(int64_t)i * C + c], 0), C - 1);
}

/* out[c][t][f] of THE RULE for the flat index j = t * F + f */
__device__ __forceinline__ float2 merged(const MergeArgs& g, int c, int64_t j) {
  const int t = (int)(j / g.F);
  const int f = (int)(j - (int64_t)t * g.F);
  const int H = g.L - g.V;
  int i = t < g.L ? 0 : (t - g.L) / H + 1;                   /* the smallest i with t < e_i ... */
  i = min(i, g.n - 1);                                       /* ... the last chunk ends at T */
  const int s = chunk_start(i, g.n, g.T, g.L, H);
  const int64_t LF = (int64_t)g.L * g.F;
  const int64_t row = (int64_t)(t - s) * g.F + f;            /* 0 <= t - s < L */
  float mag = g.mags[((int64_t)i * g.C + clamped(g.perm, i, g.C, c)) * LF + row];
  const int k = t - (s + g.L - g.V);
  if (i < g.n - 1 && k >= 0) {
    const int s2 = chunk_start(i + 1, g.n, g.T, g.L, H);     /* s2 <= e_i - V <= t < e_i <= e_{i+1} */
    const float b = g.mags[((int64_t)(i + 1) * g.C + clamped(g.perm, i + 1, g.C, c)) * LF + (int64_t)(t - s2) * g.F + f];
    mag = __fmaf_rn(g.fade[k], b - mag, mag);
  }
  const float2 ph = g.phasor[(int64_t)i * LF + row];
  return make_float2(mag * ph.x, mag * ph.y);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void stitch_merge_kernel(MergeArgs g, float2* __restrict__ out) {
  const int c = blockIdx.y;
  const int64_t TF = (int64_t)g.T * g.F;
  const int64_t j = 2 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
  if (j >= TF) return;
  float2* o = out + (int64_t)c * TF + j;
  const float2 x = merged(g, c, j);
  if (j + 1 < TF) {
    const float2 y = merged(g, c, j + 1);
    if (VEC) {                                               /* c * TF + j is even on this path */
      *reinterpret_cast<f32x4*>(o) = (f32x4){x.x, x.y, y.x, y.y};
    } else {
      o[0] = x;
      o[1] = y;
    }
  } else {
    o[0] = x;
  }
}

extern "C" int danet_stitch_merge(void* stream, int T, int L, int V, int C, int F, const float* mags,
                                  const float* phasor, const float* fade, const int32_t* perm, float* out) {
  if (!envelope_ok("merge", T, L, V, C, F)) return DANET_STITCH_ERR_ARG;
  CHECK_ARG(mags && phasor && fade && perm && out, "merge: null pointer");
  CHECK_ARG(aligned(mags, 4) && aligned(fade, 4) && aligned(perm, 4) && aligned(phasor, 8) && aligned(out, 8),
            "merge: misaligned pointer (mags, fade, perm 4, phasor, out 8 bytes)");
  MergeArgs g;
  g.T = T; g.L = L; g.V = V; g.C = C; g.F = F;
  g.n = (int)chunks_of(T, L, V);
  g.mags = mags;
  g.phasor = (const float2*)phasor;
  g.fade = fade;
  g.perm = perm;
  const int64_t TF = (int64_t)T * F;
  const dim3 grid((unsigned)((TF + 2 * kThreads - 1) / (2 * kThreads)), C);
  /* a channel starts at c * TF complex values: every pair of a thread is 16-byte aligned when out is and TF is even
   * (or there is one channel) */
  const bool vec = aligned(out, 16) && (C == 1 || (TF & 1) == 0);
  if (vec)
    stitch_merge_kernel<true><<<grid, kThreads, 0, (hipStream_t)stream>>>(g, (float2*)out);
  else
    stitch_merge_kernel<false><<<grid, kThreads, 0, (hipStream_t)stream>>>(g, (float2*)out);
  CHECK_LAUNCH();
  return DANET_STITCH_OK;
}
