/*
 * libdanet_dpcl_hip.so (include/danet_dpcl_hip.h): the deep-clustering affinity loss from weighted Gram matrices and
 * its gradient.  gfx950, wave64.
 *
 * danet_dpcl_stats.  One workgroup per (chunk, utterance).  A tile of 128 rows is staged in LDS as
 * [v | 1 | onehot(y) | 0..] with the row's weight s beside it; the chunk's G = P^T Q (P = s * [v | 1], Q the staged
 * row) is held in registers as 4 x 4 output tiles, one or two per thread, and with fewer tiles than threads the rows
 * of a staged tile are dealt to floor(256 / tiles) thread groups whose sums meet in LDS in group order.
 *
 * danet_dpcl_finalize.  One workgroup: chunk sums in float64, the division by sum s, L_b, the tables of the
 * backward pass, the mean and the sum with the main loss.
 *
 * danet_dpcl_bwd.  The head kernels' shape: one row per thread in registers, A and Bm in LDS read as broadcasts.
 *
 * The extension libraries share csrc/ext_core.h and nothing with the core library: the XCD-aware (utterance, chunk)
 * mapping of csrc/attractor.hip is restated here.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "danet_dpcl_hip.h"
#define DANET_EXT dpcl
#define DANET_EXT_UPPER DPCL
#include "ext_core.h"

static const int kThreads = 256;
static const int kTile = DANET_DPCL_TILE_ROWS;
static const int kMaxFAp = 4 * ((DANET_DPCL_MAX_E + DANET_DPCL_MAX_C + 1 + 3) / 4);   /* 72 */
static const int kBwdRows = 1024;
static const int kFinThreads = 1024;

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

/* chunk_rows(N) of THE RULE */
static int64_t chunk_rows_of(int64_t N) { return kTile * cdiv64(cdiv64(N, DANET_DPCL_MAX_CHUNKS), kTile); }

static bool envelope_ok(const char* who, int B, int64_t N, int E, int C) {
  if (B < 1 || B > DANET_DPCL_MAX_B || N < 1 || N > DANET_DPCL_MAX_N || E < 1 || E > DANET_DPCL_MAX_E || C < 1 ||
      C > DANET_DPCL_MAX_C) {
    set_error("%s: need 1 <= B <= %d, 1 <= N <= 2^31, 1 <= E <= %d, 1 <= C <= %d (got B=%d N=%lld E=%d C=%d)", who,
              DANET_DPCL_MAX_B, DANET_DPCL_MAX_E, DANET_DPCL_MAX_C, B, (long long)N, E, C);
    return false;
  }
  return true;
}

extern "C" int danet_dpcl_chunks(int64_t N) {
  if (N < 1 || N > DANET_DPCL_MAX_N) {
    set_error("chunks: N must be in [1, 2^31] (got %lld)", (long long)N);
    return 0;
  }
  return (int)cdiv64(N, chunk_rows_of(N));
}

extern "C" size_t danet_dpcl_workspace_bytes(int B, int64_t N, int E, int C) {
  if (!envelope_ok("workspace_bytes", B, N, E, C)) return (size_t)-1;
  return (size_t)B * (size_t)cdiv64(N, chunk_rows_of(N)) * (size_t)((E + 1) * (E + C + 1)) * sizeof(float);
}

/* (utterance, chunk) of this workgroup of a (nch, B) grid, XCD-aware: workgroups are dealt to the 8 XCDs round-robin
 * by linear id and the output projection writes utterance b's embedding from XCD b / (B / 8), so utterance b's
 * workgroups run on THAT XCD and find part of the embedding in its L2.  B not a multiple of 8: the plain mapping. */
__device__ __forceinline__ void utterance_chunk(int& b, int64_t& ch) {
  const int64_t nch = gridDim.x;
  const int B = gridDim.y;
  b = blockIdx.y;
  ch = blockIdx.x;
  if ((B & 7) == 0) {
    const int64_t i = blockIdx.x + nch * blockIdx.y, j = i >> 3;
    const int per = B >> 3, x = (int)(i & 7);
    b = x * per + (int)(j % per);
    ch = j / per;
  }
}

/* label and weight of row n of an utterance (sp: its src_pwr [C][N]) */
__device__ __forceinline__ void label_weight(const float* __restrict__ sp, int C, int64_t N, int64_t n, int& y,
                                             float& s) {
  float bv = sp[n];
  y = 0;
  s = bv;
  for (int c = 1; c < C; ++c) {
    const float v = sp[(int64_t)c * N + n];
    if (v > bv) { bv = v; y = c; }       /* strictly greater: a tie stays with the lowest index */
    s += v;
  }
}

/* ------------------------------------------------------------------------------------------ stats */
template <bool VEC>
__global__ __launch_bounds__(kThreads) void dpcl_stats_kernel(int64_t N, int E, int C, int64_t chunk_rows,
                                                              const float* __restrict__ embed,
                                                              const float* __restrict__ src_pwr,
                                                              float* __restrict__ partial) {
  __shared__ double Lbuf[kTile * kMaxFAp / 2];          /* the staged tile (float), later the group sums (double) */
  __shared__ float sS[kTile];
  float* L = reinterpret_cast<float*>(Lbuf);
  const int tid = threadIdx.x;
  int b;
  int64_t ch;
  utterance_chunk(b, ch);
  const int EA = E + 1, FA = E + C + 1;
  const int nte = (EA + 3) >> 2, ntf = (FA + 3) >> 2, FAp = 4 * ntf;
  const int ntiles = nte * ntf;
  const int nslots = ntiles > kThreads ? 2 : 1;
  const int groups = nslots == 2 ? 1 : kThreads / ntiles;
  /* slot k of this thread: output tile (te[k], tf[k]); row group g */
  const int g = nslots == 2 ? 0 : tid / ntiles;
  int te[2], tf[2];
  bool on[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int t = nslots == 2 ? tid + k * kThreads : tid % ntiles;
    on[k] = (k < nslots) && (t < ntiles) && (g < groups);
    te[k] = on[k] ? t / ntf : 0;
    tf[k] = on[k] ? t % ntf : 0;
  }

  const float* eb = embed + (int64_t)b * N * E;
  const float* sp = src_pwr + (int64_t)b * C * N;
  const int64_t n_begin = ch * chunk_rows, n_end = min(N, n_begin + chunk_rows);

  double acc64[2][16];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc64[k][q] = 0.0;

  for (int64_t n0 = n_begin; n0 < n_end; n0 += kTile) {
    const int rows = (int)min((int64_t)kTile, n_end - n0);
    const int nelem = rows * E;
    /* stage: the embedding rows (zeros behind the last row) ... */
    const float* src = eb + n0 * E;
    if (VEC) {
      const f32x4* src4 = reinterpret_cast<const f32x4*>(src);
      for (int q = tid; q < kTile * E / 4; q += kThreads) {
        const int i = 4 * q;
        f32x4 x = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (i < nelem) x = src4[q];                       /* nelem is a multiple of 4 on this path */
        int r = i / E, e = i - r * E;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          L[r * FAp + e] = x[k];
          if (++e == E) { e = 0; ++r; }
        }
      }
    } else {
      for (int i = tid; i < kTile * E; i += kThreads) {
        const int r = i / E, e = i - r * E;
        L[r * FAp + e] = i < nelem ? src[i] : 0.f;
      }
    }
    /* ... and per row the weight, the 1, the one-hot label and the zero padding */
    if (tid < kTile) {
      int y = -1;
      float s = 0.f;
      if (tid < rows) label_weight(sp, C, N, n0 + tid, y, s);
      sS[tid] = s;
      float* row = L + tid * FAp;
      row[E] = tid < rows ? 1.f : 0.f;
      for (int f = E + 1; f < FAp; ++f) row[f] = (f - E - 1 == y) ? 1.f : 0.f;
    }
    __syncthreads();
    /* the tile's products, float32, rows g, g + groups, ... in order */
    float acc[2][16];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[k][q] = 0.f;
    if (on[0]) {
      for (int r = g; r < kTile; r += groups) {
        const float s = sS[r];
        const float* row = L + r * FAp;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (k == 0 || on[1]) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(row + 4 * te[k]) * s;
            const f32x4 q = *reinterpret_cast<const f32x4*>(row + 4 * tf[k]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[k][4 * i + j] = __builtin_fmaf(p[i], q[j], acc[k][4 * i + j]);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc64[k][q] += (double)acc[k][q];
    __syncthreads();
  }

  float* out = partial + ((int64_t)b * gridDim.x + ch) * (EA * FA);
  if (groups > 1) {
    double* red = Lbuf;                                   /* groups * ntiles * 16 <= 4096 doubles */
    if (on[0]) {
#pragma unroll
      for (int q = 0; q < 16; ++q) red[(g * ntiles + te[0] * ntf + tf[0]) * 16 + q] = acc64[0][q];
    }
    __syncthreads();
    for (int o = tid; o < EA * FA; o += kThreads) {
      const int ea = o / FA, fa = o - ea * FA;
      const int slot = (((ea >> 2) * ntf + (fa >> 2)) << 4) + ((ea & 3) << 2) + (fa & 3);
      double sum = 0.0;
      for (int gg = 0; gg < groups; ++gg) sum += red[gg * ntiles * 16 + slot];
      out[o] = (float)sum;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!on[k]) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ea = 4 * te[k] + i, fa = 4 * tf[k] + j;
          if (ea < EA && fa < FA) out[ea * FA + fa] = (float)acc64[k][4 * i + j];
        }
    }
  }
}

extern "C" int danet_dpcl_stats(void* stream, int B, int64_t N, int E, int C, const float* embed, const float* src_pwr,
                                void* workspace, size_t workspace_bytes) {
  if (!envelope_ok("stats", B, N, E, C)) return DANET_DPCL_ERR_ARG;
  CHECK_ARG(embed && src_pwr && workspace, "stats: null pointer");
  CHECK_ARG((((uintptr_t)embed | (uintptr_t)src_pwr | (uintptr_t)workspace) & 3) == 0,
            "stats: misaligned pointer (embed, src_pwr, workspace 4-byte)");
  const size_t need = danet_dpcl_workspace_bytes(B, N, E, C);
  CHECK_ARG(workspace_bytes >= need, "stats: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
  const int64_t rows = chunk_rows_of(N);
  const dim3 grid((unsigned)cdiv64(N, rows), (unsigned)B);
  const bool vec = ((uintptr_t)embed & 15) == 0 && ((N * E) & 3) == 0;
  if (vec)
    dpcl_stats_kernel<true><<<grid, kThreads, 0, (hipStream_t)stream>>>(N, E, C, rows, embed, src_pwr,
                                                                        (float*)workspace);
  else
    dpcl_stats_kernel<false><<<grid, kThreads, 0, (hipStream_t)stream>>>(N, E, C, rows, embed, src_pwr,
                                                                         (float*)workspace);
  CHECK_LAUNCH();
  return DANET_DPCL_OK;
}

/* ------------------------------------------------------------------------------------------ finalize */
/* the sum of one entry of G over the chunks, float64 in chunk order; the (at most 16) loads are independent */
__device__ __forceinline__ double chunk_sum(const float* __restrict__ p, int nch, int64_t stride) {
  float x[DANET_DPCL_MAX_CHUNKS];
#pragma unroll
  for (int ch = 0; ch < DANET_DPCL_MAX_CHUNKS; ++ch) x[ch] = ch < nch ? p[ch * stride] : 0.f;
  double s = 0.0;
#pragma unroll
  for (int ch = 0; ch < DANET_DPCL_MAX_CHUNKS; ++ch) s += (double)x[ch];       /* (+ 0 for an absent chunk: exact) */
  return s;
}

/* One wave per utterance: wave w of the 16 takes the utterances w, w + 16, ... in turn, its 64 lanes the entries of
 * G; no barrier inside the loop.  L_b: a butterfly over the wave; the mean: every wave adds its own L_b in order,
 * thread 0 the 16 wave sums in order. */
__global__ __launch_bounds__(kFinThreads) void dpcl_finalize_kernel(int B, int nch, int E, int C,
                                                                    const float* __restrict__ partial,
                                                                    const float* __restrict__ main_loss, float alpha,
                                                                    double* __restrict__ per_utt,
                                                                    float* __restrict__ dpcl_out,
                                                                    float* __restrict__ total_out,
                                                                    float* __restrict__ tables,
                                                                    float* __restrict__ cs) {
  __shared__ double red[kFinThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int EA = E + 1, FA = E + C + 1, EF = EA * FA, TW = E + C;
  double sumL = 0.0;
  for (int b = wave; b < B; b += kFinThreads / 64) {
    const float* pb = partial + (int64_t)b * nch * EF;
    const double S = chunk_sum(pb + E * FA + E, nch, EF);
    const bool live = S > 0.0;
    double local = 0.0;
    for (int o = lane; o < EF; o += 64) {
      const int ea = o / FA, fa = o - ea * FA;
      const double gsum = chunk_sum(pb + o, nch, EF);
      const double a = live ? gsum / S : 0.0;
      if (ea < E) {
        if (fa < E) {
          tables[((int64_t)b * E + ea) * TW + fa] = (float)a;
          local += a * a;
        } else if (fa > E) {
          tables[((int64_t)b * E + ea) * TW + fa - 1] = (float)a;
          local -= 2.0 * a * a;
        }
      } else if (fa > E) {
        cs[b * (C + 1) + fa - E - 1] = (float)a;
        local += a * a;
      } else if (fa == E) {
        cs[b * (C + 1) + C] = (float)S;
      }
    }
    for (int m = 32; m > 0; m >>= 1) local += __shfl_xor(local, m, 64);
    if (lane == 0) per_utt[b] = local;
    sumL += local;
  }
  if (lane == 0) red[wave] = sumL;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kFinThreads / 64; ++w) t += red[w];
    const double d = t / (double)B;
    dpcl_out[0] = (float)d;
    total_out[0] = (float)((main_loss ? (double)main_loss[0] : 0.0) + (double)alpha * d);
  }
}

extern "C" int danet_dpcl_finalize(void* stream, int B, int64_t N, int E, int C, const void* workspace,
                                   size_t workspace_bytes, const float* main_f32, float alpha, double* per_utt_f64,
                                   float* dpcl_f32, float* total_f32, float* tables_f32, float* cs_f32) {
  if (!envelope_ok("finalize", B, N, E, C)) return DANET_DPCL_ERR_ARG;
  CHECK_ARG(workspace && per_utt_f64 && dpcl_f32 && total_f32 && tables_f32 && cs_f32, "finalize: null pointer");
  CHECK_ARG((((uintptr_t)workspace | (uintptr_t)main_f32 | (uintptr_t)dpcl_f32 | (uintptr_t)total_f32 |
              (uintptr_t)tables_f32 | (uintptr_t)cs_f32) & 3) == 0 && ((uintptr_t)per_utt_f64 & 7) == 0,
            "finalize: misaligned pointer (per_utt 8-byte, the rest 4-byte)");
  CHECK_ARG(isfinite(alpha) && alpha >= 0.f, "finalize: alpha must be finite and >= 0 (got %g)", (double)alpha);
  const size_t need = danet_dpcl_workspace_bytes(B, N, E, C);
  CHECK_ARG(workspace_bytes >= need, "finalize: workspace too small (%zu bytes, need %zu)", workspace_bytes,
            need);
  const int nch = (int)cdiv64(N, chunk_rows_of(N));
  dpcl_finalize_kernel<<<1, kFinThreads, 0, (hipStream_t)stream>>>(B, nch, E, C, (const float*)workspace, main_f32,
                                                                   alpha, per_utt_f64, dpcl_f32, total_f32, tables_f32,
                                                                   cs_f32);
  CHECK_LAUNCH();
  return DANET_DPCL_OK;
}

/* ------------------------------------------------------------------------------------------ backward */
/* EP: E rounded up to an instantiated size (a multiple of 4); VEC: E == EP and 16-byte rows */
template <int EP, bool VEC>
__global__ __launch_bounds__(kThreads) void dpcl_bwd_kernel(int64_t N, int E, int C, const float* __restrict__ embed,
                                                            const float* __restrict__ src_pwr,
                                                            const float* __restrict__ tables,
                                                            const float* __restrict__ cs,
                                                            const float* __restrict__ dloss, float scale,
                                                            float* __restrict__ dembed) {
  __shared__ __attribute__((aligned(16))) float sA[EP * EP];
  __shared__ float sB[EP * DANET_DPCL_MAX_C];
  const int tid = threadIdx.x;
  int b;
  int64_t ch;
  utterance_chunk(b, ch);
  const int TW = E + C;
  const float* tb = tables + (int64_t)b * E * TW;
  for (int i = tid; i < EP * EP; i += kThreads) {
    const int e = i / EP, f = i - e * EP;
    sA[i] = (e < E && f < E) ? tb[e * TW + f] : 0.f;
  }
  for (int i = tid; i < EP * DANET_DPCL_MAX_C; i += kThreads) {
    const int e = i / DANET_DPCL_MAX_C, k = i - e * DANET_DPCL_MAX_C;
    sB[i] = (e < E && k < C) ? tb[e * TW + E + k] : 0.f;
  }
  __syncthreads();
  const float S = cs[b * (C + 1) + C];
  const float invS = S > 0.f ? 1.f / S : 0.f;
  const float k4 = (dloss ? dloss[0] : 1.f) * scale * 4.f;
  const float* eb = embed + (int64_t)b * N * E;
  const float* sp = src_pwr + (int64_t)b * C * N;
  float* db = dembed + (int64_t)b * N * E;
  const int64_t n_begin = ch * kBwdRows;
  for (int it = 0; it < kBwdRows / kThreads; ++it) {
    const int64_t n = n_begin + it * kThreads + tid;
    if (n >= N) break;
    int y;
    float s;
    label_weight(sp, C, N, n, y, s);
    const float coef = k4 * (s * invS);
    float v[EP];
    if (VEC) {
      const f32x4* r4 = reinterpret_cast<const f32x4*>(eb + n * E);
#pragma unroll
      for (int q = 0; q < EP / 4; ++q) {
        const f32x4 x = r4[q];
        v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
      }
    } else {
#pragma unroll
      for (int e = 0; e < EP; ++e) v[e] = e < E ? eb[n * E + e] : 0.f;
    }
#pragma unroll 1
    for (int e4 = 0; e4 < EP / 4; ++e4) {
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = 4 * e4 + i;
        float acc = -sB[e * DANET_DPCL_MAX_C + y];
#pragma unroll
        for (int q = 0; q < EP / 4; ++q) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(&sA[e * EP + 4 * q]);
          /* explicit fused multiply-adds in one order: both instantiations of a row size round alike */
          acc = __builtin_fmaf(a[0], v[4 * q], acc);
          acc = __builtin_fmaf(a[1], v[4 * q + 1], acc);
          acc = __builtin_fmaf(a[2], v[4 * q + 2], acc);
          acc = __builtin_fmaf(a[3], v[4 * q + 3], acc);
        }
        o[i] = coef * acc;
      }
      if (VEC) {
        reinterpret_cast<f32x4*>(db + n * E)[e4] = o;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (4 * e4 + i < E) db[n * E + 4 * e4 + i] = o[i];
      }
    }
  }
}

template <int EP>
static void launch_bwd(hipStream_t st, dim3 grid, bool vec, int64_t N, int E, int C, const float* embed,
                       const float* src_pwr, const float* tables, const float* cs, const float* dloss, float scale,
                       float* dembed) {
  if (vec && E == EP)
    dpcl_bwd_kernel<EP, true><<<grid, kThreads, 0, st>>>(N, E, C, embed, src_pwr, tables, cs, dloss, scale, dembed);
  else
    dpcl_bwd_kernel<EP, false><<<grid, kThreads, 0, st>>>(N, E, C, embed, src_pwr, tables, cs, dloss, scale, dembed);
}

extern "C" int danet_dpcl_bwd(void* stream, int B, int64_t N, int E, int C, const float* embed, const float* src_pwr,
                              const float* tables_f32, const float* cs_f32, const float* dloss_f32, float scale,
                              float* dembed) {
  if (!envelope_ok("bwd", B, N, E, C)) return DANET_DPCL_ERR_ARG;
  CHECK_ARG(embed && src_pwr && tables_f32 && cs_f32 && dembed, "bwd: null pointer");
  CHECK_ARG((((uintptr_t)embed | (uintptr_t)src_pwr | (uintptr_t)tables_f32 | (uintptr_t)cs_f32 |
              (uintptr_t)dloss_f32 | (uintptr_t)dembed) & 3) == 0,
            "bwd: misaligned pointer (4-byte)");
  CHECK_ARG(isfinite(scale), "bwd: scale must be finite (got %g)", (double)scale);
  const dim3 grid((unsigned)cdiv64(N, kBwdRows), (unsigned)B);
  const bool vec = (((uintptr_t)embed | (uintptr_t)dembed) & 15) == 0 && (E & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (E <= 4) launch_bwd<4>(st, grid, vec, N, E, C, embed, src_pwr, tables_f32, cs_f32, dloss_f32, scale, dembed);
  else if (E <= 8) launch_bwd<8>(st, grid, vec, N, E, C, embed, src_pwr, tables_f32, cs_f32, dloss_f32, scale, dembed);
  else if (E <= 20) launch_bwd<20>(st, grid, vec, N, E, C, embed, src_pwr, tables_f32, cs_f32, dloss_f32, scale, dembed);
  else if (E <= 40) launch_bwd<40>(st, grid, vec, N, E, C, embed, src_pwr, tables_f32, cs_f32, dloss_f32, scale, dembed);
  else launch_bwd<64>(st, grid, vec, N, E, C, embed, src_pwr, tables_f32, cs_f32, dloss_f32, scale, dembed);
  CHECK_LAUNCH();
  return DANET_DPCL_OK;
}
