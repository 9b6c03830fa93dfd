/*
 * libdanet_metric_hip.so (include/danet_metric_hip.h): the waveform metric of `valid` / `test` in three
 * small kernels -- overlap-add synthesis of the references and the estimates, their Gram matrices, and the
 * permutation search that turns a Gram matrix into SI-SDR and SI-SDRi.  gfx950, wave64.
 *
 * danet_metric_synth.  One workgroup of 256 threads per (signal, tile of `hops` consecutive hops).  LDS:
 * N/2 twiddles e^(+2 pi i j / N) (sincospif, once per workgroup) and up to `max_frames` frames of N floats.
 *   split:  frame t, bin k < N/2:  Z[k] = E + i O with E = (X[k] + conj(X[N/2-k])) / N and
 *           O = (X[k] - conj(X[N/2-k])) / N * e^(+2 pi i k / N)  (the imaginary parts of X[0] and X[N/2]
 *           read as 0), stored at the bit-reversed index of k;
 *   fft:    log2(N/2) in-place radix-2 stages over all frames of the tile at once, one barrier per stage;
 *           z[m] = x[2m] + i x[2m+1], so the float view of the frame IS the real frame;
 *   gather: thread -> output sample n of the tile; its frames in ascending t.
 * danet_metric_gram.  One workgroup per (utterance, i <= j): nothing to share between workgroups, so no
 * scratch and no second launch; the waveforms of one batch sit in L2.
 * danet_metric_si_sdr.  One workgroup; a thread per utterance does the 24-permutation search in float64.
 */
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "danet_metric_hip.h"

static thread_local char g_err[256] = "";

static void metric_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* danet_metric_last_error(void) { return g_err; }
extern "C" int danet_metric_abi_version(void) { return DANET_METRIC_ABI_VERSION; }

#define METRIC_CHECK_ARG(cond, ...)   \
  do {                                \
    if (!(cond)) {                    \
      metric_set_error(__VA_ARGS__);  \
      return DANET_METRIC_ERR_ARG;    \
    }                                 \
  } while (0)

#define METRIC_CHECK_LAUNCH()                                                                          \
  do {                                                                                                 \
    const hipError_t e_ = hipGetLastError();                                                           \
    if (e_ != hipSuccess) {                                                                            \
      metric_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return DANET_METRIC_ERR_LAUNCH;                                                                  \
    }                                                                                                  \
  } while (0)

static const int kThreads = 256;
static const int kWaves = kThreads / 64;
static const int kMaxC = DANET_METRIC_MAX_C;

/* ------------------------------------------------------------------------------------ synthesis */
static const int kLdsFloats = 16384;      /* 64 KiB: the twiddles (N floats) + the frames of a tile */
static const int kMaxFrames = 32;

struct Tiling {
  int max_frames;   /* frames a tile may hold in LDS                        */
  int hops;         /* hops (S output samples each) per tile, >= 1          */
  int tiles;        /* tiles per signal                                     */
};

static bool synth_shape_ok(int B, int C, int T, int N, int S) {
  return B >= 1 && C >= 1 && T >= 2 && N >= 64 && N <= 1024 && (N & (N - 1)) == 0 && 2 * S <= N && 8 * S >= N;
}

/* a tile of h hops starting at hop h0 covers the samples [h0 S, (h0 + h) S) and needs the frames
 * floor((h0 S - N/2) / S) + 1 .. floor(((h0 + h) S - 1 + N/2) / S): with N/2 = q S + r that is h + 2q - 1
 * frames when r = 0 and h + 2q + 1 otherwise (q <= 4, and q = 4 only with r = 0: at most h + 7) */
static Tiling tiling_of(int T, int N, int S) {
  Tiling g;
  g.max_frames = kLdsFloats / N - 1;
  if (g.max_frames > kMaxFrames) g.max_frames = kMaxFrames;
  const int q = (N / 2) / S, r = (N / 2) % S;
  const int extra = r == 0 ? 2 * q - 1 : 2 * q + 1;
  g.hops = g.max_frames - extra;            /* >= 15 - 7 */
  if (g.hops > T - 1) g.hops = T - 1;
  g.tiles = (T - 1 + g.hops - 1) / g.hops;
  return g;
}

struct SynthArgs {
  const float2* ref;
  const float2* est;
  const float* window;
  float* wav;
  int C, T, N, S;
  int log2_half;     /* log2(N/2) */
  int hops, tiles, max_frames;
};

__device__ __forceinline__ int floor_div(int a, int b) {      /* b > 0 */
  const int q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kThreads) void metric_synth_kernel(SynthArgs a) {
  extern __shared__ __align__(16) float lds[];                 /* (viewed as float2 below) */
  const int N = a.N, S = a.S, T = a.T, M = N >> 1, F = M + 1;
  float2* tw = reinterpret_cast<float2*>(lds);                 /* [M]              */
  float* frames = lds + N;                                     /* [max_frames][N]  */
  const int tid = threadIdx.x;
  const int sig = (int)(blockIdx.x / (unsigned)a.tiles);       /* b * 2C + m       */
  const int tile = (int)(blockIdx.x - (unsigned)sig * (unsigned)a.tiles);
  const int b = sig / (2 * a.C), m = sig - b * 2 * a.C;
  const float2* X = (m < a.C ? a.ref + ((int64_t)b * a.C + m) * T * F
                             : a.est + ((int64_t)b * a.C + (m - a.C)) * T * F);
  const int Ls = (T - 1) * S;
  const int n0 = tile * a.hops * S;
  const int n1 = min(n0 + a.hops * S, Ls);
  const int t_first = max(floor_div(n0 - M, S) + 1, 0);
  const int t_last = min(floor_div(n1 - 1 + M, S), T - 1);
  const int nfr = min(t_last - t_first + 1, a.max_frames);     /* (the host sized the tile: never cut) */

  for (int j = tid; j < M; j += kThreads) {
    float s, c;
    sincospif((float)(2 * j) / (float)N, &s, &c);
    tw[j] = make_float2(c, s);
  }
  __syncthreads();

  /* split step: bins -> the N/2 complex inputs of the half-size transform, bit-reversed */
  const float inv_n = 1.0f / (float)N;
  const int shift = 32 - a.log2_half;
  for (int idx = tid; idx < nfr * M; idx += kThreads) {
    const int f = idx >> a.log2_half, k = idx & (M - 1);
    const float2* row = X + (int64_t)(t_first + f) * F;
    float2 p = row[k], q = row[M - k];
    if (k == 0) { p.y = 0.f; q.y = 0.f; }                      /* bins 0 and N/2: imaginary parts ignored */
    const float er = (p.x + q.x) * inv_n, ei = (p.y - q.y) * inv_n;
    const float dr = (p.x - q.x) * inv_n, di = (p.y + q.y) * inv_n;
    const float2 w = tw[k];
    const float o_r = dr * w.x - di * w.y, o_i = dr * w.y + di * w.x;
    const int rk = (int)(__brev((unsigned)k) >> shift);
    reinterpret_cast<float2*>(frames + f * N)[rk] = make_float2(er - o_i, ei + o_r);      /* E + i O */
  }
  __syncthreads();

  /* in-place radix-2 inverse transform (decimation in time) of every frame of the tile */
  const int half_m = M >> 1;
  for (int lh = 0; lh < a.log2_half; ++lh) {
    const int h = 1 << lh;
    for (int idx = tid; idx < nfr * half_m; idx += kThreads) {
      const int f = idx >> (a.log2_half - 1), j = idx & (half_m - 1);
      const int pos = j & (h - 1);
      const int i0 = ((j >> lh) << (lh + 1)) + pos;
      float2* z = reinterpret_cast<float2*>(frames + f * N);
      const float2 w = tw[pos << (a.log2_half - lh)];           /* e^(+2 pi i pos / 2h) */
      const float2 u = z[i0], v = z[i0 + h];
      const float vr = v.x * w.x - v.y * w.y, vi = v.x * w.y + v.y * w.x;
      z[i0] = make_float2(u.x + vr, u.y + vi);
      z[i0 + h] = make_float2(u.x - vr, u.y - vi);
    }
    __syncthreads();
  }

  /* gather: every output sample of the tile sums its frames, ascending t */
  float* y = a.wav + (int64_t)sig * Ls;
  for (int n = n0 + tid; n < n1; n += kThreads) {
    const int ta = max(floor_div(n - M, S) + 1, t_first);
    const int tb = min(floor_div(n + M, S), t_first + nfr - 1);
    float acc = 0.f, wsum = 0.f;
    for (int t = ta; t <= tb; ++t) {
      const int k = n - t * S + M;                              /* 0 <= k < N by the choice of ta, tb */
      const float w = a.window[k];
      acc += w * frames[(t - t_first) * N + k];
      wsum += w * w;
    }
    y[n] = wsum > 0.f ? acc / wsum : 0.f;
  }
}

static size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t danet_metric_workspace_bytes(int B, int C, int T, int N, int S) {
  if (!synth_shape_ok(B, C, T, N, S) || C > kMaxC) {
    metric_set_error("workspace_bytes: need B >= 1, 1 <= C <= %d, T >= 2, N a power of two in 64..1024 and "
                     "N/8 <= S <= N/2 (got %d, %d, %d, %d, %d)", kMaxC, B, C, T, N, S);
    return (size_t)-1;
  }
  const size_t Ls = (size_t)(T - 1) * (size_t)S, M = 2 * (size_t)C;
  return round256((size_t)B * M * Ls * sizeof(float)) + round256((size_t)B * M * M * sizeof(double)) +
         round256((size_t)B * 2 * sizeof(double)) + round256(2 * sizeof(double)) +
         round256((size_t)B * sizeof(int32_t));
}

extern "C" int danet_metric_synth(void* stream, int B, int C, int T, int N, int S, const float* ref_c64,
                                  const float* est_c64, const float* window, float* wav) {
  METRIC_CHECK_ARG(B >= 1 && C >= 1, "synth: B and C must be >= 1 (got %d, %d)", B, C);
  METRIC_CHECK_ARG(T >= 2, "synth: T must be >= 2 (got %d)", T);
  METRIC_CHECK_ARG(N >= 64 && N <= 1024 && (N & (N - 1)) == 0, "synth: N must be a power of two in 64..1024 (got %d)",
                   N);
  METRIC_CHECK_ARG(S >= 1 && 2 * (int64_t)S <= N && 8 * (int64_t)S >= N, "synth: S must be in [N/8, N/2] (got %d at N = %d)",
                   S, N);
  METRIC_CHECK_ARG(ref_c64 && est_c64 && window && wav, "synth: null pointer");
  METRIC_CHECK_ARG(((uintptr_t)ref_c64 & 7) == 0 && ((uintptr_t)est_c64 & 7) == 0 && ((uintptr_t)window & 3) == 0 &&
                       ((uintptr_t)wav & 3) == 0,
                   "synth: misaligned pointer (ref, est 8-byte; window, wav 4-byte)");
  METRIC_CHECK_ARG((int64_t)(T - 1) * S < ((int64_t)1 << 31), "synth: (T - 1) * S must be < 2^31");
  const Tiling g = tiling_of(T, N, S);
  const int64_t blocks = (int64_t)B * 2 * C * g.tiles;
  METRIC_CHECK_ARG(blocks < ((int64_t)1 << 31), "synth: B * 2C * tiles must be < 2^31");
  SynthArgs a;
  a.ref = (const float2*)ref_c64; a.est = (const float2*)est_c64; a.window = window; a.wav = wav;
  a.C = C; a.T = T; a.N = N; a.S = S;
  a.log2_half = 0;
  while ((2 << a.log2_half) < N) ++a.log2_half;
  a.hops = g.hops; a.tiles = g.tiles; a.max_frames = g.max_frames;
  const size_t lds_bytes = (size_t)(g.max_frames + 1) * N * sizeof(float);      /* <= 64 KiB */
  metric_synth_kernel<<<dim3((unsigned)blocks), kThreads, lds_bytes, (hipStream_t)stream>>>(a);
  METRIC_CHECK_LAUNCH();
  return DANET_METRIC_OK;
}

/* ----------------------------------------------------------------------------------------- Gram */
/* every lane: the sum over the workgroup, (w0 + w1) + (w2 + w3) of the waves' butterflies */
__device__ __forceinline__ double block_sum_f64(double v, double* part) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();                                             /* (part may still be read from a call before) */
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(kThreads) void metric_gram_kernel(int M, int n_pairs, int64_t Ls,
                                                              const float* __restrict__ wav,
                                                              double* __restrict__ G) {
  __shared__ double part[kWaves];
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)n_pairs);
  int p = (int)(blockIdx.x - (unsigned)b * (unsigned)n_pairs);
  int i = 0;
  while (p >= M - i) { p -= M - i; ++i; }                      /* row i of the upper triangle has M - i pairs */
  const int j = i + p;
  const float* x = wav + ((int64_t)b * M + i) * Ls;
  const float* y = wav + ((int64_t)b * M + j) * Ls;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t n = tid;
  for (; n + 3 * kThreads < Ls; n += 4 * kThreads) {
    const float x0 = x[n], x1 = x[n + kThreads], x2 = x[n + 2 * kThreads], x3 = x[n + 3 * kThreads];
    const float y0 = y[n], y1 = y[n + kThreads], y2 = y[n + 2 * kThreads], y3 = y[n + 3 * kThreads];
    a0 += (double)x0 * (double)y0;
    a1 += (double)x1 * (double)y1;
    a2 += (double)x2 * (double)y2;
    a3 += (double)x3 * (double)y3;
  }
  if (n < Ls) a0 += (double)x[n] * (double)y[n];
  if (n + kThreads < Ls) a1 += (double)x[n + kThreads] * (double)y[n + kThreads];
  if (n + 2 * kThreads < Ls) a2 += (double)x[n + 2 * kThreads] * (double)y[n + 2 * kThreads];
  const double r = block_sum_f64((a0 + a1) + (a2 + a3), part);
  if (tid == 0) {
    double* g = G + (int64_t)b * M * M;
    g[i * M + j] = r;
    g[j * M + i] = r;
  }
}

extern "C" int danet_metric_gram(void* stream, int B, int M, int64_t Ls, const float* wav, double* G) {
  METRIC_CHECK_ARG(B >= 1, "gram: B must be >= 1 (got %d)", B);
  METRIC_CHECK_ARG(M >= 1 && M <= 2 * kMaxC, "gram: M must be in 1..%d (got %d)", 2 * kMaxC, M);
  METRIC_CHECK_ARG(Ls >= 1 && Ls < ((int64_t)1 << 31), "gram: Ls must be in [1, 2^31) (got %lld)", (long long)Ls);
  METRIC_CHECK_ARG(wav && G, "gram: null pointer");
  METRIC_CHECK_ARG(((uintptr_t)wav & 3) == 0 && ((uintptr_t)G & 7) == 0, "gram: misaligned pointer (wav 4-byte, G 8-byte)");
  const int n_pairs = M * (M + 1) / 2;
  METRIC_CHECK_ARG((int64_t)B * n_pairs < ((int64_t)1 << 31), "gram: B * M * (M + 1) / 2 must be < 2^31");
  metric_gram_kernel<<<dim3((unsigned)((int64_t)B * n_pairs)), kThreads, 0, (hipStream_t)stream>>>(M, n_pairs, Ls, wav, G);
  METRIC_CHECK_LAUNCH();
  return DANET_METRIC_OK;
}

/* ------------------------------------------------------------------------------------- finalize */
__device__ __forceinline__ double sdr_db(double a, double b, double c) {
  const double t = c * c / a, r = b - t;
  if (!(t > 0.0)) return -100.0;
  if (!(r > 0.0)) return 100.0;
  const double d = 10.0 * log10(t / r);
  return d < -100.0 ? -100.0 : (d > 100.0 ? 100.0 : d);
}

/* the p-th permutation of range(C) in itertools.permutations order (csrc/pit_common.h) */
__device__ __forceinline__ void nth_perm(int C, int p, int* out) {
  int avail[kMaxC] = {0, 1, 2, 3};
  int fact = 1;
  for (int i = 2; i < C; ++i) fact *= i;
  int n = C;
  for (int i = 0; i < C; ++i) {
    const int q = p / fact;
    p -= q * fact;
    out[i] = avail[q];
    for (int j = q; j < n - 1; ++j) avail[j] = avail[j + 1];
    --n;
    if (n > 1) fact /= n;
  }
}

__global__ __launch_bounds__(kThreads) void metric_si_sdr_kernel(int B, int C, const double* __restrict__ G,
                                                                double* __restrict__ per_utt,
                                                                int32_t* __restrict__ perm_idx,
                                                                double* __restrict__ mean2) {
  __shared__ double part[kWaves];
  const int M = 2 * C;
  int nperm = 1;
  for (int i = 2; i <= C; ++i) nperm *= i;
  double sum_sdr = 0.0, sum_imp = 0.0, live_utts = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double* g = G + (int64_t)b * M * M;
    double sdr[kMaxC][kMaxC], base[kMaxC];
    bool live[kMaxC];
    double mm = 0.0;
    for (int k = 0; k < C; ++k)
      for (int l = 0; l < C; ++l) mm += g[k * M + l];
    int n_live = 0;
    for (int i = 0; i < C; ++i) {
      const double a = g[i * M + i];
      live[i] = a != 0.0;
      if (!live[i]) continue;
      ++n_live;
      for (int j = 0; j < C; ++j) sdr[i][j] = sdr_db(a, g[(C + j) * M + (C + j)], g[i * M + (C + j)]);
      double ms = 0.0;
      for (int k = 0; k < C; ++k) ms += g[k * M + i];
      base[i] = sdr_db(a, mm, ms);
    }
    int best = 0;
    double best_v = 0.0, u_sdr = 0.0, u_imp = 0.0;
    if (n_live > 0) {
      for (int p = 0; p < nperm; ++p) {
        int perm[kMaxC];
        nth_perm(C, p, perm);
        double v = 0.0;
        for (int i = 0; i < C; ++i)
          if (live[i]) v += sdr[i][perm[i]];
        if (p == 0 || v > best_v) { best = p; best_v = v; }
      }
      int perm[kMaxC];
      nth_perm(C, best, perm);
      double imp = 0.0;
      for (int i = 0; i < C; ++i)
        if (live[i]) imp += sdr[i][perm[i]] - base[i];
      u_sdr = best_v / (double)n_live;
      u_imp = imp / (double)n_live;
      sum_sdr += u_sdr;
      sum_imp += u_imp;
      live_utts += 1.0;
    }
    per_utt[2 * (int64_t)b] = u_sdr;
    per_utt[2 * (int64_t)b + 1] = u_imp;
    perm_idx[b] = best;
  }
  const double ts = block_sum_f64(sum_sdr, part);
  const double ti = block_sum_f64(sum_imp, part);
  const double tn = block_sum_f64(live_utts, part);
  if (threadIdx.x == 0) {
    mean2[0] = tn > 0.0 ? ts / tn : 0.0;
    mean2[1] = tn > 0.0 ? ti / tn : 0.0;
  }
}

extern "C" int danet_metric_si_sdr(void* stream, int B, int C, const double* G, double* per_utt, int32_t* perm_idx,
                                   double* mean2) {
  METRIC_CHECK_ARG(B >= 1, "si_sdr: B must be >= 1 (got %d)", B);
  METRIC_CHECK_ARG(C >= 1 && C <= kMaxC, "si_sdr: C must be in 1..%d (got %d)", kMaxC, C);
  METRIC_CHECK_ARG(G && per_utt && perm_idx && mean2, "si_sdr: null pointer");
  METRIC_CHECK_ARG(((uintptr_t)G & 7) == 0 && ((uintptr_t)per_utt & 7) == 0 && ((uintptr_t)mean2 & 7) == 0 &&
                       ((uintptr_t)perm_idx & 3) == 0,
                   "si_sdr: misaligned pointer (G, per_utt, mean2 8-byte; perm_idx 4-byte)");
  metric_si_sdr_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(B, C, G, per_utt, perm_idx, mean2);
  METRIC_CHECK_LAUNCH();
  return DANET_METRIC_OK;
}
