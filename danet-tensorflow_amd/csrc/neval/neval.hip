/*
 * libdanet_neval_hip.so (include/danet_neval_hip.h): the waveform metric of a noisy `valid` / `test` sweep in three
 * small kernels -- overlap-add synthesis of the references, the estimates and the scaled noise, their Gram
 * matrices, and the permutation search that turns a Gram matrix into SI-SDR, SI-SDRi against the noisy mixture and
 * the realised source-to-noise ratio.  gfx950, wave64.
 *
 * The kernels are this library's own; their arithmetic is, expression for expression, that of csrc/metric/metric.hip
 * (which stays as it is), and tests/test_gpu_neval.py holds the two together bit for bit.
 *
 * danet_neval_synth.  One workgroup of 256 threads per (signal, tile of `hops` consecutive hops), 2C + 1 signals per
 * utterance.  LDS: N/2 twiddles e^(+2 pi i j / N) (sincospif, once per workgroup) and up to `max_frames` frames of N
 * floats.  split -> in-place radix-2 inverse FFT over all frames of the tile -> gather, as in the metric.  The
 * noise row reads its bins through scaled(): fl(g * x), a product that is never contracted into the split step's
 * sums (the sources' rows take g = 1, which is exact).
 * danet_neval_gram.  One workgroup per (utterance, i <= j).
 * danet_neval_si_sdr.  One workgroup; a thread per utterance does the 24-permutation search in float64.
 */
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "danet_neval_hip.h"

static thread_local char g_err[256] = "";

static void neval_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* danet_neval_last_error(void) { return g_err; }
extern "C" int danet_neval_abi_version(void) { return DANET_NEVAL_ABI_VERSION; }

#define NEVAL_CHECK_ARG(cond, ...)   \
  do {                               \
    if (!(cond)) {                   \
      neval_set_error(__VA_ARGS__);  \
      return DANET_NEVAL_ERR_ARG;    \
    }                                \
  } while (0)

#define NEVAL_CHECK_LAUNCH()                                                                          \
  do {                                                                                                \
    const hipError_t e_ = hipGetLastError();                                                          \
    if (e_ != hipSuccess) {                                                                           \
      neval_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return DANET_NEVAL_ERR_LAUNCH;                                                                  \
    }                                                                                                 \
  } while (0)

static const int kThreads = 256;
static const int kWaves = kThreads / 64;
static const int kMaxC = DANET_NEVAL_MAX_C;
static const int kMaxM = 2 * DANET_NEVAL_MAX_C + 1;

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
  const float2* noise;
  const float* gain;      /* [B] or null */
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

/* fl(g * x): one rounding of its own; with contraction off here the product carries no licence to fuse, so what
 * consumes it cannot fold it into an fma */
__device__ __forceinline__ float scaled(float g, float x) {
#pragma clang fp contract(off)
  return g * x;
}

__global__ __launch_bounds__(kThreads) void neval_synth_kernel(SynthArgs a) {
  extern __shared__ __align__(16) float lds[];                 /* (viewed as float2 below) */
  const int N = a.N, S = a.S, T = a.T, M = N >> 1, F = M + 1;
  float2* tw = reinterpret_cast<float2*>(lds);                 /* [M]              */
  float* frames = lds + N;                                     /* [max_frames][N]  */
  const int tid = threadIdx.x;
  const int rows = 2 * a.C + 1;
  const int sig = (int)(blockIdx.x / (unsigned)a.tiles);       /* b * (2C + 1) + m */
  const int tile = (int)(blockIdx.x - (unsigned)sig * (unsigned)a.tiles);
  const int b = sig / rows, m = sig - b * rows;
  const float2* X = (m < a.C       ? a.ref + ((int64_t)b * a.C + m) * T * F
                     : m < 2 * a.C ? a.est + ((int64_t)b * a.C + (m - a.C)) * T * F
                                   : a.noise + (int64_t)b * T * F);
  const float g = (m == 2 * a.C && a.gain) ? a.gain[b] : 1.f;
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
    p.x = scaled(g, p.x); p.y = scaled(g, p.y);
    q.x = scaled(g, q.x); q.y = scaled(g, q.y);
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

extern "C" size_t danet_neval_workspace_bytes(int B, int C, int T, int N, int S) {
  if (!synth_shape_ok(B, C, T, N, S) || C > kMaxC) {
    neval_set_error("workspace_bytes: need B >= 1, 1 <= C <= %d, T >= 2, N a power of two in 64..1024 and "
                    "N/8 <= S <= N/2 (got %d, %d, %d, %d, %d)", kMaxC, B, C, T, N, S);
    return (size_t)-1;
  }
  const size_t Ls = (size_t)(T - 1) * (size_t)S, M = 2 * (size_t)C + 1;
  return round256((size_t)B * M * Ls * sizeof(float)) + round256((size_t)B * M * M * sizeof(double)) +
         round256((size_t)B * 3 * sizeof(double)) + round256(3 * sizeof(double)) +
         round256((size_t)B * sizeof(int32_t));
}

extern "C" int danet_neval_synth(void* stream, int B, int C, int T, int N, int S, const float* ref_c64,
                                 const float* est_c64, const float* noise_c64, const float* noise_gain,
                                 const float* window, float* wav) {
  NEVAL_CHECK_ARG(B >= 1 && C >= 1, "synth: B and C must be >= 1 (got %d, %d)", B, C);
  NEVAL_CHECK_ARG(T >= 2, "synth: T must be >= 2 (got %d)", T);
  NEVAL_CHECK_ARG(N >= 64 && N <= 1024 && (N & (N - 1)) == 0, "synth: N must be a power of two in 64..1024 (got %d)",
                  N);
  NEVAL_CHECK_ARG(S >= 1 && 2 * (int64_t)S <= N && 8 * (int64_t)S >= N, "synth: S must be in [N/8, N/2] (got %d at N = %d)",
                  S, N);
  NEVAL_CHECK_ARG(ref_c64 && est_c64 && noise_c64 && window && wav, "synth: null pointer");
  NEVAL_CHECK_ARG(((uintptr_t)ref_c64 & 7) == 0 && ((uintptr_t)est_c64 & 7) == 0 && ((uintptr_t)noise_c64 & 7) == 0 &&
                      ((uintptr_t)noise_gain & 3) == 0 && ((uintptr_t)window & 3) == 0 && ((uintptr_t)wav & 3) == 0,
                  "synth: misaligned pointer (ref, est, noise 8-byte; noise_gain, window, wav 4-byte)");
  NEVAL_CHECK_ARG((int64_t)(T - 1) * S < ((int64_t)1 << 31), "synth: (T - 1) * S must be < 2^31");
  const Tiling g = tiling_of(T, N, S);
  const int64_t blocks = (int64_t)B * (2 * (int64_t)C + 1) * g.tiles;
  NEVAL_CHECK_ARG(blocks < ((int64_t)1 << 31), "synth: B * (2C + 1) * tiles must be < 2^31");
  SynthArgs a;
  a.ref = (const float2*)ref_c64; a.est = (const float2*)est_c64; a.noise = (const float2*)noise_c64;
  a.gain = noise_gain; a.window = window; a.wav = wav;
  a.C = C; a.T = T; a.N = N; a.S = S;
  a.log2_half = 0;
  while ((2 << a.log2_half) < N) ++a.log2_half;
  a.hops = g.hops; a.tiles = g.tiles; a.max_frames = g.max_frames;
  const size_t lds_bytes = (size_t)(g.max_frames + 1) * N * sizeof(float);      /* <= 64 KiB */
  neval_synth_kernel<<<dim3((unsigned)blocks), kThreads, lds_bytes, (hipStream_t)stream>>>(a);
  NEVAL_CHECK_LAUNCH();
  return DANET_NEVAL_OK;
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

__global__ __launch_bounds__(kThreads) void neval_gram_kernel(int M, int n_pairs, int64_t Ls,
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

extern "C" int danet_neval_gram(void* stream, int B, int M, int64_t Ls, const float* wav, double* G) {
  NEVAL_CHECK_ARG(B >= 1, "gram: B must be >= 1 (got %d)", B);
  NEVAL_CHECK_ARG(M >= 1 && M <= kMaxM, "gram: M must be in 1..%d (got %d)", kMaxM, M);
  NEVAL_CHECK_ARG(Ls >= 1 && Ls < ((int64_t)1 << 31), "gram: Ls must be in [1, 2^31) (got %lld)", (long long)Ls);
  NEVAL_CHECK_ARG(wav && G, "gram: null pointer");
  NEVAL_CHECK_ARG(((uintptr_t)wav & 3) == 0 && ((uintptr_t)G & 7) == 0, "gram: misaligned pointer (wav 4-byte, G 8-byte)");
  const int n_pairs = M * (M + 1) / 2;
  NEVAL_CHECK_ARG((int64_t)B * n_pairs < ((int64_t)1 << 31), "gram: B * M * (M + 1) / 2 must be < 2^31");
  neval_gram_kernel<<<dim3((unsigned)((int64_t)B * n_pairs)), kThreads, 0, (hipStream_t)stream>>>(M, n_pairs, Ls, wav, G);
  NEVAL_CHECK_LAUNCH();
  return DANET_NEVAL_OK;
}

/* ------------------------------------------------------------------------------------- finalize */
__device__ __forceinline__ double sdr_db(double a, double b, double c) {
  const double t = c * c / a, r = b - t;
  if (!(t > 0.0)) return -100.0;
  if (!(r > 0.0)) return 100.0;
  const double d = 10.0 * log10(t / r);
  return d < -100.0 ? -100.0 : (d > 100.0 ? 100.0 : d);
}

/* the p-th permutation of range(C) in itertools.permutations order (csrc/pit_common.h), four bits per position
 * (position i in bits 4i..4i+3); the values still to be placed are kept packed in the same way */
__device__ __forceinline__ unsigned nth_perm(int C, int p) {
  unsigned avail = 0x3210u, out = 0u;
  int fact = 1;
  for (int i = 2; i < C; ++i) fact *= i;
  int n = C;
  for (int i = 0; i < C; ++i) {
    const int q = p / fact;
    p -= q * fact;
    out |= ((avail >> (4 * q)) & 15u) << (4 * i);
    const unsigned low = avail & ((1u << (4 * q)) - 1u);          /* drop nibble q */
    avail = low | ((avail >> (4 * (q + 1))) << (4 * q));
    --n;
    if (n > 1) fact /= n;
  }
  return out;
}

__device__ __forceinline__ double pick4(const double (&r)[kMaxC], int j) {
  return j == 0 ? r[0] : (j == 1 ? r[1] : (j == 2 ? r[2] : r[3]));
}

__global__ __launch_bounds__(kThreads) void neval_si_sdr_kernel(int B, int C, const double* __restrict__ G,
                                                               double* __restrict__ per_utt,
                                                               int32_t* __restrict__ perm_idx,
                                                               double* __restrict__ mean3) {
  __shared__ double part[kWaves];
  const int M = 2 * C + 1, nz = 2 * C;
  int nperm = 1;
  for (int i = 2; i <= C; ++i) nperm *= i;
  double sum_sdr = 0.0, sum_imp = 0.0, sum_nsnr = 0.0, live_utts = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double* g = G + (int64_t)b * M * M;
    /* every loop over the sources runs to kMaxC, unrolled, and a drawn column is picked by comparison (pick4):
     * the tables are indexed by constants alone and stay in registers (no scratch) */
    double sdr[kMaxC][kMaxC], base[kMaxC];
    bool live[kMaxC];
    double cc = 0.0;
    for (int k = 0; k < C; ++k)
      for (int l = 0; l < C; ++l) cc += g[k * M + l];
    double cn = 0.0;
    for (int k = 0; k < C; ++k) cn += g[k * M + nz];
    const double nn = g[nz * M + nz];
    const double mm = (cc + 2.0 * cn) + nn;
    int n_live = 0;
#pragma unroll
    for (int i = 0; i < kMaxC; ++i) {
      live[i] = false;
      base[i] = 0.0;
#pragma unroll
      for (int j = 0; j < kMaxC; ++j) sdr[i][j] = 0.0;
      if (i < C) {
        const double a = g[i * M + i];
        live[i] = a != 0.0;
        if (live[i]) {
          ++n_live;
#pragma unroll
          for (int j = 0; j < kMaxC; ++j)
            if (j < C) sdr[i][j] = sdr_db(a, g[(C + j) * M + (C + j)], g[i * M + (C + j)]);
          double ms = 0.0;
          for (int k = 0; k < C; ++k) ms += g[k * M + i];
          base[i] = sdr_db(a, mm, ms + g[nz * M + i]);
        }
      }
    }
    int best = 0;
    double best_v = 0.0, u_sdr = 0.0, u_imp = 0.0, u_nsnr = 0.0;
    if (n_live > 0) {
      for (int p = 0; p < nperm; ++p) {
        const unsigned perm = nth_perm(C, p);
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < kMaxC; ++i)
          if (live[i]) v += pick4(sdr[i], (int)((perm >> (4 * i)) & 15u));
        if (p == 0 || v > best_v) { best = p; best_v = v; }
      }
      const unsigned perm = nth_perm(C, best);
      double imp = 0.0;
#pragma unroll
      for (int i = 0; i < kMaxC; ++i)
        if (live[i]) imp += pick4(sdr[i], (int)((perm >> (4 * i)) & 15u)) - base[i];
      u_sdr = best_v / (double)n_live;
      u_imp = imp / (double)n_live;
      if (!(cc > 0.0)) {
        u_nsnr = -100.0;
      } else if (!(nn > 0.0)) {
        u_nsnr = 100.0;
      } else {
        const double d = 10.0 * log10(cc / nn);
        u_nsnr = d < -100.0 ? -100.0 : (d > 100.0 ? 100.0 : d);
      }
      sum_sdr += u_sdr;
      sum_imp += u_imp;
      sum_nsnr += u_nsnr;
      live_utts += 1.0;
    }
    per_utt[3 * (int64_t)b] = u_sdr;
    per_utt[3 * (int64_t)b + 1] = u_imp;
    per_utt[3 * (int64_t)b + 2] = u_nsnr;
    perm_idx[b] = best;
  }
  const double ts = block_sum_f64(sum_sdr, part);
  const double ti = block_sum_f64(sum_imp, part);
  const double tz = block_sum_f64(sum_nsnr, part);
  const double tn = block_sum_f64(live_utts, part);
  if (threadIdx.x == 0) {
    mean3[0] = tn > 0.0 ? ts / tn : 0.0;
    mean3[1] = tn > 0.0 ? ti / tn : 0.0;
    mean3[2] = tn > 0.0 ? tz / tn : 0.0;
  }
}

extern "C" int danet_neval_si_sdr(void* stream, int B, int C, const double* G, double* per_utt, int32_t* perm_idx,
                                  double* mean3) {
  NEVAL_CHECK_ARG(B >= 1, "si_sdr: B must be >= 1 (got %d)", B);
  NEVAL_CHECK_ARG(C >= 1 && C <= kMaxC, "si_sdr: C must be in 1..%d (got %d)", kMaxC, C);
  NEVAL_CHECK_ARG(G && per_utt && perm_idx && mean3, "si_sdr: null pointer");
  NEVAL_CHECK_ARG(((uintptr_t)G & 7) == 0 && ((uintptr_t)per_utt & 7) == 0 && ((uintptr_t)mean3 & 7) == 0 &&
                      ((uintptr_t)perm_idx & 3) == 0,
                  "si_sdr: misaligned pointer (G, per_utt, mean3 8-byte; perm_idx 4-byte)");
  neval_si_sdr_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(B, C, G, per_utt, perm_idx, mean3);
  NEVAL_CHECK_LAUNCH();
  return DANET_NEVAL_OK;
}
