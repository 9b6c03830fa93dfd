/*
 * libdanet_wavloss_hip.so (include/danet_wavloss_hip.h): the waveform training loss in two kernels -- the
 * finalize step that turns the metric's Gram matrices into -SI-SDR plus the pairing and the coefficients the
 * backward pass needs, and the adjoint of the metric's synthesis.  gfx950, wave64.
 *
 * danet_wavloss_fwd.  One workgroup; a thread per utterance does the 24-permutation search in float64 (the
 * arithmetic of danet_metric_si_sdr), the batch sums go over the metric's fixed tree, and a second pass of the
 * same thread over its own utterances writes pair and coef once the number of live utterances is known.
 * danet_wavloss_bwd.  One workgroup of 256 threads per (estimate, tile of frames).  LDS: N/2 twiddles
 * e^(-2 pi i j / N) (sincospif, once per workgroup), the tile's span of u, and the tile's frames of N floats.
 *   stage:  u[n] = (alpha s[n] + beta y[n]) / wsum[n] in float64, rounded once; wsum from the sample's own frames;
 *   frames: z[m] = w[2m] u[.. + 2m] + i w[2m+1] u[.. + 2m + 1], stored at the bit-reversed index of m;
 *   fft:    log2(N/2) in-place radix-2 stages (decimation in time) over all frames of the tile, one barrier each;
 *   split:  X[k] = E - i e^(-2 pi i k / N) O with E = (Z[k] + conj(Z[N/2-k])) / 2, O = (Z[k] - conj(Z[N/2-k])) / 2;
 *           bins 0 and N/2 are Re Z[0] +- Im Z[0]; scaled by dloss c_k / N and written (through the phasor or not).
 */
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "danet_wavloss_hip.h"

static thread_local char g_err[256] = "";

static void wavloss_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* danet_wavloss_last_error(void) { return g_err; }
extern "C" int danet_wavloss_abi_version(void) { return DANET_WAVLOSS_ABI_VERSION; }

#define WAVLOSS_CHECK_ARG(cond, ...)   \
  do {                                 \
    if (!(cond)) {                     \
      wavloss_set_error(__VA_ARGS__);  \
      return DANET_WAVLOSS_ERR_ARG;    \
    }                                  \
  } while (0)

#define WAVLOSS_CHECK_LAUNCH()                                                                          \
  do {                                                                                                  \
    const hipError_t e_ = hipGetLastError();                                                            \
    if (e_ != hipSuccess) {                                                                             \
      wavloss_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return DANET_WAVLOSS_ERR_LAUNCH;                                                                  \
    }                                                                                                   \
  } while (0)

static const int kThreads = 256;
static const int kWaves = kThreads / 64;
static const int kMaxC = DANET_WAVLOSS_MAX_C;

/* ------------------------------------------------------------------------------------- finalize */
/* every lane: the sum over the workgroup, (w0 + w1) + (w2 + w3) of the waves' butterflies (the tree of
 * csrc/metric/metric.hip) */
__device__ __forceinline__ double block_sum_f64(double v, double* part) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();                                             /* (part may still be read from a call before) */
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

/* sdr(i, j) of the metric; *clamped: the value is one of the rule's clamps (its gradient is 0) */
__device__ __forceinline__ double sdr_db(double a, double b, double c, bool* clamped) {
  const double t = c * c / a, r = b - t;
  *clamped = true;
  if (!(t > 0.0)) return -100.0;
  if (!(r > 0.0)) return 100.0;
  const double d = 10.0 * log10(t / r);
  if (d <= -100.0) return -100.0;
  if (d >= 100.0) return 100.0;
  *clamped = false;
  return d;
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

__global__ __launch_bounds__(kThreads) void wavloss_fwd_kernel(int B, int C, const double* __restrict__ G,
                                                              double* __restrict__ loss_f64,
                                                              float* __restrict__ loss_f32,
                                                              double* __restrict__ per_utt,
                                                              int32_t* __restrict__ perm_idx,
                                                              int32_t* __restrict__ pair,
                                                              double* __restrict__ coef) {
  __shared__ double part[kWaves];
  const int M = 2 * C;
  int nperm = 1;
  for (int i = 2; i <= C; ++i) nperm *= i;
  double sum_sdr = 0.0, live_utts = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double* g = G + (int64_t)b * M * M;
    double sdr[kMaxC][kMaxC];
    bool live[kMaxC];
    int n_live = 0;
    for (int i = 0; i < C; ++i) {
      const double a = g[i * M + i];
      live[i] = a != 0.0;
      if (!live[i]) continue;
      ++n_live;
      bool cl;
      for (int j = 0; j < C; ++j) sdr[i][j] = sdr_db(a, g[(C + j) * M + (C + j)], g[i * M + (C + j)], &cl);
    }
    int best = 0;
    double best_v = 0.0, u_sdr = 0.0;
    if (n_live > 0) {
      for (int p = 0; p < nperm; ++p) {
        int perm[kMaxC];
        nth_perm(C, p, perm);
        double v = 0.0;
        for (int i = 0; i < C; ++i)
          if (live[i]) v += sdr[i][perm[i]];
        if (p == 0 || v > best_v) { best = p; best_v = v; }
      }
      u_sdr = best_v / (double)n_live;
      sum_sdr += u_sdr;
      live_utts += 1.0;
    }
    per_utt[b] = u_sdr;
    perm_idx[b] = best;
  }
  const double ts = block_sum_f64(sum_sdr, part);
  const double tn = block_sum_f64(live_utts, part);
  if (threadIdx.x == 0) {
    const double L = tn > 0.0 ? -(ts / tn) : 0.0;
    loss_f64[0] = L;
    loss_f32[0] = (float)L;
  }
  /* second pass: the pairing and the coefficients, now that the number of live utterances is known.  A thread
   * re-reads the permutation index it wrote itself above. */
  const double K = 10.0 / log(10.0);
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double* g = G + (int64_t)b * M * M;
    int n_live = 0;
    for (int i = 0; i < C; ++i) n_live += g[i * M + i] != 0.0 ? 1 : 0;
    int perm[kMaxC];
    nth_perm(C, perm_idx[b], perm);
    int pr[kMaxC] = {-1, -1, -1, -1};
    for (int i = 0; i < C; ++i)
      if (g[i * M + i] != 0.0) pr[perm[i]] = i;
    for (int j = 0; j < C; ++j) {
      double alpha = 0.0, beta = 0.0;
      const int i = pr[j];
      if (i >= 0) {
        const double a = g[i * M + i], bb = g[(C + j) * M + (C + j)], c = g[i * M + (C + j)];
        bool cl;
        sdr_db(a, bb, c, &cl);
        if (!cl) {
          const double r = bb - c * c / a;
          const double scale = -(1.0 / ((double)n_live * tn));
          alpha = scale * (2.0 * K * bb / (c * r));
          beta = scale * (-2.0 * K / r);
        }
      }
      pair[(int64_t)b * C + j] = i;
      coef[((int64_t)b * C + j) * 2] = alpha;
      coef[((int64_t)b * C + j) * 2 + 1] = beta;
    }
  }
}

extern "C" int danet_wavloss_fwd(void* stream, int B, int C, const double* G, double* loss_f64, float* loss_f32,
                                 double* per_utt, int32_t* perm_idx, int32_t* pair, double* coef) {
  WAVLOSS_CHECK_ARG(B >= 1, "fwd: B must be >= 1 (got %d)", B);
  WAVLOSS_CHECK_ARG(C >= 1 && C <= kMaxC, "fwd: C must be in 1..%d (got %d)", kMaxC, C);
  WAVLOSS_CHECK_ARG((int64_t)B * 4 * C * C < ((int64_t)1 << 31), "fwd: B * 4 C^2 must be < 2^31");
  WAVLOSS_CHECK_ARG(G && loss_f64 && loss_f32 && per_utt && perm_idx && pair && coef, "fwd: null pointer");
  WAVLOSS_CHECK_ARG(((uintptr_t)G & 7) == 0 && ((uintptr_t)loss_f64 & 7) == 0 && ((uintptr_t)per_utt & 7) == 0 &&
                        ((uintptr_t)coef & 7) == 0 && ((uintptr_t)loss_f32 & 3) == 0 &&
                        ((uintptr_t)perm_idx & 3) == 0 && ((uintptr_t)pair & 3) == 0,
                    "fwd: misaligned pointer (G, loss_f64, per_utt, coef 8-byte; loss_f32, perm_idx, pair 4-byte)");
  wavloss_fwd_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(B, C, G, loss_f64, loss_f32, per_utt, perm_idx,
                                                                    pair, coef);
  WAVLOSS_CHECK_LAUNCH();
  return DANET_WAVLOSS_OK;
}

/* ------------------------------------------------------------------------------------- backward */
struct BwdArgs {
  const float* wav;
  const int32_t* pair;
  const double* coef;
  const float* window;
  const float* dloss;
  const float2* phasor;
  float* out;
  int C, T, N, S;
  int log2_half;     /* log2(N/2) */
  int frames, tiles; /* frames per tile, tiles per estimate */
};

__device__ __forceinline__ int floor_div(int a, int b) {      /* b > 0 */
  const int q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kThreads) void wavloss_bwd_kernel(BwdArgs a) {
  extern __shared__ __align__(16) float lds[];                 /* (viewed as float2 below) */
  const int N = a.N, S = a.S, T = a.T, C = a.C, M = N >> 1, F = M + 1;
  const int tid = threadIdx.x;
  const int sig = (int)(blockIdx.x / (unsigned)a.tiles);       /* b * C + j */
  const int tile = (int)(blockIdx.x - (unsigned)sig * (unsigned)a.tiles);
  const int b = sig / C, j = sig - b * C;
  const int t0 = tile * a.frames;
  const int nfr = min(a.frames, T - t0);                       /* >= 1: tiles = ceil(T / frames) */
  const int Ls = (T - 1) * S;
  const int span = (nfr - 1) * S + N;                          /* samples [n_lo, n_lo + span) */
  const int n_lo = t0 * S - M;
  float2* tw = reinterpret_cast<float2*>(lds);                 /* [M]                        */
  float* frames = lds + N;                                     /* [a.frames][N]              */
  float* u = frames + a.frames * N;                            /* [(a.frames - 1) * S + N]   */
  const int64_t row = ((int64_t)sig * T + t0) * F;             /* first output element of the tile */
  const bool real_out = a.phasor != nullptr;

  const int i_ref = a.pair[sig];
  if (i_ref < 0 || i_ref >= C) {                               /* (the whole workgroup: no barrier is skipped by some) */
    if (real_out) {
      for (int idx = tid; idx < nfr * F; idx += kThreads) a.out[row + idx] = 0.f;
    } else {
      float2* o = reinterpret_cast<float2*>(a.out);
      for (int idx = tid; idx < nfr * F; idx += kThreads) o[row + idx] = make_float2(0.f, 0.f);
    }
    return;
  }
  const double alpha = a.coef[2 * (int64_t)sig], beta = a.coef[2 * (int64_t)sig + 1];

  for (int k = tid; k < M; k += kThreads) {
    float s, c;
    sincospif((float)(2 * k) / (float)N, &s, &c);
    tw[k] = make_float2(c, -s);
  }
  /* stage u: every sample of the span from its own window sum; all C reference rows are read and one selected */
  const float* refs = a.wav + (int64_t)b * 2 * C * Ls;
  const float* y = refs + (int64_t)(C + j) * Ls;
  for (int i = tid; i < span; i += kThreads) {
    const int n = n_lo + i;
    float v = 0.f;
    if (n >= 0 && n < Ls) {
      const int ta = max(floor_div(n - M, S) + 1, 0);
      const int tb = min(floor_div(n + M, S), T - 1);
      float wsum = 0.f;
      for (int t = ta; t <= tb; ++t) {
        const float w = a.window[n - t * S + M];               /* 0 <= index < N by the choice of ta, tb */
        wsum += w * w;
      }
      float s = 0.f;
      for (int i2 = 0; i2 < C; ++i2) {
        const float r = refs[(int64_t)i2 * Ls + n];
        s = i2 == i_ref ? r : s;
      }
      if (wsum > 0.f) v = (float)((alpha * (double)s + beta * (double)y[n]) / (double)wsum);
    }
    u[i] = v;
  }
  __syncthreads();

  /* windowed frames -> the N/2 complex inputs of the half-size transform, bit-reversed */
  const int shift = 32 - a.log2_half;
  for (int idx = tid; idx < nfr * M; idx += kThreads) {
    const int f = idx >> a.log2_half, m = idx & (M - 1);
    const float* src = u + f * S + 2 * m;
    const int rm = (int)(__brev((unsigned)m) >> shift);
    reinterpret_cast<float2*>(frames + f * N)[rm] = make_float2(a.window[2 * m] * src[0], a.window[2 * m + 1] * src[1]);
  }
  __syncthreads();

  /* in-place radix-2 forward transform (decimation in time) of every frame of the tile */
  const int half_m = M >> 1;
  for (int lh = 0; lh < a.log2_half; ++lh) {
    const int h = 1 << lh;
    for (int idx = tid; idx < nfr * half_m; idx += kThreads) {
      const int f = idx >> (a.log2_half - 1), p = idx & (half_m - 1);
      const int pos = p & (h - 1);
      const int i0 = ((p >> lh) << (lh + 1)) + pos;
      float2* z = reinterpret_cast<float2*>(frames + f * N);
      const float2 w = tw[pos << (a.log2_half - lh)];           /* e^(-2 pi i pos / 2h) */
      const float2 x0 = z[i0], x1 = z[i0 + h];
      const float vr = x1.x * w.x - x1.y * w.y, vi = x1.x * w.y + x1.y * w.x;
      z[i0] = make_float2(x0.x + vr, x0.y + vi);
      z[i0 + h] = make_float2(x0.x - vr, x0.y - vi);
    }
    __syncthreads();
  }

  /* split step, scale, write: one output element per thread and turn */
  const float dl = a.dloss ? a.dloss[0] : 1.f;
  /* dloss c_k / N: 1/N at bins 0 and N/2; elsewhere c_k = 2 meets the 1/2 of E and O, which are kept doubled */
  const float edge = dl / (float)N, inner = edge;
  const float2* ph = real_out ? a.phasor + ((int64_t)b * T + t0) * F : nullptr;
  for (int idx = tid; idx < nfr * F; idx += kThreads) {
    const int f = idx / F, k = idx - f * F;
    const float2* z = reinterpret_cast<const float2*>(frames + f * N);
    float xr, xi;
    if (k == 0 || k == M) {
      const float2 z0 = z[0];
      xr = (k == 0 ? z0.x + z0.y : z0.x - z0.y) * edge;
      xi = 0.f;
    } else {
      const float2 p = z[k], q = z[M - k];
      const float er = p.x + q.x, ei = p.y - q.y;               /* 2 E = Z[k] + conj(Z[M-k]) */
      const float dr = p.x - q.x, di = p.y + q.y;               /* 2 O = Z[k] - conj(Z[M-k]) */
      const float2 w = tw[k];
      const float pr = w.x * dr - w.y * di, pi = w.x * di + w.y * dr;
      xr = (er + pi) * inner;                                   /* E - i w O */
      xi = (ei - pr) * inner;
    }
    if (real_out) {
      const float2 cs = ph[idx];
      a.out[row + idx] = cs.x * xr + cs.y * xi;
    } else {
      reinterpret_cast<float2*>(a.out)[row + idx] = make_float2(xr, xi);
    }
  }
}

extern "C" int danet_wavloss_bwd(void* stream, int B, int C, int T, int N, int S, const float* wav,
                                 const int32_t* pair, const double* coef, const float* window, const float* dloss,
                                 const float* phasor, float* out) {
  WAVLOSS_CHECK_ARG(B >= 1, "bwd: B must be >= 1 (got %d)", B);
  WAVLOSS_CHECK_ARG(C >= 1 && C <= kMaxC, "bwd: C must be in 1..%d (got %d)", kMaxC, C);
  WAVLOSS_CHECK_ARG(T >= 2, "bwd: T must be >= 2 (got %d)", T);
  WAVLOSS_CHECK_ARG(N >= 64 && N <= 1024 && (N & (N - 1)) == 0, "bwd: N must be a power of two in 64..1024 (got %d)", N);
  WAVLOSS_CHECK_ARG(S >= 1 && 2 * (int64_t)S <= N && 8 * (int64_t)S >= N, "bwd: S must be in [N/8, N/2] (got %d at N = %d)",
                    S, N);
  WAVLOSS_CHECK_ARG(wav && pair && coef && window && out, "bwd: null pointer");
  WAVLOSS_CHECK_ARG(((uintptr_t)wav & 3) == 0 && ((uintptr_t)pair & 3) == 0 && ((uintptr_t)window & 3) == 0 &&
                        ((uintptr_t)dloss & 3) == 0 && ((uintptr_t)coef & 7) == 0 && ((uintptr_t)phasor & 7) == 0 &&
                        ((uintptr_t)out & (phasor ? 3 : 7)) == 0,
                    "bwd: misaligned pointer (wav, pair, window, dloss 4-byte; coef, phasor 8-byte; out 8-byte in the "
                    "complex form, 4-byte in the real one)");
  WAVLOSS_CHECK_ARG((int64_t)(T - 1) * S < ((int64_t)1 << 31), "bwd: (T - 1) * S must be < 2^31");
  WAVLOSS_CHECK_ARG((int64_t)T * (N / 2 + 1) < ((int64_t)1 << 31), "bwd: T * F must be < 2^31");
  const int frames = DANET_WAVLOSS_TILE_FRAMES(N);
  const int tiles = (T + frames - 1) / frames;
  const int64_t blocks = (int64_t)B * C * tiles;
  WAVLOSS_CHECK_ARG(blocks < ((int64_t)1 << 31), "bwd: B * C * tiles must be < 2^31");
  BwdArgs a;
  a.wav = wav; a.pair = pair; a.coef = coef; a.window = window; a.dloss = dloss;
  a.phasor = (const float2*)phasor; a.out = out;
  a.C = C; a.T = T; a.N = N; a.S = S;
  a.log2_half = 0;
  while ((2 << a.log2_half) < N) ++a.log2_half;
  a.frames = frames; a.tiles = tiles;
  /* twiddles N + frames * N + span (frames - 1) * S + N floats: <= 3N/2 (1 + frames) <= 16384 at S = N/2 */
  const size_t lds_bytes = ((size_t)N + (size_t)frames * N + (size_t)(frames - 1) * S + N) * sizeof(float);
  wavloss_bwd_kernel<<<dim3((unsigned)blocks), kThreads, lds_bytes, (hipStream_t)stream>>>(a);
  WAVLOSS_CHECK_LAUNCH();
  return DANET_WAVLOSS_OK;
}
