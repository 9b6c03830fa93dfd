/*
 * libdanet_wavloss_hip.so (include/danet_wavloss_hip.h): the waveform training loss in two kernels -- the
 * finalize step that turns the metric's Gram matrices into -SI-SDR plus the pairing and the coefficients the
 * backward pass needs, and the adjoint of the metric's synthesis.  gfx950, wave64.
 *
 * The search, the batch sums' tree and the radix-2 stages are those of csrc/wave_metric.h, which
 * libdanet_metric_hip.so runs too; this file adds the loss, the second pass and the backward kernel.
 * danet_wavloss_fwd.  One workgroup; a thread per utterance runs pit_search, the batch sums go over
 * block_sum_f64, and a second pass of the same thread over its own utterances writes pair and coef once the
 * number of live utterances is known.
 * danet_wavloss_bwd.  One workgroup of 256 threads per (estimate, tile of frames).  LDS: N/2 twiddles
 * e^(-2 pi i j / N) (sincospif, once per workgroup), the tile's span of u, and the tile's frames of N floats.
 *   stage:  u[n] = (alpha s[n] + beta y[n]) / wsum[n] in float64, rounded once; wsum from the sample's own frames;
 *   frames: z[m] = w[2m] u[.. + 2m] + i w[2m+1] u[.. + 2m + 1], stored at the bit-reversed index of m;
 *   fft:    radix2_stages over all frames of the tile: with these twiddles, the forward transform;
 *   split:  X[k] = E - i e^(-2 pi i k / N) O with E = (Z[k] + conj(Z[N/2-k])) / 2, O = (Z[k] - conj(Z[N/2-k])) / 2;
 *           bins 0 and N/2 are Re Z[0] +- Im Z[0]; scaled by dloss c_k / N and written (through the phasor or not).
 */
#include <hip/hip_runtime.h>

#include "danet_wavloss_hip.h"
#define DANET_EXT wavloss
#define DANET_EXT_UPPER WAVLOSS
#include "ext_core.h"
#include "wave_metric.h"

static_assert(kMaxC == DANET_WAVLOSS_MAX_C, "csrc/wave_metric.h and include/danet_wavloss_hip.h disagree");

/* ------------------------------------------------------------------------------------- finalize */
__global__ __launch_bounds__(kThreads) void wavloss_fwd_kernel(int B, int C, const double* __restrict__ G,
                                                              double* __restrict__ loss_f64,
                                                              float* __restrict__ loss_f32,
                                                              double* __restrict__ per_utt,
                                                              int32_t* __restrict__ perm_idx,
                                                              int32_t* __restrict__ pair,
                                                              double* __restrict__ coef) {
  __shared__ double part[kWaves];
  const int M = 2 * C;
  double sum_sdr = 0.0, live_utts = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    PitSearch s;
    pit_search(G + (int64_t)b * M * M, M, C, s, NoBase());
    double u_sdr = 0.0;
    if (s.n_live > 0) {
      u_sdr = s.best_v / (double)s.n_live;
      sum_sdr += u_sdr;
      live_utts += 1.0;
    }
    per_utt[b] = u_sdr;
    perm_idx[b] = s.best;
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
    const unsigned perm = nth_perm(C, perm_idx[b]);
    unsigned pr = 0xffffu;                                     /* estimate j -> its live reference, 15: none */
    for (int i = 0; i < C; ++i)
      if (g[i * M + i] != 0.0) {
        const int sh = 4 * perm_at(perm, i);
        pr = (pr & ~(15u << sh)) | ((unsigned)i << sh);
      }
    for (int j = 0; j < C; ++j) {
      double alpha = 0.0, beta = 0.0;
      const int i = perm_at(pr, j) < C ? perm_at(pr, j) : -1;
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
  CHECK_ARG(B >= 1, "fwd: B must be >= 1 (got %d)", B);
  CHECK_ARG(C >= 1 && C <= kMaxC, "fwd: C must be in 1..%d (got %d)", kMaxC, C);
  CHECK_ARG((int64_t)B * 4 * C * C < ((int64_t)1 << 31), "fwd: B * 4 C^2 must be < 2^31");
  CHECK_ARG(G && loss_f64 && loss_f32 && per_utt && perm_idx && pair && coef, "fwd: null pointer");
  CHECK_ARG(((uintptr_t)G & 7) == 0 && ((uintptr_t)loss_f64 & 7) == 0 && ((uintptr_t)per_utt & 7) == 0 &&
                ((uintptr_t)coef & 7) == 0 && ((uintptr_t)loss_f32 & 3) == 0 &&
                ((uintptr_t)perm_idx & 3) == 0 && ((uintptr_t)pair & 3) == 0,
            "fwd: misaligned pointer (G, loss_f64, per_utt, coef 8-byte; loss_f32, perm_idx, pair 4-byte)");
  wavloss_fwd_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(B, C, G, loss_f64, loss_f32, per_utt, perm_idx,
                                                                    pair, coef);
  CHECK_LAUNCH();
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

  /* the forward transform of every frame of the tile */
  radix2_stages(frames, tw, nfr, N, a.log2_half);

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
  CHECK_ARG(B >= 1, "bwd: B must be >= 1 (got %d)", B);
  CHECK_ARG(C >= 1 && C <= kMaxC, "bwd: C must be in 1..%d (got %d)", kMaxC, C);
  CHECK_ARG(T >= 2, "bwd: T must be >= 2 (got %d)", T);
  CHECK_ARG(N >= 64 && N <= 1024 && (N & (N - 1)) == 0, "bwd: N must be a power of two in 64..1024 (got %d)", N);
  CHECK_ARG(S >= 1 && 2 * (int64_t)S <= N && 8 * (int64_t)S >= N, "bwd: S must be in [N/8, N/2] (got %d at N = %d)",
            S, N);
  CHECK_ARG(wav && pair && coef && window && out, "bwd: null pointer");
  CHECK_ARG(((uintptr_t)wav & 3) == 0 && ((uintptr_t)pair & 3) == 0 && ((uintptr_t)window & 3) == 0 &&
                ((uintptr_t)dloss & 3) == 0 && ((uintptr_t)coef & 7) == 0 && ((uintptr_t)phasor & 7) == 0 &&
                ((uintptr_t)out & (phasor ? 3 : 7)) == 0,
            "bwd: misaligned pointer (wav, pair, window, dloss 4-byte; coef, phasor 8-byte; out 8-byte in the "
            "complex form, 4-byte in the real one)");
  CHECK_ARG((int64_t)(T - 1) * S < ((int64_t)1 << 31), "bwd: (T - 1) * S must be < 2^31");
  CHECK_ARG((int64_t)T * (N / 2 + 1) < ((int64_t)1 << 31), "bwd: T * F must be < 2^31");
  const int frames = DANET_WAVLOSS_TILE_FRAMES(N);
  const int tiles = (T + frames - 1) / frames;
  const int64_t blocks = (int64_t)B * C * tiles;
  CHECK_ARG(blocks < ((int64_t)1 << 31), "bwd: B * C * tiles must be < 2^31");
  BwdArgs a;
  a.wav = wav; a.pair = pair; a.coef = coef; a.window = window; a.dloss = dloss;
  a.phasor = (const float2*)phasor; a.out = out;
  a.C = C; a.T = T; a.N = N; a.S = S;
  a.log2_half = log2_half(N);
  a.frames = frames; a.tiles = tiles;
  /* twiddles N + frames * N + span (frames - 1) * S + N floats: <= 3N/2 (1 + frames) <= 16384 at S = N/2 */
  const size_t lds_bytes = ((size_t)N + (size_t)frames * N + (size_t)(frames - 1) * S + N) * sizeof(float);
  wavloss_bwd_kernel<<<dim3((unsigned)blocks), kThreads, lds_bytes, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_WAVLOSS_OK;
}
