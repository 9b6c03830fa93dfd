/*
 * libdanet_neval_hip.so (include/danet_neval_hip.h): the waveform metric of a noisy `valid` / `test` sweep in three
 * small kernels -- overlap-add synthesis of the references, the estimates and the scaled noise, their Gram
 * matrices, and the permutation search that turns a Gram matrix into SI-SDR, SI-SDRi against the noisy mixture and
 * the realised source-to-noise ratio.  gfx950, wave64.
 *
 * The numerics are those of csrc/wave_metric.h, which describes them and which libdanet_metric_hip.so runs too;
 * tests/test_gpu_neval.py holds the two libraries together bit for bit.  This file adds the entry points and
 * danet_neval_synth.  2C + 1 signals per utterance: references, estimates, noise.  Every row reads its bins
 * through scaled(): fl(g * x), a product that is never contracted into the split step's sums (the sources' rows
 * take g = 1, which is exact).
 * danet_neval_gram.  gram_pair over M <= 2 MAX_C + 1 rows.
 * danet_neval_si_sdr.  One workgroup; a thread per utterance runs pit_search and takes the baseline of SI-SDRi
 * from the noisy mixture: <m, m> = (cc + 2 cn) + nn, <m, s_i> = sum_k G[k][i] + G[n][i]; nSNR = 10 log10(cc / nn)
 * is the third output per utterance.
 */
#include <hip/hip_runtime.h>

#include "danet_neval_hip.h"
#define DANET_EXT neval
#define DANET_EXT_UPPER NEVAL
#include "ext_core.h"
#include "wave_metric.h"

static_assert(kMaxC == DANET_NEVAL_MAX_C, "csrc/wave_metric.h and include/danet_neval_hip.h disagree");
static const int kMaxM = 2 * DANET_NEVAL_MAX_C + 1;

/* ------------------------------------------------------------------------------------ synthesis */
/* fl(g * x): one rounding of its own; with contraction off here the product carries no licence to fuse, so what
 * consumes it cannot fold it into an fma */
__device__ __forceinline__ float scaled(float g, float x) {
#pragma clang fp contract(off)
  return g * x;
}

struct LoadScaled {                                            /* a bin times the row's gain */
  float g;
  __device__ __forceinline__ float operator()(float x) const { return scaled(g, x); }
};

struct NevalSynthArgs {
  const float2* ref;
  const float2* est;
  const float2* noise;
  const float* gain;      /* [B] or null */
  SynthArgs s;
};

__global__ __launch_bounds__(kThreads) void neval_synth_kernel(NevalSynthArgs a) {
  const int C = a.s.C, T = a.s.T, F = (a.s.N >> 1) + 1;
  const int rows = 2 * C + 1;
  const int sig = (int)(blockIdx.x / (unsigned)a.s.tiles);     /* b * (2C + 1) + m */
  const int tile = (int)(blockIdx.x - (unsigned)sig * (unsigned)a.s.tiles);
  const int b = sig / rows, m = sig - b * rows;
  const float2* X = (m < C       ? a.ref + ((int64_t)b * C + m) * T * F
                     : m < 2 * C ? a.est + ((int64_t)b * C + (m - C)) * T * F
                                 : a.noise + (int64_t)b * T * F);
  const float g = (m == 2 * C && a.gain) ? a.gain[b] : 1.f;
  synth_tile(a.s, X, sig, tile, LoadScaled{g});
}

extern "C" size_t danet_neval_workspace_bytes(int B, int C, int T, int N, int S) {
  if (!synth_shape_ok(B, C, T, N, S) || C > kMaxC) {
    set_error("workspace_bytes: need B >= 1, 1 <= C <= %d, T >= 2, N a power of two in 64..1024 and "
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
  CHECK_ARG(B >= 1 && C >= 1, "synth: B and C must be >= 1 (got %d, %d)", B, C);
  CHECK_ARG(T >= 2, "synth: T must be >= 2 (got %d)", T);
  CHECK_ARG(N >= 64 && N <= 1024 && (N & (N - 1)) == 0, "synth: N must be a power of two in 64..1024 (got %d)",
            N);
  CHECK_ARG(S >= 1 && 2 * (int64_t)S <= N && 8 * (int64_t)S >= N, "synth: S must be in [N/8, N/2] (got %d at N = %d)",
            S, N);
  CHECK_ARG(ref_c64 && est_c64 && noise_c64 && window && wav, "synth: null pointer");
  CHECK_ARG(((uintptr_t)ref_c64 & 7) == 0 && ((uintptr_t)est_c64 & 7) == 0 && ((uintptr_t)noise_c64 & 7) == 0 &&
                ((uintptr_t)noise_gain & 3) == 0 && ((uintptr_t)window & 3) == 0 && ((uintptr_t)wav & 3) == 0,
            "synth: misaligned pointer (ref, est, noise 8-byte; noise_gain, window, wav 4-byte)");
  CHECK_ARG((int64_t)(T - 1) * S < ((int64_t)1 << 31), "synth: (T - 1) * S must be < 2^31");
  const NevalSynthArgs a = {(const float2*)ref_c64, (const float2*)est_c64, (const float2*)noise_c64, noise_gain,
                            synth_args(C, T, N, S, window, wav)};
  const int64_t blocks = (int64_t)B * (2 * (int64_t)C + 1) * a.s.tiles;
  CHECK_ARG(blocks < ((int64_t)1 << 31), "synth: B * (2C + 1) * tiles must be < 2^31");
  neval_synth_kernel<<<dim3((unsigned)blocks), kThreads, synth_lds_bytes(a.s), (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_NEVAL_OK;
}

/* ----------------------------------------------------------------------------------------- Gram */
__global__ __launch_bounds__(kThreads) void neval_gram_kernel(int M, int n_pairs, int64_t Ls,
                                                             const float* __restrict__ wav,
                                                             double* __restrict__ G) {
  __shared__ double part[kWaves];
  gram_pair(M, n_pairs, Ls, wav, G, part);
}

extern "C" int danet_neval_gram(void* stream, int B, int M, int64_t Ls, const float* wav, double* G) {
  CHECK_ARG(B >= 1, "gram: B must be >= 1 (got %d)", B);
  CHECK_ARG(M >= 1 && M <= kMaxM, "gram: M must be in 1..%d (got %d)", kMaxM, M);
  CHECK_ARG(Ls >= 1 && Ls < ((int64_t)1 << 31), "gram: Ls must be in [1, 2^31) (got %lld)", (long long)Ls);
  CHECK_ARG(wav && G, "gram: null pointer");
  CHECK_ARG(((uintptr_t)wav & 3) == 0 && ((uintptr_t)G & 7) == 0, "gram: misaligned pointer (wav 4-byte, G 8-byte)");
  const int n_pairs = M * (M + 1) / 2;
  CHECK_ARG((int64_t)B * n_pairs < ((int64_t)1 << 31), "gram: B * M * (M + 1) / 2 must be < 2^31");
  neval_gram_kernel<<<dim3((unsigned)((int64_t)B * n_pairs)), kThreads, 0, (hipStream_t)stream>>>(M, n_pairs, Ls, wav, G);
  CHECK_LAUNCH();
  return DANET_NEVAL_OK;
}

/* ------------------------------------------------------------------------------------- finalize */
__global__ __launch_bounds__(kThreads) void neval_si_sdr_kernel(int B, int C, const double* __restrict__ G,
                                                               double* __restrict__ per_utt,
                                                               int32_t* __restrict__ perm_idx,
                                                               double* __restrict__ mean3) {
  __shared__ double part[kWaves];
  const int M = 2 * C + 1, nz = 2 * C;
  double sum_sdr = 0.0, sum_imp = 0.0, sum_nsnr = 0.0, live_utts = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double* g = G + (int64_t)b * M * M;
    double cc = 0.0;
    for (int k = 0; k < C; ++k)
      for (int l = 0; l < C; ++l) cc += g[k * M + l];
    double cn = 0.0;
    for (int k = 0; k < C; ++k) cn += g[k * M + nz];
    const double nn = g[nz * M + nz];
    const double mm = (cc + 2.0 * cn) + nn;
    PitSearch s;
    pit_search(g, M, C, s, [&](int i, double a) {
      double ms = 0.0;
      for (int k = 0; k < C; ++k) ms += g[k * M + i];
      return sdr_db(a, mm, ms + g[nz * M + i]);
    });
    double u_sdr = 0.0, u_imp = 0.0, u_nsnr = 0.0;
    if (s.n_live > 0) {
      u_sdr = s.best_v / (double)s.n_live;
      u_imp = pit_improvement(s, C) / (double)s.n_live;
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
    perm_idx[b] = s.best;
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
  CHECK_ARG(B >= 1, "si_sdr: B must be >= 1 (got %d)", B);
  CHECK_ARG(C >= 1 && C <= kMaxC, "si_sdr: C must be in 1..%d (got %d)", kMaxC, C);
  CHECK_ARG(G && per_utt && perm_idx && mean3, "si_sdr: null pointer");
  CHECK_ARG(((uintptr_t)G & 7) == 0 && ((uintptr_t)per_utt & 7) == 0 && ((uintptr_t)mean3 & 7) == 0 &&
                ((uintptr_t)perm_idx & 3) == 0,
            "si_sdr: misaligned pointer (G, per_utt, mean3 8-byte; perm_idx 4-byte)");
  neval_si_sdr_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(B, C, G, per_utt, perm_idx, mean3);
  CHECK_LAUNCH();
  return DANET_NEVAL_OK;
}
