/*
 * libdanet_metric_hip.so (include/danet_metric_hip.h): the waveform metric of `valid` / `test` in three
 * small kernels -- overlap-add synthesis of the references and the estimates, their Gram matrices, and the
 * permutation search that turns a Gram matrix into SI-SDR and SI-SDRi.  gfx950, wave64.
 *
 * The numerics are those of csrc/wave_metric.h, which describes them; this file adds the entry points, the choice
 * of rows and the baseline.
 * danet_metric_synth.  2C signals per utterance, references first, every bin loaded as it is stored.
 * danet_metric_gram.  gram_pair over M <= 2 MAX_C rows.
 * danet_metric_si_sdr.  One workgroup; a thread per utterance runs pit_search and takes the baseline of SI-SDRi
 * from the same matrix by linearity: <m, m> = sum_kl G[k][l], <m, s_i> = sum_k G[k][i].  Two outputs per utterance.
 */
#include <hip/hip_runtime.h>

#include "danet_metric_hip.h"
#define DANET_EXT metric
#define DANET_EXT_UPPER METRIC
#include "ext_core.h"
#include "wave_metric.h"

static_assert(kMaxC == DANET_METRIC_MAX_C, "csrc/wave_metric.h and include/danet_metric_hip.h disagree");

/* ------------------------------------------------------------------------------------ synthesis */
struct MetricSynthArgs {
  const float2* ref;
  const float2* est;
  SynthArgs s;
};

__global__ __launch_bounds__(kThreads) void metric_synth_kernel(MetricSynthArgs a) {
  const int C = a.s.C, T = a.s.T, F = (a.s.N >> 1) + 1;
  const int sig = (int)(blockIdx.x / (unsigned)a.s.tiles);     /* b * 2C + m       */
  const int tile = (int)(blockIdx.x - (unsigned)sig * (unsigned)a.s.tiles);
  const int b = sig / (2 * C), m = sig - b * 2 * C;
  const float2* X = (m < C ? a.ref + ((int64_t)b * C + m) * T * F
                           : a.est + ((int64_t)b * C + (m - C)) * T * F);
  synth_tile(a.s, X, sig, tile, LoadBin());
}

extern "C" size_t danet_metric_workspace_bytes(int B, int C, int T, int N, int S) {
  if (!synth_shape_ok(B, C, T, N, S) || C > kMaxC) {
    set_error("workspace_bytes: need B >= 1, 1 <= C <= %d, T >= 2, N a power of two in 64..1024 and "
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
  CHECK_ARG(B >= 1 && C >= 1, "synth: B and C must be >= 1 (got %d, %d)", B, C);
  CHECK_ARG(T >= 2, "synth: T must be >= 2 (got %d)", T);
  CHECK_ARG(N >= 64 && N <= 1024 && (N & (N - 1)) == 0, "synth: N must be a power of two in 64..1024 (got %d)",
            N);
  CHECK_ARG(S >= 1 && 2 * (int64_t)S <= N && 8 * (int64_t)S >= N, "synth: S must be in [N/8, N/2] (got %d at N = %d)",
            S, N);
  CHECK_ARG(ref_c64 && est_c64 && window && wav, "synth: null pointer");
  CHECK_ARG(((uintptr_t)ref_c64 & 7) == 0 && ((uintptr_t)est_c64 & 7) == 0 && ((uintptr_t)window & 3) == 0 &&
                ((uintptr_t)wav & 3) == 0,
            "synth: misaligned pointer (ref, est 8-byte; window, wav 4-byte)");
  CHECK_ARG((int64_t)(T - 1) * S < ((int64_t)1 << 31), "synth: (T - 1) * S must be < 2^31");
  const MetricSynthArgs a = {(const float2*)ref_c64, (const float2*)est_c64, synth_args(C, T, N, S, window, wav)};
  const int64_t blocks = (int64_t)B * 2 * C * a.s.tiles;
  CHECK_ARG(blocks < ((int64_t)1 << 31), "synth: B * 2C * tiles must be < 2^31");
  metric_synth_kernel<<<dim3((unsigned)blocks), kThreads, synth_lds_bytes(a.s), (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_METRIC_OK;
}

/* ----------------------------------------------------------------------------------------- Gram */
__global__ __launch_bounds__(kThreads) void metric_gram_kernel(int M, int n_pairs, int64_t Ls,
                                                              const float* __restrict__ wav,
                                                              double* __restrict__ G) {
  __shared__ double part[kWaves];
  gram_pair(M, n_pairs, Ls, wav, G, part);
}

extern "C" int danet_metric_gram(void* stream, int B, int M, int64_t Ls, const float* wav, double* G) {
  CHECK_ARG(B >= 1, "gram: B must be >= 1 (got %d)", B);
  CHECK_ARG(M >= 1 && M <= 2 * kMaxC, "gram: M must be in 1..%d (got %d)", 2 * kMaxC, M);
  CHECK_ARG(Ls >= 1 && Ls < ((int64_t)1 << 31), "gram: Ls must be in [1, 2^31) (got %lld)", (long long)Ls);
  CHECK_ARG(wav && G, "gram: null pointer");
  CHECK_ARG(((uintptr_t)wav & 3) == 0 && ((uintptr_t)G & 7) == 0, "gram: misaligned pointer (wav 4-byte, G 8-byte)");
  const int n_pairs = M * (M + 1) / 2;
  CHECK_ARG((int64_t)B * n_pairs < ((int64_t)1 << 31), "gram: B * M * (M + 1) / 2 must be < 2^31");
  metric_gram_kernel<<<dim3((unsigned)((int64_t)B * n_pairs)), kThreads, 0, (hipStream_t)stream>>>(M, n_pairs, Ls, wav, G);
  CHECK_LAUNCH();
  return DANET_METRIC_OK;
}

/* ------------------------------------------------------------------------------------- finalize */
__global__ __launch_bounds__(kThreads) void metric_si_sdr_kernel(int B, int C, const double* __restrict__ G,
                                                                double* __restrict__ per_utt,
                                                                int32_t* __restrict__ perm_idx,
                                                                double* __restrict__ mean2) {
  __shared__ double part[kWaves];
  const int M = 2 * C;
  double sum_sdr = 0.0, sum_imp = 0.0, live_utts = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double* g = G + (int64_t)b * M * M;
    double mm = 0.0;
    for (int k = 0; k < C; ++k)
      for (int l = 0; l < C; ++l) mm += g[k * M + l];
    PitSearch s;
    pit_search(g, M, C, s, [&](int i, double a) {
      double ms = 0.0;
      for (int k = 0; k < C; ++k) ms += g[k * M + i];
      return sdr_db(a, mm, ms);
    });
    double u_sdr = 0.0, u_imp = 0.0;
    if (s.n_live > 0) {
      u_sdr = s.best_v / (double)s.n_live;
      u_imp = pit_improvement(s, C) / (double)s.n_live;
      sum_sdr += u_sdr;
      sum_imp += u_imp;
      live_utts += 1.0;
    }
    per_utt[2 * (int64_t)b] = u_sdr;
    per_utt[2 * (int64_t)b + 1] = u_imp;
    perm_idx[b] = s.best;
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
  CHECK_ARG(B >= 1, "si_sdr: B must be >= 1 (got %d)", B);
  CHECK_ARG(C >= 1 && C <= kMaxC, "si_sdr: C must be in 1..%d (got %d)", kMaxC, C);
  CHECK_ARG(G && per_utt && perm_idx && mean2, "si_sdr: null pointer");
  CHECK_ARG(((uintptr_t)G & 7) == 0 && ((uintptr_t)per_utt & 7) == 0 && ((uintptr_t)mean2 & 7) == 0 &&
                ((uintptr_t)perm_idx & 3) == 0,
            "si_sdr: misaligned pointer (G, per_utt, mean2 8-byte; perm_idx 4-byte)");
  metric_si_sdr_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(B, C, G, per_utt, perm_idx, mean2);
  CHECK_LAUNCH();
  return DANET_METRIC_OK;
}
