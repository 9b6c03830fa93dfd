/*
 * libdanet_metric_hip.so -- C ABI of the waveform metric of `valid` / `test` (EVAL_SI_SDR): scale-invariant
 * SDR of the separated WAVEFORMS and its improvement over the unprocessed mixture, in three small kernels
 * whose outputs can each be read back: waveforms, Gram matrices, decibels.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other seven libraries stay as they
 * are.  Same conventions as include/danet_mix_hip.h: caller-owned DEVICE pointers, fp32 / interleaved
 * complex64 / float64, `stream` a hipStream_t passed as void*, 0 = DANET_METRIC_OK and negative = error with a
 * thread-local message in danet_metric_last_error(), asynchronous launches, no process environment read, no
 * allocation.
 *
 * THE RULE.
 *
 * Inputs.  References S[B][C][T][F] (the batch valid_step receives) and estimates E[B][C][T][F] (the
 * separated magnitudes with the mixture phase re-attached, UNPERMUTED), complex64, F = N/2 + 1.
 *
 * Synthesis.  This is not utils.istft (which keeps the reference's semantics: it drops the last N/S frames
 * and divides by near-zero window sums at the edges).  Ls = (T - 1) * S samples in the coordinates of the
 * original signal; frame t of the STFT covers the samples [tS - N/2, tS + N/2).  With f_t = irfft_N(X_t)
 * and k = n - tS + N/2,
 *     y[n] = ( sum_t w[k] f_t[k] ) / ( sum_t w[k]^2 ),   over 0 <= t < T with 0 <= k < N,
 * the sums taken in ascending t, in float32 (a sample whose window sum is 0 is 0).  f_t follows the numpy
 * convention: the 1/N is included and the imaginary parts of bins 0 and N/2 are ignored.  Output: float32
 * wav[B][2C][Ls], the C references of an utterance first, then its C estimates.  The 1/sum(w) of the STFT
 * is not undone: the metric is invariant to it.  Every output sample sums its frames itself (gather): no
 * atomics, so two launches agree bit for bit.
 *
 * Gram.  G[b][i][j] = sum_n wav[b][i][n] * wav[b][j][n] over all 2C x 2C pairs: float64 products (exact)
 * and float64 sums over a fixed tree.  The upper triangle is computed, both halves are written.
 *
 * Finalize (float64).  For reference i and estimate j: a = G[i][i], b = G[C+j][C+j], c = G[i][C+j],
 * t = c^2 / a, r = b - t, and
 *     sdr(i, j) = -100 when t <= 0;  +100 when r <= 0 (and t > 0);  else 10 log10(t / r) clamped to
 *     [-100, 100].
 * A reference with a = 0 is silent and takes no part.  The permutation p maximises sum_i sdr(i, p(i)) over
 * the live references i (added in ascending i); ties go to the first permutation in
 * itertools.permutations(range(C)) order, the project's tie rule.  Baseline: the mixture m is the sum of the
 * references, so <m, s_i> = sum_k G[k][i] (ascending k) and <m, m> = sum_k sum_l G[k][l] (row by row);
 * base_i = sdr with (a, b, c) = (G[i][i], <m, m>, <m, s_i>).  Per utterance: the mean over the live
 * references of sdr(i, p(i)) and of sdr(i, p(i)) - base_i, (0, 0) when no reference is live.  Per batch: the
 * mean over the utterances that have a live reference, or 0 if there is none.
 */
#ifndef DANET_METRIC_HIP_H
#define DANET_METRIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/metric/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_METRIC_ABI_VERSION 1

#define DANET_METRIC_OK 0
#define DANET_METRIC_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_METRIC_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_METRIC_MAX_C 4   /* MAXC of csrc/pit_common.h: 24 permutations at the most */

int danet_metric_abi_version(void);
const char* danet_metric_last_error(void);

/* Bytes of one buffer that holds everything the three entry points write for one batch, each part at a
 * multiple of 256 bytes, in this order:
 *     wav      float32 [B][2C][Ls]      Ls = (T - 1) * S
 *     G        float64 [B][2C][2C]
 *     per_utt  float64 [B][2]
 *     mean2    float64 [2]
 *     perm_idx int32   [B]
 * i.e. the sum of the five sizes, each rounded up to a multiple of 256.  (size_t)-1 for a shape outside the
 * envelope of danet_metric_synth or C > DANET_METRIC_MAX_C.                                           */
size_t danet_metric_workspace_bytes(int B, int C, int T, int N, int S);

/* wav[b][c] = synthesis of ref_c64[b][c], wav[b][C + c] = synthesis of est_c64[b][c] (THE RULE), ONE launch.
 *
 * Geometry: one workgroup of 256 threads takes one signal and a tile of consecutive hops.  It turns the
 * frames the tile needs into real frames in LDS -- a REAL-input inverse transform: the N/2 + 1 bins are
 * folded into N/2 complex values (the split step), an N/2-point complex radix-2 inverse FFT runs in place,
 * and its interleaved output is the real frame -- and then every output sample gathers its frames.  The
 * frames that straddle a tile's edge (N/S - 1 of them when S divides N/2) are recomputed by the
 * neighbouring tile.  Twiddles are COMPUTED IN THE KERNEL, once per workgroup, into LDS
 * (sincospif(2j/N), j < N/2); nothing is uploaded.  Every value is written with ordinary vector stores.
 *
 * window: N float32 in device memory (the analysis window; it is only read).
 * B, C >= 1; T >= 2; N a power of two in 64..1024; N/8 <= S <= N/2 (S need not divide N); B * 2C * tiles
 * < 2^31; ref_c64, est_c64 8-byte and window, wav 4-byte aligned.  A violation returns DANET_METRIC_ERR_ARG and
 * launches nothing.  Nothing the device alone can see (the values of the spectra and of the window) can
 * move a read or a write: every address is a function of the arguments above.                        */
int danet_metric_synth(void* stream, int B, int C, int T, int N, int S, const float* ref_c64,
                       const float* est_c64, const float* window, float* wav);

/* G[b][i][j] = sum over n < Ls of wav[b][i][n] * wav[b][j][n] for b < B and i, j < M (M = 2C for the
 * metric), ONE launch: one workgroup of 256 threads per (b, i <= j).  A thread adds its products (sample
 * tid, tid + 256, ...) in float64 to four accumulators in rotation and joins them as (a0 + a1) + (a2 + a3);
 * the workgroup sum is a fixed butterfly over the 64 lanes of a wave and (w0 + w1) + (w2 + w3) over the four
 * waves.  The tree depends on Ls alone, so two calls agree bit for bit and G is symmetric bit for bit
 * (thread 0 writes G[b][i][j] and G[b][j][i]).  No term passes through more than Ls / 1024 + 11 additions.
 * B >= 1; 1 <= M <= 2 * DANET_METRIC_MAX_C; 1 <= Ls < 2^31; B * M * (M + 1) / 2 < 2^31; wav 4-byte, G
 * 8-byte aligned.  A violation returns DANET_METRIC_ERR_ARG and launches nothing.                            */
int danet_metric_gram(void* stream, int B, int M, int64_t Ls, const float* wav, double* G);

/* The finalize step of THE RULE on G[B][2C][2C], ONE launch of one workgroup: per_utt[b] = (SI-SDR,
 * SI-SDRi) of utterance b in dB, perm_idx[b] the index of its permutation in itertools.permutations order
 * (0 when no reference is live), mean2 = the batch means.  A thread takes the utterances tid, tid + 256,
 * ... in order; the batch sums go over the same fixed tree as danet_metric_gram.  The per-utterance outputs
 * exist for tests and for callers that want a histogram.
 * B >= 1; 1 <= C <= DANET_METRIC_MAX_C; G, per_utt, mean2 8-byte, perm_idx 4-byte aligned.  A violation
 * returns DANET_METRIC_ERR_ARG and launches nothing.                                                         */
int danet_metric_si_sdr(void* stream, int B, int C, const double* G, double* per_utt, int32_t* perm_idx,
                        double* mean2);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_METRIC_HIP_H */
