/*
 * libdanet_neval_hip.so -- C ABI of the waveform metric of a NOISY `valid` / `test` sweep (NOISE_EVAL_DIR with
 * EVAL_SI_SDR): scale-invariant SDR of the separated waveforms, its improvement over the mixture THE MODEL WAS
 * GIVEN -- the sources plus a noise component that is not a target -- and the realised source-to-noise ratio, in
 * three small kernels whose outputs can each be read back: waveforms, Gram matrices, decibels.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other libraries stay as they are, and
 * libdanet_metric_hip.so (include/danet_metric_hip.h), whose rule this one extends by one row, is not touched.  Same
 * conventions as include/danet_metric_hip.h: caller-owned DEVICE pointers, fp32 / interleaved complex64 / float64,
 * `stream` a hipStream_t passed as void*, 0 = DANET_NEVAL_OK and negative = error with a thread-local message in
 * danet_neval_last_error(), asynchronous launches, no process environment read, no allocation.
 *
 * THE RULE.  C sources, M = 2C + 1 signals per utterance, n = 2C the index of the noise row.
 *
 * Inputs.  References S[B][C][T][F] (the clean sources valid_step receives), estimates E[B][C][T][F] (the
 * separated magnitudes with the phase of the NOISY mixture re-attached, UNPERMUTED), the noise Z[B][T][F], all
 * complex64 with F = N/2 + 1, and a float32 gain g[B] (a null pointer: g = 1).
 *
 * Synthesis.  The synthesis of include/danet_metric_hip.h, unchanged: Ls = (T - 1) * S samples, frame t covers the
 * samples [tS - N/2, tS + N/2), and with f_t = irfft_N(X_t) and k = n - tS + N/2
 *     y[n] = ( sum_t w[k] f_t[k] ) / ( sum_t w[k]^2 ),   over 0 <= t < T with 0 <= k < N,
 * the sums in ascending t, in float32 (a sample whose window sum is 0 is 0); the 1/N is included and the imaginary
 * parts of bins 0 and N/2 are ignored.  Output: float32 wav[B][M][Ls]: rows 0..C-1 the references, rows C..2C-1 the
 * estimates, row n the same synthesis of the spectra (fl(g re Z), fl(g im Z)) -- each product rounded ON ITS OWN to
 * float32 and never contracted into the arithmetic that follows: exactly the term danet_noise_frontend_fwd
 * (include/danet_noise_hip.h) adds to the mixture.  Every output sample sums its frames itself (gather): no
 * atomics, so two launches agree bit for bit.
 *
 * Gram.  G[b][i][j] = sum_n wav[b][i][n] * wav[b][j][n] over all M x M pairs: float64 products (exact) and float64
 * sums over a fixed tree.  The upper triangle is computed, both halves are written.
 *
 * Finalize (float64).  sdr(a, b, c): t = c^2 / a, r = b - t, and
 *     sdr = -100 when t <= 0;  +100 when r <= 0 (and t > 0);  else 10 log10(t / r) clamped to [-100, 100].
 * For reference i and estimate j, sdr(i, j) = sdr(G[i][i], G[C+j][C+j], G[i][C+j]).  A reference with G[i][i] = 0 is
 * silent and takes no part.  The permutation p maximises sum_i sdr(i, p(i)) over the live references i (added in
 * ascending i); ties go to the first permutation in itertools.permutations(range(C)) order.  All of that reads the
 * 2C x 2C block alone and is the rule of include/danet_metric_hip.h.
 * Baseline: the mixture is m = sum of the references + the noise row.  With
 *     cc = sum_k sum_l G[k][l] over k, l < C (row by row),  cn = sum_k G[k][n] (ascending k < C),  nn = G[n][n]:
 *     <m, m>   = (cc + 2 cn) + nn
 *     <m, s_i> = (sum_k G[k][i], ascending k < C) + G[n][i]
 *     base_i   = sdr(G[i][i], <m, m>, <m, s_i>).
 * nSNR, the ratio of the clean mixture to the noise: -100 when cc <= 0; +100 when nn <= 0 (and cc > 0); else
 * 10 log10(cc / nn) clamped to [-100, 100].
 * Per utterance: (the mean over the live references of sdr(i, p(i)), the mean of sdr(i, p(i)) - base_i, nSNR), or
 * (0, 0, 0) when no reference is live.  Per batch: the means of the three over the utterances that have a live
 * reference, or 0 if there is none.  With a zero noise row cn = nn = 0 and G[n][i] = 0, so the first two figures
 * equal danet_metric_si_sdr's on the 2C x 2C block as values.
 */
#ifndef DANET_NEVAL_HIP_H
#define DANET_NEVAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/neval/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_NEVAL_ABI_VERSION 1

#define DANET_NEVAL_OK 0
#define DANET_NEVAL_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_NEVAL_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_NEVAL_MAX_C 4   /* MAXC of csrc/pit_common.h: 24 permutations at the most, M <= 9 */

int danet_neval_abi_version(void);
const char* danet_neval_last_error(void);

/* Bytes of one buffer that holds everything the three entry points write for one batch, each part at a
 * multiple of 256 bytes, in this order (M = 2C + 1):
 *     wav      float32 [B][M][Ls]      Ls = (T - 1) * S
 *     G        float64 [B][M][M]
 *     per_utt  float64 [B][3]
 *     mean3    float64 [3]
 *     perm_idx int32   [B]
 * i.e. the sum of the five sizes, each rounded up to a multiple of 256.  (size_t)-1 for a shape outside the
 * envelope of danet_neval_synth or C > DANET_NEVAL_MAX_C.                                              */
size_t danet_neval_workspace_bytes(int B, int C, int T, int N, int S);

/* wav[b][c] = synthesis of ref_c64[b][c], wav[b][C + c] = synthesis of est_c64[b][c], wav[b][2C] = synthesis of
 * fl(noise_gain[b] * noise_c64[b]) (THE RULE), ONE launch.
 *
 * Geometry: that of danet_metric_synth.  One workgroup of 256 threads takes one signal and a tile of consecutive
 * hops; it turns the frames the tile needs into real frames in LDS -- the N/2 + 1 bins folded into N/2 complex
 * values (the split step), an N/2-point complex radix-2 inverse FFT in place, whose interleaved output is the real
 * frame -- and then every output sample gathers its frames.  Twiddles are computed in the kernel, once per
 * workgroup, into LDS (sincospif(2j/N), j < N/2); nothing is uploaded.  The arithmetic of a row is, expression for
 * expression, that of danet_metric_synth, so rows 0..2C-1 are the rows that entry point writes and the noise row at
 * a null gain is the row it writes for the same spectra.  Every value is written with ordinary vector stores.
 *
 * noise_c64: complex64 [B][T][F]; noise_gain: float32 [B] or NULL (= 1); window: N float32 in device memory.
 * B, C >= 1; T >= 2; N a power of two in 64..1024; N/8 <= S <= N/2 (S need not divide N); (T - 1) * S < 2^31;
 * B * (2C + 1) * tiles < 2^31; ref_c64, est_c64, noise_c64 8-byte and noise_gain, window, wav 4-byte aligned.  A
 * violation returns DANET_NEVAL_ERR_ARG and launches nothing.  Nothing the device alone can see (the values of
 * the spectra, the gains and the window) can move a read or a write: every address is a function of the
 * arguments above.                                                                                       */
int danet_neval_synth(void* stream, int B, int C, int T, int N, int S, const float* ref_c64, const float* est_c64,
                      const float* noise_c64, const float* noise_gain, const float* window, float* wav);

/* G[b][i][j] = sum over n < Ls of wav[b][i][n] * wav[b][j][n] for b < B and i, j < M (M = 2C + 1 for this
 * metric), ONE launch: one workgroup of 256 threads per (b, i <= j).  The tree of danet_metric_gram: a thread adds
 * its products (sample tid, tid + 256, ...) in float64 to four accumulators in rotation and joins them as
 * (a0 + a1) + (a2 + a3); the workgroup sum is a fixed butterfly over the 64 lanes of a wave and (w0 + w1) +
 * (w2 + w3) over the four waves.  The tree depends on Ls alone, so two calls agree bit for bit, G is symmetric bit
 * for bit (thread 0 writes G[b][i][j] and G[b][j][i]), and for M <= 8 the result is danet_metric_gram's.
 * B >= 1; 1 <= M <= 2 * DANET_NEVAL_MAX_C + 1; 1 <= Ls < 2^31; B * M * (M + 1) / 2 < 2^31; wav 4-byte, G 8-byte
 * aligned.  A violation returns DANET_NEVAL_ERR_ARG and launches nothing.                                    */
int danet_neval_gram(void* stream, int B, int M, int64_t Ls, const float* wav, double* G);

/* The finalize step of THE RULE on G[B][2C + 1][2C + 1], ONE launch of one workgroup: per_utt[b] = (SI-SDR,
 * SI-SDRi, nSNR) of utterance b in dB, perm_idx[b] the index of its permutation in itertools.permutations order
 * (0 when no reference is live), mean3 = the batch means.  A thread takes the utterances tid, tid + 256, ... in
 * order; the batch sums go over the same fixed tree as danet_neval_gram.
 * B >= 1; 1 <= C <= DANET_NEVAL_MAX_C; G, per_utt, mean3 8-byte, perm_idx 4-byte aligned.  A violation returns
 * DANET_NEVAL_ERR_ARG and launches nothing.                                                                  */
int danet_neval_si_sdr(void* stream, int B, int C, const double* G, double* per_utt, int32_t* perm_idx,
                       double* mean3);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_NEVAL_HIP_H */
