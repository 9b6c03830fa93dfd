/*
 * libdanet_wavloss_hip.so -- C ABI of the waveform training loss (TRAIN_LOSS = "si-sdr"): minus the
 * scale-invariant SDR of the separated WAVEFORMS under the metric's own permutation rule, and its gradient with
 * respect to the estimates' spectra.  Two kernels: a finalize step on the Gram matrices that yields the loss and
 * what the backward pass needs, and the adjoint of the synthesis.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other nine libraries stay as they are.
 * Same conventions as include/danet_metric_hip.h: caller-owned DEVICE pointers, fp32 / interleaved complex64 /
 * float64, `stream` a hipStream_t passed as void*, 0 = DANET_WAVLOSS_OK and negative = error with a
 * thread-local message in danet_wavloss_last_error(), asynchronous launches, no process environment read, no
 * allocation.
 *
 * THE RULE.
 *
 * Synthesis and Gram.  Those of include/danet_metric_hip.h, applied exactly as the metric applies them: the
 * references S[B][C][T][F] and the estimates E[B][C][T][F] (the separated magnitudes with the mixture phase
 * re-attached, UNPERMUTED) are synthesised by danet_metric_synth into wav[B][2C][Ls], Ls = (T - 1) * S, the C
 * references of an utterance first, and danet_metric_gram turns them into G[B][2C][2C].  This library starts
 * from G and wav; wav must live until the backward pass has run.
 *
 * Forward finalize (float64), on G.  sdr(i, j), the live-reference rule (a reference with G[i][i] = 0 is silent
 * and takes no part), the permutation search over the live references and its tie rule (the first permutation in
 * itertools.permutations(range(C)) order) are those of danet_metric_si_sdr.  With p the permutation found,
 *     L = -( mean over the utterances that have a live reference of
 *            the mean over their live references i of sdr(i, p(i)) ),        L = 0 if no utterance has one:
 * L = -mean2[0] of the metric, from the same sums.  Per estimate j of utterance b:
 *     pair[b][j] = i when p(i) = j and reference i is live, -1 otherwise;
 *     coef[b][j] = (alpha, beta), the coefficients of dL / dy_j = alpha s_i + beta y_j  (s_i the paired
 *     reference's waveform, y_j the estimate's).  With a = G[i][i], b = G[C+j][C+j], c = G[i][C+j], t = c^2 / a,
 *     r = b - c^2 / a and K = 10 / ln 10:
 *         d sdr / d y_j = K (2 b / (c r)) s_i - K (2 / r) y_j,
 *         (alpha, beta) = -(1 / (n_live_b * n_utt_live)) * (2 K b / (c r), -2 K / r),
 *     n_live_b the live references of utterance b and n_utt_live the utterances that have one.  (alpha, beta) =
 *     (0, 0) when pair is -1, and when the pair's sdr was clamped: t <= 0, r <= 0 or |10 log10(t / r)| >= 100.
 *
 * Backward, for estimate (b, j) with i = pair[b][j]:
 *     u[n] = (alpha * wav[b][i][n] + beta * wav[b][C+j][n]) / wsum[n],  0 <= n < Ls: the combination and the
 *     division in float64, rounded ONCE to float32.  wsum[n] = sum_t w[k]^2 over 0 <= t < T with k = n - tS + N/2
 *     in [0, N), in ascending t, in float32: the synthesis rule's window sum.  u = 0 where wsum is 0, and
 *     outside [0, Ls).
 *     frame t, k < N:  f_t[k] = w[k] * u[tS - N/2 + k]                                       (float32)
 *     dX_t[f] = dloss * (c_f / N) * rfft_N(f_t)[f],  f <= N/2,  c_0 = c_{N/2} = 1 and c_f = 2 otherwise;
 *     the imaginary parts at bins 0 and N/2 are exactly 0.
 * Gradients are in the convention dL/dRe + i dL/dIm.  A row with pair = -1 (or a pair outside [0, C)) is all
 * zeros.  The float64 combination removes the cancellation rounding 2^-24 |alpha s| / |grad| of a float32 one.
 * With a phasor[B][T][F][2] = (cos phi, sin phi) of the mixture, the output is the real
 *     dsep[b][j][t][f] = cos(phi) Re(dX) + sin(phi) Im(dX),
 * the adjoint of the phase re-attach E = sep * (cos phi + i sin phi): the complex gradient never touches memory.
 */
#ifndef DANET_WAVLOSS_HIP_H
#define DANET_WAVLOSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/wavloss/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_WAVLOSS_ABI_VERSION 1

#define DANET_WAVLOSS_OK 0
#define DANET_WAVLOSS_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_WAVLOSS_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_WAVLOSS_MAX_C 4   /* DANET_METRIC_MAX_C: 24 permutations at the most */

/* Frames of one tile of danet_wavloss_bwd: min(32, (16384 - 3N/2) / (3N/2)) -- 32 up to N = 256, 20 at N = 512,
 * 9 at N = 1024.  A function of N alone (sized for S = N/2, the largest span), so that a test can aim at it. */
#define DANET_WAVLOSS_TILE_FRAMES(N) \
  ((16384 - 3 * (N) / 2) / (3 * (N) / 2) < 32 ? (16384 - 3 * (N) / 2) / (3 * (N) / 2) : 32)

int danet_wavloss_abi_version(void);
const char* danet_wavloss_last_error(void);

/* The forward finalize step of THE RULE on G[B][2C][2C], ONE launch of one workgroup of 256 threads.  A thread
 * takes the utterances tid, tid + 256, ... in order; the batch sums go over the fixed tree of danet_metric_gram
 * ((w0 + w1) + (w2 + w3) of the waves' butterflies), so loss_f64[0] is -mean2[0] of danet_metric_si_sdr bit for
 * bit and two calls agree bit for bit.  Outputs: loss_f64[1]; loss_f32[1], the same value rounded (the scalar
 * autograd carries); per_utt[B], the mean sdr over the live references of utterance b in dB (0 without one);
 * perm_idx[B], the index of p in itertools.permutations order (0 without a live reference); pair[B][C];
 * coef[B][C][2].
 * B >= 1; 1 <= C <= DANET_WAVLOSS_MAX_C; B * 4 C^2 < 2^31; no null pointer; G, loss_f64, per_utt, coef 8-byte and
 * loss_f32, perm_idx, pair 4-byte aligned.  A violation returns DANET_WAVLOSS_ERR_ARG and launches nothing.   */
int danet_wavloss_fwd(void* stream, int B, int C, const double* G, double* loss_f64, float* loss_f32,
                      double* per_utt, int32_t* perm_idx, int32_t* pair, double* coef);

/* The backward step of THE RULE, ONE launch: the adjoint of danet_metric_synth on the estimates' rows, fused
 * with the gradient combination, the window-sum division and (with a phasor) the adjoint of the phase re-attach.
 *
 * Geometry: one workgroup of 256 threads takes one estimate (b, j) and a tile of DANET_WAVLOSS_TILE_FRAMES(N)
 * consecutive frames.  It stages the tile's span of u ((frames - 1) * S + N samples) in LDS, each sample formed
 * from its own window sum; multiplies every frame by the window into LDS as N/2 complex values z[m] = f[2m] +
 * i f[2m+1] at bit-reversed positions; runs an N/2-point complex radix-2 forward FFT in place over all frames of
 * the tile at once (one barrier per stage, 2 + log2(N/2) barriers per tile); and in the split step turns
 * Z[k], Z[N/2 - k] into bin k, scales it and writes it.  Twiddles are COMPUTED IN THE KERNEL, once per
 * workgroup, into LDS (sincospif(2j/N), j < N/2); nothing is uploaded.  LDS: at most 64 KiB.  Every output
 * element is written once by one thread's own sum, with ordinary vector stores: no atomics, no
 * read-modify-write on memory, so repeated launches agree bit for bit.  The reference row of an estimate is
 * SELECTED among the C rows that are all read, so every address is a function of the arguments below alone;
 * nothing the device alone can see (pair, coef, the waveforms, the window, dloss, the phasor) can move a read or
 * a write.
 *
 * wav float32 [B][2C][(T - 1) * S] (danet_metric_synth's output); pair int32 [B][C]; coef float64 [B][C][2];
 * window N float32; dloss a DEVICE float scalar or null (= 1); phasor float32 [B][T][F][2] or null.
 * out: with phasor null, complex64 dX[B][C][T][F] (interleaved); otherwise float32 dsep[B][C][T][F].  F = N/2 + 1.
 * The envelope of danet_metric_synth: B >= 1; 1 <= C <= DANET_WAVLOSS_MAX_C; T >= 2; N a power of two in
 * 64..1024; N/8 <= S <= N/2; (T - 1) * S, T * F and B * C * tiles < 2^31; wav, pair, window, dloss 4-byte, coef and
 * phasor 8-byte aligned; out 8-byte aligned in the complex form and 4-byte in the real one.  A violation returns
 * DANET_WAVLOSS_ERR_ARG and launches nothing.                                                            */
int danet_wavloss_bwd(void* stream, int B, int C, int T, int N, int S, const float* wav, const int32_t* pair,
                      const double* coef, const float* window, const float* dloss, const float* phasor,
                      float* out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_WAVLOSS_HIP_H */
