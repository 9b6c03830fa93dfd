/*
 * libdanet_phase_hip.so -- C ABI of the phase refinement of the separated spectra (PHASE_REFINE_ITERS): MISI,
 * multiple-input spectrogram inversion (Gunawan & Sen 2010), on the separated magnitudes.  Every separated spectrum
 * this project writes or scores carries the mixture's phase; K iterations of "synthesise every source, spread the
 * mixture residual over the sources, analyse again, keep the magnitudes and take the new phases" replace it by a
 * phase that is consistent with the magnitudes.  No parameters, no training.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other seventeen libraries stay as they are.
 * Same conventions as include/danet_metric_hip.h: caller-owned DEVICE pointers, fp32 / interleaved complex64,
 * `stream` a hipStream_t passed as void*, 0 = DANET_PHASE_OK and negative = error with a thread-local message in
 * danet_phase_last_error(), asynchronous launches, no process environment read, no allocation, no atomics: every
 * output element is written once by one thread with an ordinary vector store, so repeated calls agree bit for bit.
 * The plain form on purpose: two bounded launches per iteration, no waiting between workgroups, no persistent grid.
 *
 * THE RULE.
 *
 * Inputs.  est0 complex64 [B][C][T][F], today's separated spectra with any phase.  mixrows complex64
 * [B][Cm][T][F], Cm >= 1: the mixture spectrum is mix = mixrows[.][0] + mixrows[.][1] + ..., the rows in ascending
 * order starting from row 0, each part in float32 (Cm = 1: the mixture itself; Cm = C: the sources).  w float32
 * [N], the stride S, the iteration count K >= 0.  F = N/2 + 1, Ls = (T - 1) S.
 *
 * Magnitudes.  A = |est0| in the hypot form: sqrt(re^2 + im^2) taken in float64, where the squares are exact and
 * nothing overflows, and rounded ONCE to float32 (within 2^-24 A of the exact value).  Formed once; it never changes
 * afterwards.  X^0 = est0.
 *
 * Synthesis.  synth(.) is danet_metric_synth's rule (include/danet_metric_hip.h) and its code (synth_tile of
 * csrc/wave_metric.h, unchanged): frames by the inverse real FFT (the imaginary parts of bins 0 and N/2 ignored),
 * overlap-added with w in ascending t, divided by the overlap-added squared window, Ls samples.  y = synth(mix),
 * computed once.
 *
 * Iteration k -> k + 1.
 *   1. x_c = synth(X^k_c), c < C.
 *   2. z_c[n] = x_c[n] + (y[n] - (x_0[n] + x_1[n] + ...)) / C: the sum in ascending c starting from x_0, every
 *      operation in float32, the division by (float)C.
 *   3. Z_c[t][f] is the UNSCALED windowed real FFT of frame t of z_c: frame t covers the samples
 *      [tS - N/2, tS + N/2), zero outside [0, Ls), times w;  Z[f] = sum_k w[k] z[tS - N/2 + k] e^(-2 pi i f k / N).
 *      No 1 / sum(w) is applied: at this scale a consistent X maps to itself.  The imaginary parts of bins 0 and
 *      N/2 are exactly 0.
 *   4. m2 = re^2 + im^2 of Z in float32.  Where m2 > 0 and finite,
 *          X^{k+1} = A * (Z / sqrtf(m2))      (per part: a correctly rounded square root, division and product),
 *      and both parts are +0 there where A = 0.  Otherwise (m2 is 0, infinite or NaN) X^{k+1} = X^k at that bin,
 *      bit for bit.
 *   5. The imaginary parts the synthesis ignores (bins 0 and N/2) are whatever step 4 gives.
 * The result is X^K; K = 0 returns est0 bit for bit.
 *
 * Consequence.  After step 2 the refined sources sum to y, the mixture's waveform, in the time domain (up to
 * rounding): with a noisy mixture the noise is therefore shared among the refined sources.
 *
 * Envelope: that of danet_metric_synth -- B >= 1; T >= 2; N a power of two in 64..1024; N/8 <= S <= N/2 -- with
 * 1 <= C <= DANET_PHASE_MAX_C, 1 <= Cm <= DANET_PHASE_MAX_C, and both index products B * max(C, Cm) * T * F and
 * B * (C + 1) * Ls below 2^31.
 *
 * WORKSPACE.  One caller-owned buffer of danet_phase_workspace_bytes(B, C, T, N, S) bytes, 8-byte aligned, three
 * parts in this order, each rounded up to a multiple of 256 bytes:
 *     A    float32   [B][C][T][F]     the magnitudes
 *     mix  complex64 [B][T][F]        the mixture sum
 *     wav  float32   [B][C + 1][Ls]   rows 0..C-1: x_c of the current iterate; row C: y
 * danet_phase_init fills A, mix and row C of wav; danet_phase_synth rows 0..C-1; danet_phase_project reads A and
 * wav.  The contents must live from init to the last project call.
 */
#ifndef DANET_PHASE_HIP_H
#define DANET_PHASE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/phase/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_PHASE_ABI_VERSION 1

#define DANET_PHASE_OK 0
#define DANET_PHASE_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_PHASE_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_PHASE_MAX_C 4

/* Frames of one tile of danet_phase_project: min(32, (16384 - 3N/2) / (3N/2)) -- 32 up to N = 256, 20 at N = 512,
 * 9 at N = 1024 (DANET_WAVLOSS_TILE_FRAMES: the same LDS budget).  A function of N alone (sized for S = N/2, the
 * largest span), so that a test can aim at it. */
#define DANET_PHASE_TILE_FRAMES(N) \
  ((16384 - 3 * (N) / 2) / (3 * (N) / 2) < 32 ? (16384 - 3 * (N) / 2) / (3 * (N) / 2) : 32)

int danet_phase_abi_version(void);
const char* danet_phase_last_error(void);

/* Bytes of the WORKSPACE above; (size_t)-1 with a message when the shape is outside the envelope. */
size_t danet_phase_workspace_bytes(int B, int C, int T, int N, int S);

/* TWO launches.  The first is pointwise, a thread per element of est0: A = |est0| into the workspace, x = est0
 * (x == est0 is allowed: a thread writes the element it read), and, for the first B * T * F threads, the mixture sum
 * into the workspace.  The second synthesises y from the mixture sum into row C of wav (one workgroup of 256
 * threads per (utterance, tile of hops), the geometry of danet_metric_synth).
 * est0, x complex64 [B][C][T][F]; mixrows complex64 [B][Cm][T][F]; window N float32.  The envelope of THE RULE; no
 * null pointer; est0, mixrows, x, ws 8-byte and window 4-byte aligned.  A violation returns DANET_PHASE_ERR_ARG and
 * launches nothing.                                                                                          */
int danet_phase_init(void* stream, int B, int C, int Cm, int T, int N, int S, const float* est0,
                     const float* mixrows, const float* window, void* ws, float* x);

/* Step 1 of an iteration, ONE launch: the C rows x_c = synth(x[b][c]) of every utterance into rows 0..C-1 of wav,
 * one workgroup per (b, c, tile of hops).  Same envelope, pointers and errors as danet_phase_init.            */
int danet_phase_synth(void* stream, int B, int C, int T, int N, int S, const float* x, const float* window,
                      void* ws);

/* Steps 2-4 of an iteration, ONE launch, x updated in place.
 *
 * Geometry: one workgroup of 256 threads takes one signal (b, c) and a tile of DANET_PHASE_TILE_FRAMES(N)
 * consecutive frames.  It computes the N/2 twiddles e^(-2 pi i j / N) once (sincospif, into LDS); stages the tile's
 * span of z_c ((frames - 1) * S + N samples) in LDS, reading y and all C rows of the utterance (the row c is
 * SELECTED among the C that are all read, so every address is a function of the arguments alone); multiplies every
 * frame by the window into LDS as N/2 complex values f[2m] + i f[2m+1] at bit-reversed positions; runs an
 * N/2-point complex radix-2 forward FFT in place over all frames of the tile at once (one barrier per stage);
 * and in the split step turns Z[k], Z[N/2 - k] into bin k, normalises and stores.  LDS: N + frames * N +
 * (frames - 1) * S + N floats, at most 64 KiB.
 * Bin-to-lane mapping of the split step: the tile's nfr * F output bins are numbered idx = f * F + k, which is their
 * order in memory, and thread tid takes idx = tid, tid + 256, ...: the 64 lanes of a wave load A (256 bytes), load
 * the old x (512 bytes) and store x (and z_out) at 64 CONSECUTIVE complex64 elements, one full-width coalesced
 * access each; in LDS they read Z[k] at consecutive and Z[N/2 - k] at descending consecutive float2.  A thread reads
 * the old value of only the bin it writes, and the staging reads wav, never x: no workgroup reads what another
 * writes.
 *
 * x complex64 [B][C][T][F], read and written; z_out null or complex64 [B][C][T][F], which then receives Z (so that
 * the transform can be checked apart from the ill-conditioned normalisation).  Same envelope and errors as
 * danet_phase_init; x, z_out, ws 8-byte and window 4-byte aligned.                                             */
int danet_phase_project(void* stream, int B, int C, int T, int N, int S, const float* window, void* ws, float* x,
                        float* z_out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_PHASE_HIP_H */
