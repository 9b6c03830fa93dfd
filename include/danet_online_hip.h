/*
 * libdanet_online_hip.so -- C ABI of the online attractor estimator (INFER_ESTIMATOR_METHOD = "online"): attractors
 * that are updated frame by frame from the frames seen so far, after the Online Deep Attractor Network (Han, Wang,
 * Luo, Mesgarani 2019), instead of ONE attractor set per recording formed from all of its frames.  The per-frame
 * update is the EM step the `anchor` estimator ends with, on running sums with a forgetting factor.  No parameters
 * of its own, no training, no backward.  gfx950 only.
 *
 * WHAT IT IS AND IS NOT.  The estimator is causal IN THE EMBEDDING: frame t's attractors depend on the embedding of
 * frames <= t only, and the state travels in and out of danet_online_scan, so a block-wise caller needs nothing more
 * from this library.  It does NOT make the model streaming: the encoders `lstm-orig` and `bilstm-orig` centre their
 * input and their last layer over the whole utterance and their recurrent entry points start from a zero state, so
 * the embedding itself still depends on every frame.  End-to-end streaming needs a causal encoder too.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other eighteen libraries stay as they are.
 * Same conventions as include/danet_phase_hip.h: caller-owned DEVICE pointers, `stream` a hipStream_t passed as
 * void*, 0 = DANET_ONLINE_OK and negative = error with a thread-local message in danet_online_last_error(),
 * asynchronous launches, no process environment read, no allocation, no atomics: every output element is written
 * once by one thread with an ordinary vector store, so repeated calls agree bit for bit.  No waiting between
 * workgroups, no persistent grid: the scan is one workgroup per utterance that walks its frames.
 *
 * THE RULE.
 *
 * Inputs per utterance.  embedding V float32 [T][F][E]; weights W float32 [T][F] (the front-end's mix_pwr); initial
 * attractors A0 float32 [C][E]; the activation act (0 = softmax over C, 1 = sigmoid: the separator's own); the
 * forgetting factor lambda, a double with 0 < lambda <= 1; the hold length T0 >= 1; eps >= 0; t_first >= 0, the
 * absolute index of the call's first frame.
 *
 * State per utterance, float64: S[C][E], n[C] and the attractors in force A[C][E] (float32 values, stored widened).
 * danet_online_init sets S = 0, n = 0, A = A0.
 *
 * For each frame t, in order:
 *   1. l[f][c] = V[t][f] . A[c]: float32 fused multiply-adds, e ascending from +0.
 *   2. m[f][c] = act(l[f]).  Softmax subtracts the row maximum, takes expf, sums in ascending c and divides, as
 *      danet_separate_fwd does; sigmoid is 1 / (1 + expf(-l)).
 *   3. s[c][e] = sum_f W[t][f] m[f][c] V[t][f][e] and q[c] = sum_f W[t][f] m[f][c]: the product W m is rounded to
 *      float32 once and serves both; float32 sums in one fixed order over f (SUMMATION ORDER, below).  The order is a
 *      function of F alone (and of E for s): it does not depend on B, on T, or on how the frames are cut into calls.
 *   4. S = lambda S + s and n = lambda n + q, in float64 (one fused multiply-add each).
 *   5. If t >= T0 (absolute index): for every c with n[c] > eps, A[c] = (float)(S[c] / n[c]), the float64 quotient
 *      rounded once; the others keep their A[c].  If t < T0, A is unchanged: the hold, during which the state
 *      accumulates under A0.
 *   6. attr[t] = A: float32 [T][C][E], the trajectory.
 * Frame t's attractors depend on frames <= t only.  danet_online_scan runs the frames t_first .. t_first + T - 1 of
 * every utterance from `state` and leaves the state after the last frame in `state`: two consecutive calls over the
 * halves of a recording are BIT FOR BIT one call over the whole, and utterance b alone is bit for bit utterance b
 * inside a larger batch.
 *
 * STATE LAYOUT.  danet_online_state_bytes(C, E) = 8 (2 C E + C) bytes per utterance, float64, in this order:
 *     S  [C][E]     n  [C]     A  [C][E]
 * The utterances of a batch follow each other without padding: state is float64 [B][2 C E + C].
 *
 * SUMMATION ORDER (256 threads, thread k = 64 wave + lane).
 *   q: thread k adds W m of its bins f = k, k + 256, ... in ascending f; the 64 lanes of a wave are summed by the
 *      fixed butterfly of data-parallel-primitive adds (lane ^ 1, lane ^ 2, the other quad, the other half row, row
 *      1 += row 0 and row 3 += row 2, rows 2 and 3 += row 1), and the four wave sums are added in ascending wave.
 *   s: P = max(E, 4), G = 256 / P rounded down.  Thread k < G P takes e = k mod P and the bins f = g, g + G, ...
 *      (g = k / P) with one fused multiply-add per bin from +0; the G partial sums of (c, e) are added in ascending g
 *      starting from +0.
 *
 * THE MASKS OF THE TRAJECTORY.  danet_online_separate writes out[b][c][t][f] = W[b][t][f] * act(V[b][t][f] .
 * attr[b][t][c]): the separator's formula with a per-frame attractor, and the same logit and activation code as
 * steps 1 and 2.  The scan does only what is serial; this second evaluation of the masks, with the UPDATED A_t, is
 * fully parallel.
 * ERROR BOUND of danet_online_separate against exact arithmetic on the same float32 inputs.  A logit formed by E
 * float32 fused multiply-adds is within dl = (E + 1) 2^-24 sum_e |v_e a_e| of exact.  A softmax or sigmoid output
 * moves by at most half the largest logit error (|d softmax_c| <= 2 m_c (1 - m_c) max_j |dl_j|, |d sigmoid| <=
 * dl / 4); the exponential, the sum, the division and the product with W add a few units of 2^-24, taken as 8:
 *     |out - exact| <= |W| (max_c dl_c / 2 + 8 * 2^-24).
 *
 * Envelope: B >= 1; 1 <= C <= DANET_ONLINE_MAX_C; 1 <= E <= DANET_ONLINE_MAX_E; 1 <= F <= DANET_ONLINE_MAX_F;
 * 1 <= T <= DANET_ONLINE_MAX_T per call (longer recordings go block by block); 0 <= t_first; the index products
 * B T F E, B C T F and B T C E below 2^31.  A violation returns DANET_ONLINE_ERR_ARG before any launch.
 */
#ifndef DANET_ONLINE_HIP_H
#define DANET_ONLINE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/online/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_ONLINE_ABI_VERSION 1

#define DANET_ONLINE_OK 0
#define DANET_ONLINE_ERR_ARG (-1)     /* bad shape or value / null or misaligned pointer */
#define DANET_ONLINE_ERR_LAUNCH (-2)  /* hipLaunch failure                               */

#define DANET_ONLINE_MAX_C 4
#define DANET_ONLINE_MAX_E 64
#define DANET_ONLINE_MAX_F 1025
#define DANET_ONLINE_MAX_T 65536

int danet_online_abi_version(void);
const char* danet_online_last_error(void);

/* Bytes of the state of ONE utterance (STATE LAYOUT above); (size_t)-1 with a message when C or E is outside the
 * envelope. */
size_t danet_online_state_bytes(int C, int E);

/* ONE pointwise launch: S = 0, n = 0, A = a0 for every utterance.  a0 float32 [B][C][E]; state float64
 * [B][2 C E + C].  B >= 1, C and E in the envelope, B (2 C E + C) below 2^31; no null pointer; a0 4-byte and state
 * 8-byte aligned.  A violation returns DANET_ONLINE_ERR_ARG and launches nothing.                             */
int danet_online_init(void* stream, int B, int C, int E, const float* a0, void* state);

/* ONE launch, one workgroup of 256 threads per utterance, which walks the T frames of the call (THE RULE).
 *
 * Per frame, three workgroup barriers.  (a) A thread per bin (bins f = k, k + 256, ...: at most five) forms the
 * logits against the attractor table in LDS (16-byte reads of the row when E is a multiple of 4, broadcast 16-byte
 * LDS reads of the table), the masks, W m into LDS as one 16-byte slot per bin, and the q partial sums (the DPP
 * butterfly).  The first 16 bytes of each of its rows of frame t + 1 are fetched into registers while frame t
 * reduces, which also brings the lines of that frame into the cache.  (b) Thread (e, g) contracts the bins
 * g, g + G, ... of column e against the W m slots: C accumulators per thread, consecutive lanes on consecutive
 * addresses.  (c) Thread c E + e adds the G partial sums, updates its S, its copy of n[c] and its A in registers
 * (float64), stores attr[t][c][e] and puts A back into the table.  Loads go out in batches (four 16-byte pieces of
 * a row in (a), eight column values in (b)) so that several are in flight per thread.  Nothing is held per thread
 * beyond 4 logits, 4 + 4 accumulators, five row heads and one such batch: no scratch anywhere in the envelope.
 *
 * embed float32 [B][T][F][E], w float32 [B][T][F], state float64 [B][2 C E + C] (read and written), attr float32
 * [B][T][C][E].  The envelope of THE RULE; act 0 or 1; 0 < lambda <= 1; T0 >= 1; eps >= 0 and finite; no null
 * pointer; embed 16-byte aligned when E is a multiple of 4 and 4-byte otherwise, w and attr 4-byte, state 8-byte
 * aligned.  A violation returns DANET_ONLINE_ERR_ARG and launches nothing.                                     */
int danet_online_scan(void* stream, int B, int C, int T, int F, int E, int act, double lambda, int T0,
                      int64_t t_first, double eps, const float* embed, const float* w, void* state, float* attr);

/* ONE launch, one workgroup of 256 threads per frame (b, t): the frame's attractors into LDS, then a thread per
 * bin.  w float32 [B][T][F], attr float32 [B][T][C][E], embed float32 [B][T][F][E], out float32 [B][C][T][F].  The
 * envelope of THE RULE; act 0 or 1; no null pointer; embed aligned as for danet_online_scan, the others 4-byte.
 * A violation returns DANET_ONLINE_ERR_ARG and launches nothing.                                             */
int danet_online_separate(void* stream, int act, int B, int C, int T, int F, int E, const float* w,
                          const float* attr, const float* embed, float* out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_ONLINE_HIP_H */
