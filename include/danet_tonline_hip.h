/*
 * libdanet_tonline_hip.so -- C ABI of the truth-online estimator (TRAIN_ESTIMATOR_METHOD = "truth-online") and of the
 * backward of the per-frame-attractor separator: what a model that streams with INFER_ESTIMATOR_METHOD = "online"
 * (include/danet_online_hip.h) is TRAINED with.  After the Online Deep Attractor Network (Han, Wang, Luo, Mesgarani
 * 2019): during training the attractors of frame t are the running, forgetting-weighted means of the embedding under
 * the IDEAL assignment of the frames seen so far; the estimated assignment of danet_online_scan is used at test time
 * only.  That estimator is linear in the embedding, so its backward is exact and cheap.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other twenty libraries stay as they are.
 * Same conventions as include/danet_online_hip.h: caller-owned DEVICE pointers, `stream` a hipStream_t passed as
 * void*, 0 = DANET_TONLINE_OK and negative = error with a thread-local message in danet_tonline_last_error(),
 * asynchronous launches, no process environment read, no allocation, no atomics: every output element is written
 * once by one thread with an ordinary vector store, so repeated calls agree bit for bit.  No waiting between
 * workgroups, no persistent grid.  Everything proportional to B T F E is one workgroup per frame (b, t); the two
 * scans are one workgroup per utterance and touch T (C E + C) values, never the embedding.
 *
 * THE RULE.
 *
 * Inputs per utterance.  embedding V float32 [T][F][E]; source magnitudes P float32 [C][T][F] (batch layout
 * [B][C][T][F]); weights W float32 [T][F] (the front-end's mix_pwr); the forgetting factor lambda, a double with
 * 0 < lambda <= 1; the hold length T0 >= 1; eps >= 0.
 *
 *   1. The label k(t, f) is the lowest c that maximises P[c][t][f] (tf.argmax: the tie rule of
 *      danet_attractor_truth_fwd in its truth-weighted mode).
 *   2. Frame sums: s_t[c][e] = sum_{f: k(t,f) = c} W[t][f] V[t][f][e] and q_t[c] = sum_{f: k(t,f) = c} W[t][f]:
 *      float32, one fused multiply-add per bin for s and one add per bin for q, in one fixed order over f (SUMMATION
 *      ORDER, below).  The order is a function of F alone (and of E for s): it does not depend on B, on T, or on the
 *      utterance's position in the batch.  (A bin adds W V to its own source and 0 V to the others: a non-finite
 *      embedding value makes the sums of every source of its frame non-finite.)
 *   3. S_t = lambda S_{t-1} + s_t and n_t = lambda n_{t-1} + q_t, in float64 from zero, one fused multiply-add each:
 *      the accumulation of danet_online_scan step 4, hold frames included.
 *   4. tau(t) = min(max(t, T0 - 1), T - 1) and A_t[c] = (float)(S_tau[c] / (n_tau[c] + eps)): the quotient is formed
 *      in float64 and rounded once; the denominator is the reference's truth-weighted one (app/modules.py:482).
 *      Where n_tau[c] + eps is 0 (eps = 0 and no bin so far), A_t[c] = 0.  The hold mirrors inference: the first T0
 *      frames share the attractors formed from all of them, as `online` gives them the anchor estimator's A0 of those
 *      frames; from T0 - 1 on, frame t sees frames <= t.  A source with no bin so far has A = 0.
 *   5. attr[t] = A_t: float32 [T][C][E], the trajectory; den[t][c] = n_tau(t)[c] + eps: float64 [T][C], saved for the
 *      backward.
 *
 * Backward, given G = dL/dattr [T][C][E], with u0 = min(T0, T) - 1:
 *      H_u[c][e] = (sum_{t: tau(t) = u} G_t[c][e]) / (n_u[c] + eps) in float64: G_u / den[u] for u > u0, the sum of
 *      G_0 .. G_u0 (float64, ascending t from 0) over den[u0] for u = u0, 0 for u < u0; 0 where the denominator is 0.
 *      R_u = H_u + lambda R_{u+1} with R_T = 0: one float64 fused multiply-add per frame, u descending.
 *      dV[u][f][e] = W[u][f] * (float)R_u[k(u,f)][e].  There is no gradient to W or P.
 * It is exact for a source that is silent over a prefix of the recording: there H is G / eps, but R_u[c] is read only
 * by the bins of source c at frame u, and R_u holds the H of frames >= u only, so no bin carries it.
 *
 * The separator's backward.  The forward is danet_online_separate: out[c][t][f] = W act(V[t][f] . A_t[c]).  Given
 * D = dL/dout [C][T][F], with the masks m recomputed by the logit and activation code of danet_online_separate (float32
 * fused multiply-adds in ascending e from +0; softmax subtracts the row maximum) and g_c = W D_c:
 *      softmax: dl_c = m_c (g_c - sum_j m_j g_j), the sum by fused multiply-adds in ascending j from +0;
 *      sigmoid: dl_c = (m_c (1 - m_c)) g_c;
 *      dV[t][f][e] = sum_c dl_c A_t[c][e], fused multiply-adds in ascending c from +0;
 *      dA_t[c][e] = sum_f dl_c[f] V[t][f][e], in the order of s below.
 *
 * SUMMATION ORDER (256 threads, thread k = 64 wave + lane).
 *   q: thread k adds the W of its bins f = k, k + 256, ... to the sum of their source in ascending f; the 64 lanes of a
 *      wave are summed by the fixed butterfly of data-parallel-primitive adds of danet_online_hip.h (lane ^ 1, lane ^
 *      2, the other quad, the other half row, row 1 += row 0 and row 3 += row 2, rows 2 and 3 += row 1), and the four
 *      wave sums are added in ascending wave.
 *   s and dA: L = 4 when E is a multiple of 4 (a lane takes 16 bytes of a row), else 1; Q = E / L lanes per row,
 *      G = 256 / Q rounded down.  Thread k < G Q takes the columns L (k mod Q) .. + L - 1 of the bins f = g, g + G, ...
 *      (g = k / Q), with one fused multiply-add per bin and column from +0.  The G partial sums of (c, e) are added in
 *      blocks of 16: each block in ascending g from +0, then the block sums in ascending block from +0.
 *
 * ERROR BOUND of attr against exact arithmetic on the same float32 inputs, u = 2^-24.  A term of s passes through at
 * most N_s = ceil(F / G) + min(G, 16) + ceil(G / 16) float32 roundings, a term of q through N_q = ceil(F / 256) + 9.
 * With Sabs_t[c][e] and nabs_t[c] the running sums of step 3 taken over |W V| and |W| (exact), and tau = tau(t):
 *     |attr[t][c][e] - exact| <= u ((N_s + 2) Sabs_tau[c][e] + (N_q + 2) |A| nabs_tau[c]) / |n_tau[c] + eps| + u |A|
 * with A the exact quotient.  The first term is the float32 sums, to first order in the quotient; the 2 beside N
 * covers the second order and the float64 recurrence (at most 65536 steps of 2^-53 each, 2^-37 in all); the last term
 * is the one rounding of the quotient.
 *
 * Envelope, that of include/danet_online_hip.h (danet_online_separate is the forward of danet_tonline_separate_bwd):
 * B >= 1; 1 <= C <= DANET_TONLINE_MAX_C; 1 <= E <= DANET_TONLINE_MAX_E; 1 <= F <= DANET_TONLINE_MAX_F;
 * 1 <= T <= DANET_TONLINE_MAX_T per call; the index products B T F E, B C T F and B T C E below 2^31.  A violation
 * returns DANET_TONLINE_ERR_ARG before any launch.
 */
#ifndef DANET_TONLINE_HIP_H
#define DANET_TONLINE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/tonline/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                 */
#pragma GCC visibility push(default)

#define DANET_TONLINE_ABI_VERSION 1

#define DANET_TONLINE_OK 0
#define DANET_TONLINE_ERR_ARG (-1)     /* bad shape or value / null or misaligned pointer */
#define DANET_TONLINE_ERR_LAUNCH (-2)  /* hipLaunch failure                               */

#define DANET_TONLINE_MAX_C 4
#define DANET_TONLINE_MAX_E 64
#define DANET_TONLINE_MAX_F 1025
#define DANET_TONLINE_MAX_T 65536

int danet_tonline_abi_version(void);
const char* danet_tonline_last_error(void);

/* Steps 1 and 2.  ONE launch, one workgroup of 256 threads per frame (b, t), two workgroup barriers.  (a) A thread per
 * bin (bins f = k, k + 256, ...: at most five) forms the label, puts W into the label's entry of the bin's 16-byte
 * LDS slot and adds it to the q partial sums (the DPP butterfly).  (b) Thread (g, j) contracts the rows g, g + G, ...
 * against their slots: 16-byte row loads when E is a multiple of 4, four rows in flight, consecutive lanes on
 * consecutive addresses.  (c) Thread c E + e adds the G partial sums of (c, e) and stores s; thread c stores q.
 * 4 x 4 accumulators and four 16-byte pieces per thread, 33 KB of LDS: no scratch anywhere in the envelope.
 *
 * embed float32 [B][T][F][E], src_pwr float32 [B][C][T][F], w float32 [B][T][F] -> s float32 [B][T][C][E], q float32
 * [B][T][C].  The envelope of THE RULE; no null pointer; embed 16-byte aligned when E is a multiple of 4 and 4-byte
 * otherwise, the others 4-byte.  A violation returns DANET_TONLINE_ERR_ARG and launches nothing.             */
int danet_tonline_frame_sums(void* stream, int B, int C, int T, int F, int E, const float* embed,
                             const float* src_pwr, const float* w, float* s, float* q);

/* Steps 3 to 5.  ONE launch, one workgroup per utterance that walks the T frames: thread c E + e holds S[c][e] and a
 * copy of n[c] in float64 registers, loads eight frames of s and q ahead and stores attr[t][c][e]; the thread of e = 0
 * stores den[t][c].  The frames of the hold are stored when frame min(T0, T) - 1 has been reached.
 *
 * s float32 [B][T][C][E], q float32 [B][T][C] -> attr float32 [B][T][C][E], den float64 [B][T][C].  B >= 1, C, E and T
 * in the envelope, B T C E below 2^31; 0 < lambda <= 1; T0 >= 1; eps >= 0 and finite; no null pointer; s, q, attr
 * 4-byte and den 8-byte aligned.  A violation returns DANET_TONLINE_ERR_ARG and launches nothing.            */
int danet_tonline_scan(void* stream, int B, int C, int T, int E, double lambda, int T0, double eps, const float* s,
                       const float* q, float* attr, double* den);

/* The backward of steps 3 to 5.  ONE launch, one workgroup per utterance that walks the frames in reverse: thread
 * c E + e forms H and R in float64 (Backward, above; the hold -- every t < T0 feeds u = min(T0, T) - 1 -- is handled
 * here) and stores r[u][c][e] = (float)R_u[c][e].
 *
 * dattr float32 [B][T][C][E], den float64 [B][T][C] (as danet_tonline_scan left it) -> r float32 [B][T][C][E].  The
 * shapes and values of danet_tonline_scan; no null pointer; dattr, r 4-byte and den 8-byte aligned.  A violation
 * returns DANET_TONLINE_ERR_ARG and launches nothing.                                                        */
int danet_tonline_scan_bwd(void* stream, int B, int C, int T, int E, double lambda, int T0, const float* dattr,
                           const double* den, float* r);

/* dV = W * R[k].  ONE launch, one workgroup per frame (b, t): the frame's R into LDS, a thread per bin forms the label
 * again (step 1), then every thread stores 16 bytes (E a multiple of 4; else one value) of the frame's F E values at
 * a time, consecutive lanes on consecutive addresses.
 *
 * src_pwr float32 [B][C][T][F], w float32 [B][T][F], r float32 [B][T][C][E] -> dembed float32 [B][T][F][E], every
 * element written.  The envelope of THE RULE; no null pointer; dembed aligned as embed of danet_tonline_frame_sums,
 * the others 4-byte.  A violation returns DANET_TONLINE_ERR_ARG and launches nothing.                        */
int danet_tonline_sums_bwd(void* stream, int B, int C, int T, int F, int E, const float* src_pwr, const float* w,
                           const float* r, float* dembed);

/* The separator's backward.  ONE launch, one workgroup per frame (b, t), three barriers: the frame's attractors into
 * LDS; a thread per bin recomputes m, forms dl and puts it into the bin's 16-byte LDS slot; thread (g, j) loads its
 * piece of the rows g, g + G, ..., stores the same piece of dV and adds dl V to its partial sums of dA; thread c E + e
 * adds the G partial sums and stores dattr.  The embedding is read twice (logits, contraction; the second time
 * from the cache) and dV written once.
 *
 * act 0 = softmax over C, 1 = sigmoid.  w float32 [B][T][F], attr float32 [B][T][C][E], embed float32 [B][T][F][E],
 * dout float32 [B][C][T][F] -> dembed float32 [B][T][F][E], dattr float32 [B][T][C][E], every element written.  The
 * envelope of THE RULE; no null pointer; embed and dembed 16-byte aligned when E is a multiple of 4 and 4-byte
 * otherwise, the others 4-byte.  A violation returns DANET_TONLINE_ERR_ARG and launches nothing.             */
int danet_tonline_separate_bwd(void* stream, int act, int B, int C, int T, int F, int E, const float* w,
                               const float* attr, const float* embed, const float* dout, float* dembed,
                               float* dattr);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_TONLINE_HIP_H */
