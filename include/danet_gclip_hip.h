/*
 * libdanet_gclip_hip.so -- C ABI of global-norm gradient clipping (GRAD_CLIP_NORM): the L2 norm of the whole flat
 * gradient and the clip + TF1-Adam update scaled by the clip coefficient, which never leaves the device.  Two
 * launches per step: a sum of squares into per-workgroup partials, and the optimizer kernel of the core library
 * with a prologue that turns the partials into the gradient factor.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other eleven libraries stay as they are.
 * Same conventions as include/danet_mix_hip.h: caller-owned DEVICE pointers, fp32 / float64, `stream` a
 * hipStream_t passed as void*, 0 = DANET_GCLIP_OK and negative = error with a thread-local message in
 * danet_gclip_last_error(), asynchronous launches, no process environment read, no allocation.
 *
 * THE RULE.  g is the flat gradient of n float32 values after the all-reduce, s the grad_scale the reduction
 * returns (1 / world), M the key's value (max_norm).
 *
 * Sum of squares.  S = sum(g_i^2).  Every square is formed in float64, where the square of a float32 is exact;
 * the sum is float64 over a fixed tree:
 *     slice(n)    = max(4096, 4 * ceil(ceil(n / 1024) / 4))        elements of one partial, a multiple of 4
 *     partials(n) = ceil(n / slice(n))                              1 <= partials(n) <= 1024
 *     terms(n)    = ceil(slice(n) / 1024) + 2                       terms one thread adds serially, at the most
 * Partial p covers g[p * slice, min(n, (p + 1) * slice)).  With head = the 0..3 elements in front of the first
 * 16-byte boundary of the partial's span, its 16-byte vectors q = 0, 1, ... behind them and the 0..3 tail
 * elements, thread t of 256 adds, in this order, into an accumulator that starts at 0: the vectors q = t, t + 256,
 * ..., each as (x0^2 + x1^2) + (x2^2 + x3^2); head element t (t < head); tail element t (t < tail).  The 256
 * accumulators are added by a butterfly over the 64 lanes of a wave (partner lane ^ 32, 16, 8, 4, 2, 1 in turn) and
 * (w0 + w1) + (w2 + w3) over the four waves.  The head of every partial is that of g itself (slice is a multiple
 * of 4), so a partial depends on the values, n and the address of g modulo 16 bytes, and on nothing else.
 * S = the sum of the partials: thread t of 256 adds the partials t, t + 256, t + 512, t + 768 (those below
 * partials(n)) in this order into an accumulator that starts at 0, then the same butterfly and (w0 + w1) + (w2 + w3).
 * Longest chain of additions: terms(n) + 2 + 8 in a partial, 4 + 8 over the partials: terms(n) + 22.
 *
 * Norm.         norm = |s| * sqrt(S)                                                     (float64)
 * Coefficient.  coef = M / (norm + 1e-6) if norm + 1e-6 > M, else 1                       (float64)
 *               torch.nn.utils.clip_grad_norm_.  A NaN norm compares false and gives 1; an infinite norm gives 0.
 * Factor.       k = (float)((double)s * coef): one rounding.
 * Update.       Exactly the element update of danet_adam_clip_step (include/danet_hip.h) with grad_scale = k:
 *               g' = g_i * k; with clip > 0, g' = NaN if g' is NaN, else min(max(g', -clip), clip); then TF1-Adam.
 *               The value clip is applied AFTER the scaling.  A NaN gradient element stays NaN in its own element
 *               (and makes norm NaN, coef 1); there is no skip logic.
 */
#ifndef DANET_GCLIP_HIP_H
#define DANET_GCLIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/gclip/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_GCLIP_ABI_VERSION 1

#define DANET_GCLIP_OK 0
#define DANET_GCLIP_ERR_ARG (-1)     /* bad size / null or misaligned pointer / bad max_norm */
#define DANET_GCLIP_ERR_LAUNCH (-2)  /* hipLaunch failure                                    */

#ifndef DANET_GCLIP_MAX_PARTIALS       /* (tools/bench_gclip.py builds variants with 256 and 512 to measure the choice) */
#define DANET_GCLIP_MAX_PARTIALS 1024
#endif
#define DANET_GCLIP_MIN_SLICE 4096
#define DANET_GCLIP_MAX_N ((int64_t)1 << 40)

int danet_gclip_abi_version(void);
const char* danet_gclip_last_error(void);

/* partials(n) of THE RULE, a pure function; 0 (and a message) for n < 1 or n > DANET_GCLIP_MAX_N. */
int danet_gclip_partials(int64_t n);

/* The sum of squares of THE RULE, ONE launch of partials(n) workgroups of 256 threads: workgroup p writes
 * partials_f64[p], one float64, with an ordinary vector store from one thread.  16-byte loads over the aligned
 * middle of the span, four in flight per thread.  No atomic, no read-modify-write: repeats agree bit for bit.
 * 1 <= n <= DANET_GCLIP_MAX_N; no null pointer; grad 4-byte and partials_f64 8-byte aligned; n_partials ==
 * danet_gclip_partials(n).  A violation returns DANET_GCLIP_ERR_ARG and launches nothing.                  */
int danet_gclip_sumsq(void* stream, int64_t n, const float* grad, double* partials_f64, int n_partials);

/* Norm, coefficient, factor and update of THE RULE, ONE launch with the grid of danet_adam_clip_step
 * (min(2048, ceil(ceil(n / 4) / 256)) workgroups of 256 threads when theta, grad, m and v are all 16-byte aligned,
 * min(2048, ceil(n / 256)) otherwise; the same 16-byte path and the same tail).  EVERY workgroup first adds the
 * n_partials partials in the order of THE RULE (at most 8 KiB read), so all workgroups arrive at the same k bit
 * for bit; workgroup 0 writes norm_out_f64 = {norm, coef}.  The kernel boundary behind danet_gclip_sumsq is the
 * only synchronisation: no hand-off between workgroups, no fence, no spin.  zero_grad != 0: the gradient is
 * overwritten with 0 after use.  clip <= 0: no value clip.
 * 1 <= n <= DANET_GCLIP_MAX_N; no null pointer; theta, grad, m, v 4-byte and partials_f64, norm_out_f64 8-byte
 * aligned; max_norm finite and > 0; n_partials == danet_gclip_partials(n).  A violation returns
 * DANET_GCLIP_ERR_ARG and launches nothing.                                                                 */
int danet_gclip_adam_step(void* stream, int64_t n, float* theta, float* grad, float* m, float* v, float lr_t,
                          float beta1, float beta2, float eps, float clip, float grad_scale, int zero_grad,
                          double max_norm, const double* partials_f64, int n_partials, double* norm_out_f64);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_GCLIP_HIP_H */
