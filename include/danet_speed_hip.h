/*
 * libdanet_speed_hip.so -- C ABI of the speed perturbation of the `wavdir` dataset
 * (SPEED_PERTURB_RANGE): every utterance of a ragged batch resampled by its own rational factor
 * p / 512 from the device-resident pool into a scratch waveform buffer, in one launch, in front of
 * danet_prep_stft_batch.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the core, conv, dropout, prep and mix ABIs stay
 * as they are.  Same conventions as include/danet_prep_hip.h: caller-owned DEVICE pointers, fp32,
 * `stream` a hipStream_t passed as void*, 0 = DANET_SPEED_OK and negative = error with a thread-local
 * message in danet_speed_last_error(), asynchronous launches, no process environment read, no
 * allocation.  The library contains no transcendental math: the filter table is an INPUT.
 *
 * THE RULE.  Q = DANET_SPEED_PHASES = 512 phases, Z = 16, 2Z = DANET_SPEED_TAPS = 32 taps,
 * P = SPEED_PERTURB_RANGE, 0 <= P <= 0.25.
 *
 *   Speed of an utterance (host side), drawn anew for every utterance of every train batch:
 *     u = rng.uniform(-P, P);  p = Q + rint(Q * u), clipped to [Q - floor(Q*P), Q + floor(Q*P)].
 *     The speed factor is p / Q: larger than Q means faster and shorter.
 *   Output length of an L-sample utterance: L' = floor((L - 1) * Q / p) + 1, in 64-bit integers
 *     (L' = L at p = Q; L = 1000, p = 576 gives 889).  An utterance whose L' would fall below FFT_SIZE
 *     keeps p = Q.
 *   Output sample n, 0 <= n < L':
 *     m = (n * p) div Q and phi = (n * p) mod Q, exact 64-bit integer arithmetic;
 *     y[n] = sum over j in [0, 2Z) of tab[phi][j] * x[m + j - (Z - 1)], x outside [0, L) zero;
 *     float32 products, float32 accumulation (the kernel: one chain of fused multiply-adds, j
 *     ascending, from +0).
 *   The table, tab[phi][j] = h(j - (Z - 1) - phi / Q), float32 [Q][2Z] = 64 KB:
 *     h(t) = fc * sinc(fc * t) * 0.5 * (1 + cos(pi * t / Z)) for |t| < Z, else 0;
 *     sinc(a) = sin(pi a) / (pi a), sinc(0) = 1;  fc = 1 / (1 + P).  sin(pi a) is evaluated as
 *     (-1)^k sin(pi (a - k)) with k = rint(a), so that it is exactly 0 at an integer a; a zero tap is +0.
 *     ONE band limit for the whole run: the fastest draw does not alias, and bandwidth does not
 *     correlate with the drawn speed.  The Python layer computes it in float64 numpy, rounds it once to
 *     float32 and uploads it once per dataset; the host restatement and the kernel use the same bits.
 *   Consequence: at P = 0, fc = 1 and row 0 of the table is the unit impulse at j = Z - 1, and every p
 *     equals Q, so phi = 0 and m = n for every n: the output equals the input bit for bit (every finite
 *     input; a negative zero comes out as +0).
 *
 * Draws (host side) come from a numpy RandomState the dataset owns per subset, seeded by
 * (dist.shard_seed(1337), subset index, 1): a stream of its own beside the mix stream (seeded without the
 * trailing 1), never python's `random` or np.random.  Only `train` is perturbed; its stream runs on across
 * epochs; ranks draw differently.  One uniform() call draws a whole batch, before the batch's pads and
 * crop are planned on the new lengths L'.
 */
#ifndef DANET_SPEED_HIP_H
#define DANET_SPEED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/speed/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_SPEED_ABI_VERSION 1

#define DANET_SPEED_OK 0
#define DANET_SPEED_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_SPEED_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_SPEED_PHASES 512       /* Q                                       */
#define DANET_SPEED_TAPS 32          /* 2Z                                      */
#define DANET_SPEED_P_MIN (DANET_SPEED_PHASES - DANET_SPEED_PHASES / 4)
#define DANET_SPEED_P_MAX (DANET_SPEED_PHASES + DANET_SPEED_PHASES / 4)

/* one row of the descriptor table (40 bytes, device memory, 8-byte aligned) */
typedef struct danet_speed_utt {
  int64_t src_offset;  /* first sample of the utterance, in floats from `src_pool`      */
  int64_t src_length;  /* L, samples                                                    */
  int64_t dst_offset;  /* first output sample, in floats from `dst`                     */
  int64_t dst_length;  /* output samples to write (the rule's L', or fewer)             */
  int32_t p;           /* speed numerator, DANET_SPEED_P_MIN <= p <= DANET_SPEED_P_MAX  */
  int32_t reserved;    /* 0                                                             */
} danet_speed_utt_t;

int danet_speed_abi_version(void);
const char* danet_speed_last_error(void);

/* L' = floor((L - 1) * Q / p) + 1; host only.  -1 (and a message) for L < 1, L > 2^40 or p outside
 * [DANET_SPEED_P_MIN, DANET_SPEED_P_MAX].                                                       */
int64_t danet_speed_out_len(int64_t L, int p);

/* dst[dst_offset_u + n] = y_u[n] of the rule, for u < n_utt and 0 <= n < dst_length_u, where x_u[i] =
 * src_pool[src_offset_u + i] for 0 <= i < src_length_u and zero elsewhere.  `table`: the float32
 * [DANET_SPEED_PHASES][DANET_SPEED_TAPS] filter table in device memory.
 *
 * Every float of every [dst_offset_u, dst_offset_u + dst_length_u) is written exactly once per launch
 * (the spans of different rows must not overlap) and nothing outside those spans is touched.  The value
 * of a sample depends on (x_u, p_u, n, table) alone: not on n_utt, not on the neighbouring rows, not on
 * the addresses.  No read-modify-write on memory is used, so two launches agree bit for bit.
 *
 * Geometry: a persistent grid of one 512-thread workgroup per compute unit (fewer for little work).  A
 * workgroup copies the table into LDS once (row pitch 36 floats: the 16-byte reads of lanes at
 * different phases spread over all banks), then walks the rows' tiles of 1024 outputs, taking every
 * tile whose running index is its own modulo the grid.  A tile's input span (at most 1024 * p / Q + 2Z
 * floats) is staged in LDS with 16-byte loads from 16-byte aligned addresses, 4-byte loads at the ends
 * of the utterance; lane l of the workgroup owns outputs l and l + 512 of the tile, 32 fused
 * multiply-adds each, so stores and staged reads of neighbouring lanes are neighbours in memory.
 *
 * What only the device can see is CLAMPED, never trusted: the part of a source span that leaves
 * [0, src_len) reads as zero, the part of a destination span that leaves [0, dst_len) is not written, a
 * negative length is 0, a length above 2^40 is cut to it, p is clamped into its range -- no read or write
 * goes out of bounds.  The Python layer validates the table before it uploads it.
 * n_utt >= 1; 0 <= src_len, dst_len <= 2^40; src_pool and dst 4-byte, desc 8-byte, table 16-byte
 * aligned.  A violation the host can see returns DANET_SPEED_ERR_ARG and launches nothing.        */
int danet_speed_resample(void* stream, int n_utt, const float* src_pool, int64_t src_len,
                         const danet_speed_utt_t* desc, const float* table, float* dst, int64_t dst_len);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_SPEED_HIP_H */
