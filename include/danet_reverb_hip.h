/*
 * libdanet_reverb_hip.so -- C ABI of the reverberation of the `wavdir` dataset (REVERB_RT60_MAX): every
 * utterance of a ragged batch convolved with one row of a bank of synthetic room responses, from the
 * device-resident pool (or the speed scratch) into a scratch waveform buffer, in one launch, in front of
 * danet_prep_stft_batch.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the core, conv, dropout, prep, mix and speed ABIs
 * stay as they are.  Same conventions as include/danet_speed_hip.h: caller-owned DEVICE pointers, fp32,
 * `stream` a hipStream_t passed as void*, 0 = DANET_REVERB_OK and negative = error with a thread-local
 * message in danet_reverb_last_error(), asynchronous launches, no process environment read, no
 * allocation.  The library holds no random numbers and no transcendental math: the bank is an INPUT.
 *
 * THE RULE.  NB = DANET_REVERB_ROWS = 32 responses, R = REVERB_RT60_MAX in seconds, 0 <= R <= 1.0,
 * K taps each, at most DANET_REVERB_MAX_TAPS = 8192; one descriptor row is 48 bytes.
 *
 *   Tap count: K = 4 * ceil(R * SMPRATE / 4), at least 4 and at most DANET_REVERB_MAX_TAPS (a larger one
 *     is an error of the configuration, not a clamp).
 *   The bank, float32 [NB][K], computed by the Python layer in float64 numpy, rounded once to float32,
 *     validated as finite and uploaded once per dataset:
 *     row 0 is the unit impulse (dry);
 *     row k >= 1:  RT60_k = R * k / (NB - 1);
 *       g = RandomState([1337, 2, k]).standard_normal(K)   (NOT shard-seeded: the bank is a property of
 *         the configuration, the same on every rank);
 *       t[n] = g[n] * exp(-3 ln(10) * n / (RT60_k * SMPRATE)) for 1 <= n < K, t[0] = 0
 *         (60 dB of energy decay after RT60_k seconds);
 *       the tail scaled so that sum t^2 = 10^(-DRR_k / 10), DRR_k = 10 - 10 * k / (NB - 1) dB
 *         (direct-to-reverberant ratio: 10 dB at the driest row, 0 dB at row NB - 1);
 *       h = (delta + t) / sqrt(1 + sum t^2): a direct path at sample 0 and unit energy, so that the
 *         expected power of a source is kept.
 *     R = 0: RT60_k = 0 means no tail, every row is the unit impulse.
 *   Draw (host side): every utterance of every train batch draws its row k = rng.randint(0, NB), one call
 *     per batch, from a numpy RandomState the dataset owns, seeded by (dist.shard_seed(1337), subset
 *     index, 2): a stream of its own beside the mix stream (no trailing number) and the speed stream
 *     (trailing 1), never python's `random` or np.random.  Only `train` is reverberated; its stream runs
 *     on across epochs; ranks draw differently.
 *   Output sample n of an L-sample utterance x, 0 <= n < L (the tail beyond L is truncated: lengths,
 *     frame counts, pads and the crop plan are those without the key):
 *       y[n] = sum over j in [0, K) of h_k[j] * x[n - j],  x outside [0, L) zero;
 *     float32 products and accumulation, fused: ONE chain acc = fmaf(h_k[j], x[n - j], acc), j ASCENDING,
 *     from acc = +0.  The chain of sample n runs over j < min(K, 4 * ceil(min(1024 * (n div 1024 + 1), L)
 *     / 4)): the terms left out multiply samples in front of the utterance, which are zero, so only the
 *     sign of a zero result can depend on it, and the limit is a function of (n, L, K) alone.
 *   Consequence: the value of a sample depends on (x, h_k, n) alone -- not on the span asked for, not on
 *     the tile, not on the neighbouring rows, not on the addresses.  With row 0 the output equals the
 *     input as values (every finite input; a negative zero may come out as +0).
 */
#ifndef DANET_REVERB_HIP_H
#define DANET_REVERB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/reverb/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_REVERB_ABI_VERSION 1

#define DANET_REVERB_OK 0
#define DANET_REVERB_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_REVERB_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_REVERB_ROWS 32          /* NB                                     */
#define DANET_REVERB_MIN_TAPS 4
#define DANET_REVERB_MAX_TAPS 8192

/* one row of the descriptor table (48 bytes, device memory, 8-byte aligned) */
typedef struct danet_reverb_utt {
  int64_t src_offset;  /* first sample of the utterance, in floats from `src`          */
  int64_t src_length;  /* L, samples                                                   */
  int64_t dst_offset;  /* where output sample 0 would go, in floats from `dst`         */
  int64_t out_begin;   /* first output sample asked for                                */
  int64_t out_count;   /* output samples asked for                                     */
  int32_t row;         /* row of the bank, 0 <= row < DANET_REVERB_ROWS                */
  int32_t reserved;    /* 0                                                            */
} danet_reverb_utt_t;

int danet_reverb_abi_version(void);
const char* danet_reverb_last_error(void);

/* dst[dst_offset_u + n] = y_u[n] of the rule, for u < n_utt and every n of
 * [out_begin_u, out_begin_u + out_count_u) intersected with [0, src_length_u), where x_u[i] =
 * src[src_offset_u + i] for 0 <= i < src_length_u and zero elsewhere, and h = bank[row_u][0 .. n_taps).
 * `bank`: float32 [DANET_REVERB_ROWS][n_taps] in device memory.
 *
 * Each such float is written exactly once per launch (the spans of different rows must not overlap, and
 * `dst` must not overlap `src`) and nothing else is touched.  The value of a sample depends on
 * (x_u, h, n) alone.  No read-modify-write on memory is used, so two launches agree bit for bit, and a
 * span launch equals the slice of the whole-utterance launch bit for bit.
 *
 * Geometry: a persistent grid of at most four 128-thread workgroups per compute unit.  Every workgroup
 * walks the descriptor rows in order with a running tile count and takes the tiles whose running index
 * is its own modulo the grid.  A tile is the part of a row's span inside one block of 1024 outputs,
 * blocks counted from output sample 0; its taps are walked in chunks of at most 1024: the chunk of the
 * response and the 1024 + chunk input samples it meets are staged in LDS (16-byte loads where the
 * address allows, sample by sample elsewhere, zeros outside the utterance), and lane l owns the eight
 * consecutive outputs 8 l .. 8 l + 7 of the block in registers and slides a twelve-sample register
 * window of x over the taps: per four taps one 16-byte LDS read of x and one broadcast 16-byte LDS read
 * of h feed 32 fused multiply-adds.
 *
 * What only the device can see is CLAMPED, never trusted: the part of a source span that leaves
 * [0, src_len) reads as zero, a negative src_length is 0 and one above 2^40 is cut to it, the span is cut
 * to [0, src_length), the part of it whose destination leaves [0, dst_len) is not written, `row` is
 * clamped into [0, DANET_REVERB_ROWS) -- no read or write goes out of bounds.  The Python layer
 * validates the bank before it uploads it.
 * n_utt >= 1; n_taps a multiple of 4 in [DANET_REVERB_MIN_TAPS, DANET_REVERB_MAX_TAPS];
 * 0 <= src_len, dst_len <= 2^40; src and dst 4-byte, desc 8-byte, bank 16-byte aligned.  A violation
 * the host can see returns DANET_REVERB_ERR_ARG and launches nothing.                              */
int danet_reverb_apply(void* stream, int n_utt, const float* src, int64_t src_len,
                       const danet_reverb_utt_t* desc, const float* bank, int n_taps, float* dst,
                       int64_t dst_len);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_REVERB_HIP_H */
