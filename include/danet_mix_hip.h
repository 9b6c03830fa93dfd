/*
 * libdanet_mix_hip.so -- C ABI of the mixture level control of the `wavdir` dataset
 * (MIX_SNR_RANGE / MIX_LEVEL_RANGE): the power of every utterance of a device-resident pool, measured
 * once per pool, and a per-utterance gain applied in place to the batch danet_prep_stft_batch wrote.
 * gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the core, conv, dropout and prep ABIs stay as
 * they are.  Same conventions as include/danet_prep_hip.h: caller-owned DEVICE pointers, fp32 /
 * interleaved complex64, `stream` a hipStream_t passed as void*, 0 = DANET_MIX_OK and negative =
 * error with a thread-local message in danet_mix_last_error(), asynchronous launches, no process
 * environment read, no allocation.
 *
 * THE GAIN RULE (host side, float64; the library only measures P and applies g).  A batch of B*C rows
 * is B groups of C = MAX_N_SIGNAL consecutive rows, the grouping .view(B, C, ...) implies.  For one
 * group, with P_c = sum(x^2) / len the mean power of utterance c over its whole file, R =
 * MIX_SNR_RANGE and L = MIX_LEVEL_RANGE (dB, each may be unset):
 *   1. G = exp(mean(log P_c)) over the rows with P_c > 0: the geometric mean keeps the stored scale.
 *   2. R set: u_0 = 0 and u_c = rng.uniform(-R, R) for c = 1..C-1, every one drawn whether or not the
 *      row is silent; d_c = u_c - mean(u_0..u_{C-1}).  C = 2 gives (-u/2, +u/2): a relative level
 *      uniform in [-R, R] dB, symmetric like the reference's u_coeff / v_coeff
 *      (app/datasets/WSJ0/process.py:67-118).
 *   3. R unset: d_c = 0 and nothing is equalised -- the factor sqrt(G / P_c) below is 1.
 *   4. L set: l = rng.uniform(-L, L), one draw per group; else l = 0.
 *   5. g_c = sqrt(G / P_c) * 10^((d_c + l) / 20), rounded once to float32; a row with P_c = 0 has
 *      g_c = 1.
 * `rng` is a numpy RandomState the dataset owns (never python's `random` or np.random); draw order
 * per batch: group by group, first the C-1 offsets, then the level; only the draws of a set key are
 * made, so the number of draws depends on shapes alone.
 */
#ifndef DANET_MIX_HIP_H
#define DANET_MIX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/mix/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_MIX_ABI_VERSION 1

#define DANET_MIX_OK 0
#define DANET_MIX_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_MIX_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

int danet_mix_abi_version(void);
const char* danet_mix_last_error(void);

/* Scratch bytes of danet_mix_power for n_utt rows of at most max_len samples (0 when every row is
 * one slice; (size_t)-1 for n_utt < 1 or max_len outside [0, 2^39]).                          */
size_t danet_mix_workspace_bytes(int n_utt, int64_t max_len);

/* out_f64[u] = sum of x^2 over pool[offsets[u] .. offsets[u] + lengths[u]) for u < n_utt.
 *
 * Every square is formed and every sum is accumulated in float64 (the square of a float32 is exact
 * there).  The order of the additions is a fixed tree that depends on (offset, length, max_len) and
 * the pool's address modulo 16 alone -- not on n_utt, not on timing -- so two calls agree bit for
 * bit; no floating-point read-modify-write on memory is used.  No term passes through more than
 * 2^22 additions (max_len <= 2^39), which bounds the relative error of the sum of these
 * non-negative terms by 2^22 * 2^-53.
 *
 * Geometry: a row is cut into slices of max(65536, ceil(max_len / 256) rounded up to a multiple of
 * 4) samples, one workgroup per (row, slice); a workgroup whose slice starts beyond its row ends at
 * once.  With more than one slice per row the slice sums go through `ws` and a second launch adds
 * each row's in index order.  Loads are 16-byte wherever the address allows, 4-byte at a slice's
 * misaligned head and tail.
 *
 * offsets, lengths: int64 in device memory, in floats from `pool`.  max_len: an upper bound of the
 * lengths that the caller vouches for.  What only the device can see is CLAMPED, never trusted: a
 * row whose [offset, offset + length) leaves the pool is cut to the pool, a negative length is 0, a
 * row longer than max_len is cut to max_len -- nothing is read or written out of bounds.
 * n_utt >= 1; pool_len >= 0; 0 <= max_len <= 2^39; n_utt * slices per row < 2^31; pool 4-byte,
 * offsets, lengths, out_f64 and ws 8-byte aligned; ws_bytes >= danet_mix_workspace_bytes(n_utt,
 * max_len) (ws may be null when that is 0).  A violation the host can see returns
 * DANET_MIX_ERR_ARG and launches nothing.                                                      */
int danet_mix_power(void* stream, int n_utt, const float* pool, int64_t pool_len, const int64_t* offsets,
                    const int64_t* lengths, int64_t max_len, double* out_f64, void* ws, size_t ws_bytes);

/* buf_c64[u][t][0..F) *= gains[u] for u < n_utt, t < t_count, in place: interleaved complex64, row
 * pitch ld >= F complex elements, utterance pitch t_count * ld -- the batch danet_prep_stft_batch
 * wrote.  Both parts of every element inside the F columns become the single rounding fl(g * x):
 * zeros stay zeros, g = 1 leaves every bit.  The pitch gaps and everything outside the buffer are
 * never touched.  gains: n_utt float32 in device memory.
 * n_utt, t_count, F >= 1; ld < 2^40; n_utt * workgroups per utterance < 2^31; buf_c64 8-byte, gains
 * 4-byte aligned.  A violation returns DANET_MIX_ERR_ARG and launches nothing.                */
int danet_mix_scale_c64(void* stream, int n_utt, int t_count, int F, float* buf_c64, int64_t ld,
                        const float* gains);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_MIX_HIP_H */
