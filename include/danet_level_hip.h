/*
 * libdanet_level_hip.so -- C ABI of the active-speech-level measurement of the `wavdir` dataset
 * (MIX_LEVEL_MEASURE = "active"): per utterance of a device-resident pool and per threshold of a table, the
 * number of samples the ITU-T P.56 (method B) activity detector calls active.  Measured once per pool, like
 * danet_mix_power; nothing on the per-batch path.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so; every other ABI stays as it is.  Same conventions as
 * include/danet_mix_hip.h: caller-owned DEVICE pointers, `stream` a hipStream_t passed as void*, 0 =
 * DANET_LEVEL_OK and negative = error with a thread-local message in danet_level_last_error(), asynchronous
 * launches, no process environment read, no allocation, no libm call: g and the hangover are arguments and
 * the thresholds an input table, all computed by the caller.
 *
 * THE LEVEL RULE (host side, float64; the library only counts).  P.56 method B with the threshold grid
 * anchored on the file's own rms, so the measure does not depend on the stored scale.  Per dataset:
 *   fs = SMPRATE,  g = exp(-1 / (0.03 fs)),  k = 1 - g,  I = ceil(0.2 fs) samples of hangover,  M = 15.9 dB.
 * Per file x[0..L) with sumsq = sum(x^2) and P = sumsq / L its mean power (danet_mix_power):
 *   1. envelope:   p[n] = g p[n-1] + k |x[n]|,  q[n] = g q[n-1] + k p[n],  p[-1] = q[-1] = 0,  0 <= n < L.
 *   2. thresholds: c_j = sqrt(P) * 2^(j - 10), j = 0..15: rms / 1024 ... 32 rms in factor-2 steps.  The
 *      margin crossing sits near active rms / 6.2, inside the grid for any activity factor above 3e-5.
 *   3. counts:     a_j = the number of n for which some m <= n has q[m] >= c_j and n - m <= I (the
 *      standard's counter loop with the hangover counter started at I).  THIS is what the library computes.
 *   4. finish:     A_j = 10 log10(sumsq / a_j), C_j = 20 log10(c_j).  Take the first j with a_j > 0 and
 *      A_j - C_j <= M.  j = 0: level = A_0.  Otherwise interpolate linearly in dB between j-1 and j:
 *      w = (A_{j-1} - C_{j-1} - M) / ((A_{j-1} - C_{j-1}) - (A_j - C_j)), level = A_{j-1} + w (A_j - A_{j-1}).
 *      The active power is 10^(level / 10).  Where no such j exists (a file shorter than its own attack,
 *      a_0 = 0) the active power is P.  A silent file (P = 0) keeps 0 and is never finished.
 * With MIX_LEVEL_MEASURE = "active" the dataset puts the active power A_c wherever the gain rule of
 * include/danet_mix_hip.h and the noise rule of include/danet_noise_hip.h use a SOURCE's mean power P_c: G,
 * sqrt(G / P_c) and P_s = sum g_c^2 P_c.  The noise file's own P_n stays its mean power over its whole
 * length: noise has no pauses to exclude.
 */
#ifndef DANET_LEVEL_HIP_H
#define DANET_LEVEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/level/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_LEVEL_ABI_VERSION 1

#define DANET_LEVEL_OK 0
#define DANET_LEVEL_ERR_ARG (-1)     /* bad shape / value, null or misaligned pointer, short workspace */
#define DANET_LEVEL_ERR_LAUNCH (-2)  /* hipLaunch failure                                               */

#define DANET_LEVEL_THRESHOLDS 16    /* thresholds, and counts, per utterance    */
#define DANET_LEVEL_TILE 1024        /* samples of a row one thread walks        */

int danet_level_abi_version(void);
const char* danet_level_last_error(void);

/* Scratch bytes of danet_level_activity for n_utt rows of at most max_len samples: with T =
 * max(1, ceil(max_len / DANET_LEVEL_TILE)) tiles per row, n_utt * T * (16 + 12 * DANET_LEVEL_THRESHOLDS);
 * (size_t)-1 for n_utt < 1, max_len outside [0, 2^31] or n_utt * T >= 2^31.                    */
size_t danet_level_workspace_bytes(int n_utt, int64_t max_len);

/* counts[u][j] = a_j of the rule above for the row pool[offsets[u] .. offsets[u] + lengths[u]), with the
 * thresholds thr[u][0..16), for u < n_utt: int64, every element written (0 for an empty row).  The
 * thresholds need not be ordered; each is counted on its own.
 *
 * ARITHMETIC.  The envelope is float64 throughout (|x| of a float32 is exact there); k = 1 - g is formed
 * once on the host.  The ORDER of the operations is the library's: a row is cut into tiles of
 * DANET_LEVEL_TILE samples, and four launches follow --
 *   1. per (row, tile), one thread: the end state (p, q) of the tile from a zero start;
 *   2. per row, one thread: the state that enters every tile, carried in tile order by
 *      p_in' = p_loc + G p_in,  q_in' = q_loc + G q_in + K p_in,  G = g^TILE,  K = k TILE g^TILE
 *      (the recurrence is linear; G by ten squarings on the host);
 *   3. per (row, tile), one thread: the recurrence again from the carried state and, per threshold, the
 *      count with no hangover coming in, the first and the last index at or above the threshold;
 *   4. per (row, threshold), one thread: the tiles in order -- to the tile's count it adds
 *      max(0, min(prev_last + I + 1, tile_start + first) - tile_start), `first` the tile's length when
 *      nothing in it reaches the threshold, and moves prev_last on.
 * Integer counts are combined in this fixed order through `ws`; there is no read-modify-write on memory,
 * floating-point or integer, so the result is a pure function of (row contents, g, hang, thresholds): it
 * does not depend on n_utt, max_len, the row's place in the pool or timing, and two calls agree bit for bit.
 *
 * ACCURACY.  With u = 2^-53 and tau = 1 / (1 - g) = 0.03 fs: every term of p and q is non-negative, so
 * rounding errors never cancel into something larger than their sum.  One step multiplies what p holds by
 * at most (1 + u) and adds k |x| rounded once (an fma: <= 2u on the new term); one step of q the same on
 * top of p's.  A contribution of age a to q[n] therefore carries a relative error of at most about
 * 3 (a + 2) u, and its weight k^2 (a + 1) g^a has mean age 2 tau: over any stretch whose envelope does not
 * fall by more than a constant factor per tau -- speech, noise, pauses above a noise floor -- the computed q
 * lies within about 6 u tau of the exact one, relative.  The carry adds G and K once per row (ten squarings:
 * <= 2^10 u relative) and one (1 + 3u) per tile crossed, 1 / TILE of a step's share.  For tau <= 4096
 * (0.03 fs <= 4096) that is 6 * 2^-53 * 4096 + 2^-43 < 2^-38: the q the kernel compares lies within 2^-34
 * relative of the exact recurrence with room to spare, under 1e-11.  (After a burst that falls into digital
 * silence the OLD terms dominate and the bound grows with their age, 3 a u; thresholds sit at rms / 1024 or
 * above, where a decaying tail spends a few tau.)  Counts are therefore EXACT whenever the exact q stays
 * outside (1 -+ 1e-9) c_j.
 *
 * offsets, lengths: int64 in device memory, in floats from `pool`.  max_len: an upper bound of the lengths
 * that the caller vouches for.  What only the device can see is CLAMPED exactly as danet_mix_power clamps
 * it, never trusted: a row whose [offset, offset + length) leaves the pool is cut to the pool, a negative
 * length is 0, a row longer than max_len is cut to max_len -- nothing is read out of bounds, and `counts`
 * and `ws` are never written outside [n_utt][16] and danet_level_workspace_bytes(n_utt, max_len).
 * n_utt >= 1; pool_len >= 0; 0 <= max_len <= 2^31; n_utt * tiles per row < 2^31; 0 < g < 1; 0 <= hang <=
 * 2^40; pool 4-byte, offsets, lengths, thr and counts 8-byte, ws 16-byte aligned and none of them null;
 * ws_bytes >= danet_level_workspace_bytes(n_utt, max_len).  A violation the host can see returns DANET_LEVEL_ERR_ARG
 * and launches nothing.  Launches 2 and 4 walk a row's tiles in one thread: the latency of a call grows
 * with its longest row.                                                                            */
int danet_level_activity(void* stream, int n_utt, const float* pool, int64_t pool_len, const int64_t* offsets,
                         const int64_t* lengths, int64_t max_len, double g, int64_t hang, const double* thr,
                         int64_t* counts, void* ws, size_t ws_bytes);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_LEVEL_HIP_H */
