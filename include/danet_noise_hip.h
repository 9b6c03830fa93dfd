/*
 * libdanet_noise_hip.so -- C ABI of the additive noise of the `wavdir` dataset (NOISE_DIR, NOISE_SNR_MIN,
 * NOISE_SNR_MAX): the model's front-end with one more component in the mixture that is NOT a target --
 * mixture = sum of the C sources + gain * noise -- in one pass.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the core, conv, dropout, prep, mix, speed, reverb and
 * metric ABIs stay as they are.  Same conventions as include/danet_mix_hip.h: caller-owned DEVICE pointers,
 * fp32 / interleaved complex64, `stream` a hipStream_t passed as void*, 0 = DANET_NOISE_OK and negative = error
 * with a thread-local message in danet_noise_last_error(), asynchronous launches, no process environment read,
 * no allocation.
 *
 * THE NOISE RULE (host side, float64 numpy; the library only adds fl(g * n)).  `train` batches only.  A batch is
 * B mixtures of C = MAX_N_SIGNAL consecutive rows, planned as without the keys (speed, pads, crop, reverb rows,
 * gains); T_max is its frame count, N = FFT_SIZE, S = FFT_STRIDE, frames(L) = danet_prep_num_frames(L, N, S).
 * `rng` is a numpy RandomState the dataset owns per subset, seeded by (dist.shard_seed(1337), subset index, 3):
 * a fifth stream, so python's `random`, np.random and the mix, speed and reverb streams draw what they draw
 * without the keys; it runs on across epochs and ranks draw differently.  Per batch THREE calls, in this order,
 * each of size B:
 *   1. f   = rng.randint(0, n_noise, size=B)          the noise file of every mixture
 *   2. u   = rng.random_sample(B)                     where it is cut, or where it is placed
 *   3. snr = rng.uniform(lo, hi, size=B)              dB, lo = NOISE_SNR_MIN, hi = NOISE_SNR_MAX
 * SEGMENT.  A noise row is an ordinary 24-byte danet_prep_utt_t row into the noise pool (offset, length,
 * pad_left).  Lfull = (T_max - 1) * S has exactly T_max frames and is >= N because the batch's longest
 * utterance is.  With Ln the length of file f and off_f its offset in the pool:
 *   Ln >= Lfull:  start = min(int(u * (Ln - Lfull + 1)), Ln - Lfull);  row = (off_f + start, Lfull, 0)
 *   Ln <  Lfull:  the whole file, placed like a short utterance: T_n = frames(Ln),
 *                 row = (off_f, Ln, min(int(u * (T_max - T_n + 1)), T_max - T_n)); noise is zero outside its frames.
 * GAIN.  float64 on the host, rounded ONCE to float32:
 *   P_s[b] = sum over the mixture's rows c of float64(g_c)^2 * P_c, P_c the STORED file's mean power (as for
 *            MIX_SNR_RANGE under speed and reverb) and g_c the row's float32 mix gain, 1 with the MIX_* keys null;
 *   P_n[f] = the noise file's mean power over its whole length (danet_mix_power on the noise pool, once);
 *   g_n[b] = sqrt(P_s / P_n[f]) * 10^(-snr / 20);   g_n[b] = 0 when P_s == 0 or P_n[f] == 0.
 * The SNR is defined against the sum of the sources' whole-file powers: inside a source's pauses and in the
 * padding the mixture is noise only.  That is intended.
 */
#ifndef DANET_NOISE_HIP_H
#define DANET_NOISE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/noise/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_NOISE_ABI_VERSION 1
#define DANET_NOISE_MAX_C 8

#define DANET_NOISE_OK 0
#define DANET_NOISE_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_NOISE_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

int danet_noise_abi_version(void);
const char* danet_noise_last_error(void);

/* The front-end of danet_frontend_fwd (include/danet_hip.h) over the mixture of C sources and one noise row.
 * Per batch item b < B and element n < N, for the real and the imaginary part alike:
 *     re = ((0.f + s_0) + ... + s_{C-1}) + fl(gain[b] * noise)
 * The product is rounded to float32 FIRST, the sum after it: there is no fused multiply-add, so the result is
 * the one danet_frontend_fwd gives on C + 1 rows whose last is the noise scaled in float32.  Then exactly that
 * kernel's calls:
 *     src_pwr[b][c][n] = hypotf(s_c.x, s_c.y)        mix_pwr[b][n] = hypotf(re, im)
 *     mix_log[b][n] = log1pf(mix_pwr)                ph = atan2f(im, re);  phasor[b][n] = (cosf(ph), sinf(ph))
 *     mix_c64[b][n] = (re, im) when mix_c64 is not null
 * gain == NULL: the noise is added unscaled.  Inputs are only read.
 *
 * One pass, one complex element per lane (8-byte accesses of the complex rows, 4-byte stores of the real ones;
 * the pass is bound by the latency of the function calls above, not by bandwidth: csrc/noise/noise.hip); a value
 * does not depend on where its row lies.  Writes are ordinary vector stores.
 * B >= 1; 1 <= C <= DANET_NOISE_MAX_C; 1 <= N < 2^40 and B * C * N < 2^58; src_c64, noise_c64, phasor and
 * mix_c64 8-byte, gain, mix_pwr, mix_log and src_pwr 4-byte aligned; src_c64, noise_c64, mix_pwr, mix_log,
 * phasor and src_pwr not null.  A violation returns DANET_NOISE_ERR_ARG and launches nothing.               */
int danet_noise_frontend_fwd(void* stream, int B, int C, int64_t N,
                             const float* src_c64,   /* [B][C][N] complex64 */
                             const float* noise_c64, /* [B][N] complex64    */
                             const float* gain,      /* [B] or NULL = 1     */
                             float* mix_pwr, float* mix_log, float* phasor /* [B][N][2] */,
                             float* src_pwr /* [B][C][N] */,
                             float* mix_c64 /* [B][N] complex64 or NULL */);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_NOISE_HIP_H */
