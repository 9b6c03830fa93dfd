/*
 * libdanet_prep_hip.so -- C ABI of the dataset front-end of the `wavdir` dataset: the STFT of a
 * RAGGED batch of waveforms that stay resident in device memory, written straight into the
 * zero-padded (and optionally cropped) batch the model consumes.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the core ABI stays as it is, and
 * danet_stft / danet_istft stay the front-end of every other path.  Same conventions as
 * include/danet_hip.h: caller-owned DEVICE pointers, fp32 / interleaved complex64, `stream` a
 * hipStream_t passed as void*, 0 = DANET_PREP_OK and negative = error with a thread-local message in
 * danet_prep_last_error(), asynchronous launches, no process environment read, no allocation.
 *
 * THE TRANSFORM is the reference's scipy.signal.stft(x, window, nperseg=N, noverlap=N-S)[2].T
 * (app/utils.py:117-122), as danet_stft computes it: N/2 zeros on both sides of the waveform, a zero
 * tail so that the last frame is full, frame t = extended samples [t*S, t*S+N) (integer framing),
 * times the window, N-point real FFT, bins 0..N/2, times 1/sum(window).
 *
 * THE BATCH.  `pool` holds the waveforms back to back; row u of `desc` says where utterance u lies
 * and where it goes.  Utterance u has T_u = danet_prep_num_frames(length_u, N, S) frames of its own;
 * on a virtual time axis of T_out frames they occupy [pad_left_u, pad_left_u + T_u) and every other
 * frame is zero (utils.random_zeropad, app/utils.py:78-92).  One launch writes frames
 * [t_begin, t_begin + t_count) of that axis for every utterance (the crop of main.py:422-426).
 */
#ifndef DANET_PREP_HIP_H
#define DANET_PREP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/prep/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_PREP_ABI_VERSION 1

#define DANET_PREP_OK 0
#define DANET_PREP_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_PREP_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

/* one row of the descriptor table (24 bytes, device memory, 8-byte aligned) */
typedef struct danet_prep_utt {
  int64_t offset;    /* first sample of the utterance, in floats from `pool`  */
  int64_t length;    /* samples                                               */
  int32_t pad_left;  /* zero frames in front of it on the virtual time axis   */
  int32_t reserved;  /* 0                                                     */
} danet_prep_utt_t;

int danet_prep_abi_version(void);
const char* danet_prep_last_error(void);

/* Frames of an Ls-sample waveform; host only, the same answer as danet_stft_num_frames
 * (1 + ceil(Ls / S) when S divides N).  DANET_PREP_ERR_ARG for Ls < N (scipy raises), N <= 0,
 * S <= 0 or S > N.                                                                          */
int danet_prep_num_frames(int64_t Ls, int N, int S);

/* Bytes of the plan of an N-point transform ((size_t)-1: N is not a power of two in [64, 4096]). */
size_t danet_prep_workspace_bytes(int N);

/* One-off setup per (N, window): writes into the caller-owned, 16-byte aligned `plan_ws` the
 * twiddle table exp(-2 pi i k / N), k < N/2 (sincospi: correctly rounded), and 1/sum(window)
 * formed as danet_stft forms it: the float32 window summed in float64, reciprocal, rounded to
 * float32.  No batch launch recomputes either.  `window`: N floats.                          */
int danet_prep_stft_plan(void* stream, int N, const float* window, void* plan_ws, size_t plan_bytes);

/* out_c64[u][t - t_begin][0..F) for u < n_utt, t_begin <= t < t_begin + t_count, F = N/2 + 1,
 * interleaved complex64, row pitch ld_out >= F complex elements (utterance pitch t_count * ld_out).
 * Every element inside the F columns is written exactly once per launch, frames outside
 * [pad_left_u, pad_left_u + T_u) as bitwise +0.0: no memset precedes the call.  The pitch gaps and
 * everything outside the buffer are never touched.  The value of a frame does not depend on
 * t_begin, t_count or n_utt: a cropped launch equals the slice of the full one bit for bit.
 *
 * pool_len: floats in `pool`.  N a power of two in [64, 4096]; 0 < S <= N; n_utt >= 1 (no 65535
 * ceiling); T_out >= 1; 0 <= t_begin, t_count >= 1, t_begin + t_count <= T_out;
 * n_utt * ceil(t_count / frames per workgroup) < 2^31.  pool, window 4-byte, desc and out_c64
 * 8-byte, plan_ws 16-byte aligned.  A violation the host can see returns DANET_PREP_ERR_ARG and
 * launches nothing.  What only the device can see is CLAMPED, never trusted: a row whose
 * [offset, offset + length) leaves the pool is cut to the pool, a row left with length < N has no
 * frames of its own (all zeros), and frames that pad_left_u + T_u would put beyond T_out are simply
 * not part of any launch -- no read or write goes out of bounds.  The Python layer validates the
 * table before it uploads it.                                                                 */
int danet_prep_stft_batch(void* stream, int n_utt, const float* pool, int64_t pool_len,
                          const danet_prep_utt_t* desc, int T_out, int t_begin, int t_count, int N, int S,
                          const float* window, const void* plan_ws, float* out_c64, int64_t ld_out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_PREP_HIP_H */
