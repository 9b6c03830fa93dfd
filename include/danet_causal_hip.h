/*
 * libdanet_causal_hip.so -- C ABI of the causal encoder and of block-wise streaming inference: a running-mean
 * centring whose state travels in and out, a stack of unidirectional LSTM layers that runs a block of frames FROM
 * CARRIED STATE, and a skinny product whose result for a row does not depend on how many rows it is called with.
 * Together with libdanet_online_hip.so (the online attractor estimator, whose state travels too) they make the model
 * streaming: the embedding of frame t depends on frames <= t only, and a recording fed in blocks of any size gives bit
 * for bit what it gives in one piece.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other nineteen libraries stay as they are.
 * Same conventions as include/danet_online_hip.h: caller-owned DEVICE pointers, `stream` a hipStream_t passed as
 * void*, 0 = DANET_CAUSAL_OK and negative = error with a thread-local message in danet_causal_last_error(),
 * asynchronous launches, no process environment read, no allocation, no atomics: within a launch every output
 * element is written once, by one thread, with an ordinary vector store, so repeated calls agree bit for bit.  (An
 * LSTM block is several launches ordered on the stream: c is rewritten once per frame, always by the thread that owns
 * it, and h reaches the state through the workspace and the last launch.)  No waiting between workgroups and no
 * persistent grid: what depends on another workgroup's result is another launch.
 *
 * THE RULE.
 *
 * 1. Causal centring (danet_causal_center_fwd).  Per utterance, with the state (S, n), two float64 values, zero for a
 *    fresh utterance, and for each frame t of the call in order:
 *        r_t  = sum over d < D of in[t][d], in float64 (ROW SUM ORDER below: a function of D alone)
 *        S    = S + r_t          (float64, sequentially in t)
 *        n    = n + 1
 *        mu_t = (float)(S / (n * D))
 *        out[t][d] = in[t][d] - mu_t        (one float32 subtraction)
 *    and the state after the last frame goes back into `state`.  A call over T frames is therefore BIT FOR BIT two
 *    calls over its halves, and utterance b alone is bit for bit utterance b inside a larger batch.
 *    Error against exact arithmetic on the same float32 input: |out - exact| <= 2^-23 (|x| + |mu|) (the rounding of
 *    mu to float32 and of the difference; the float64 sums contribute n D 2^-53 relative, far below).
 *
 *    Its adjoint over a whole utterance from a zero state (danet_causal_center_bwd, training only):
 *        g_t   = sum over d < D of dout[t][d], in float64, same order
 *        s_t'  = sum over t >= t' of g_t / ((t + 1) D), in float64, sequentially from the last frame down
 *        din[t'][d] = dout[t'][d] - (float)s_t'
 *
 *    ROW SUM ORDER.  64 partial sums p_j, j = 0..63: p_j adds (double)in[d] for d = j, j + 64, ... in ascending d
 *    from +0; then p_j += p_(j ^ 32), p_j += p_(j ^ 16), ..., p_j += p_(j ^ 1) (a butterfly in which every p_j ends
 *    as the same value).
 *
 * 2. The skinny product (one device core, used by danet_causal_lstm_block and danet_causal_project).  For a row x
 *    of K values and a column w of K values, Kp = K rounded up to a multiple of 4 (the tail counted as zeros):
 *        slice s = 0..15 takes the groups of four k = 4 (s + 16 j) .. 4 (s + 16 j) + 3, j = 0, 1, ... while below Kp,
 *        and forms p_s by float32 fused multiply-adds in ascending k from +0;
 *        the product is ((((p_0 + p_1) + (p_2 + p_3)) + ((p_4 + p_5) + (p_6 + p_7))) +
 *                        (((p_8 + p_9) + (p_10 + p_11)) + ((p_12 + p_13) + (p_14 + p_15)))).
 *    The order is a function of K alone: not of the number of rows, of which rows share a workgroup, of the number of
 *    columns or of the leading dimensions.
 *
 * 3. The LSTM block (danet_causal_lstm_block).  L stacked unidirectional layers, gate order g | i | f | o and cell
 *    math of danet_lstm_fwd (include/danet_hip.h): for layer l and frame t of the block, with x_t^(0) the input row
 *    and x_t^(l) = h_t^(l-1) above,
 *        a = product([x_t^(l), h_(t-1)^(l)], W_l) + b_l      (rule 2 with K = D_l + H, then ONE float32 add of b_l)
 *        g = a[0:H], i = sigmoid(a[H:2H]), f = sigmoid(a[2H:3H]), o = sigmoid(a[3H:4H])
 *        c_t = i g + f c_(t-1),   h_t = o tanh(c_t)
 *    with the hardware exponential and reciprocal of the core's recurrent kernels.  h_(-1)^(l) and c_(-1)^(l) are the
 *    carried state, and the state after the block's last frame replaces it.  The value of (l, t, b) depends neither
 *    on Tb, nor on where the block starts, nor on the other rows of the batch: Tb frames in one call are BIT FOR BIT
 *    the same frames in several calls.
 *
 * A violation of an envelope below returns DANET_CAUSAL_ERR_ARG with a message before any launch.
 */
#ifndef DANET_CAUSAL_HIP_H
#define DANET_CAUSAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/causal/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_CAUSAL_ABI_VERSION 1

#define DANET_CAUSAL_OK 0
#define DANET_CAUSAL_ERR_ARG (-1)     /* bad shape or value / null or misaligned pointer */
#define DANET_CAUSAL_ERR_LAUNCH (-2)  /* hipLaunch failure                               */

#define DANET_CAUSAL_MAX_T 65536      /* frames per centring call                        */
#define DANET_CAUSAL_MAX_D 4096       /* columns of a centred row                        */
#define DANET_CAUSAL_MAX_L 8
#define DANET_CAUSAL_MAX_B 16         /* rows of an LSTM block                           */
#define DANET_CAUSAL_MAX_TB 64        /* frames of an LSTM block                         */
#define DANET_CAUSAL_MAX_H 608
#define DANET_CAUSAL_MAX_D0 1028
#define DANET_CAUSAL_MAX_K (DANET_CAUSAL_MAX_D0 + DANET_CAUSAL_MAX_H)   /* of the skinny product */
#define DANET_CAUSAL_MAX_M 1024       /* rows of danet_causal_project                    */

int danet_causal_abi_version(void);
const char* danet_causal_last_error(void);

/* Rule 1, ONE launch: one workgroup of 256 threads per utterance walks the frames of the call 64 at a time -- the
 * row sums of the 64 frames (a wave per row), the sequential float64 prefix (one thread), the subtraction (all
 * threads, the rows read a second time from the cache) -- so no workspace is needed and no workgroup waits for
 * another.  in / out float32, layouts as for danet_center: 0 = batch-major [B][T][ld], 1 = time-major [T][B][ld],
 * chosen independently; the columns D .. ld_out - 1 of out are zero-filled.  state float64 [B][2] = (S, n), read and
 * updated in place.  B >= 1, 1 <= T <= DANET_CAUSAL_MAX_T, 1 <= D <= DANET_CAUSAL_MAX_D, ld_in >= D, ld_out >= D,
 * B T ld below 2^40; no null pointer; in / out 4-byte and state 8-byte aligned; in and out do not overlap.      */
int danet_causal_center_fwd(void* stream, int B, int T, int D, const float* in, int in_layout, int ld_in, float* out,
                            int out_layout, int ld_out, void* state);

/* The adjoint of rule 1 over a whole utterance from a zero state, ONE launch of the same shape walking the frames
 * from the last one down.  Only the columns < D of din are written.  Envelope as above.                        */
int danet_causal_center_bwd(void* stream, int B, int T, int D, const float* dout, int dout_layout, int ld_dout,
                            float* din, int din_layout, int ld_din);

/* Bytes of the workspace of danet_causal_lstm_block: the per-layer block buffers h^(l)_t, float32 [L][Tb][B][H].
 * (size_t)-1 with a message outside the envelope.                                                              */
size_t danet_causal_lstm_ws_bytes(int L, int B, int Tb, int H);

/* Rule 3.  One launch per anti-diagonal k = l + t, k = 0 .. Tb + L - 2: launch k computes every (l, k - l) with
 * 0 <= k - l < Tb, blockIdx.y = layer, blockIdx.x = a group of 16 units (all four gates of them: 64 columns of W_l),
 * 256 threads = 16 column quads x 16 K slices.  It reads h^(l-1)_t and h^(l)_(t-1), which launch k - 1 wrote into the
 * block buffers in ws.  [x_t, h_(t-1)] of every row is staged in LDS (16-byte broadcast reads), W is read with
 * 16-byte loads, 64 bytes per gate and row of W per workgroup, the 16 slices meet in LDS (rule 2), and thread
 * (row, unit) does the cell math; c is updated in place by the thread that owns it.  One last launch copies the
 * block's final h from ws into `h` (a launch of a one-frame block reads ALL of h while its workgroups produce the
 * new one, so the new one cannot go there directly): Tb + L launches in all, and no workgroup waits for another.
 *
 * x float32 [Tb][B][ldx] (time-major, D0 valid columns); W[l] float32 [D_l + H][4H] contiguous, D_0 = D0 and
 * D_l = H above, rows 0 .. D_l - 1 the input half; bias[l] float32 [4H]; W and bias are HOST arrays of L device
 * pointers.  h, c float32 [L][B][H], read and overwritten with the state after the block's last frame.  y float32
 * [Tb][B][ldy]: the top layer's output in its columns < H (the others are not written).  ws: at least
 * danet_causal_lstm_ws_bytes(L, B, Tb, H) bytes, contents irrelevant.
 * Envelope: 1 <= L <= 8, 1 <= B <= 16, 1 <= Tb <= 64, H % 4 == 0, 4 <= H <= 608, 1 <= D0 <= 1028, ldx >= D0,
 * ldy >= H; no null pointer; W[l] and ws 16-byte aligned, the others 4-byte.                                  */
int danet_causal_lstm_block(void* stream, int L, int B, int Tb, int D0, int H, const float* x, int ldx,
                            const float* const* W, const float* const* bias, float* h, float* c, float* y, int ldy,
                            void* ws, size_t ws_bytes);

/* out[r][o] = product(A[r], Wout[:, o]) (rule 2), ONE launch: blockIdx.x = 64 columns, blockIdx.y = a group of rows
 * (16, or 4 / 1 when M is no larger), the same device core as the LSTM step's product.  Row r of out is bit for bit
 * the same whatever M.  A float32 [M][lda], Wout float32 [K][ldw], out float32 [M][ldo].  1 <= M <= 1024,
 * 1 <= K <= DANET_CAUSAL_MAX_K, 1 <= N < 2^24, lda >= K, ldw >= N, ldo >= N; no null pointer, 4-byte aligned (16-byte
 * loads of Wout are used when it is 16-byte aligned and N and ldw are multiples of 4; the arithmetic is the same). */
int danet_causal_project(void* stream, int M, int K, int N, const float* A, int lda, const float* Wout, int ldw,
                         float* out, int ldo);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_CAUSAL_HIP_H */
