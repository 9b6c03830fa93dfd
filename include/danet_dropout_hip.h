/*
 * libdanet_dropout_hip.so -- C ABI of the inverted-dropout operator of the BiLSTM encoders
 * (reference app/modules.py:137, `tf.nn.dropout(s_output, keep_prob)`), gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the core ABI stays as it
 * is.  Same conventions as include/danet_hip.h: caller-owned DEVICE pointers,
 * fp32, `stream` a hipStream_t passed as void*, 0 = DANET_DROPOUT_OK and negative =
 * error with a thread-local message in danet_dropout_last_error(), asynchronous
 * launches, no process environment read, no allocation.
 *
 * THE MASK IS A CONTRACT.  It is never stored: forward, backward and any restatement on
 * another machine regenerate it from the call's arguments alone.
 *
 *   generator  Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 (on counter word 0)
 *              and 0xCD9E8D57 (on counter word 2), Weyl key increments 0x9E3779B9 (key word 0)
 *              and 0xBB67AE85 (key word 1), ten rounds, the key bumped between rounds.  One round:
 *                  (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0))
 *   key        (key0, key1)
 *   counter    (g & 0xffffffff, g >> 32, stream_id, step) with g = e >> 2, where
 *              e = r * cols + c is the LOGICAL index of element [r][c] of the [rows][cols]
 *              matrix (64-bit).  It does not depend on ldx, ldy or on launch geometry.
 *   element e  uses output word (e & 3) and is KEPT iff word < threshold (unsigned 32-bit).
 *   host side  threshold = min(2^32 - 1, floor(keep * 2^32));  scale = (float)(1.0 / keep), one
 *              double division rounded once to fp32.
 *
 * Known answers (counter; key -> output): zero; zero -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8,
 * all-ones; all-ones -> 408f276d 41c83b0e a20bc7c6 6d5451fd,
 * 243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1.
 */
#ifndef DANET_DROPOUT_HIP_H
#define DANET_DROPOUT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/dropout/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_DROPOUT_ABI_VERSION 1

#define DANET_DROPOUT_OK 0
#define DANET_DROPOUT_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_DROPOUT_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

int danet_dropout_abi_version(void);
const char* danet_dropout_last_error(void);

/* y[r][c] = keep(e) ? x[r][c] * scale : 0 for r < rows, c < cols (mask as above); x at row pitch
 * ldx, y at row pitch ldy (elements), ldx, ldy >= cols, independent of each other.  y == x (in
 * place, then ldx == ldy) is allowed; otherwise the two must not overlap.  The pitch gaps
 * (columns cols..ld-1) are neither read into a result nor written.  A dropped element is +0
 * whatever x holds there (NaN and infinity included).  The operator is its own gradient: the
 * backward pass calls it on dy with the same (threshold, scale, key0, key1, stream_id, step).
 * rows, cols >= 1, rows * cols < 2^62, rows * ld < 2^62; threshold >= 1; x, y 4-byte aligned.
 * With cols, ldx, ldy multiples of 4 and x, y 16-byte aligned every access is a 16-byte one;
 * anything else takes an element-wise path with the same result.  A violation returns
 * DANET_DROPOUT_ERR_ARG and launches nothing.                                               */
int danet_dropout_apply(void* stream, int64_t rows, int64_t cols, const float* x, int64_t ldx,
                        float* y, int64_t ldy, uint32_t threshold, float scale, uint32_t key0,
                        uint32_t key1, uint32_t stream_id, uint32_t step);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_DROPOUT_HIP_H */
