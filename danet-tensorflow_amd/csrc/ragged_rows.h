/*
 * The ragged-row core of the wavdir libraries, once: how a kernel turns a row of a table it does not trust into a
 * span it may touch.  Device code only; a descriptor is clamped, never refused.
 *
 * clamp_row.  Rows of one float pool given as offsets[] and lengths[] (libdanet_mix_hip.so, libdanet_level_hip.so):
 * the argument struct of a kernel derives from RowTable.
 * cut_span.  A span of a descriptor row against the buffer it points into (libdanet_speed_hip.so, both spans;
 * libdanet_reverb_hip.so, the source span).
 */
#ifndef DANET_RAGGED_ROWS_H
#define DANET_RAGGED_ROWS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

struct RowTable {
  const float* pool;
  int64_t pool_len;
  const int64_t* offsets;
  const int64_t* lengths;
  int64_t max_len;
};

/* the row is clamped, never trusted: -> [off, off + len) inside the pool, 0 <= len <= max_len */
__device__ __forceinline__ void clamp_row(const RowTable& a, int u, int64_t& off, int64_t& len) {
  off = a.offsets[u];
  len = a.lengths[u];
  if (len < 0) len = 0;
  if (off < 0) {
    len = (off <= -len) ? 0 : len + off;      /* the part in front of the pool is cut off */
    off = 0;
  }
  if (off > a.pool_len) off = a.pool_len;
  if (len > a.pool_len - off) len = a.pool_len - off;
  if (len > a.max_len) len = a.max_len;
}

static const int64_t kMaxSpan = (int64_t)1 << 40;      /* the longest span and the largest buffer of cut_span */

/* [0, len) cut to the indices i with 0 <= off + i < total -> [lo, hi), empty as lo = hi = 0 */
__device__ __forceinline__ void cut_span(int64_t off, int64_t len, int64_t total, int64_t& lo, int64_t& hi) {
  if (len < 0) len = 0;
  if (len > kMaxSpan) len = kMaxSpan;
  lo = 0;
  hi = 0;
  if (off < total && off > -len) {                /* not entirely behind or in front of the buffer */
    lo = off < 0 ? -off : 0;                      /* off > -len >= -2^40: no overflow              */
    hi = len < total - off ? len : total - off;   /* off < total <= 2^40                           */
  }
}

#endif
