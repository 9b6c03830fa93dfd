/*
 * libdanet_dropout_hip.so (include/danet_dropout_hip.h): inverted dropout over a pitched fp32
 * matrix with a regenerated Philox4x32-10 mask.  gfx950.
 *
 * Streaming work: 8 bytes of traffic per element against ~12 integer multiplies per FOUR elements,
 * so the kernel is written for the memory system.  One thread owns one group of four consecutive
 * LOGICAL elements (one Philox evaluation): on the fast path that is one 16-byte load and one
 * 16-byte store, lane i of a wave at base + 16 i.  Two groups are in flight per thread and
 * iteration (both loads are issued before the first multiply); the grid is a multiple of the
 * device's CU count and strides over the rest.  No LDS, no atomics.  Row / column of a group come
 * from ONE division; indices are 32-bit unless rows * ld does not fit.
 */
#include <hip/hip_runtime.h>

#include "danet_dropout_hip.h"
#define DANET_EXT dropout
#define DANET_EXT_UPPER DROPOUT
#include "ext_core.h"

struct Philox {
  uint32_t w[4];
};

/* Philox4x32-10 of counter (g_lo, g_hi, stream_id, step) under key (k0, k1) */
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox p;
  p.w[0] = c0; p.w[1] = c1; p.w[2] = c2; p.w[3] = c3;
  return p;
}

struct DropArgs {
  const float* x;
  float* y;
  uint64_t cols, ldx, ldy;
  uint64_t ngroups;      /* ceil(rows * cols / 4) */
  uint64_t nelem;        /* rows * cols */
  uint32_t threshold, key0, key1, stream_id, step;
  float scale;
  int dense;             /* ldx == ldy == cols: the element index is the offset */
};

/* fast path: cols, ldx, ldy multiples of 4, x and y 16-byte aligned -> a group never leaves its row */
template <typename I>
__global__ __launch_bounds__(256) void dropout_vec4_kernel(DropArgs a) {
  const I n = (I)a.ngroups;
  const I stride = (I)gridDim.x * 256;
  const I cols4 = (I)(a.cols >> 2), ldx = (I)a.ldx, ldy = (I)a.ldy;
  for (I g = (I)blockIdx.x * 256 + threadIdx.x; g < n; g += 2 * stride) {
    const I g2 = g + stride;
    const bool two = g2 < n;
    I ox = g * 4, oy = g * 4, ox2 = g2 * 4, oy2 = g2 * 4;
    if (!a.dense) {
      const I r = g / cols4, c = (g - r * cols4) * 4;
      ox = r * ldx + c;
      oy = r * ldy + c;
      const I r2 = g2 / cols4, c2 = (g2 - r2 * cols4) * 4;
      ox2 = r2 * ldx + c2;
      oy2 = r2 * ldy + c2;
    }
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + ox);
    f32x4 v2 = {0.f, 0.f, 0.f, 0.f};
    if (two) v2 = *reinterpret_cast<const f32x4*>(a.x + ox2);
    const Philox p = philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), a.stream_id, a.step,
                                   a.key0, a.key1);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = p.w[j] < a.threshold ? v[j] * a.scale : 0.f;
    *reinterpret_cast<f32x4*>(a.y + oy) = o;
    if (two) {
      const Philox q = philox4x32_10((uint32_t)g2, (uint32_t)((uint64_t)g2 >> 32), a.stream_id, a.step,
                                     a.key0, a.key1);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = q.w[j] < a.threshold ? v2[j] * a.scale : 0.f;
      *reinterpret_cast<f32x4*>(a.y + oy2) = o;
    }
  }
}

/* everything else: 4-byte accesses; a group may straddle a row end and the last one may be short */
template <typename I>
__global__ __launch_bounds__(256) void dropout_scalar_kernel(DropArgs a) {
  const I n = (I)a.ngroups, nelem = (I)a.nelem;
  const I stride = (I)gridDim.x * 256;
  const I cols = (I)a.cols, ldx = (I)a.ldx, ldy = (I)a.ldy;
  for (I g = (I)blockIdx.x * 256 + threadIdx.x; g < n; g += stride) {
    const Philox p = philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), a.stream_id, a.step,
                                   a.key0, a.key1);
    I e = g * 4;
    I r = e / cols, c = e - r * cols;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e < nelem) {
        const float v = a.x[r * ldx + c];
        a.y[r * ldy + c] = p.w[j] < a.threshold ? v * a.scale : 0.f;
      }
      ++e;
      if (++c == cols) { c = 0; ++r; }
    }
  }
}

/* workgroups per CU of the grid: 8 resident (256 threads, < 32 VGPRs) x 2 rounds, so that the tail of
 * a tensor a little larger than one round is spread by the dispatcher, not by a stride loop */
static const int kBlocksPerCU = 16;

static int device_cus(void) {
  static thread_local int dev_cached = -1, cus = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev != dev_cached) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      return 0;
    dev_cached = dev;
    cus = n;
  }
  return cus;
}

extern "C" int danet_dropout_apply(void* stream, int64_t rows, int64_t cols, const float* x, int64_t ldx,
                                   float* y, int64_t ldy, uint32_t threshold, float scale, uint32_t key0,
                                   uint32_t key1, uint32_t stream_id, uint32_t step) {
  const int64_t lim = (int64_t)1 << 62;
  CHECK_ARG(x != nullptr && y != nullptr, "dropout_apply: null pointer");
  CHECK_ARG(rows >= 1 && cols >= 1, "dropout_apply: rows and cols must be >= 1 (got %lld x %lld)",
            (long long)rows, (long long)cols);
  CHECK_ARG(ldx >= cols && ldy >= cols, "dropout_apply: ldx, ldy must be >= cols (%lld, %lld < %lld)",
            (long long)ldx, (long long)ldy, (long long)cols);
  CHECK_ARG(cols < lim / rows && ldx < lim / rows && ldy < lim / rows,
            "dropout_apply: rows * ld must be < 2^62");
  CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0,
            "dropout_apply: x and y must be 4-byte aligned");
  CHECK_ARG(threshold >= 1, "dropout_apply: threshold must be >= 1 (0 keeps nothing)");
  CHECK_ARG(x != y || ldx == ldy, "dropout_apply: in place (x == y) needs ldx == ldy");
  CHECK_ARG(scale == scale && scale - scale == 0.f, "dropout_apply: scale must be finite");
  const int cus = device_cus();
  if (cus <= 0) {
    set_error("dropout_apply: no HIP device");
    return DANET_DROPOUT_ERR_LAUNCH;
  }
  DropArgs a;
  a.x = x; a.y = y;
  a.cols = (uint64_t)cols; a.ldx = (uint64_t)ldx; a.ldy = (uint64_t)ldy;
  a.nelem = (uint64_t)rows * (uint64_t)cols;
  a.ngroups = (a.nelem + 3) >> 2;
  a.threshold = threshold; a.key0 = key0; a.key1 = key1; a.stream_id = stream_id; a.step = step;
  a.scale = scale;
  a.dense = (ldx == cols && ldy == cols) ? 1 : 0;
  const bool vec = ((cols | ldx | ldy) & 3) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  /* 32-bit indices while every offset, and the 2-stride look-ahead of the group index, fit */
  const uint64_t ld = (uint64_t)(ldx > ldy ? ldx : ldy);
  const bool small = (uint64_t)rows * ld < ((uint64_t)1 << 31);
  const uint64_t per = vec ? 512 : 256;      /* groups per workgroup and iteration */
  uint64_t blocks = (a.ngroups + per - 1) / per;
  const uint64_t cap = (uint64_t)cus * kBlocksPerCU;
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = (hipStream_t)stream;
  if (vec) {
    if (small) dropout_vec4_kernel<uint32_t><<<grid, 256, 0, s>>>(a);
    else dropout_vec4_kernel<uint64_t><<<grid, 256, 0, s>>>(a);
  } else {
    if (small) dropout_scalar_kernel<uint32_t><<<grid, 256, 0, s>>>(a);
    else dropout_scalar_kernel<uint64_t><<<grid, 256, 0, s>>>(a);
  }
  CHECK_LAUNCH();
  return DANET_DROPOUT_OK;
}
