/*
 * The float64 sum of squares of a slice of floats over one workgroup of 256 threads, once: what mix_power_kernel
 * (csrc/mix) and gclip_sumsq_kernel (csrc/gclip) both run.  gfx950, wave64.  Included after ext_core.h (f32x4).
 *
 * slice_sumsq.  A thread's share of x[0..n): the 16-byte vectors from the first 16-byte aligned address on, at
 * stride 256 with four loads in flight, the four exact float64 squares of a vector added as (a + b) + (c + d) and
 * that to the accumulator; then the up to three floats in front (thread t takes x[t]) and behind.
 * wave_sums.  A fixed butterfly over the 64 lanes of a wave (cross-lane moves, no LDS), the four wave sums into
 * part[]; behind its barrier four_waves(part) is (w0 + w1) + (w2 + w3).  Who adds them and where the sum goes is
 * the kernel's own ending.  (block_sum_f64 of csrc/wave_metric.h is another tree with another barrier.)
 */
#ifndef DANET_SUMSQ_F64_H
#define DANET_SUMSQ_F64_H

#include <hip/hip_runtime.h>
#include <stdint.h>

static const int kThreads = 256;
static const int kWaves = kThreads / 64;

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }
__device__ __forceinline__ double sq4(f32x4 v) { return (sq(v[0]) + sq(v[1])) + (sq(v[2]) + sq(v[3])); }

__device__ __forceinline__ double slice_sumsq(const float* x, int64_t n) {
  const int tid = threadIdx.x;
  const int64_t head = min(n, (int64_t)((4 - (int)(((uintptr_t)x >> 2) & 3)) & 3));
  const int64_t nvec = (n - head) >> 2;
  const int64_t tail = n - head - 4 * nvec;
  const f32x4* xv = reinterpret_cast<const f32x4*>(x + head);

  double acc = 0.0;
  int64_t i = tid;
  for (; i + 3 * kThreads < nvec; i += 4 * kThreads) {
    const f32x4 v0 = xv[i], v1 = xv[i + kThreads], v2 = xv[i + 2 * kThreads], v3 = xv[i + 3 * kThreads];
    acc += sq4(v0);
    acc += sq4(v1);
    acc += sq4(v2);
    acc += sq4(v3);
  }
  for (; i < nvec; i += kThreads) acc += sq4(xv[i]);
  if (tid < head) acc += sq(x[tid]);
  if (tid < tail) acc += sq(x[head + 4 * nvec + tid]);
  return acc;
}

__device__ __forceinline__ void wave_sums(double acc, double* part) {
  const int tid = threadIdx.x;
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);     /* every lane: the wave's sum */
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
}

__device__ __forceinline__ double four_waves(const double* part) { return (part[0] + part[1]) + (part[2] + part[3]); }

#endif
