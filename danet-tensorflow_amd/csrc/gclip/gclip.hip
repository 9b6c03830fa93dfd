/*
 * libdanet_gclip_hip.so (include/danet_gclip_hip.h): the global L2 norm of the flat gradient and the clip + Adam
 * update scaled by the clip coefficient.  gfx950, wave64.
 *
 * danet_gclip_sumsq.  The slice sum of csrc/sumsq_f64.h, which describes it and which mix_power_kernel runs too, on
 * one flat buffer: one workgroup of 256 threads per partial; every thread adds the four wave sums and thread 0
 * stores the one float64 of the workgroup.
 *
 * danet_gclip_adam_step.  adam_clip_kernel of csrc/pointwise.hip (adam_one of csrc/adam_one.h, the same grid, the
 * same 16-byte path and tail) behind a prologue in which EVERY workgroup adds the partials in one fixed order and
 * forms norm, coef and the factor k itself: no workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "danet_gclip_hip.h"
#define DANET_EXT gclip
#define DANET_EXT_UPPER GCLIP
#include "ext_core.h"
#include "adam_one.h"
#include "sumsq_f64.h"

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

/* slice(n) of THE RULE */
static int64_t slice_of(int64_t n) {
  int64_t s = (cdiv64(n, DANET_GCLIP_MAX_PARTIALS) + 3) & ~(int64_t)3;
  return s < DANET_GCLIP_MIN_SLICE ? DANET_GCLIP_MIN_SLICE : s;
}

extern "C" int danet_gclip_partials(int64_t n) {
  if (n < 1 || n > DANET_GCLIP_MAX_N) {
    set_error("partials: n must be in [1, 2^40] (got %lld)", (long long)n);
    return 0;
  }
  return (int)cdiv64(n, slice_of(n));
}

/* ---------------------------------------------------------------------------------- sum of squares */
/* every thread: the sum of the 256 accumulators over the fixed tree of THE RULE */
__device__ __forceinline__ double block_sum(double acc, double* part) {
  wave_sums(acc, part);
  return four_waves(part);
}

__global__ __launch_bounds__(kThreads) void gclip_sumsq_kernel(int64_t n_total, int64_t slice,
                                                                const float* __restrict__ g,
                                                                double* __restrict__ partials) {
  __shared__ double part[kWaves];
  const int64_t b = (int64_t)blockIdx.x * slice;           /* < n_total: the grid is partials(n) */
  const int64_t n = min(slice, n_total - b);
  const double r = block_sum(slice_sumsq(g + b, n), part);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

extern "C" int danet_gclip_sumsq(void* stream, int64_t n, const float* grad, double* partials_f64, int n_partials) {
  CHECK_ARG(n >= 1 && n <= DANET_GCLIP_MAX_N, "sumsq: n must be in [1, 2^40] (got %lld)", (long long)n);
  CHECK_ARG(grad && partials_f64, "sumsq: null pointer");
  CHECK_ARG(((uintptr_t)grad & 3) == 0 && ((uintptr_t)partials_f64 & 7) == 0,
            "sumsq: misaligned pointer (grad 4-byte, partials 8-byte)");
  const int64_t slice = slice_of(n);
  const int want = (int)cdiv64(n, slice);
  CHECK_ARG(n_partials == want, "sumsq: n_partials must be danet_gclip_partials(n) = %d (got %d)", want,
            n_partials);
  gclip_sumsq_kernel<<<dim3((unsigned)want), kThreads, 0, (hipStream_t)stream>>>(n, slice, grad, partials_f64);
  CHECK_LAUNCH();
  return DANET_GCLIP_OK;
}

/* ---------------------------------------------------------------------------------- clip + TF1 Adam */
__global__ __launch_bounds__(256) void gclip_adam_kernel(
    int64_t n, float* __restrict__ theta, float* __restrict__ grad, float* __restrict__ m,
    float* __restrict__ v, float lr_t, float b1, float b2, float eps, float clip, float s,
    int zero_grad, int vec, double max_norm, const double* __restrict__ partials, int n_partials,
    double* __restrict__ norm_out) {
  __shared__ double part[kWaves];
  /* the partials t, t + 256, t + 512, t + 768 in this order; every workgroup the same tree, so the same k */
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < DANET_GCLIP_MAX_PARTIALS / kThreads; ++q) {
    const int p = (int)threadIdx.x + q * kThreads;
    if (p < n_partials) acc += partials[p];
  }
  const double S = block_sum(acc, part);
  const double norm = fabs((double)s) * sqrt(S);
  const double lim = norm + 1e-6;
  const double coef = (lim > max_norm) ? max_norm / lim : 1.0;     /* a NaN norm compares false */
  const float gscale = (float)((double)s * coef);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    norm_out[0] = norm;
    norm_out[1] = coef;
  }

  const int64_t n4 = vec ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < n4; i += stride) {
    f32x4 th = reinterpret_cast<f32x4*>(theta)[i], g = reinterpret_cast<f32x4*>(grad)[i];
    f32x4 mi = reinterpret_cast<f32x4*>(m)[i], vi = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float t_ = th[c], g_ = g[c], m_ = mi[c], v_ = vi[c];
      adam_one(t_, g_, m_, v_, lr_t, b1, b2, eps, clip, gscale);
      th[c] = t_; mi[c] = m_; vi[c] = v_;
    }
    reinterpret_cast<f32x4*>(theta)[i] = th;
    reinterpret_cast<f32x4*>(m)[i] = mi;
    reinterpret_cast<f32x4*>(v)[i] = vi;
    if (zero_grad) reinterpret_cast<f32x4*>(grad)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t i = n4 * 4 + t0; i < n; i += stride) {
    float th = theta[i], g = grad[i], mi = m[i], vi = v[i];
    adam_one(th, g, mi, vi, lr_t, b1, b2, eps, clip, gscale);
    theta[i] = th; m[i] = mi; v[i] = vi;
    if (zero_grad) grad[i] = 0.f;
  }
}

extern "C" int danet_gclip_adam_step(void* stream, int64_t n, float* theta, float* grad, float* m, float* v,
                                     float lr_t, float beta1, float beta2, float eps, float clip, float grad_scale,
                                     int zero_grad, double max_norm, const double* partials_f64, int n_partials,
                                     double* norm_out_f64) {
  CHECK_ARG(n >= 1 && n <= DANET_GCLIP_MAX_N, "adam_step: n must be in [1, 2^40] (got %lld)", (long long)n);
  CHECK_ARG(theta && grad && m && v && partials_f64 && norm_out_f64, "adam_step: null pointer");
  CHECK_ARG((((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 3) == 0 &&
                (((uintptr_t)partials_f64 | (uintptr_t)norm_out_f64) & 7) == 0,
            "adam_step: misaligned pointer (theta, grad, m, v 4-byte; partials, norm_out 8-byte)");
  CHECK_ARG(isfinite(max_norm) && max_norm > 0.0, "adam_step: max_norm must be finite and > 0 (got %g)",
            max_norm);
  const int want = (int)cdiv64(n, slice_of(n));
  CHECK_ARG(n_partials == want, "adam_step: n_partials must be danet_gclip_partials(n) = %d (got %d)", want,
            n_partials);
  const int vec = (((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const int grid = (int)min((int64_t)2048, cdiv64(vec ? cdiv64(n, 4) : n, 256));
  gclip_adam_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(n, theta, grad, m, v, lr_t, beta1, beta2, eps, clip,
                                                           grad_scale, zero_grad, vec, max_norm, partials_f64,
                                                           n_partials, norm_out_f64);
  CHECK_LAUNCH();
  return DANET_GCLIP_OK;
}
