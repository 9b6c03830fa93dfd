/*
 * libdanet_gclip_hip.so (include/danet_gclip_hip.h): the global L2 norm of the flat gradient and the clip + Adam
 * update scaled by the clip coefficient.  gfx950, wave64.
 *
 * danet_gclip_sumsq.  The slice loop of mix_power_kernel (csrc/mix/mix.hip) on one flat buffer: one workgroup of
 * 256 threads per partial, 16-byte loads at stride 256 with four in flight, the exact float64 squares of a vector
 * added as (a + b) + (c + d), a fixed butterfly over the wave and (w0 + w1) + (w2 + w3) through LDS; thread 0
 * stores the one float64 of the workgroup.
 *
 * danet_gclip_adam_step.  adam_clip_kernel of csrc/pointwise.hip (adam_one verbatim, the same grid, the same
 * 16-byte path and tail) behind a prologue in which EVERY workgroup adds the partials in one fixed order and forms
 * norm, coef and the factor k itself: no workgroup waits for another.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "danet_gclip_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

static thread_local char g_err[256] = "";

static void gclip_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* danet_gclip_last_error(void) { return g_err; }
extern "C" int danet_gclip_abi_version(void) { return DANET_GCLIP_ABI_VERSION; }

#define GCLIP_CHECK_ARG(cond, ...)   \
  do {                               \
    if (!(cond)) {                   \
      gclip_set_error(__VA_ARGS__);  \
      return DANET_GCLIP_ERR_ARG;    \
    }                                \
  } while (0)

#define GCLIP_CHECK_LAUNCH()                                                                          \
  do {                                                                                                \
    const hipError_t e_ = hipGetLastError();                                                          \
    if (e_ != hipSuccess) {                                                                           \
      gclip_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return DANET_GCLIP_ERR_LAUNCH;                                                                  \
    }                                                                                                 \
  } while (0)

static const int kThreads = 256;
static const int kWaves = kThreads / 64;

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

/* slice(n) of THE RULE */
static int64_t slice_of(int64_t n) {
  int64_t s = (cdiv64(n, DANET_GCLIP_MAX_PARTIALS) + 3) & ~(int64_t)3;
  return s < DANET_GCLIP_MIN_SLICE ? DANET_GCLIP_MIN_SLICE : s;
}

extern "C" int danet_gclip_partials(int64_t n) {
  if (n < 1 || n > DANET_GCLIP_MAX_N) {
    gclip_set_error("partials: n must be in [1, 2^40] (got %lld)", (long long)n);
    return 0;
  }
  return (int)cdiv64(n, slice_of(n));
}

/* ---------------------------------------------------------------------------------- sum of squares */
__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }
__device__ __forceinline__ double sq4(f32x4 v) { return (sq(v[0]) + sq(v[1])) + (sq(v[2]) + sq(v[3])); }

/* every thread: the sum of the 256 accumulators over the fixed tree of THE RULE */
__device__ __forceinline__ double block_sum(double acc, double* part) {
  const int tid = threadIdx.x;
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);     /* every lane: the wave's sum */
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(kThreads) void gclip_sumsq_kernel(int64_t n_total, int64_t slice,
                                                                const float* __restrict__ g,
                                                                double* __restrict__ partials) {
  __shared__ double part[kWaves];
  const int tid = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * slice;           /* < n_total: the grid is partials(n) */
  const int64_t n = min(slice, n_total - b);
  const float* x = g + b;
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

  const double r = block_sum(acc, part);
  if (tid == 0) partials[blockIdx.x] = r;
}

extern "C" int danet_gclip_sumsq(void* stream, int64_t n, const float* grad, double* partials_f64, int n_partials) {
  GCLIP_CHECK_ARG(n >= 1 && n <= DANET_GCLIP_MAX_N, "sumsq: n must be in [1, 2^40] (got %lld)", (long long)n);
  GCLIP_CHECK_ARG(grad && partials_f64, "sumsq: null pointer");
  GCLIP_CHECK_ARG(((uintptr_t)grad & 3) == 0 && ((uintptr_t)partials_f64 & 7) == 0,
                  "sumsq: misaligned pointer (grad 4-byte, partials 8-byte)");
  const int64_t slice = slice_of(n);
  const int want = (int)cdiv64(n, slice);
  GCLIP_CHECK_ARG(n_partials == want, "sumsq: n_partials must be danet_gclip_partials(n) = %d (got %d)", want,
                  n_partials);
  gclip_sumsq_kernel<<<dim3((unsigned)want), kThreads, 0, (hipStream_t)stream>>>(n, slice, grad, partials_f64);
  GCLIP_CHECK_LAUNCH();
  return DANET_GCLIP_OK;
}

/* ---------------------------------------------------------------------------------- clip + TF1 Adam */
/* adam_one of csrc/pointwise.hip, verbatim */
__device__ __forceinline__ void adam_one(float& th, float& gi, float& mi, float& vi, float lr_t,
                                         float b1, float b2, float eps, float clip, float gscale) {
  float g = gi * gscale;
  if (clip > 0.f) g = (g != g) ? g : fminf(fmaxf(g, -clip), clip);   // main.py:359-362
  mi = b1 * mi + (1.f - b1) * g;
  vi = b2 * vi + (1.f - b2) * g * g;
  th -= lr_t * mi / (sqrtf(vi) + eps);                              // eps outside the root (TF1)
}

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
  GCLIP_CHECK_ARG(n >= 1 && n <= DANET_GCLIP_MAX_N, "adam_step: n must be in [1, 2^40] (got %lld)", (long long)n);
  GCLIP_CHECK_ARG(theta && grad && m && v && partials_f64 && norm_out_f64, "adam_step: null pointer");
  GCLIP_CHECK_ARG((((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 3) == 0 &&
                      (((uintptr_t)partials_f64 | (uintptr_t)norm_out_f64) & 7) == 0,
                  "adam_step: misaligned pointer (theta, grad, m, v 4-byte; partials, norm_out 8-byte)");
  GCLIP_CHECK_ARG(isfinite(max_norm) && max_norm > 0.0, "adam_step: max_norm must be finite and > 0 (got %g)",
                  max_norm);
  const int want = (int)cdiv64(n, slice_of(n));
  GCLIP_CHECK_ARG(n_partials == want, "adam_step: n_partials must be danet_gclip_partials(n) = %d (got %d)", want,
                  n_partials);
  const int vec = (((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const int grid = (int)min((int64_t)2048, cdiv64(vec ? cdiv64(n, 4) : n, 256));
  gclip_adam_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(n, theta, grad, m, v, lr_t, beta1, beta2, eps, clip,
                                                           grad_scale, zero_grad, vec, max_norm, partials_f64,
                                                           n_partials, norm_out_f64);
  GCLIP_CHECK_LAUNCH();
  return DANET_GCLIP_OK;
}
