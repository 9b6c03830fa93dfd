/*
 * libdanet_noise_hip.so (include/danet_noise_hip.h): the model's front-end over the mixture of C sources and
 * one scaled noise row that is not a target.  gfx950, wave64.
 *
 * danet_noise_frontend_fwd.  One pass.  The batch item b has a grid dimension of its own (no division per
 * element); a workgroup is ONE wave that takes 64 consecutive elements of one item, a lane one complex element:
 * 8-byte loads and stores of the complex rows, 4-byte stores of the real ones, coalesced.  The C source loads of
 * an element are independent (C is a template parameter, the loop is unrolled), so they are all in flight together.
 * MEASURED, and the reason for this shape: at the cfg-2 shape the pass moves 25 MB in 7 us, under half of what HBM
 * delivers -- it is bound by the latency of the hypot / log1p / atan2 / sincos chains, not by bandwidth.  Two
 * elements per lane behind 16-byte accesses halve the number of waves that hide that latency and cost 8.8 us
 * against 7.0 us for this form and 7.8 us for the core kernel on C + 1 rows (tools/bench_noise.py, README);
 * workgroups of one wave instead of four spread the 8256 waves evenly over the SIMDs (7.0 against 7.3 us).
 * Contraction is OFF for this file: fl(g * n) is rounded before it is added, as the header promises.
 */
#include <hip/hip_runtime.h>

#include "danet_noise_hip.h"
#define DANET_EXT noise
#define DANET_EXT_UPPER NOISE
#include "ext_core.h"

#pragma clang fp contract(off)


static const int kThreads = 64;          /* one wave per workgroup */
static const int64_t kMaxN = (int64_t)1 << 40;
static const int64_t kMaxTotal = (int64_t)1 << 58;
static const unsigned kMaxGridX = 1u << 20;      /* workgroups along N; a workgroup strides on beyond them */
static const unsigned kMaxGridY = 65535u;        /* batch items; a workgroup strides on beyond them        */

struct NoiseArgs {
  const float2* src;
  const float2* noise;
  const float* gain;
  float* mix_pwr;
  float* mix_log;
  float2* phasor;
  float* src_pwr;
  float2* mix;
  int64_t N;
  int B;
};

template <int C>
__global__ __launch_bounds__(kThreads) void noise_frontend_kernel(NoiseArgs a) {
  const int64_t N = a.N;
  for (int b = (int)blockIdx.y; b < a.B; b += (int)gridDim.y) {
    const float g = a.gain ? a.gain[b] : 1.f;
    const int64_t mrow = (int64_t)b * N;                    /* the item's row of every [B][N] array */
    const float2* __restrict__ src = a.src + mrow * C;      /* its C source rows, N apart           */
    float* __restrict__ sp = a.src_pwr + mrow * C;
    for (int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x; n < N; n += (int64_t)gridDim.x * kThreads) {
      float2 s[C];
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] = src[(int64_t)c * N + n];
      const float2 nz = a.noise[mrow + n];
      float re = 0.f, im = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        re = re + s[c].x;
        im = im + s[c].y;
        sp[(int64_t)c * N + n] = hypotf(s[c].x, s[c].y);
      }
      /* two roundings (contraction is off): the product, then the sum */
      const float gx = g * nz.x, gy = g * nz.y;
      re = re + gx;
      im = im + gy;
      const float mag = hypotf(re, im);
      if (a.mix) a.mix[mrow + n] = make_float2(re, im);
      a.mix_pwr[mrow + n] = mag;
      a.mix_log[mrow + n] = log1pf(mag);
      const float ph = atan2f(im, re);
      a.phasor[mrow + n] = make_float2(cosf(ph), sinf(ph));
    }
  }
}

template <int C>
static void launch(dim3 grid, hipStream_t stream, const NoiseArgs& a) {
  noise_frontend_kernel<C><<<grid, kThreads, 0, stream>>>(a);
}

extern "C" int danet_noise_frontend_fwd(void* stream, int B, int C, int64_t N, const float* src_c64,
                                        const float* noise_c64, const float* gain, float* mix_pwr, float* mix_log,
                                        float* phasor, float* src_pwr, float* mix_c64) {
  CHECK_ARG(B >= 1, "frontend_fwd: B must be >= 1 (got %d)", B);
  CHECK_ARG(C >= 1 && C <= DANET_NOISE_MAX_C, "frontend_fwd: C must be in [1, %d] (got %d)", DANET_NOISE_MAX_C,
            C);
  CHECK_ARG(N >= 1 && N < kMaxN, "frontend_fwd: N must be in [1, 2^40) (got %lld)", (long long)N);
  CHECK_ARG((int64_t)B * C <= kMaxTotal / N, "frontend_fwd: B * C * N must be < 2^58");
  CHECK_ARG(src_c64 && noise_c64 && mix_pwr && mix_log && phasor && src_pwr,
            "frontend_fwd: null pointer (src, noise, mix_pwr, mix_log, phasor and src_pwr are required)");
  CHECK_ARG(((uintptr_t)src_c64 & 7) == 0 && ((uintptr_t)noise_c64 & 7) == 0 && ((uintptr_t)phasor & 7) == 0 &&
                ((uintptr_t)mix_c64 & 7) == 0 && ((uintptr_t)gain & 3) == 0 && ((uintptr_t)mix_pwr & 3) == 0 &&
                ((uintptr_t)mix_log & 3) == 0 && ((uintptr_t)src_pwr & 3) == 0,
            "frontend_fwd: misaligned pointer (src, noise, phasor, mix_c64 8-byte; gain, mix_pwr, mix_log, "
            "src_pwr 4-byte)");
  NoiseArgs a;
  a.src = (const float2*)src_c64; a.noise = (const float2*)noise_c64; a.gain = gain;
  a.mix_pwr = mix_pwr; a.mix_log = mix_log; a.phasor = (float2*)phasor; a.src_pwr = src_pwr;
  a.mix = (float2*)mix_c64; a.N = N; a.B = B;
  const int64_t chunks = (N + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)(chunks < (int64_t)kMaxGridX ? chunks : (int64_t)kMaxGridX),
                  (unsigned)B < kMaxGridY ? (unsigned)B : kMaxGridY);
  const hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: launch<1>(grid, s, a); break;
    case 2: launch<2>(grid, s, a); break;
    case 3: launch<3>(grid, s, a); break;
    case 4: launch<4>(grid, s, a); break;
    case 5: launch<5>(grid, s, a); break;
    case 6: launch<6>(grid, s, a); break;
    case 7: launch<7>(grid, s, a); break;
    default: launch<8>(grid, s, a); break;
  }
  CHECK_LAUNCH();
  return DANET_NOISE_OK;
}
