// Can the half-empty last k-block of lstm_fwd_fx_kernel's recurrent half (one real 16-k group paired with 16 k of
// zeros) run on v_mfma_f32_16x16x16_bf16 instead of v_mfma_f32_16x16x32_bf16?  Two questions:
//   1. rate: back-to-back instructions of either form on ONE SIMD (one wave, one workgroup), in the kernel's own
//      issue pattern (two column tiles x two accumulators, six piece products) and as one dependent chain
//   2. value: is the 16-k form on operand a bit for bit the 32-k form on [a | 0]?  Pieces (hi, mid, lo) of random
//      fp32 values of every binade up to 2^60, denormals, signed zeros; both accumulator chains of the kernel
//      (pieces PA / PB, t6 & 1), random start values; the zero half meets zero weights (the kernel's case) and
//      random weights
// hipcc --offload-arch=gfx950 -O3 -x hip tools/csrc/mfma_bf16_k16_vs_k32.hip -o /tmp/mfma_k16 && /tmp/mfma_k16
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <random>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

#define OP32(w0, w1, w2, w3) __builtin_bit_cast(bf16x8, (u32x4){w0, w1, w2, w3})
#define OP16(w0, w1) __builtin_bit_cast(s16x4, (u32x2){w0, w1})

// ---------------------------------------------------------------- rate
// MODE 0: 32-k form, 1: 16-k form; CHAINS accumulators taken in turn (4 = the kernel's pattern, 1 = one chain)
template <int MODE, int CHAINS>
__global__ __launch_bounds__(64) void rate(const uint32_t* in, float* out, unsigned long long* ticks, int iters) {
  const int lane = threadIdx.x;
  uint32_t a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { a[i] = in[lane * 8 + i]; b[i] = in[lane * 8 + 4 + i]; }
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  __builtin_amdgcn_s_waitcnt(0);
  const unsigned long long c0 = clock64(), w0 = wall_clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int s = 0; s < 12; ++s) {
      f32x4& d = acc[s % CHAINS];
      if (MODE == 0) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(OP32(a[0], a[1], a[2], a[3]), OP32(b[0], b[1], b[2], b[3]), d, 0, 0, 0);
      else d = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(OP16(a[0], a[1]), OP16(b[0], b[1]), d, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][3];
  asm volatile("" : "+v"(s));
  const unsigned long long c1 = clock64(), w1 = wall_clock64();
  if (lane == 0) { ticks[0] = c1 - c0; ticks[1] = w1 - w0; }
  if (s == 123.456f) out[0] = s;
}

// ---------------------------------------------------------------- value
// per trial and lane: A pieces [3][2 words] (4 k), B pieces [3][4 words] (words 2, 3: the weights the zero half
// meets), start accumulators [2][4]
#define TRIAL_WORDS (6 + 12 + 8)
__global__ __launch_bounds__(64) void value(const uint32_t* in, int ntrial, int zero_w, unsigned long long* bad, uint32_t* first) {
  const int lane = threadIdx.x;
  for (int tr = blockIdx.x; tr < ntrial; tr += gridDim.x) {
    const uint32_t* p = in + ((size_t)tr * 64 + lane) * TRIAL_WORDS;
    uint32_t a[3][2], b[3][4];
    f32x4 c32[2], c16[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) { a[i][0] = p[2 * i]; a[i][1] = p[2 * i + 1]; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) b[i][j] = (j >= 2 && zero_w) ? 0u : p[6 + 4 * i + j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) c32[i][j] = c16[i][j] = __uint_as_float(p[18 + 4 * i + j]);
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int t6 = 0; t6 < 6; ++t6) {
      const uint32_t* A = a[PA[t6]];
      const uint32_t* B = b[PB[t6]];
      c32[t6 & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(OP32(A[0], A[1], 0u, 0u), OP32(B[0], B[1], B[2], B[3]), c32[t6 & 1], 0, 0, 0);
      c16[t6 & 1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(OP16(A[0], A[1]), OP16(B[0], B[1]), c16[t6 & 1], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t x = __float_as_uint(c32[i][j]), y = __float_as_uint(c16[i][j]);
        if (x != y && atomicAdd(bad, 1ull) == 0) { first[0] = tr; first[1] = lane; first[2] = x; first[3] = y; }
      }
  }
}

static uint16_t bf16_rne(float x) {
  uint32_t u; memcpy(&u, &x, 4);
  u += 0x7FFF + ((u >> 16) & 1);
  return (uint16_t)(u >> 16);
}
static float bf16_f(uint16_t b) { uint32_t u = (uint32_t)b << 16; float x; memcpy(&x, &u, 4); return x; }
static void split3(float x, uint16_t* o) {
  o[0] = bf16_rne(x);
  const float r = x - bf16_f(o[0]);
  o[1] = bf16_rne(r);
  o[2] = bf16_rne(r - bf16_f(o[1]));
}

int main() {
  std::mt19937 rng(7);
  // kind 0: |x| ~ 1 (the kernel's data); 1: every binade 2^-126 .. 2^60; 2: denormals; 3: a mix with signed zeros
  auto draw = [&](int kind) -> float {
    const uint32_t r = rng();
    uint32_t u;
    if (kind == 0) { float f = std::normal_distribution<float>(0.f, 1.f)(rng); memcpy(&u, &f, 4); return f; }
    if (kind == 1) u = (r & 0x807FFFFFu) | ((1u + (rng() % 186u)) << 23);
    else if (kind == 2) u = r & 0x807FFFFFu;
    else {
      const uint32_t c = rng() % 8u;
      if (c == 0) u = r & 0x80000000u;
      else if (c == 1) u = r & 0x807FFFFFu;
      else u = (r & 0x807FFFFFu) | ((1u + (rng() % 186u)) << 23);
    }
    float f; memcpy(&f, &u, 4); return f;
  };
  const int NT = 8192;
  std::vector<uint32_t> h((size_t)NT * 64 * TRIAL_WORDS);
  uint32_t* din; unsigned long long* dbad; uint32_t* dfirst;
  hipMalloc(&din, h.size() * 4); hipMalloc(&dbad, 8); hipMalloc(&dfirst, 16);
  const char* kn[] = {"normal(0,1)", "every binade to 2^60", "denormals", "mix with signed zeros"};
  unsigned long long total_bad = 0;
  for (int kind = 0; kind < 4; ++kind) {
    for (size_t tl = 0; tl < (size_t)NT * 64; ++tl) {
      uint32_t* p = h.data() + tl * TRIAL_WORDS;
      uint16_t pa[4][3], pb[8][3];
      for (int e = 0; e < 4; ++e) split3(draw(kind), pa[e]);
      for (int e = 0; e < 8; ++e) split3(draw(kind), pb[e]);
      for (int i = 0; i < 3; ++i) {
        for (int w = 0; w < 2; ++w) p[2 * i + w] = pa[2 * w][i] | ((uint32_t)pa[2 * w + 1][i] << 16);
        for (int w = 0; w < 4; ++w) p[6 + 4 * i + w] = pb[2 * w][i] | ((uint32_t)pb[2 * w + 1][i] << 16);
      }
      for (int j = 0; j < 8; ++j) { float c = (j & 1) ? draw(kind) : 0.f * draw(3); memcpy(&p[18 + j], &c, 4); }
    }
    hipMemcpy(din, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    for (int zero_w = 1; zero_w >= 0; --zero_w) {
      unsigned long long bad = 0; uint32_t first[4] = {0, 0, 0, 0};
      hipMemset(dbad, 0, 8);
      value<<<256, 64>>>(din, NT, zero_w, dbad, dfirst);
      hipMemcpy(&bad, dbad, 8, hipMemcpyDeviceToHost);
      hipMemcpy(first, dfirst, 16, hipMemcpyDeviceToHost);
      printf("value  %-24s zero half meets %-14s: %llu of %llu words differ", kn[kind],
             zero_w ? "zero weights" : "random weights", bad, (unsigned long long)NT * 64 * 8);
      if (bad) printf("  (first: trial %u lane %u  32-k %08x  16-k %08x)", first[0], first[1], first[2], first[3]);
      printf("\n");
      total_bad += bad;
    }
  }
  // rate
  float* out; unsigned long long* dt;
  hipMalloc(&out, 4); hipMalloc(&dt, 16);
  const int iters = 20000;
  double clk[2][2];
  for (int chains = 4; chains >= 1; chains -= 3)
    for (int mode = 0; mode < 2; ++mode) {
      unsigned long long t[2] = {0, 0};
      for (int rep = 0; rep < 3; ++rep) {
        if (chains == 4) { if (mode) rate<1, 4><<<1, 64>>>(din, out, dt, iters); else rate<0, 4><<<1, 64>>>(din, out, dt, iters); }
        else { if (mode) rate<1, 1><<<1, 64>>>(din, out, dt, iters); else rate<0, 1><<<1, 64>>>(din, out, dt, iters); }
        hipMemcpy(t, dt, 16, hipMemcpyDeviceToHost);
      }
      const double n = (double)iters * 12;
      clk[chains == 1][mode] = t[0] / n;
      printf("rate   %s, %d accumulator(s) in turn: %6.2f shader clocks, %6.2f ns per instruction\n",
             mode ? "v_mfma_f32_16x16x16_bf16" : "v_mfma_f32_16x16x32_bf16", chains, t[0] / n, t[1] * 10.0 / n);
    }
  printf("ratio 16-k / 32-k: %.2f (four accumulators), %.2f (one chain); bit-identical: %s\n",
         clk[0][1] / clk[0][0], clk[1][1] / clk[1][0], total_bad ? "NO" : "yes");
  return 0;
}
