/*
 * libdanet_online_hip.so: the online attractor estimator (include/danet_online_hip.h, THE RULE): a serial scan over
 * the frames of every utterance, one workgroup per utterance, and the fully parallel separator with a per-frame
 * attractor.  Three kernels, no workspace, no atomics, every output element written once by one thread.
 */
#include "danet_online_hip.h"
#define DANET_EXT online
#define DANET_EXT_UPPER ONLINE
#include "ext_core.h"

#include <math.h>
#include <stdint.h>

static constexpr int kNT = 256;                      // threads of every workgroup here
static constexpr int kNW = kNT / 64;
static constexpr int kMaxC = DANET_ONLINE_MAX_C;
static constexpr int kMaxE = DANET_ONLINE_MAX_E;
static constexpr int kMaxF = DANET_ONLINE_MAX_F;
static constexpr int kMaxJ = (kMaxF + kNT - 1) / kNT;  // bins per thread of the scan: 5
static constexpr int kUnroll = 8;                      // bins in flight per thread in the contraction of the scan
static_assert(kMaxC == 4, "a bin's W m is one 16-byte LDS slot");
static_assert(kMaxC * kMaxE == kNT, "thread k loads table entry k and owns state entry k");

// ---- the wave sum of the head kernels (wave_sum_n of the core library): adds inside a row of 16 lanes, two row
// broadcasts and one readlane per value, step by step ACROSS the values so that consecutive instructions are
// independent.  Fixed order; every lane of the wave must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_shuffled(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, true));
}
template <int N>
__device__ __forceinline__ void wave_sum_n(float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_shuffled<0xB1, 0xF>(v[i]);     // quad_perm [1,0,3,2]: lane ^ 1
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_shuffled<0x4E, 0xF>(v[i]);     // quad_perm [2,3,0,1]: lane ^ 2
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_shuffled<0x141, 0xF>(v[i]);    // row_half_mirror: the other quad
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_shuffled<0x140, 0xF>(v[i]);    // row_mirror: the other half row
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_shuffled<0x142, 0xA>(v[i]);    // row_bcast:15 into rows 1 and 3
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_shuffled<0x143, 0xC>(v[i]);    // row_bcast:31 into rows 2 and 3
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[i]), 63));
}

// ---- steps 1 and 2 of THE RULE for one bin, shared by the scan and the separator ------------------------------
// the first 16 bytes of an embedding row (E a multiple of 4: the row is 16-byte aligned), or its first element
__device__ __forceinline__ f32x4 row_head(const float* __restrict__ row, int E) {
  if ((E & 3) == 0) return *reinterpret_cast<const f32x4*>(row);
  return (f32x4){row[0], 0.f, 0.f, 0.f};
}

// lg[c] += v . tab[c][e .. e + 3] for c < C, in ascending e
__device__ __forceinline__ void fma_chunk(f32x4 v, int e, int C, const float* tab, float (&lg)[kMaxC]) {
#pragma unroll
  for (int c = 0; c < kMaxC; ++c)
    if (c < C) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(tab + c * kMaxE + e);
      lg[c] = fmaf(v.x, a.x, lg[c]);
      lg[c] = fmaf(v.y, a.y, lg[c]);
      lg[c] = fmaf(v.z, a.z, lg[c]);
      lg[c] = fmaf(v.w, a.w, lg[c]);
    }
}

// lg[c] = row . tab[c], fused multiply-adds in ascending e from +0; tab is the LDS table [kMaxC][kMaxE].  The row is
// fetched kBatch loads at a time, all of a batch in flight together (E is uniform: the guards are scalar branches).
static constexpr int kBatch = 4;
__device__ __forceinline__ void bin_logits(const float* __restrict__ row, int E, int C, const float* tab, f32x4 head,
                                           float (&lg)[kMaxC]) {
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) lg[c] = 0.f;
  if ((E & 3) == 0) {
    fma_chunk(head, 0, C, tab, lg);
    for (int e = 4; e < E; e += 4 * kBatch) {
      f32x4 v[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k)
        if (e + 4 * k < E) v[k] = *reinterpret_cast<const f32x4*>(row + e + 4 * k);
#pragma unroll
      for (int k = 0; k < kBatch; ++k)
        if (e + 4 * k < E) fma_chunk(v[k], e + 4 * k, C, tab, lg);
    }
  } else {
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) lg[c] = fmaf(head.x, tab[c * kMaxE], lg[c]);
    for (int e = 1; e < E; e += 2 * kBatch) {
      float x[2 * kBatch];
#pragma unroll
      for (int k = 0; k < 2 * kBatch; ++k)
        if (e + k < E) x[k] = row[e + k];
#pragma unroll
      for (int k = 0; k < 2 * kBatch; ++k)
        if (e + k < E) {
#pragma unroll
          for (int c = 0; c < kMaxC; ++c)
            if (c < C) lg[c] = fmaf(x[k], tab[c * kMaxE + e + k], lg[c]);
        }
    }
  }
}

// lg -> the masks, in place; the entries c >= C become 0
__device__ __forceinline__ void activate(int act, int C, float (&lg)[kMaxC]) {
  if (act == 0) {
    float mx = lg[0];
#pragma unroll
    for (int c = 1; c < kMaxC; ++c)
      if (c < C) mx = fmaxf(mx, lg[c]);
    float den = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) {
        lg[c] = expf(lg[c] - mx);
        den += lg[c];
      }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) lg[c] = (c < C) ? lg[c] / den : 0.f;
  } else {
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) lg[c] = (c < C) ? 1.0f / (1.0f + expf(-lg[c])) : 0.f;
  }
}

// ---- danet_online_init ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void online_init_kernel(int64_t total, int C, int E, const float* __restrict__ a0,
                                                          double* __restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (i >= total) return;
  const int CE = C * E, per = 2 * CE + C;
  const int64_t b = i / per;
  const int k = (int)(i - b * per);
  state[i] = (k < CE + C) ? 0.0 : (double)a0[b * CE + (k - CE - C)];
}

// ---- danet_online_scan ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void online_scan_kernel(int C, int T, int F, int E, int act, double lambda, int T0,
                                                          int64_t t_first, double eps,
                                                          const float* __restrict__ embed, const float* __restrict__ w,
                                                          double* __restrict__ state, float* __restrict__ attr) {
  __shared__ __attribute__((aligned(16))) float tab[kMaxC * kMaxE];    // the attractors in force
  __shared__ __attribute__((aligned(16))) float wm[kMaxF * kMaxC];     // W m of the frame, a 16-byte slot per bin
  __shared__ float part[kMaxC * kNT];                                  // [c][thread]: the partial sums of s
  __shared__ float qw[kNW * kMaxC];                                    // [wave][c]: the wave sums of q
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int CE = C * E;
  const int P = E < 4 ? 4 : E, G = kNT / P, pg = tid / P, pe = tid - pg * P;
  // thread c E + e owns S[c][e], A[c][e] and a copy of n[c], in registers for the whole call
  const bool owner = tid < CE;
  const int oc = owner ? tid / E : 0, oe = owner ? tid - oc * E : 0;
  double* st = state + (int64_t)b * (2 * CE + C);
  double S = 0.0, n = 0.0;
  float a = 0.f;
  if (owner) {
    S = st[tid];
    n = st[CE + oc];
    a = (float)st[CE + C + tid];
  }
  {
    const int c = tid / kMaxE, e = tid % kMaxE;
    tab[tid] = (c < C && e < E) ? (float)st[CE + C + c * E + e] : 0.f;
  }
  const float* vt = embed + (int64_t)b * T * F * E;
  const float* wt = w + (int64_t)b * T * F;
  float* at = attr + (int64_t)b * T * CE;
  f32x4 head[kMaxJ];
#pragma unroll
  for (int j = 0; j < kMaxJ; ++j) {
    const int f = tid + j * kNT;
    head[j] = (f < F) ? row_head(vt + (int64_t)f * E, E) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  for (int t = 0; t < T; ++t, vt += (int64_t)F * E, wt += F, at += CE) {
    // (a) a thread per bin: logits, masks, W m into LDS, the q partial sums
    float qa[kMaxC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kMaxJ; ++j) {
      const int f = tid + j * kNT;
      if (f < F) {
        float lg[kMaxC];
        bin_logits(vt + (int64_t)f * E, E, C, tab, head[j], lg);
        activate(act, C, lg);
        const float wv = wt[f];
        const f32x4 o = {wv * lg[0], wv * lg[1], wv * lg[2], wv * lg[3]};
        *reinterpret_cast<f32x4*>(wm + f * kMaxC) = o;
        qa[0] += o.x; qa[1] += o.y; qa[2] += o.z; qa[3] += o.w;
      }
    }
    wave_sum_n<kMaxC>(qa);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) qw[wave * kMaxC + c] = qa[c];
    }
    __syncthreads();
    // the row heads of frame t + 1, in flight while this frame reduces
    if (t + 1 < T) {
#pragma unroll
      for (int j = 0; j < kMaxJ; ++j) {
        const int f = tid + j * kNT;
        if (f < F) head[j] = row_head(vt + (int64_t)(F + f) * E, E);
      }
    }
    // (b) thread (pe, pg): column pe of the bins pg, pg + G, ... against their W m
    float acc[kMaxC] = {0.f, 0.f, 0.f, 0.f};
    if (pe < E && pg < G) {
      for (int f0 = pg; f0 < F; f0 += kUnroll * G) {    // kUnroll loads in flight together, then their multiply-adds
        float x[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
          const int f = f0 + k * G;
          if (f < F) x[k] = vt[(int64_t)f * E + pe];
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
          const int f = f0 + k * G;
          if (f < F) {
            const f32x4 m = *reinterpret_cast<const f32x4*>(wm + f * kMaxC);
            acc[0] = fmaf(m.x, x[k], acc[0]);
            acc[1] = fmaf(m.y, x[k], acc[1]);
            acc[2] = fmaf(m.z, x[k], acc[2]);
            acc[3] = fmaf(m.w, x[k], acc[3]);
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) part[c * kNT + tid] = acc[c];
    __syncthreads();
    // (c) the owners: the G partial sums, the float64 state, the attractor of this frame
    if (owner) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += part[oc * kNT + g * P + oe];
      float q = qw[oc];
#pragma unroll
      for (int v = 1; v < kNW; ++v) q += qw[v * kMaxC + oc];
      S = fma(lambda, S, (double)s);
      n = fma(lambda, n, (double)q);
      if (t_first + t >= (int64_t)T0 && n > eps) a = (float)(S / n);
      tab[oc * kMaxE + oe] = a;
      at[tid] = a;
    }
    __syncthreads();
  }
  if (owner) {
    st[tid] = S;
    if (oe == 0) st[CE + oc] = n;
    st[CE + C + tid] = (double)a;
  }
}

// ---- danet_online_separate --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void online_separate_kernel(int act, int C, int T, int F, int E,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ attr,
                                                              const float* __restrict__ embed,
                                                              float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tab[kMaxC * kMaxE];
  const int tid = threadIdx.x;
  const int64_t bt = blockIdx.x;                     // b T + t
  const int64_t b = bt / T, t = bt - b * T;
  {
    const int c = tid / kMaxE, e = tid % kMaxE;
    tab[tid] = (c < C && e < E) ? attr[bt * C * E + c * E + e] : 0.f;
  }
  __syncthreads();
  const float* vt = embed + bt * F * E;
  const float* wt = w + bt * F;
  for (int f = tid; f < F; f += kNT) {
    const float* row = vt + (int64_t)f * E;
    float lg[kMaxC];
    bin_logits(row, E, C, tab, row_head(row, E), lg);
    activate(act, C, lg);
    const float wv = wt[f];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) out[((b * C + c) * T + t) * F + f] = wv * lg[c];
  }
}

// ---- the host side ----------------------------------------------------------------------------------------------
static bool ce_ok(const char* who, int C, int E) {
  if (C < 1 || C > kMaxC || E < 1 || E > kMaxE) {
    set_error("%s: need 1 <= C <= %d and 1 <= E <= %d (got C = %d, E = %d)", who, kMaxC, kMaxE, C, E);
    return false;
  }
  return true;
}

static bool envelope_ok(const char* who, int B, int C, int T, int F, int E) {
  if (!ce_ok(who, C, E)) return false;
  if (B < 1 || T < 1 || T > DANET_ONLINE_MAX_T || F < 1 || F > kMaxF) {
    set_error("%s: need B >= 1, 1 <= T <= %d and 1 <= F <= %d (got B = %d, T = %d, F = %d)", who, DANET_ONLINE_MAX_T,
              kMaxF, B, T, F);
    return false;
  }
  const int64_t BT = (int64_t)B * T, lim = (int64_t)1 << 31;
  if (BT * F * E >= lim || BT * C * F >= lim || BT * C * E >= lim) {
    set_error("%s: B T F E, B C T F and B T C E must be < 2^31 (got B = %d, C = %d, T = %d, F = %d, E = %d)", who, B, C,
              T, F, E);
    return false;
  }
  return true;
}

static bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" size_t danet_online_state_bytes(int C, int E) {
  if (!ce_ok("state_bytes", C, E)) return (size_t)-1;
  return sizeof(double) * (size_t)(2 * C * E + C);
}

extern "C" int danet_online_init(void* stream, int B, int C, int E, const float* a0, void* state) {
  if (!ce_ok("init", C, E)) return DANET_ONLINE_ERR_ARG;
  CHECK_ARG(B >= 1, "init: need B >= 1 (got %d)", B);
  const int64_t total = (int64_t)B * (2 * C * E + C);
  CHECK_ARG(total < ((int64_t)1 << 31), "init: B (2 C E + C) must be < 2^31 (got B = %d, C = %d, E = %d)", B, C, E);
  CHECK_ARG(a0 && state, "init: null pointer");
  CHECK_ARG(aligned_to(a0, 4) && aligned_to(state, 8), "init: misaligned pointer (a0 4-byte; state 8-byte)");
  online_init_kernel<<<(unsigned)((total + kNT - 1) / kNT), kNT, 0, (hipStream_t)stream>>>(total, C, E, a0,
                                                                                          (double*)state);
  CHECK_LAUNCH();
  return DANET_ONLINE_OK;
}

extern "C" int danet_online_scan(void* stream, int B, int C, int T, int F, int E, int act, double lambda, int T0,
                                 int64_t t_first, double eps, const float* embed, const float* w, void* state,
                                 float* attr) {
  if (!envelope_ok("scan", B, C, T, F, E)) return DANET_ONLINE_ERR_ARG;
  CHECK_ARG(act == 0 || act == 1, "scan: act must be 0 (softmax) or 1 (sigmoid) (got %d)", act);
  CHECK_ARG(lambda > 0.0 && lambda <= 1.0, "scan: need 0 < lambda <= 1 (got %g)", lambda);
  CHECK_ARG(T0 >= 1, "scan: need T0 >= 1 (got %d)", T0);
  CHECK_ARG(t_first >= 0, "scan: need t_first >= 0 (got %lld)", (long long)t_first);
  CHECK_ARG(eps >= 0.0 && eps <= 1.7e308, "scan: eps must be finite and >= 0 (got %g)", eps);
  CHECK_ARG(embed && w && state && attr, "scan: null pointer");
  CHECK_ARG(aligned_to(embed, (E & 3) ? 4 : 16) && aligned_to(w, 4) && aligned_to(attr, 4) && aligned_to(state, 8),
            "scan: misaligned pointer (embed 16-byte when E is a multiple of 4, else 4-byte; w, attr 4-byte; state "
            "8-byte)");
  online_scan_kernel<<<B, kNT, 0, (hipStream_t)stream>>>(C, T, F, E, act, lambda, T0, t_first, eps, embed, w,
                                                        (double*)state, attr);
  CHECK_LAUNCH();
  return DANET_ONLINE_OK;
}

extern "C" int danet_online_separate(void* stream, int act, int B, int C, int T, int F, int E, const float* w,
                                     const float* attr, const float* embed, float* out) {
  if (!envelope_ok("separate", B, C, T, F, E)) return DANET_ONLINE_ERR_ARG;
  CHECK_ARG(act == 0 || act == 1, "separate: act must be 0 (softmax) or 1 (sigmoid) (got %d)", act);
  CHECK_ARG(w && attr && embed && out, "separate: null pointer");
  CHECK_ARG(aligned_to(embed, (E & 3) ? 4 : 16) && aligned_to(w, 4) && aligned_to(attr, 4) && aligned_to(out, 4),
            "separate: misaligned pointer (embed 16-byte when E is a multiple of 4, else 4-byte; w, attr, out 4-byte)");
  online_separate_kernel<<<(unsigned)((int64_t)B * T), kNT, 0, (hipStream_t)stream>>>(act, C, T, F, E, w, attr, embed,
                                                                                     out);
  CHECK_LAUNCH();
  return DANET_ONLINE_OK;
}
