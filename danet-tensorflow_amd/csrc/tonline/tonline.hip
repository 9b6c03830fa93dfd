/*
 * libdanet_tonline_hip.so: the truth-online estimator with its backward, and the backward of the per-frame-attractor
 * separator (include/danet_tonline_hip.h, THE RULE).  Five kernels: three with one workgroup per frame (b, t), two
 * scans with one workgroup per utterance over T (C E + C) values.  No workspace, no atomics, every output element
 * written once by one thread.
 */
#include "danet_tonline_hip.h"
#define DANET_EXT tonline
#define DANET_EXT_UPPER TONLINE
#include "ext_core.h"

#include <math.h>
#include <stdint.h>

static constexpr int kNT = 256;                      // threads of every workgroup here
static constexpr int kNW = kNT / 64;
static constexpr int kMaxC = DANET_TONLINE_MAX_C;
static constexpr int kMaxE = DANET_TONLINE_MAX_E;
static constexpr int kMaxF = DANET_TONLINE_MAX_F;
static constexpr int kMaxJ = (kMaxF + kNT - 1) / kNT;  // bins per thread of a thread-per-bin phase: 5
static constexpr int kUnroll = 4;                      // rows in flight per thread in the contraction
static constexpr int kBlock = 16;                      // partial sums per block of the final addition
static constexpr int kAhead = 8;                       // frames a scan loads ahead
static constexpr int kPart = kMaxC * 4 * kNT;          // floats of the partial sums: G Q <= 256 threads x 4 columns x C
static_assert(kMaxC == 4, "a bin's slot is 16 bytes of LDS");
static_assert(kMaxC * kMaxE == kNT, "thread k loads table entry k and owns state entry k");

// ---- the wave sum of danet_online_scan (csrc/online/online.hip): adds inside a row of 16 lanes, two row broadcasts
// and one readlane per value.  Fixed order; every lane of the wave must be active.
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

// ---- the logits and the activation of danet_online_separate, statement for statement (csrc/online/online.hip keeps
// its own copy: the masks recomputed here must be the masks of that forward) ----------------------------------------
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

// lg[c] = row . tab[c], fused multiply-adds in ascending e from +0; tab is the LDS table [kMaxC][kMaxE]
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

// ---- what the three frame kernels share ------------------------------------------------------------------------
// step 1 of THE RULE: the lowest c that maximises P[c][t][f]; pf points at P[b][0][t][f], plane = T F
__device__ __forceinline__ int bin_label(const float* __restrict__ pf, int64_t plane, int C) {
  float best = pf[0];
  int k = 0;
#pragma unroll
  for (int c = 1; c < kMaxC; ++c)
    if (c < C) {
      const float x = pf[c * plane];
      if (x > best) {
        best = x;
        k = c;
      }
    }
  return k;
}

__device__ __forceinline__ f32x4 fma4(float s, f32x4 v, f32x4 a) {
  return (f32x4){fmaf(s, v.x, a.x), fmaf(s, v.y, a.y), fmaf(s, v.z, a.z), fmaf(s, v.w, a.w)};
}

// SUMMATION ORDER, s and dA: part[(g kMaxC + c) E + e] = sum over the bins f = g, g + G, ... of slot[f][c] *
// vt[f][e], one fused multiply-add per bin from +0.  kDv: the same thread stores dvt[f][e] = sum_c slot[f][c] *
// tab[c][e] (ascending c from +0) for the piece of the row it has loaded.  vt, dvt: the frame's [F][E]; slot: LDS
// [F][kMaxC], zero for c >= C; tab: LDS [kMaxC][kMaxE].
template <bool kDv>
__device__ __forceinline__ void contract(const float* __restrict__ vt, int F, int E, int C, const float* slot,
                                         const float* tab, float* part, float* __restrict__ dvt) {
  const int tid = threadIdx.x;
  if ((E & 3) == 0) {
    const int Q = E >> 2, G = kNT / Q, g = tid / Q, e = 4 * (tid - g * Q);
    if (g >= G) return;
    f32x4 acc[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 a[kMaxC];
    if (kDv) {
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) a[c] = *reinterpret_cast<const f32x4*>(tab + c * kMaxE + e);
    }
    for (int f0 = g; f0 < F; f0 += kUnroll * G) {      // kUnroll loads in flight together, then their multiply-adds
      f32x4 v[kUnroll];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const int f = f0 + k * G;
        if (f < F) v[k] = *reinterpret_cast<const f32x4*>(vt + (int64_t)f * E + e);
      }
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const int f = f0 + k * G;
        if (f < F) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(slot + f * kMaxC);
          acc[0] = fma4(m.x, v[k], acc[0]);
          acc[1] = fma4(m.y, v[k], acc[1]);
          acc[2] = fma4(m.z, v[k], acc[2]);
          acc[3] = fma4(m.w, v[k], acc[3]);
          if (kDv) {
            f32x4 d = fma4(m.x, a[0], (f32x4){0.f, 0.f, 0.f, 0.f});
            if (C > 1) d = fma4(m.y, a[1], d);
            if (C > 2) d = fma4(m.z, a[2], d);
            if (C > 3) d = fma4(m.w, a[3], d);
            *reinterpret_cast<f32x4*>(dvt + (int64_t)f * E + e) = d;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) *reinterpret_cast<f32x4*>(part + (g * kMaxC + c) * E + e) = acc[c];
  } else {
    const int G = kNT / E, g = tid / E, e = tid - g * E;
    if (g >= G) return;
    float acc[kMaxC] = {0.f, 0.f, 0.f, 0.f};
    float a[kMaxC];
    if (kDv) {
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) a[c] = tab[c * kMaxE + e];
    }
    for (int f0 = g; f0 < F; f0 += 2 * kUnroll * G) {
      float x[2 * kUnroll];
#pragma unroll
      for (int k = 0; k < 2 * kUnroll; ++k) {
        const int f = f0 + k * G;
        if (f < F) x[k] = vt[(int64_t)f * E + e];
      }
#pragma unroll
      for (int k = 0; k < 2 * kUnroll; ++k) {
        const int f = f0 + k * G;
        if (f < F) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(slot + f * kMaxC);
          acc[0] = fmaf(m.x, x[k], acc[0]);
          acc[1] = fmaf(m.y, x[k], acc[1]);
          acc[2] = fmaf(m.z, x[k], acc[2]);
          acc[3] = fmaf(m.w, x[k], acc[3]);
          if (kDv) {
            float d = fmaf(m.x, a[0], 0.f);
            if (C > 1) d = fmaf(m.y, a[1], d);
            if (C > 2) d = fmaf(m.z, a[2], d);
            if (C > 3) d = fmaf(m.w, a[3], d);
            dvt[(int64_t)f * E + e] = d;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) part[(g * kMaxC + c) * E + e] = acc[c];
  }
}

// the G partial sums of (c, e): blocks of kBlock in ascending g from +0, then the block sums in ascending block
__device__ __forceinline__ float block_sum(const float* part, int E, int c, int e) {
  const int G = kNT / ((E & 3) ? E : (E >> 2));
  float total = 0.f;
  for (int g0 = 0; g0 < G; g0 += kBlock) {
    const int g1 = g0 + kBlock < G ? g0 + kBlock : G;
    float blk = 0.f;
    for (int g = g0; g < g1; ++g) blk += part[(g * kMaxC + c) * E + e];
    total += blk;
  }
  return total;
}

// ---- danet_tonline_frame_sums -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void tonline_frame_sums_kernel(int C, int T, int F, int E,
                                                                 const float* __restrict__ embed,
                                                                 const float* __restrict__ src_pwr,
                                                                 const float* __restrict__ w, float* __restrict__ s,
                                                                 float* __restrict__ q) {
  __shared__ __attribute__((aligned(16))) float slot[kMaxF * kMaxC];   // W in the label's entry, a 16-byte slot per bin
  __shared__ __attribute__((aligned(16))) float part[kPart];
  __shared__ float qw[kNW * kMaxC];                                    // [wave][c]: the wave sums of q
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t bt = blockIdx.x;                     // b T + t
  const int64_t b = bt / T, t = bt - b * T, plane = (int64_t)T * F;
  const float* pt = src_pwr + (b * C * T + t) * F;
  const float* wt = w + bt * F;
  // (a) a thread per bin: the label, W into its slot, the q partial sums
  float qa[kMaxC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kMaxJ; ++j) {
    const int f = tid + j * kNT;
    if (f < F) {
      const int k = bin_label(pt + f, plane, C);
      const float wv = wt[f];
      const f32x4 o = {k == 0 ? wv : 0.f, k == 1 ? wv : 0.f, k == 2 ? wv : 0.f, k == 3 ? wv : 0.f};
      *reinterpret_cast<f32x4*>(slot + f * kMaxC) = o;
      qa[0] += o.x; qa[1] += o.y; qa[2] += o.z; qa[3] += o.w;
    }
  }
  wave_sum_n<kMaxC>(qa);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) qw[wave * kMaxC + c] = qa[c];
  }
  __syncthreads();
  // (b) thread (g, j): its columns of the rows g, g + G, ... against their slots
  contract<false>(embed + bt * F * E, F, E, C, slot, nullptr, part, nullptr);
  __syncthreads();
  // (c) the G partial sums; the four wave sums
  const int CE = C * E;
  if (tid < CE) {
    const int c = tid / E;
    s[bt * CE + tid] = block_sum(part, E, c, tid - c * E);
  }
  if (tid < C) {
    float x = qw[tid];
#pragma unroll
    for (int v = 1; v < kNW; ++v) x += qw[v * kMaxC + tid];
    q[bt * C + tid] = x;
  }
}

// ---- danet_tonline_scan -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void tonline_scan_kernel(int C, int T, int E, double lambda, int T0, double eps,
                                                           const float* __restrict__ s, const float* __restrict__ q,
                                                           float* __restrict__ attr, double* __restrict__ den) {
  const int tid = threadIdx.x, CE = C * E;
  if (tid >= CE) return;                             // no barrier in this kernel
  const int oc = tid / E;
  const bool first = tid == oc * E;                  // the thread that stores den[t][oc]
  const int64_t b = blockIdx.x;
  const float* sb = s + b * T * CE + tid;
  const float* qb = q + b * T * C + oc;
  float* ab = attr + b * T * CE + tid;
  double* db = den + b * T * C + oc;
  const int u0 = (T0 < T ? T0 : T) - 1;              // the frame whose attractors the hold shares
  double S = 0.0, n = 0.0;
  for (int t0 = 0; t0 < T; t0 += kAhead) {           // kAhead frames of loads in flight, then their recurrence
    float sv[kAhead], qv[kAhead];
#pragma unroll
    for (int i = 0; i < kAhead; ++i)
      if (t0 + i < T) {
        sv[i] = sb[(int64_t)(t0 + i) * CE];
        qv[i] = qb[(int64_t)(t0 + i) * C];
      }
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const int t = t0 + i;
      if (t < T) {
        S = fma(lambda, S, (double)sv[i]);
        n = fma(lambda, n, (double)qv[i]);
        if (t >= u0) {
          const double d = n + eps;
          const float a = d != 0.0 ? (float)(S / d) : 0.f;
          const int x0 = t == u0 ? 0 : t;            // frame u0 stores the hold as well
          for (int x = x0; x <= t; ++x) {
            ab[(int64_t)x * CE] = a;
            if (first) db[(int64_t)x * C] = d;
          }
        }
      }
    }
  }
}

// ---- danet_tonline_scan_bwd -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void tonline_scan_bwd_kernel(int C, int T, int E, double lambda, int T0,
                                                               const float* __restrict__ dattr,
                                                               const double* __restrict__ den,
                                                               float* __restrict__ r) {
  const int tid = threadIdx.x, CE = C * E;
  if (tid >= CE) return;                             // no barrier in this kernel
  const int oc = tid / E;
  const int64_t b = blockIdx.x;
  const float* gb = dattr + b * T * CE + tid;
  const double* db = den + b * T * C + oc;
  float* rb = r + b * T * CE + tid;
  const int u0 = (T0 < T ? T0 : T) - 1;
  double R = 0.0;
  // u = T - 1 .. u0 + 1: H_u = G_u / den[u]
  for (int t0 = T - 1; t0 > u0; t0 -= kAhead) {
    float gv[kAhead];
    double dv[kAhead];
#pragma unroll
    for (int i = 0; i < kAhead; ++i)
      if (t0 - i > u0) {
        gv[i] = gb[(int64_t)(t0 - i) * CE];
        dv[i] = db[(int64_t)(t0 - i) * C];
      }
#pragma unroll
    for (int i = 0; i < kAhead; ++i)
      if (t0 - i > u0) {
        const double H = dv[i] != 0.0 ? (double)gv[i] / dv[i] : 0.0;
        R = fma(lambda, R, H);
        rb[(int64_t)(t0 - i) * CE] = (float)R;
      }
  }
  // u = u0: every frame of the hold feeds it, G_0 .. G_u0 in ascending t
  double Gs = 0.0;
  for (int t0 = 0; t0 <= u0; t0 += kAhead) {
    float gv[kAhead];
#pragma unroll
    for (int i = 0; i < kAhead; ++i)
      if (t0 + i <= u0) gv[i] = gb[(int64_t)(t0 + i) * CE];
#pragma unroll
    for (int i = 0; i < kAhead; ++i)
      if (t0 + i <= u0) Gs += (double)gv[i];
  }
  const double d0 = db[(int64_t)u0 * C];
  R = fma(lambda, R, d0 != 0.0 ? Gs / d0 : 0.0);
  rb[(int64_t)u0 * CE] = (float)R;
  // u < u0: H_u = 0
  for (int u = u0 - 1; u >= 0; --u) {
    R = lambda * R;
    rb[(int64_t)u * CE] = (float)R;
  }
}

// ---- danet_tonline_sums_bwd -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void tonline_sums_bwd_kernel(int C, int T, int F, int E,
                                                               const float* __restrict__ src_pwr,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ r,
                                                               float* __restrict__ dembed) {
  __shared__ __attribute__((aligned(16))) float tab[kMaxC * kMaxE];    // R of the frame
  __shared__ float wl[kMaxF];                                          // W of the bin
  __shared__ int lab[kMaxF];                                           // k of the bin
  const int tid = threadIdx.x;
  const int64_t bt = blockIdx.x;
  const int64_t b = bt / T, t = bt - b * T, plane = (int64_t)T * F;
  {
    const int c = tid / kMaxE, e = tid % kMaxE;
    tab[tid] = (c < C && e < E) ? r[bt * C * E + c * E + e] : 0.f;
  }
  const float* pt = src_pwr + (b * C * T + t) * F;
  const float* wt = w + bt * F;
  for (int f = tid; f < F; f += kNT) {
    lab[f] = bin_label(pt + f, plane, C);
    wl[f] = wt[f];
  }
  __syncthreads();
  float* dvt = dembed + bt * F * E;
  if ((E & 3) == 0) {
    const int n4 = F * (E >> 2);
    for (int i = tid; i < n4; i += kNT) {
      const int f = (4 * i) / E, e = 4 * i - f * E;
      const f32x4 a = *reinterpret_cast<const f32x4*>(tab + lab[f] * kMaxE + e);
      const float wv = wl[f];
      *reinterpret_cast<f32x4*>(dvt + 4 * (int64_t)i) = (f32x4){wv * a.x, wv * a.y, wv * a.z, wv * a.w};
    }
  } else {
    const int n = F * E;
    for (int i = tid; i < n; i += kNT) {
      const int f = i / E, e = i - f * E;
      dvt[i] = wl[f] * tab[lab[f] * kMaxE + e];
    }
  }
}

// ---- danet_tonline_separate_bwd ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void tonline_separate_bwd_kernel(int act, int C, int T, int F, int E,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ attr,
                                                                   const float* __restrict__ embed,
                                                                   const float* __restrict__ dout,
                                                                   float* __restrict__ dembed,
                                                                   float* __restrict__ dattr) {
  __shared__ __attribute__((aligned(16))) float tab[kMaxC * kMaxE];    // the attractors of the frame
  __shared__ __attribute__((aligned(16))) float slot[kMaxF * kMaxC];   // dl of the bin, a 16-byte slot per bin
  __shared__ __attribute__((aligned(16))) float part[kPart];
  const int tid = threadIdx.x;
  const int64_t bt = blockIdx.x;
  const int64_t b = bt / T, t = bt - b * T, plane = (int64_t)T * F;
  {
    const int c = tid / kMaxE, e = tid % kMaxE;
    tab[tid] = (c < C && e < E) ? attr[bt * C * E + c * E + e] : 0.f;
  }
  __syncthreads();
  const float* vt = embed + bt * F * E;
  const float* wt = w + bt * F;
  const float* dt = dout + (b * C * T + t) * F;
  // a thread per bin: the masks of the forward, then dl
  for (int f = tid; f < F; f += kNT) {
    const float* row = vt + (int64_t)f * E;
    float lg[kMaxC];
    bin_logits(row, E, C, tab, row_head(row, E), lg);
    activate(act, C, lg);
    const float wv = wt[f];
    float g[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) g[c] = (c < C) ? wv * dt[c * plane + f] : 0.f;
    float dl[kMaxC];
    if (act == 0) {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < C) dot = fmaf(lg[c], g[c], dot);
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) dl[c] = lg[c] * (g[c] - dot);      // lg[c] = 0 for c >= C
    } else {
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) dl[c] = (lg[c] * (1.0f - lg[c])) * g[c];
    }
    *reinterpret_cast<f32x4*>(slot + f * kMaxC) = (f32x4){dl[0], dl[1], dl[2], dl[3]};
  }
  __syncthreads();
  // thread (g, j): its piece of dV of the rows g, g + G, ... and its partial sums of dA
  contract<true>(vt, F, E, C, slot, tab, part, dembed + bt * F * E);
  __syncthreads();
  const int CE = C * E;
  if (tid < CE) {
    const int c = tid / E;
    dattr[bt * CE + tid] = block_sum(part, E, c, tid - c * E);
  }
}

// ---- the host side ----------------------------------------------------------------------------------------------
static bool scan_envelope_ok(const char* who, int B, int C, int T, int E) {
  if (C < 1 || C > kMaxC || E < 1 || E > kMaxE) {
    set_error("%s: need 1 <= C <= %d and 1 <= E <= %d (got C = %d, E = %d)", who, kMaxC, kMaxE, C, E);
    return false;
  }
  if (B < 1 || T < 1 || T > DANET_TONLINE_MAX_T) {
    set_error("%s: need B >= 1 and 1 <= T <= %d (got B = %d, T = %d)", who, DANET_TONLINE_MAX_T, B, T);
    return false;
  }
  if ((int64_t)B * T * C * E >= ((int64_t)1 << 31)) {
    set_error("%s: B T C E must be < 2^31 (got B = %d, C = %d, T = %d, E = %d)", who, B, C, T, E);
    return false;
  }
  return true;
}

static bool envelope_ok(const char* who, int B, int C, int T, int F, int E) {
  if (!scan_envelope_ok(who, B, C, T, E)) return false;
  if (F < 1 || F > kMaxF) {
    set_error("%s: need 1 <= F <= %d (got F = %d)", who, kMaxF, F);
    return false;
  }
  const int64_t BT = (int64_t)B * T, lim = (int64_t)1 << 31;
  if (BT * F * E >= lim || BT * C * F >= lim) {
    set_error("%s: B T F E and B C T F must be < 2^31 (got B = %d, C = %d, T = %d, F = %d, E = %d)", who, B, C, T, F,
              E);
    return false;
  }
  return true;
}

static bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int danet_tonline_frame_sums(void* stream, int B, int C, int T, int F, int E, const float* embed,
                                        const float* src_pwr, const float* w, float* s, float* q) {
  if (!envelope_ok("frame_sums", B, C, T, F, E)) return DANET_TONLINE_ERR_ARG;
  CHECK_ARG(embed && src_pwr && w && s && q, "frame_sums: null pointer");
  CHECK_ARG(aligned_to(embed, (E & 3) ? 4 : 16) && aligned_to(src_pwr, 4) && aligned_to(w, 4) && aligned_to(s, 4) &&
                aligned_to(q, 4),
            "frame_sums: misaligned pointer (embed 16-byte when E is a multiple of 4, else 4-byte; src_pwr, w, s, q "
            "4-byte)");
  tonline_frame_sums_kernel<<<(unsigned)((int64_t)B * T), kNT, 0, (hipStream_t)stream>>>(C, T, F, E, embed, src_pwr,
                                                                                        w, s, q);
  CHECK_LAUNCH();
  return DANET_TONLINE_OK;
}

extern "C" int danet_tonline_scan(void* stream, int B, int C, int T, int E, double lambda, int T0, double eps,
                                  const float* s, const float* q, float* attr, double* den) {
  if (!scan_envelope_ok("scan", B, C, T, E)) return DANET_TONLINE_ERR_ARG;
  CHECK_ARG(lambda > 0.0 && lambda <= 1.0, "scan: need 0 < lambda <= 1 (got %g)", lambda);
  CHECK_ARG(T0 >= 1, "scan: need T0 >= 1 (got %d)", T0);
  CHECK_ARG(eps >= 0.0 && eps <= 1.7e308, "scan: eps must be finite and >= 0 (got %g)", eps);
  CHECK_ARG(s && q && attr && den, "scan: null pointer");
  CHECK_ARG(aligned_to(s, 4) && aligned_to(q, 4) && aligned_to(attr, 4) && aligned_to(den, 8),
            "scan: misaligned pointer (s, q, attr 4-byte; den 8-byte)");
  tonline_scan_kernel<<<B, kNT, 0, (hipStream_t)stream>>>(C, T, E, lambda, T0, eps, s, q, attr, den);
  CHECK_LAUNCH();
  return DANET_TONLINE_OK;
}

extern "C" int danet_tonline_scan_bwd(void* stream, int B, int C, int T, int E, double lambda, int T0,
                                      const float* dattr, const double* den, float* r) {
  if (!scan_envelope_ok("scan_bwd", B, C, T, E)) return DANET_TONLINE_ERR_ARG;
  CHECK_ARG(lambda > 0.0 && lambda <= 1.0, "scan_bwd: need 0 < lambda <= 1 (got %g)", lambda);
  CHECK_ARG(T0 >= 1, "scan_bwd: need T0 >= 1 (got %d)", T0);
  CHECK_ARG(dattr && den && r, "scan_bwd: null pointer");
  CHECK_ARG(aligned_to(dattr, 4) && aligned_to(r, 4) && aligned_to(den, 8),
            "scan_bwd: misaligned pointer (dattr, r 4-byte; den 8-byte)");
  tonline_scan_bwd_kernel<<<B, kNT, 0, (hipStream_t)stream>>>(C, T, E, lambda, T0, dattr, den, r);
  CHECK_LAUNCH();
  return DANET_TONLINE_OK;
}

extern "C" int danet_tonline_sums_bwd(void* stream, int B, int C, int T, int F, int E, const float* src_pwr,
                                      const float* w, const float* r, float* dembed) {
  if (!envelope_ok("sums_bwd", B, C, T, F, E)) return DANET_TONLINE_ERR_ARG;
  CHECK_ARG(src_pwr && w && r && dembed, "sums_bwd: null pointer");
  CHECK_ARG(aligned_to(dembed, (E & 3) ? 4 : 16) && aligned_to(src_pwr, 4) && aligned_to(w, 4) && aligned_to(r, 4),
            "sums_bwd: misaligned pointer (dembed 16-byte when E is a multiple of 4, else 4-byte; src_pwr, w, r "
            "4-byte)");
  tonline_sums_bwd_kernel<<<(unsigned)((int64_t)B * T), kNT, 0, (hipStream_t)stream>>>(C, T, F, E, src_pwr, w, r,
                                                                                      dembed);
  CHECK_LAUNCH();
  return DANET_TONLINE_OK;
}

extern "C" int danet_tonline_separate_bwd(void* stream, int act, int B, int C, int T, int F, int E, const float* w,
                                          const float* attr, const float* embed, const float* dout, float* dembed,
                                          float* dattr) {
  if (!envelope_ok("separate_bwd", B, C, T, F, E)) return DANET_TONLINE_ERR_ARG;
  CHECK_ARG(act == 0 || act == 1, "separate_bwd: act must be 0 (softmax) or 1 (sigmoid) (got %d)", act);
  CHECK_ARG(w && attr && embed && dout && dembed && dattr, "separate_bwd: null pointer");
  CHECK_ARG(aligned_to(embed, (E & 3) ? 4 : 16) && aligned_to(dembed, (E & 3) ? 4 : 16) && aligned_to(w, 4) &&
                aligned_to(attr, 4) && aligned_to(dout, 4) && aligned_to(dattr, 4),
            "separate_bwd: misaligned pointer (embed, dembed 16-byte when E is a multiple of 4, else 4-byte; w, attr, "
            "dout, dattr 4-byte)");
  tonline_separate_bwd_kernel<<<(unsigned)((int64_t)B * T), kNT, 0, (hipStream_t)stream>>>(act, C, T, F, E, w, attr,
                                                                                          embed, dout, dembed, dattr);
  CHECK_LAUNCH();
  return DANET_TONLINE_OK;
}
