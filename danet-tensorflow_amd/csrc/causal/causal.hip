/*
 * libdanet_causal_hip.so: the causal encoder's kernels and block-wise streaming inference
 * (include/danet_causal_hip.h, THE RULE): a running-mean centring with carried state and its adjoint, L stacked
 * unidirectional LSTM layers over a block of frames from carried state, one launch per anti-diagonal, and the
 * skinny product both that step and the output projection run on.  No atomics, no waiting between workgroups, every
 * output element written once by one thread.
 */
#include "danet_causal_hip.h"
#define DANET_EXT causal
#define DANET_EXT_UPPER CAUSAL
#include "ext_core.h"

#include <math.h>
#include <stdint.h>

static constexpr int kNT = 256;                      // threads of every workgroup here
static constexpr int kNW = kNT / 64;
static constexpr int kChunk = 64;                    // frames the centring walks at a time
static constexpr int kQ = 16;                        // column quads of a workgroup of the skinny product
static constexpr int kS = kNT / kQ;                  // K slices
static constexpr int kCols = 4 * kQ;                 // columns of a workgroup: 64
static constexpr int kUnits = kCols / 4;             // LSTM units of a workgroup: 16 (all four gates of each)
static constexpr int kRedLd = kCols + 16;            // row pitch of the partial sums in LDS
static constexpr int kMaxK = DANET_CAUSAL_MAX_K;
static constexpr int kMaxL = DANET_CAUSAL_MAX_L;
static_assert(kS == 16, "rule 2 names sixteen slices");
static_assert(kMaxK % 4 == 0 && kMaxK >= kS * kRedLd, "the staged rows and the partial sums share one LDS array");

// ---- rule 1: the causal centring and its adjoint ----------------------------------------------------------------
__device__ __forceinline__ int64_t row_index(int layout, int B, int T, int b, int t) {
  return layout == 0 ? (int64_t)b * T + t : (int64_t)t * B + b;
}

// ROW SUM ORDER of the header; every lane of the wave must be active, and every lane returns the sum
__device__ __forceinline__ double row_sum(const float* __restrict__ row, int D, int lane) {
  double p = 0.0;
  for (int d = lane; d < D; d += 64) p += (double)row[d];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) p += __shfl_xor(p, m, 64);
  return p;
}

// BWD false: out = in - running mean, from `state`; true: the adjoint over a whole utterance, last frame first
template <bool BWD>
__global__ __launch_bounds__(kNT) void center_kernel(int B, int T, int D, const float* __restrict__ in, int in_layout,
                                                     int ld_in, float* __restrict__ out, int out_layout, int ld_out,
                                                     double* __restrict__ state) {
  __shared__ double rs[kChunk];
  __shared__ float mu[kChunk];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  double S = 0.0, n = 0.0;
  if (!BWD && tid == 0) {
    S = state[2 * b];
    n = state[2 * b + 1];
  }
  const int width = BWD ? D : ld_out;                // columns written per row
  for (int c0 = 0; c0 < T; c0 += kChunk) {
    const int nf = T - c0 < kChunk ? T - c0 : kChunk;
    for (int i = wave; i < nf; i += kNW) {
      const int t = BWD ? T - 1 - c0 - i : c0 + i;
      const double p = row_sum(in + row_index(in_layout, B, T, b, t) * ld_in, D, lane);
      if (lane == 0) rs[i] = p;
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < nf; ++i) {
        if (BWD) {
          const int t = T - 1 - c0 - i;
          S += rs[i] / ((double)(t + 1) * (double)D);
          mu[i] = (float)S;
        } else {
          S += rs[i];
          n += 1.0;
          mu[i] = (float)(S / (n * (double)D));
        }
      }
    }
    __syncthreads();
    for (int i = wave; i < nf; i += kNW) {
      const int t = BWD ? T - 1 - c0 - i : c0 + i;
      const float* __restrict__ src = in + row_index(in_layout, B, T, b, t) * ld_in;
      float* __restrict__ dst = out + row_index(out_layout, B, T, b, t) * ld_out;
      const float m = mu[i];
      for (int d = lane; d < width; d += 64) dst[d] = d < D ? src[d] - m : 0.f;
    }
    __syncthreads();
  }
  if (!BWD && tid == 0) {
    state[2 * b] = S;
    state[2 * b + 1] = n;
  }
}

// ---- rule 2: the skinny product ---------------------------------------------------------------------------------
// Thread (s, q) = (tid / 16, tid % 16): K slice s of the four columns of quad q, for the NR rows staged in LDS.
template <int NR>
struct Skinny {
  static constexpr int kFloats = NR * kMaxK;         // xs [NR][Kp], then red [kS][NR][kRedLd] in the same array
};

// four consecutive columns of one row of W: one 16-byte load, or up to four guarded 4-byte loads
__device__ __forceinline__ f32x4 load_w4(const float* __restrict__ p, bool vec, int ncol) {
  if (vec) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  v.x = p[0];
  if (ncol > 1) v.y = p[1];
  if (ncol > 2) v.z = p[2];
  if (ncol > 3) v.w = p[3];
  return v;
}

// the partial sums p_s of rule 2 for this thread's four columns (wq: their address in row 0 of W; ncol of them exist)
// and the NR rows xs [NR][Kp]
template <int NR>
__device__ __forceinline__ void skinny_partials(const float* xs, int Kp, int K, const float* __restrict__ wq,
                                                int64_t ldw, bool vec, int ncol, int s, f32x4 (&acc)[NR]) {
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (ncol <= 0) return;
#pragma unroll 2
  for (int k0 = 4 * s; k0 < Kp; k0 += 4 * kS) {
    f32x4 w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[i] = (k0 + i < K) ? load_w4(wq + (int64_t)(k0 + i) * ldw, vec, ncol) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + r * Kp + k0);
      f32x4 a = acc[r];
      a.x = fmaf(xv.x, w[0].x, a.x); a.y = fmaf(xv.x, w[0].y, a.y); a.z = fmaf(xv.x, w[0].z, a.z); a.w = fmaf(xv.x, w[0].w, a.w);
      a.x = fmaf(xv.y, w[1].x, a.x); a.y = fmaf(xv.y, w[1].y, a.y); a.z = fmaf(xv.y, w[1].z, a.z); a.w = fmaf(xv.y, w[1].w, a.w);
      a.x = fmaf(xv.z, w[2].x, a.x); a.y = fmaf(xv.z, w[2].y, a.y); a.z = fmaf(xv.z, w[2].z, a.z); a.w = fmaf(xv.z, w[2].w, a.w);
      a.x = fmaf(xv.w, w[3].x, a.x); a.y = fmaf(xv.w, w[3].y, a.y); a.z = fmaf(xv.w, w[3].z, a.z); a.w = fmaf(xv.w, w[3].w, a.w);
      acc[r] = a;
    }
  }
}

// every thread's partial sums into red (the array the rows were staged in: all reads of them are over)
template <int NR>
__device__ __forceinline__ void skinny_exchange(float* red, int s, int q, const f32x4 (&acc)[NR]) {
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NR; ++r) *reinterpret_cast<f32x4*>(red + (s * NR + r) * kRedLd + 4 * q) = acc[r];
  __syncthreads();
}

// the fixed tree of rule 2 over the sixteen partial sums of (row r, local column col)
template <int NR>
__device__ __forceinline__ float skinny_sum(const float* red, int r, int col) {
  float p[kS];
#pragma unroll
  for (int s = 0; s < kS; ++s) p[s] = red[(s * NR + r) * kRedLd + col];
#pragma unroll
  for (int w = 1; w < kS; w *= 2)
#pragma unroll
    for (int s = 0; s < kS; s += 2 * w) p[s] = p[s] + p[s + w];
  return p[0];
}

// ---- rule 3: one anti-diagonal of the LSTM block ----------------------------------------------------------------
// gate math of the core's recurrent kernels (sigmoid_hw / tanh_hw there: v_exp_f32 / v_rcp_f32)
__device__ __forceinline__ float sigmoid_hw(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_hw(float x) {
  const float e = __expf(-2.0f * fabsf(x));
  const float t = (1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e);
  return copysignf(t, x);
}

struct LstmArgs {
  const float* W[kMaxL];
  const float* bias[kMaxL];
  const float* x;
  float* h;
  float* c;
  float* y;
  float* hbuf;                                       // ws: h^(l)_t, [L][Tb][B][H]
  int L, B, Tb, D0, H, ldx, ldy;
};

template <int NR>
__global__ __launch_bounds__(kNT) void lstm_diag_kernel(LstmArgs a, int k) {
  __shared__ __attribute__((aligned(16))) float sm[Skinny<NR>::kFloats];
  const int tid = threadIdx.x, q = tid & (kQ - 1), s = tid / kQ;
  const int B = a.B, H = a.H, Tb = a.Tb;
  const int l_lo = k - Tb + 1 > 0 ? k - Tb + 1 : 0;
  const int l = l_lo + blockIdx.y, t = k - l;
  const int D = l == 0 ? a.D0 : H, K = D + H, Kp = (K + 3) & ~3;
  const int64_t BH = (int64_t)B * H;
  const float* __restrict__ xin = l == 0 ? a.x + (int64_t)t * B * a.ldx : a.hbuf + ((int64_t)(l - 1) * Tb + t) * BH;
  const int ldin = l == 0 ? a.ldx : H;
  const float* __restrict__ hprev = t == 0 ? a.h + l * BH : a.hbuf + ((int64_t)l * Tb + t - 1) * BH;
  // [x_t, h_(t-1)] of every row, zero behind K and in the rows behind B
  for (int r = 0; r < NR; ++r)
    for (int kk = tid; kk < Kp; kk += kNT) {
      float v = 0.f;
      if (r < B) {
        if (kk < D) v = xin[(int64_t)r * ldin + kk];
        else if (kk < K) v = hprev[(int64_t)r * H + kk - D];
      }
      sm[r * Kp + kk] = v;
    }
  __syncthreads();
  // quad q: gate q / 4, units 4 (q % 4) .. + 3 of this workgroup's sixteen
  const int unit0 = blockIdx.x * kUnits + 4 * (q & 3);
  const float* __restrict__ Wl = a.W[l];
  f32x4 acc[NR];
  skinny_partials<NR>(sm, Kp, K, Wl + (int64_t)(q >> 2) * H + unit0, 4 * (int64_t)H, true, unit0 < H ? 4 : 0, s, acc);
  skinny_exchange<NR>(sm, s, q, acc);
  const int r = tid / kUnits, u = tid & (kUnits - 1), unit = blockIdx.x * kUnits + u;
  if (r < NR && r < B && unit < H) {
    const float* __restrict__ bl = a.bias[l];
    const float g = skinny_sum<NR>(sm, r, u) + bl[unit];
    const float ig = sigmoid_hw(skinny_sum<NR>(sm, r, kUnits + u) + bl[H + unit]);
    const float fg = sigmoid_hw(skinny_sum<NR>(sm, r, 2 * kUnits + u) + bl[2 * H + unit]);
    const float og = sigmoid_hw(skinny_sum<NR>(sm, r, 3 * kUnits + u) + bl[3 * H + unit]);
    float* cp = a.c + l * BH + (int64_t)r * H + unit;
    const float cs = ig * g + fg * *cp;
    const float hv = og * tanh_hw(cs);
    *cp = cs;
    a.hbuf[((int64_t)l * Tb + t) * BH + (int64_t)r * H + unit] = hv;
    if (l == a.L - 1) a.y[((int64_t)t * B + r) * a.ldy + unit] = hv;
  }
}

// anti-diagonal k, whose nl layers are a.L's l_lo .. l_lo + nl - 1 (the entry point has checked every argument)
template <int NR>
static void launch_diag(const LstmArgs& a, int k, int nl, hipStream_t st) {
  lstm_diag_kernel<NR><<<dim3((a.H + kUnits - 1) / kUnits, nl), kNT, 0, st>>>(a, k);
}

// h[l] = the block's last h^(l)
__global__ __launch_bounds__(kNT) void lstm_finish_kernel(int L, int Tb, int BH, const float* __restrict__ hbuf,
                                                          float* __restrict__ h) {
  const int i = blockIdx.x * kNT + threadIdx.x;
  if (i >= L * BH) return;
  const int l = i / BH;
  h[i] = hbuf[((int64_t)l * Tb + Tb - 1) * BH + (i - l * BH)];
}

// ---- the projection ---------------------------------------------------------------------------------------------
template <int NR>
__global__ __launch_bounds__(kNT) void project_kernel(int M, int K, int N, const float* __restrict__ A, int lda,
                                                      const float* __restrict__ W, int ldw, float* __restrict__ out,
                                                      int ldo, int vec) {
  __shared__ __attribute__((aligned(16))) float sm[Skinny<NR>::kFloats];
  const int tid = threadIdx.x, q = tid & (kQ - 1), s = tid / kQ;
  const int Kp = (K + 3) & ~3, r0 = blockIdx.y * NR, c0 = blockIdx.x * kCols;
  for (int r = 0; r < NR; ++r)
    for (int kk = tid; kk < Kp; kk += kNT) sm[r * Kp + kk] = (r0 + r < M && kk < K) ? A[(int64_t)(r0 + r) * lda + kk] : 0.f;
  __syncthreads();
  const int col = c0 + 4 * q;
  f32x4 acc[NR];
  skinny_partials<NR>(sm, Kp, K, W + col, ldw, vec != 0, N - col < 4 ? N - col : 4, s, acc);
  skinny_exchange<NR>(sm, s, q, acc);
  for (int i = tid; i < NR * kCols; i += kNT) {
    const int r = i / kCols, cl = i & (kCols - 1);
    if (r0 + r < M && c0 + cl < N) out[(int64_t)(r0 + r) * ldo + c0 + cl] = skinny_sum<NR>(sm, r, cl);
  }
}

// ---- the host side ----------------------------------------------------------------------------------------------
static bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static bool center_ok(const char* who, int B, int T, int D, const void* in, int in_layout, int ld_in, const void* out,
                      int out_layout, int ld_out) {
  if (B < 1 || T < 1 || T > DANET_CAUSAL_MAX_T || D < 1 || D > DANET_CAUSAL_MAX_D) {
    set_error("%s: need B >= 1, 1 <= T <= %d and 1 <= D <= %d (got B = %d, T = %d, D = %d)", who, DANET_CAUSAL_MAX_T,
              DANET_CAUSAL_MAX_D, B, T, D);
    return false;
  }
  if ((in_layout != 0 && in_layout != 1) || (out_layout != 0 && out_layout != 1)) {
    set_error("%s: a layout is 0 (batch-major) or 1 (time-major) (got %d and %d)", who, in_layout, out_layout);
    return false;
  }
  if (ld_in < D || ld_out < D) {
    set_error("%s: a leading dimension is below D = %d (got %d and %d)", who, D, ld_in, ld_out);
    return false;
  }
  const int64_t lim = (int64_t)1 << 40;
  if ((int64_t)B * T * ld_in >= lim || (int64_t)B * T * ld_out >= lim) {
    set_error("%s: B T ld must be < 2^40 (got B = %d, T = %d, ld = %d and %d)", who, B, T, ld_in, ld_out);
    return false;
  }
  if (!in || !out) {
    set_error("%s: null pointer", who);
    return false;
  }
  if (!aligned_to(in, 4) || !aligned_to(out, 4)) {
    set_error("%s: misaligned pointer (4-byte)", who);
    return false;
  }
  return true;
}

extern "C" int danet_causal_center_fwd(void* stream, int B, int T, int D, const float* in, int in_layout, int ld_in,
                                       float* out, int out_layout, int ld_out, void* state) {
  if (!center_ok("center_fwd", B, T, D, in, in_layout, ld_in, out, out_layout, ld_out)) return DANET_CAUSAL_ERR_ARG;
  CHECK_ARG(state && aligned_to(state, 8), "center_fwd: state is null or not 8-byte aligned");
  center_kernel<false><<<B, kNT, 0, (hipStream_t)stream>>>(B, T, D, in, in_layout, ld_in, out, out_layout, ld_out,
                                                          (double*)state);
  CHECK_LAUNCH();
  return DANET_CAUSAL_OK;
}

extern "C" int danet_causal_center_bwd(void* stream, int B, int T, int D, const float* dout, int dout_layout,
                                       int ld_dout, float* din, int din_layout, int ld_din) {
  if (!center_ok("center_bwd", B, T, D, dout, dout_layout, ld_dout, din, din_layout, ld_din))
    return DANET_CAUSAL_ERR_ARG;
  center_kernel<true><<<B, kNT, 0, (hipStream_t)stream>>>(B, T, D, dout, dout_layout, ld_dout, din, din_layout, ld_din,
                                                         nullptr);
  CHECK_LAUNCH();
  return DANET_CAUSAL_OK;
}

static bool lstm_dims_ok(const char* who, int L, int B, int Tb, int H) {
  if (L < 1 || L > kMaxL || B < 1 || B > DANET_CAUSAL_MAX_B || Tb < 1 || Tb > DANET_CAUSAL_MAX_TB || H < 4 ||
      H > DANET_CAUSAL_MAX_H || (H & 3)) {
    set_error("%s: need 1 <= L <= %d, 1 <= B <= %d, 1 <= Tb <= %d, 4 <= H <= %d and H %% 4 == 0 (got L = %d, B = %d, "
              "Tb = %d, H = %d)", who, kMaxL, DANET_CAUSAL_MAX_B, DANET_CAUSAL_MAX_TB, DANET_CAUSAL_MAX_H, L, B, Tb, H);
    return false;
  }
  return true;
}

extern "C" size_t danet_causal_lstm_ws_bytes(int L, int B, int Tb, int H) {
  if (!lstm_dims_ok("lstm_ws_bytes", L, B, Tb, H)) return (size_t)-1;
  return sizeof(float) * (size_t)L * Tb * B * H;
}

extern "C" int danet_causal_lstm_block(void* stream, int L, int B, int Tb, int D0, int H, const float* x, int ldx,
                                       const float* const* W, const float* const* bias, float* h, float* c, float* y,
                                       int ldy, void* ws, size_t ws_bytes) {
  if (!lstm_dims_ok("lstm_block", L, B, Tb, H)) return DANET_CAUSAL_ERR_ARG;
  CHECK_ARG(D0 >= 1 && D0 <= DANET_CAUSAL_MAX_D0, "lstm_block: need 1 <= D0 <= %d (got %d)", DANET_CAUSAL_MAX_D0, D0);
  CHECK_ARG(ldx >= D0 && ldy >= H, "lstm_block: need ldx >= D0 and ldy >= H (got ldx = %d, D0 = %d, ldy = %d, H = %d)",
            ldx, D0, ldy, H);
  CHECK_ARG(x && W && bias && h && c && y && ws, "lstm_block: null pointer");
  const size_t need = sizeof(float) * (size_t)L * Tb * B * H;
  CHECK_ARG(ws_bytes >= need, "lstm_block: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
  CHECK_ARG(aligned_to(x, 4) && aligned_to(h, 4) && aligned_to(c, 4) && aligned_to(y, 4) && aligned_to(ws, 16),
            "lstm_block: misaligned pointer (x, h, c, y 4-byte; ws 16-byte)");
  LstmArgs a;
  for (int l = 0; l < kMaxL; ++l) {
    a.W[l] = l < L ? W[l] : nullptr;
    a.bias[l] = l < L ? bias[l] : nullptr;
    if (l < L) {
      CHECK_ARG(a.W[l] && a.bias[l], "lstm_block: W[%d] or bias[%d] is null", l, l);
      CHECK_ARG(aligned_to(a.W[l], 16) && aligned_to(a.bias[l], 4),
                "lstm_block: misaligned pointer (W[%d] 16-byte, bias[%d] 4-byte)", l, l);
    }
  }
  a.x = x; a.h = h; a.c = c; a.y = y; a.hbuf = (float*)ws;
  a.L = L; a.B = B; a.Tb = Tb; a.D0 = D0; a.H = H; a.ldx = ldx; a.ldy = ldy;
  const hipStream_t st = (hipStream_t)stream;
  for (int k = 0; k < Tb + L - 1; ++k) {
    const int l_lo = k - Tb + 1 > 0 ? k - Tb + 1 : 0, l_hi = k < L - 1 ? k : L - 1;
    const int nl = l_hi - l_lo + 1;
    if (B == 1) launch_diag<1>(a, k, nl, st);
    else if (B <= 4) launch_diag<4>(a, k, nl, st);
    else launch_diag<16>(a, k, nl, st);
    CHECK_LAUNCH();
  }
  const int total = L * B * H;
  lstm_finish_kernel<<<(total + kNT - 1) / kNT, kNT, 0, st>>>(L, Tb, B * H, a.hbuf, h);
  CHECK_LAUNCH();
  return DANET_CAUSAL_OK;
}

extern "C" int danet_causal_project(void* stream, int M, int K, int N, const float* A, int lda, const float* Wout,
                                    int ldw, float* out, int ldo) {
  CHECK_ARG(M >= 1 && M <= DANET_CAUSAL_MAX_M && K >= 1 && K <= kMaxK && N >= 1 && N < (1 << 24),
            "project: need 1 <= M <= %d, 1 <= K <= %d and 1 <= N < 2^24 (got M = %d, K = %d, N = %d)",
            DANET_CAUSAL_MAX_M, kMaxK, M, K, N);
  CHECK_ARG(lda >= K && ldw >= N && ldo >= N,
            "project: need lda >= K, ldw >= N and ldo >= N (got lda = %d, K = %d, ldw = %d, ldo = %d, N = %d)", lda, K,
            ldw, ldo, N);
  CHECK_ARG(A && Wout && out, "project: null pointer");
  CHECK_ARG(aligned_to(A, 4) && aligned_to(Wout, 4) && aligned_to(out, 4), "project: misaligned pointer (4-byte)");
  const int vec = aligned_to(Wout, 16) && (N & 3) == 0 && (ldw & 3) == 0;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)((N + kCols - 1) / kCols);
  if (M == 1) project_kernel<1><<<dim3(gx, 1), kNT, 0, st>>>(M, K, N, A, lda, Wout, ldw, out, ldo, vec);
  else if (M <= 4) project_kernel<4><<<dim3(gx, 1), kNT, 0, st>>>(M, K, N, A, lda, Wout, ldw, out, ldo, vec);
  else project_kernel<16><<<dim3(gx, (unsigned)((M + 15) / 16)), kNT, 0, st>>>(M, K, N, A, lda, Wout, ldw, out, ldo, vec);
  CHECK_LAUNCH();
  return DANET_CAUSAL_OK;
}
