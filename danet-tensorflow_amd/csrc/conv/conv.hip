// 2-D convolution operators of the conv-bilstm-v1 encoder (include/danet_conv_hip.h).
//
// All three products are implicit GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32
// accumulation).  Operand map of that instruction: lane l holds A[row l&15][k l>>4] and
// B[k l>>4][col l&15]; the 4 results of lane l are C[4*(l>>4) + r][l&15], r = 0..3.
//
//   forward   M = output pixels (a wave: two rows t0, t0+1 x 16 columns), N = Cout, K = Cin*k*k.
//             The two rows are two accumulator sets, so the 2x2 pool windows of a wave's tile
//             (rows t0/t0+1, columns 4q+2h, 4q+2h+1) sit in ONE lane: the pool is register-only.
//   dgrad     M = input pixels (same tiling), N = Cin, K = Cout*k*k of the flipped kernel; the A
//             loader forms g = dy * lrelu'(y) (routed through the saved argmax when pooled).
//   wgrad     M = Cin*k*k rows of dw plus one row of ones (= db), N = Cout, K = the pixels of
//             one slab of (b, t) rows; every slab writes its own fp32 partial, a second kernel
//             sums the slabs in a fixed order (deterministic, no atomics).
#include <hip/hip_runtime.h>

#include "danet_conv_hip.h"
#define DANET_EXT conv
#define DANET_EXT_UPPER CONV
#include "ext_core.h"

typedef danet_conv_desc_t Desc;

// ------------------------------------------------------------------ addressing
// stored output position: pooled (tp, fp) with pool, conv (t, f) otherwise (depth-to-space mapped)
__device__ __forceinline__ int64_t y_off(const Desc& d, int b, int co, int t, int f) {
  if (d.d2s)
    return b * d.y_stride[0] + (co >> 2) * d.y_stride[1] + (2 * t + ((co >> 1) & 1)) * d.y_stride[2] +
           (2 * f + (co & 1)) * d.y_stride[3];
  return b * d.y_stride[0] + co * d.y_stride[1] + t * d.y_stride[2] + f * d.y_stride[3];
}

// g = dy * lrelu'(y) at conv-output position (co, t, f) inside the layer (0 <= t < T, 0 <= f < F).
// Pooled: only the window position named by argmax carries the pooled gradient; positions the
// 'valid' pool drops get 0.  lrelu' from the saved output: y > 0 ? 1 : alpha (alpha at z == 0,
// where tf.maximum(alpha*z, z) takes the alpha*z branch).
__device__ __forceinline__ float load_g(const Desc& d, const float* __restrict__ dy,
                                        const float* __restrict__ y, const uint8_t* __restrict__ am,
                                        int b, int co, int t, int f) {
  int64_t o;
  if (d.pool) {
    const int tp = t >> 1, fp = f >> 1, Tp = d.T >> 1, Fp = d.F >> 1;
    if (tp >= Tp || fp >= Fp) return 0.f;
    const int64_t ai = (((int64_t)b * d.Cout + co) * Tp + tp) * Fp + fp;
    if (am[ai] != (((t & 1) << 1) | (f & 1))) return 0.f;
    o = y_off(d, b, co, tp, fp);
  } else {
    o = y_off(d, b, co, t, f);
  }
  return dy[o] * (y[o] > 0.f ? 1.f : d.alpha);
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// (b, t0, f0) of the wave's pixel tile: two rows x 16 columns
__device__ __forceinline__ bool pixel_tile(const Desc& d, int& b, int& t0, int& f0) {
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nft = (d.F + 15) >> 4, ntt = (d.T + 1) >> 1;
  if (tile >= (int64_t)d.B * ntt * nft) return false;
  f0 = (int)(tile % nft) * 16;
  const int64_t r = tile / nft;
  t0 = (int)(r % ntt) * 2;
  b = (int)(r / ntt);
  return true;
}

// ------------------------------------------------------------------ forward
template <int KS, int NT>
__global__ __launch_bounds__(256) void conv_fwd_kernel(Desc d, const float* __restrict__ x,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ bias,
                                                       float* __restrict__ y, uint8_t* __restrict__ am) {
  constexpr int P = KS / 2;
  int b, t0, f0;
  if (!pixel_tile(d, b, t0, f0)) return;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int Cin = d.Cin, Cout = d.Cout, T = d.T, F = d.F;
  const int Ktot = Cin * KS * KS;
  f32x4 acc0[NT], acc1[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc0[n] = acc1[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  // k = (i*KS + j)*Cin + ci (w's [k][k][Cin][Cout] row order), advanced by 4 per step
  int ci = lk % Cin, i = (lk / Cin) / KS, j = (lk / Cin) % KS;
  const float* xb = x + b * d.x_stride[0];
  const int fa = f0 + li - P;
  for (int kk = 0; kk < Ktot; kk += 4) {
    const int k = kk + lk;
    float a0 = 0.f, a1 = 0.f;
    const int f = fa + j, ta = t0 + i - P;
    if (k < Ktot && f >= 0 && f < F) {
      const float* xc = xb + ci * d.x_stride[1] + f * d.x_stride[3];
      if (ta >= 0 && ta < T) a0 = xc[ta * d.x_stride[2]];
      if (ta + 1 >= 0 && ta + 1 < T) a1 = xc[(ta + 1) * d.x_stride[2]];
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int co = n * 16 + li;
      const float bw = (k < Ktot && co < Cout) ? w[k * Cout + co] : 0.f;
      acc0[n] = mfma4(a0, bw, acc0[n]);
      acc1[n] = mfma4(a1, bw, acc1[n]);
    }
    ci += 4;
    while (ci >= Cin) {
      ci -= Cin;
      if (++j == KS) { j = 0; ++i; }
    }
  }
  const int fq = f0 + lk * 4;           // this lane's 4 output columns fq .. fq+3
  const float alpha = d.alpha;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int co = n * 16 + li;
    if (co >= Cout) continue;
    const float bv = bias[co];
    float v0[4], v1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z0 = acc0[n][r] + bv, z1 = acc1[n][r] + bv;
      v0[r] = z0 > 0.f ? z0 : alpha * z0;
      v1[r] = z1 > 0.f ? z1 : alpha * z1;
    }
    if (!d.pool) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (fq + r >= F) break;
        y[y_off(d, b, co, t0, fq + r)] = v0[r];
        if (t0 + 1 < T) y[y_off(d, b, co, t0 + 1, fq + r)] = v1[r];
      }
    } else {
      const int Tp = T >> 1, Fp = F >> 1, tp = t0 >> 1;
      if (tp >= Tp) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int fp = (fq >> 1) + h;
        if (fp >= Fp) break;
        // first maximum in row-major window order (t0,f) (t0,f+1) (t0+1,f) (t0+1,f+1)
        float best = v0[2 * h];
        int arg = 0;
        if (v0[2 * h + 1] > best) { best = v0[2 * h + 1]; arg = 1; }
        if (v1[2 * h] > best) { best = v1[2 * h]; arg = 2; }
        if (v1[2 * h + 1] > best) { best = v1[2 * h + 1]; arg = 3; }
        y[y_off(d, b, co, tp, fp)] = best;
        am[(((int64_t)b * Cout + co) * Tp + tp) * Fp + fp] = (uint8_t)arg;
      }
    }
  }
}

// ------------------------------------------------------------------ backward, data
template <int KS, int NT>
__global__ __launch_bounds__(256) void conv_dgrad_kernel(Desc d, const float* __restrict__ dy,
                                                         const float* __restrict__ y,
                                                         const uint8_t* __restrict__ am,
                                                         const float* __restrict__ w,
                                                         float* __restrict__ dx) {
  constexpr int P = KS / 2;
  int b, t0, f0;
  if (!pixel_tile(d, b, t0, f0)) return;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int Cin = d.Cin, Cout = d.Cout, T = d.T, F = d.F;
  const int Ktot = Cout * KS * KS;
  f32x4 acc0[NT], acc1[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc0[n] = acc1[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  // k = (i*KS + j)*Cout + co; dx[t][f] += g[t+P-i][f+P-j] * w[i][j][ci][co]
  int co = lk % Cout, i = (lk / Cout) / KS, j = (lk / Cout) % KS;
  const int fa = f0 + li + P;
  for (int kk = 0; kk < Ktot; kk += 4) {
    const int k = kk + lk;
    float a0 = 0.f, a1 = 0.f;
    const int f = fa - j, tg = t0 + P - i;
    if (k < Ktot && f >= 0 && f < F) {
      if (tg >= 0 && tg < T) a0 = load_g(d, dy, y, am, b, co, tg, f);
      if (tg + 1 >= 0 && tg + 1 < T) a1 = load_g(d, dy, y, am, b, co, tg + 1, f);
    }
    const int wrow = (i * KS + j) * Cin;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int ci = n * 16 + li;
      const float bw = (k < Ktot && ci < Cin) ? w[(wrow + ci) * Cout + co] : 0.f;
      acc0[n] = mfma4(a0, bw, acc0[n]);
      acc1[n] = mfma4(a1, bw, acc1[n]);
    }
    co += 4;
    while (co >= Cout) {
      co -= Cout;
      if (++j == KS) { j = 0; ++i; }
    }
  }
  const int fq = f0 + lk * 4;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int ci = n * 16 + li;
    if (ci >= Cin) continue;
    float* o = dx + b * d.x_stride[0] + ci * d.x_stride[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (fq + r >= F) break;
      o[t0 * d.x_stride[2] + (fq + r) * d.x_stride[3]] = acc0[n][r];
      if (t0 + 1 < T) o[(t0 + 1) * d.x_stride[2] + (fq + r) * d.x_stride[3]] = acc1[n][r];
    }
  }
}

// ------------------------------------------------------------------ backward, weights + bias
struct WgradPlan {
  int Ktot, Mtot, nmt, rows_per_slab, nslab;
};

static WgradPlan wgrad_plan(const Desc& d) {
  WgradPlan p;
  p.Ktot = d.Cin * d.k * d.k;
  p.Mtot = p.Ktot + 1;                        // + the row of ones: db
  p.nmt = (p.Mtot + 15) / 16;
  const int64_t R = (int64_t)d.B * d.T;       // (b, t) rows, split into slabs
  int64_t target = 4096 / p.nmt;              // ~4096 waves in flight
  if (target < 1) target = 1;
  p.rows_per_slab = (int)((R + target - 1) / target);
  p.nslab = (int)((R + p.rows_per_slab - 1) / p.rows_per_slab);
  return p;
}

template <int KS, int NT>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(Desc d, WgradPlan pl, const float* __restrict__ x,
                                                         const float* __restrict__ dy,
                                                         const float* __restrict__ y,
                                                         const uint8_t* __restrict__ am,
                                                         float* __restrict__ part) {
  constexpr int P = KS / 2;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (int64_t)pl.nslab * pl.nmt) return;
  const int mt = (int)(wid % pl.nmt), s = (int)(wid / pl.nmt);
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int Cin = d.Cin, Cout = d.Cout, T = d.T, F = d.F;
  // this lane's A row m: a dw row (i, j, ci), the row of ones, or padding
  const int m = mt * 16 + li;
  const int kind = m < pl.Ktot ? 0 : (m == pl.Ktot ? 1 : 2);
  const int ci = kind == 0 ? m % Cin : 0, rr = kind == 0 ? m / Cin : 0;
  const int i = rr / KS, j = rr % KS;
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t R = (int64_t)d.B * T;
  const int64_t r0 = (int64_t)s * pl.rows_per_slab;
  const int64_t r1 = r0 + pl.rows_per_slab < R ? r0 + pl.rows_per_slab : R;
  for (int64_t row = r0; row < r1; ++row) {
    const int b = (int)(row / T), t = (int)(row % T);
    const int ta = t + i - P;
    const bool trow = kind == 0 && ta >= 0 && ta < T;
    const float* xr = x + b * d.x_stride[0] + ci * d.x_stride[1] + ta * d.x_stride[2];
    for (int fb = 0; fb < F; fb += 4) {
      const int f = fb + lk;
      const bool fin = f < F;
      float a = 0.f;
      if (fin) {
        if (kind == 1) {
          a = 1.f;
        } else if (trow) {
          const int fx = f + j - P;
          if (fx >= 0 && fx < F) a = xr[fx * d.x_stride[3]];
        }
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int co = n * 16 + li;
        const float gv = (fin && co < Cout) ? load_g(d, dy, y, am, b, co, t, f) : 0.f;
        acc[n] = mfma4(a, gv, acc[n]);
      }
    }
  }
  float* ps = part + (int64_t)s * pl.Mtot * Cout;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int co = n * 16 + li;
    if (co >= Cout) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mo = mt * 16 + lk * 4 + r;
      if (mo < pl.Mtot) ps[(int64_t)mo * Cout + co] = acc[n][r];
    }
  }
}

// 16 columns x 16 slab groups per block: thread (c, g) sums slabs g, g+16, .. of column c, then the
// 16 group sums are added in group order -- the same order every run
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(WgradPlan pl, int Cout, const float* __restrict__ part,
                                                                float* __restrict__ dw, float* __restrict__ db,
                                                                int accumulate) {
  __shared__ float red[16][17];
  const int n = pl.Mtot * Cout;
  const int c = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int idx = blockIdx.x * 16 + c;
  float s = 0.f;
  if (idx < n)
    for (int k = grp; k < pl.nslab; k += 16) s += part[(int64_t)k * n + idx];
  red[grp][c] = s;
  __syncthreads();
  if (grp != 0 || idx >= n) return;
  float t = 0.f;
#pragma unroll
  for (int g = 0; g < 16; ++g) t += red[g][c];
  float* o = idx < pl.Ktot * Cout ? dw + idx : db + (idx - pl.Ktot * Cout);
  *o = accumulate ? *o + t : t;
}

__global__ __launch_bounds__(256) void conv_add_kernel(int64_t n, const float* a, const float* b, float* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = a[i] + b[i];
}

// ------------------------------------------------------------------ host
static int check_desc(const Desc* d, const char* who) {
  CHECK_ARG(d, "%s: null descriptor", who);
  CHECK_ARG(d->k == 3 || d->k == 5, "%s: k must be 3 or 5 (got %d)", who, d->k);
  CHECK_ARG(d->B >= 1 && d->T >= 1 && d->F >= 1, "%s: B, T, F must be >= 1", who);
  CHECK_ARG(d->Cin >= 1 && d->Cin <= 64 && d->Cout >= 1 && d->Cout <= 64,
            "%s: Cin, Cout must be in [1, 64] (got %d, %d)", who, d->Cin, d->Cout);
  CHECK_ARG(d->alpha >= 0.f && d->alpha < 1.f, "%s: alpha must be in [0, 1)", who);
  CHECK_ARG((d->pool == 0 || d->pool == 1) && (d->d2s == 0 || d->d2s == 1) && !(d->pool && d->d2s),
            "%s: pool and d2s are 0/1 flags and exclusive", who);
  CHECK_ARG(!d->pool || (d->T >= 2 && d->F >= 2), "%s: pool needs T, F >= 2", who);
  CHECK_ARG(!d->d2s || d->Cout % 4 == 0, "%s: d2s needs Cout %% 4 == 0", who);
  for (int a = 0; a < 4; ++a)
    CHECK_ARG(d->x_stride[a] >= 0 && d->y_stride[a] >= 0, "%s: negative stride", who);
  CHECK_ARG((int64_t)d->B * ((d->T + 1) / 2) * ((d->F + 15) / 16) < (1LL << 31) / 4 &&
                (int64_t)d->B * d->T < (1LL << 31),
            "%s: too many pixels", who);
  return DANET_CONV_OK;
}

static inline int ntiles(int n) { return n <= 16 ? 1 : (n <= 32 ? 2 : 4); }

#define CONV_DISPATCH(KERNEL, ks, nt, grid, stream, ...)                                   \
  do {                                                                                     \
    if (ks == 3) {                                                                         \
      if (nt == 1) KERNEL<3, 1><<<grid, 256, 0, stream>>>(__VA_ARGS__);                    \
      else if (nt == 2) KERNEL<3, 2><<<grid, 256, 0, stream>>>(__VA_ARGS__);               \
      else KERNEL<3, 4><<<grid, 256, 0, stream>>>(__VA_ARGS__);                            \
    } else {                                                                               \
      if (nt == 1) KERNEL<5, 1><<<grid, 256, 0, stream>>>(__VA_ARGS__);                    \
      else if (nt == 2) KERNEL<5, 2><<<grid, 256, 0, stream>>>(__VA_ARGS__);               \
      else KERNEL<5, 4><<<grid, 256, 0, stream>>>(__VA_ARGS__);                            \
    }                                                                                      \
  } while (0)

static int pixel_grid(const Desc& d) {
  const int64_t tiles = (int64_t)d.B * ((d.T + 1) / 2) * ((d.F + 15) / 16);
  return (int)((tiles + 3) / 4);
}

extern "C" size_t danet_conv_workspace_bytes(int op, const danet_conv_desc_t* d) {
  if (op != DANET_CONV_WS_BWD_WEIGHT) {
    set_error("danet_conv_workspace_bytes: unknown op %d", op);
    return (size_t)-1;
  }
  if (check_desc(d, "danet_conv_workspace_bytes") != DANET_CONV_OK) return (size_t)-1;
  const WgradPlan p = wgrad_plan(*d);
  return (size_t)p.nslab * p.Mtot * d->Cout * sizeof(float);
}

extern "C" int danet_conv_fwd(void* stream, const danet_conv_desc_t* d, const float* x, const float* w,
                              const float* bias, float* y, uint8_t* argmax) {
  const int rc = check_desc(d, "danet_conv_fwd");
  if (rc) return rc;
  CHECK_ARG(x && w && bias && y, "danet_conv_fwd: null pointer");
  CHECK_ARG(!d->pool || argmax, "danet_conv_fwd: pool needs argmax");
  CONV_DISPATCH(conv_fwd_kernel, d->k, ntiles(d->Cout), pixel_grid(*d), (hipStream_t)stream, *d, x, w, bias,
                y, argmax);
  CHECK_LAUNCH();
  return DANET_CONV_OK;
}

extern "C" int danet_conv_bwd_data(void* stream, const danet_conv_desc_t* d, const float* dy, const float* y,
                                   const uint8_t* argmax, const float* w, float* dx) {
  const int rc = check_desc(d, "danet_conv_bwd_data");
  if (rc) return rc;
  CHECK_ARG(dy && y && w && dx, "danet_conv_bwd_data: null pointer");
  CHECK_ARG(!d->pool || argmax, "danet_conv_bwd_data: pool needs argmax");
  CONV_DISPATCH(conv_dgrad_kernel, d->k, ntiles(d->Cin), pixel_grid(*d), (hipStream_t)stream, *d, dy, y,
                argmax, w, dx);
  CHECK_LAUNCH();
  return DANET_CONV_OK;
}

extern "C" int danet_conv_bwd_weight(void* stream, const danet_conv_desc_t* d, const float* x, const float* dy,
                                     const float* y, const uint8_t* argmax, float* dw, float* db,
                                     int accumulate, void* ws, size_t ws_bytes) {
  const int rc = check_desc(d, "danet_conv_bwd_weight");
  if (rc) return rc;
  CHECK_ARG(x && dy && y && dw && db && ws, "danet_conv_bwd_weight: null pointer");
  CHECK_ARG(!d->pool || argmax, "danet_conv_bwd_weight: pool needs argmax");
  const WgradPlan p = wgrad_plan(*d);
  if (ws_bytes < (size_t)p.nslab * p.Mtot * d->Cout * sizeof(float)) {
    set_error("danet_conv_bwd_weight: workspace too small");
    return DANET_CONV_ERR_WORKSPACE;
  }
  float* part = (float*)ws;
  const int grid = (int)(((int64_t)p.nslab * p.nmt + 3) / 4);
  CONV_DISPATCH(conv_wgrad_kernel, d->k, ntiles(d->Cout), grid, (hipStream_t)stream, *d, p, x, dy, y, argmax,
                part);
  CHECK_LAUNCH();
  const int n = p.Mtot * d->Cout;
  conv_wgrad_reduce_kernel<<<(n + 15) / 16, 256, 0, (hipStream_t)stream>>>(p, d->Cout, part, dw, db,
                                                                           accumulate ? 1 : 0);
  CHECK_LAUNCH();
  return DANET_CONV_OK;
}

extern "C" int danet_conv_add(void* stream, int64_t n, const float* a, const float* b, float* out) {
  CHECK_ARG(n > 0 && a && b && out, "danet_conv_add: bad args");
  int64_t g = (n + 255) / 256;
  const int grid = (int)(g < 4096 ? g : 4096);
  conv_add_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(n, a, b, out);
  CHECK_LAUNCH();
  return DANET_CONV_OK;
}
