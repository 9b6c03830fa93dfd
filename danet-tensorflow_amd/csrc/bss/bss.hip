/*
 * libdanet_bss_hip.so (include/danet_bss_hip.h): the BSS-eval figures of `valid` / `test` -- lagged float64
 * correlations of the synthesised waveforms, the block-Toeplitz systems they define, a batched blocked Cholesky
 * solve, and the permutation search that turns the quadratic forms into SDR, SIR, SAR and SDRi.  gfx950, wave64.
 *
 * danet_bss_xcorr.       A lane per lag, a workgroup per (utterance, pair of signals, 256 lags); both signals of a
 *                        tile in LDS as float64.
 * danet_bss_systems.     Element-wise: every entry of G, Gs, Xg, Xs is a copy or the ascending-k baseline sum.
 * danet_bss_chol_solve.  Right-looking, 64 columns a panel: potrf (LDS), trsm (a lane per row), syrk (f64 MFMA on
 *                        64 x 64 tiles of every matrix of the batch), then one launch for both triangular solves.
 * danet_bss_finalize.    One workgroup: a wave per dot product, a thread per utterance for the table and the search.
 */
#include <hip/hip_runtime.h>

#include "danet_bss_hip.h"
#define DANET_EXT bss
#define DANET_EXT_UPPER BSS
#include "ext_core.h"

static const int kMaxC = DANET_BSS_MAX_C;
static const int kMaxL = DANET_BSS_MAX_L;
static const int kNB = DANET_BSS_BLOCK;       /* 64: panel width, tile edge, lanes of a wave */
static const int kPad = kNB + 1;              /* row stride of a 64-column block in LDS      */
static const double kDblMax = 1.7976931348623157e308;

typedef double f64x4 __attribute__((ext_vector_type(4)));

static inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

static inline bool shape_ok(int B, int C, int L) {
  return B >= 1 && B <= DANET_BSS_MAX_BATCH && C >= 1 && C <= kMaxC && L >= 1 && L <= kMaxL;
}

#define CHECK_SHAPE(what)                                                                                      \
  CHECK_ARG(shape_ok(B, C, L), what ": need 1 <= B <= %d, 1 <= C <= %d and 1 <= L <= %d (got %d, %d, %d)",    \
            DANET_BSS_MAX_BATCH, kMaxC, kMaxL, B, C, L)

static inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" size_t danet_bss_workspace_bytes(int B, int C, int L) {
  if (!shape_ok(B, C, L)) {
    set_error("workspace_bytes: need 1 <= B <= %d, 1 <= C <= %d and 1 <= L <= %d (got %d, %d, %d)",
              DANET_BSS_MAX_BATCH, kMaxC, kMaxL, B, C, L);
    return (size_t)-1;
  }
  const size_t b = (size_t)B, c = (size_t)C, l = (size_t)L, n = c * l, d = sizeof(double), w = sizeof(int32_t);
  return round256(b * c * c * (2 * l - 1) * d) + round256(b * c * c * l * d) + round256(b * c * d) +
         round256(b * n * n * d) + round256(b * c * l * l * d) + round256(b * c * n * d) +
         round256(b * c * (c + 1) * l * d) + round256(b * w) + round256(b * c * w) + round256(b * 4 * d) +
         round256(b * w) + round256(b * w) + round256(4 * d);
}

/* ------------------------------------------------------------------------------------ correlations */
static const int kXLags = 256;     /* threads of a workgroup = lags it takes */
static const int kXTile = 1024;    /* samples of a tile                      */

/* job `job` of an utterance: rows xr, yr of wav[b], first lag, number of lags; kind 0 = R_ik (p = i, q = k),
 * 1 = D_ji (p = j, q = i), 2 = ee_j (p = j).  The C (C + 1) / 2 pairs i <= k first, then the C * C pairs
 * (j, i), then the C estimates. */
struct XJob { int xr, yr, lag0, nlag, kind, p, q; };

__device__ __forceinline__ XJob xcorr_job(int C, int L, int job) {
  XJob j;
  const int n_rr = C * (C + 1) / 2;
  if (job < n_rr) {
    int i = 0, p = job;
    while (p >= C - i) { p -= C - i; ++i; }
    const int k = i + p;
    j.xr = i; j.yr = k; j.kind = 0; j.p = i; j.q = k;
    j.lag0 = i == k ? 0 : -(L - 1);
    j.nlag = i == k ? L : 2 * L - 1;
  } else if (job < n_rr + C * C) {
    const int e = job - n_rr, jj = e / C, i = e - jj * C;
    j.xr = i; j.yr = C + jj; j.kind = 1; j.p = jj; j.q = i;
    j.lag0 = 0; j.nlag = L;
  } else {
    const int jj = job - n_rr - C * C;
    j.xr = C + jj; j.yr = C + jj; j.kind = 2; j.p = jj; j.q = 0;
    j.lag0 = 0; j.nlag = 1;
  }
  return j;
}

__global__ __launch_bounds__(kXLags) void bss_xcorr_kernel(int C, int L, int Ls, const float* __restrict__ wav,
                                                           double* __restrict__ R, double* __restrict__ D,
                                                           double* __restrict__ ee) {
  __shared__ double xs[kXTile];
  __shared__ double ys[kXTile + kXLags];
  const int b = blockIdx.z, chunk = blockIdx.x, tid = threadIdx.x;
  const XJob j = xcorr_job(C, L, (int)blockIdx.y);
  if (chunk * kXLags >= j.nlag) return;                        /* (uniform over the workgroup) */
  const int tau0 = j.lag0 + chunk * kXLags;                    /* the lag of lane 0 */
  const float* x = wav + ((int64_t)b * 2 * C + j.xr) * Ls;
  const float* y = wav + ((int64_t)b * 2 * C + j.yr) * Ls;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t n0 = 0; n0 < Ls; n0 += kXTile) {
    const int nt = (int)min((int64_t)kXTile, (int64_t)Ls - n0), nt4 = (nt + 3) & ~3;
    __syncthreads();                                           /* the tile before has been read */
    for (int m = tid; m < nt4; m += kXLags) xs[m] = m < nt ? (double)x[n0 + m] : 0.0;
    for (int m = tid; m < nt4 + kXLags; m += kXLags) {
      const int64_t g = n0 + tau0 + m;
      ys[m] = (g >= 0 && g < Ls) ? (double)y[g] : 0.0;
    }
    __syncthreads();
    const double* yp = ys + tid;                               /* yp[m] = y[n0 + m + the lane's lag] */
    for (int m = 0; m < nt4; m += 4) {
      a0 += xs[m] * yp[m];
      a1 += xs[m + 1] * yp[m + 1];
      a2 += xs[m + 2] * yp[m + 2];
      a3 += xs[m + 3] * yp[m + 3];
    }
  }
  const double r = (a0 + a1) + (a2 + a3);
  const int t = chunk * kXLags + tid;
  if (t >= j.nlag) return;
  const int tau = j.lag0 + t, W = 2 * L - 1;
  if (j.kind == 0) {
    double* rb = R + (int64_t)b * C * C * W;
    rb[((int64_t)j.p * C + j.q) * W + (tau + L - 1)] = r;
    rb[((int64_t)j.q * C + j.p) * W + (L - 1 - tau)] = r;
  } else if (j.kind == 1) {
    D[(((int64_t)b * C + j.p) * C + j.q) * L + tau] = r;
  } else {
    ee[(int64_t)b * C + j.p] = r;
  }
}

extern "C" int danet_bss_xcorr(void* stream, int B, int C, int64_t Ls, int L, const float* wav, double* R,
                               double* D, double* ee) {
  CHECK_SHAPE("xcorr");
  CHECK_ARG(Ls >= 1 && Ls < ((int64_t)1 << 31), "xcorr: Ls must be in [1, 2^31) (got %lld)", (long long)Ls);
  CHECK_ARG(wav && R && D && ee, "xcorr: null pointer");
  CHECK_ARG(aligned(wav, 4) && aligned(R, 8) && aligned(D, 8) && aligned(ee, 8),
            "xcorr: misaligned pointer (wav 4-byte; R, D, ee 8-byte)");
  const int jobs = C * (C + 1) / 2 + C * C + C, chunks = (2 * L - 1 + kXLags - 1) / kXLags;
  bss_xcorr_kernel<<<dim3(chunks, jobs, B), kXLags, 0, (hipStream_t)stream>>>(C, L, (int)Ls, wav, R, D, ee);
  CHECK_LAUNCH();
  return DANET_BSS_OK;
}

/* ------------------------------------------------------------------------------------------ systems */
__global__ __launch_bounds__(256) void bss_systems_kernel(int C, int L, const double* __restrict__ R,
                                                          const double* __restrict__ D, double* __restrict__ G,
                                                          double* __restrict__ Gs, double* __restrict__ Xg,
                                                          double* __restrict__ Xs) {
  const int b = blockIdx.y, n = C * L, W = 2 * L - 1;
  const int nG = n * n, nGs = C * L * L, nXg = C * n, nXs = C * (C + 1) * L;
  const double* rb = R + (int64_t)b * C * C * W;
  const double* db = D + (int64_t)b * C * C * L;
  bool live[kMaxC];
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) live[i] = i < C && rb[((int64_t)i * C + i) * W + (L - 1)] != 0.0;
  auto is_live = [&](int i) { return i == 0 ? live[0] : (i == 1 ? live[1] : (i == 2 ? live[2] : live[3])); };
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nG + nGs + nXg + nXs; e += gridDim.x * 256) {
    if (e < nG) {
      const int row = e / n, col = e - row * n;
      const int i = row / L, t1 = row - i * L, k = col / L, t2 = col - k * L;
      double v;
      if (is_live(i) && is_live(k)) v = rb[((int64_t)i * C + k) * W + (t1 - t2 + L - 1)];
      else v = row == col ? 1.0 : 0.0;
      G[(int64_t)b * nG + e] = v;
    } else if (e < nG + nGs) {
      const int f = e - nG;
      const int i = f / (L * L), r = f - i * L * L, t1 = r / L, t2 = r - t1 * L;
      Gs[(int64_t)b * nGs + f] = is_live(i) ? rb[((int64_t)i * C + i) * W + (t1 - t2 + L - 1)] : (t1 == t2 ? 1.0 : 0.0);
    } else if (e < nG + nGs + nXg) {
      const int f = e - nG - nGs;
      const int jj = f / n, r = f - jj * n, i = r / L;
      Xg[(int64_t)b * nXg + f] = is_live(i) ? db[(int64_t)jj * n + r] : 0.0;
    } else {
      const int f = e - nG - nGs - nXg;
      const int i = f / ((C + 1) * L), r = f - i * (C + 1) * L, jj = r / L, t = r - jj * L;
      double v = 0.0;
      if (is_live(i)) {
        if (jj < C) v = db[((int64_t)jj * C + i) * L + t];
        else
          for (int k = 0; k < C; ++k) v += rb[((int64_t)i * C + k) * W + (t + L - 1)];
      }
      Xs[(int64_t)b * nXs + f] = v;
    }
  }
}

extern "C" int danet_bss_systems(void* stream, int B, int C, int L, const double* R, const double* D, double* G,
                                 double* Gs, double* Xg, double* Xs) {
  CHECK_SHAPE("systems");
  CHECK_ARG(R && D && G && Gs && Xg && Xs, "systems: null pointer");
  CHECK_ARG(aligned(R, 8) && aligned(D, 8) && aligned(G, 8) && aligned(Gs, 8) && aligned(Xg, 8) && aligned(Xs, 8),
            "systems: misaligned pointer (all 8-byte)");
  const int n = C * L, total = n * n + C * L * L + C * n + C * (C + 1) * L;      /* < 2^23 */
  int blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  bss_systems_kernel<<<dim3(blocks, B), 256, 0, (hipStream_t)stream>>>(C, L, R, D, G, Gs, Xg, Xs);
  CHECK_LAUNCH();
  return DANET_BSS_OK;
}

/* ----------------------------------------------------------------------------------------- Cholesky */
/* the diagonal block of panel k0 (kw = min(64, n - k0) columns), one workgroup of 256 threads per matrix */
__global__ __launch_bounds__(256) void bss_potrf_kernel(int n, int k0, double* __restrict__ A,
                                                        int32_t* __restrict__ flags) {
  __shared__ double s[kNB * kPad];
  const int tid = threadIdx.x, kw = min(kNB, n - k0);
  double* a = A + (int64_t)blockIdx.x * n * n;
  for (int idx = tid; idx < kNB * kNB; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    s[r * kPad + c] = (r < kw && c <= r) ? a[(int64_t)(k0 + r) * n + (k0 + c)] : 0.0;
  }
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < kw; ++j) {
    const double d = s[j * kPad + j];
    bad = bad || !(d > 0.0 && d <= kDblMax);
    const double sd = __dsqrt_rn(d);
    __syncthreads();                                           /* every thread has read the pivot */
    if (tid == 0) s[j * kPad + j] = sd;
    if (tid > j && tid < kw) s[tid * kPad + j] = s[tid * kPad + j] / sd;
    __syncthreads();
    for (int idx = (j + 1) * kNB + tid; idx < kw * kNB; idx += 256) {
      const int r = idx >> 6, c = idx & 63;
      if (c > j && c <= r) s[r * kPad + c] -= s[r * kPad + j] * s[c * kPad + j];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kNB * kNB; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    if (r < kw && c <= r) a[(int64_t)(k0 + r) * n + (k0 + c)] = s[r * kPad + c];
  }
  if (tid == 0) flags[blockIdx.x] = (k0 == 0 ? 0 : flags[blockIdx.x]) | (bad ? 1 : 0);
}

/* rows i0 .. i0 + 63 below the (full, 64-column) panel k0: X L_kk^T = A, a lane per row, one wave per workgroup;
 * the result goes to A[i][k0 + c] and, transposed, to A[k0 + c][i] */
__global__ __launch_bounds__(kNB) void bss_trsm_kernel(int n, int k0, double* __restrict__ A) {
  __shared__ double lk[kNB * (kNB + 1) / 2];                   /* the lower triangle, row r at r (r + 1) / 2 */
  __shared__ double as[kNB * kPad];
  const int tid = threadIdx.x;
  double* a = A + (int64_t)blockIdx.y * n * n;
  const int i0 = k0 + kNB + (int)blockIdx.x * kNB, rows = min(kNB, n - i0);
  for (int idx = tid; idx < kNB * kNB; idx += kNB) {
    const int r = idx >> 6, c = idx & 63;
    if (c <= r) lk[r * (r + 1) / 2 + c] = a[(int64_t)(k0 + r) * n + (k0 + c)];
    as[r * kPad + c] = r < rows ? a[(int64_t)(i0 + r) * n + (k0 + c)] : 0.0;
  }
  __syncthreads();
  double* row = as + tid * kPad;
  for (int c = 0; c < kNB; ++c) {
    const double* l = lk + c * (c + 1) / 2;
    double v = row[c];
    for (int j = 0; j < c; ++j) v -= row[j] * l[j];
    row[c] = v / l[c];
  }
  __syncthreads();
  for (int idx = tid; idx < kNB * kNB; idx += kNB) {
    const int r = idx >> 6, c = idx & 63;
    if (r < rows) a[(int64_t)(i0 + r) * n + (k0 + c)] = as[r * kPad + c];
  }
  for (int idx = tid; idx < kNB * kNB; idx += kNB) {
    const int c = idx >> 6, r = idx & 63;
    if (r < rows) a[(int64_t)(k0 + c) * n + (i0 + r)] = as[r * kPad + c];
  }
}

/* the trailing update behind the (full) panel k0: tile (bi >= bj) of the lower triangle of A[k0 + 64 ..],
 * A_ij -= L_ik L_jk^T, 256 threads: wave w takes rows 16 w .. 16 w + 15 of the tile and all 64 columns in four
 * 16 x 16 MFMA accumulators.  v_mfma_f64_16x16x4_f64: lane l feeds A[row l & 15][k = l >> 4] and
 * B[k = l >> 4][col l & 15], and holds D[row (l >> 4) + 4 reg][col l & 15], reg < 4. */
static const int kSlab = 32, kSlabPad = kSlab + 1;
__global__ __launch_bounds__(256) void bss_syrk_kernel(int n, int k0, double* __restrict__ A) {
  __shared__ double sa[kNB * kSlabPad];
  __shared__ double sb[kNB * kSlabPad];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double* a = A + (int64_t)blockIdx.y * n * n;
  int t = (int)blockIdx.x, bi = 0;
  while (t > bi) { t -= bi + 1; ++bi; }                        /* row bi of the triangle has bi + 1 tiles */
  const int i0 = k0 + kNB + bi * kNB, j0 = k0 + kNB + t * kNB;
  f64x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = (f64x4){0.0, 0.0, 0.0, 0.0};
  for (int kc = 0; kc < kNB; kc += kSlab) {
    __syncthreads();
    for (int idx = tid; idx < kNB * kSlab; idx += 256) {
      const int r = idx >> 5, c = idx & 31;
      sa[r * kSlabPad + c] = i0 + r < n ? a[(int64_t)(i0 + r) * n + (k0 + kc + c)] : 0.0;
      sb[r * kSlabPad + c] = j0 + r < n ? a[(int64_t)(j0 + r) * n + (k0 + kc + c)] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kSlab; kk += 4) {
      const double av = sa[(16 * wave + (lane & 15)) * kSlabPad + kk + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double bv = sb[(16 * q + (lane & 15)) * kSlabPad + kk + (lane >> 4)];
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = i0 + 16 * wave + (lane >> 4) + 4 * reg, c = j0 + 16 * q + (lane & 15);
      if (r < n && c <= r) a[(int64_t)r * n + c] -= acc[q][reg];
    }
  }
}

/* both triangular solves of one right-hand side of one matrix, 256 threads.  Block by block: thread (c, q) adds
 * A[r][k0 + c] * v[r] over the rows r = first + q, first + q + 4, ... of the finished part (above the block in the
 * forward sweep: the transposed copies; below it in the backward sweep), the four q join as (p0 + p1) + (p2 + p3),
 * and wave 0 substitutes through the diagonal block, a lane per unknown. */
__global__ __launch_bounds__(256) void bss_trisolve_kernel(int n, int nrhs, const double* __restrict__ A,
                                                           double* __restrict__ X) {
  __shared__ double v[DANET_BSS_MAX_N];
  __shared__ double lk[kNB * kPad];
  __shared__ double part[4 * kNB];
  const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  const double* a = A + (int64_t)blockIdx.y * n * n;
  double* x = X + ((int64_t)blockIdx.y * nrhs + blockIdx.x) * n;
  for (int i = tid; i < n; i += 256) v[i] = x[i];
  const int nblk = (n + kNB - 1) / kNB;
  for (int pass = 0; pass < 2; ++pass) {
    for (int step = 0; step < nblk; ++step) {
      const int kb = pass == 0 ? step : nblk - 1 - step;
      const int k0 = kb * kNB, kw = min(kNB, n - k0);
      const int first = pass == 0 ? 0 : k0 + kw, last = pass == 0 ? k0 : n;
      __syncthreads();                                         /* v of the block before is complete */
      double acc = 0.0;
      if (c < kw)
        for (int r = first + q; r < last; r += 4) acc += a[(int64_t)r * n + (k0 + c)] * v[r];
      part[q * kNB + c] = acc;
      for (int idx = tid; idx < kNB * kNB; idx += 256) {
        const int r = idx >> 6, cc = idx & 63;
        lk[r * kPad + cc] = (r < kw && cc <= r) ? a[(int64_t)(k0 + r) * n + (k0 + cc)] : (r == cc ? 1.0 : 0.0);
      }
      __syncthreads();
      if (tid < kNB) {
        double t = tid < kw ? v[k0 + tid] - ((part[tid] + part[kNB + tid]) + (part[2 * kNB + tid] + part[3 * kNB + tid]))
                            : 0.0;
        if (pass == 0) {
          for (int j = 0; j < kw; ++j) {                       /* L y = t */
            const double xj = __shfl(t, j, 64) / lk[j * kPad + j];
            if (tid == j) t = xj;
            else if (tid > j) t -= lk[tid * kPad + j] * xj;
          }
        } else {
          for (int j = kw - 1; j >= 0; --j) {                  /* L^T x = t */
            const double xj = __shfl(t, j, 64) / lk[j * kPad + j];
            if (tid == j) t = xj;
            else if (tid < j) t -= lk[j * kPad + tid] * xj;
          }
        }
        if (tid < kw) v[k0 + tid] = t;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) x[i] = v[i];
}

extern "C" int danet_bss_chol_solve(void* stream, int nmat, int n, int nrhs, double* A, double* X, int32_t* flags) {
  CHECK_ARG(nmat >= 1 && nmat <= DANET_BSS_MAX_BATCH, "chol_solve: nmat must be in 1..%d (got %d)",
            DANET_BSS_MAX_BATCH, nmat);
  CHECK_ARG(n >= 1 && n <= DANET_BSS_MAX_N, "chol_solve: n must be in 1..%d (got %d)", DANET_BSS_MAX_N, n);
  CHECK_ARG(nrhs >= 1 && nrhs <= DANET_BSS_MAX_RHS, "chol_solve: nrhs must be in 1..%d (got %d)", DANET_BSS_MAX_RHS,
            nrhs);
  CHECK_ARG(A && X && flags, "chol_solve: null pointer");
  CHECK_ARG(aligned(A, 8) && aligned(X, 8) && aligned(flags, 4),
            "chol_solve: misaligned pointer (A, X 8-byte; flags 4-byte)");
  hipStream_t s = (hipStream_t)stream;
  for (int k0 = 0; k0 < n; k0 += kNB) {
    bss_potrf_kernel<<<dim3(nmat), 256, 0, s>>>(n, k0, A, flags);
    CHECK_LAUNCH();
    const int below = n - k0 - kNB;                            /* rows under a full panel */
    if (below > 0) {
      const int mb = (below + kNB - 1) / kNB;
      bss_trsm_kernel<<<dim3(mb, nmat), kNB, 0, s>>>(n, k0, A);
      CHECK_LAUNCH();
      bss_syrk_kernel<<<dim3(mb * (mb + 1) / 2, nmat), 256, 0, s>>>(n, k0, A);
      CHECK_LAUNCH();
    }
  }
  bss_trisolve_kernel<<<dim3(nrhs, nmat), 256, 0, s>>>(n, nrhs, A, X);
  CHECK_LAUNCH();
  return DANET_BSS_OK;
}

/* ----------------------------------------------------------------------------------------- finalize */
static const int kFinThreads = 1024, kFinWaves = kFinThreads / 64;
static const int kFinUtts = 32;                                /* utterances of one pass            */
static const int kFinDots = kMaxC + kMaxC * (kMaxC + 1);       /* pall_j, then st_ij with j = C: base */

__device__ __forceinline__ double bss_q(double a, double b) {
  if (!(a > 0.0)) return -100.0;
  if (!(b > 0.0)) return 100.0;
  const double d = 10.0 * log10(a / b);
  return d < -100.0 ? -100.0 : (d > 100.0 ? 100.0 : d);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

/* every thread: the sum over the workgroup of 1024 -- the waves' butterflies joined pairwise in order */
__device__ __forceinline__ double fin_block_sum(double v, double* part) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double p[kFinWaves];
#pragma unroll
  for (int w = 0; w < kFinWaves; ++w) p[w] = part[w];
#pragma unroll
  for (int h = 1; h < kFinWaves; h <<= 1)
#pragma unroll
    for (int w = 0; w < kFinWaves; w += 2 * h) p[w] += p[w + h];
  return p[0];
}

/* the p-th permutation of range(C) in itertools.permutations (lexicographic) order -> perm[0..C-1] */
__device__ __forceinline__ void nth_perm(int C, int p, int* perm) {
  int avail[kMaxC] = {0, 1, 2, 3};
  int fact = 1;
  for (int i = 2; i < C; ++i) fact *= i;
  for (int i = 0; i < C; ++i) {
    const int qd = p / fact;
    p -= qd * fact;
    perm[i] = avail[qd];
    for (int m = qd; m + 1 < kMaxC; ++m) avail[m] = avail[m + 1];
    if (C - 1 - i > 1) fact /= (C - 1 - i);
  }
}

__global__ __launch_bounds__(kFinThreads) void bss_finalize_kernel(
    int B, int C, int L, const double* __restrict__ R, const double* __restrict__ D, const double* __restrict__ ee,
    const double* __restrict__ Xg, const double* __restrict__ Xs, const int32_t* __restrict__ fg,
    const int32_t* __restrict__ fs, int b0, int B_all, double* per_utt, int32_t* perm_idx, int32_t* flags,
    double* __restrict__ mean4) {
  __shared__ double dots[kFinUtts * kFinDots];
  __shared__ double part[kFinWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = C * L, W = 2 * L - 1, nd = C + C * (C + 1);
  for (int u0 = 0; u0 < B; u0 += kFinUtts) {
    const int nu = min(kFinUtts, B - u0);
    __syncthreads();                                           /* dots of the pass before have been read */
    for (int job = wave; job < nu * nd; job += kFinWaves) {
      const int u = job / nd, d = job - u * nd, b = u0 + u;
      const double* rb = R + (int64_t)b * C * C * W;
      double acc = 0.0;
      if (d < C) {
        const double* rhs = D + ((int64_t)b * C + d) * n;
        const double* sol = Xg + ((int64_t)b * C + d) * n;
        for (int t = lane; t < n; t += 64) acc += rhs[t] * sol[t];
      } else {
        const int e = d - C, i = e / (C + 1), jj = e - i * (C + 1);
        const double* sol = Xs + (((int64_t)b * C + i) * (C + 1) + jj) * L;
        if (jj < C) {
          const double* rhs = D + (((int64_t)b * C + jj) * C + i) * L;
          for (int t = lane; t < L; t += 64) acc += rhs[t] * sol[t];
        } else {
          for (int t = lane; t < L; t += 64) {
            double m = 0.0;
            for (int k = 0; k < C; ++k) m += rb[((int64_t)i * C + k) * W + (t + L - 1)];
            acc += m * sol[t];
          }
        }
      }
      acc = wave_sum(acc);
      if (lane == 0) dots[u * kFinDots + d] = acc;
    }
    __syncthreads();
    if (tid < nu) {
      const int b = u0 + tid;
      const double* rb = R + (int64_t)b * C * C * W;
      const double* dt = dots + tid * kFinDots;
      bool live[kMaxC];
      int n_live = 0, flag = fg[b] != 0 ? 1 : 0;
      double mm = 0.0;
      for (int i = 0; i < C; ++i) {
        live[i] = rb[((int64_t)i * C + i) * W + (L - 1)] != 0.0;
        n_live += live[i] ? 1 : 0;
        if (fs[(int64_t)b * C + i] != 0) flag = 1;
        for (int k = 0; k < C; ++k) mm += rb[((int64_t)i * C + k) * W + (L - 1)];
      }
      double o_sdr = 0.0, o_sir = 0.0, o_sar = 0.0, o_imp = 0.0;
      int best = 0;
      if (flag == 0 && n_live > 0) {
        double sdr[kMaxC][kMaxC], sir[kMaxC][kMaxC], sar[kMaxC], base[kMaxC];
        for (int jj = 0; jj < C; ++jj) {
          const double e = ee[(int64_t)b * C + jj], pall = dt[jj];
          sar[jj] = bss_q(pall, e - pall);
          for (int i = 0; i < C; ++i) {
            const double st = dt[C + i * (C + 1) + jj];
            sdr[i][jj] = bss_q(st, e - st);
            sir[i][jj] = bss_q(st, pall - st);
          }
        }
        for (int i = 0; i < C; ++i) {
          const double st = dt[C + i * (C + 1) + C];
          base[i] = bss_q(st, mm - st);
        }
        int nperm = 1;
        for (int i = 2; i <= C; ++i) nperm *= i;
        double best_v = 0.0;
        int perm[kMaxC];
        for (int p = 0; p < nperm; ++p) {
          nth_perm(C, p, perm);
          double s = 0.0;
          for (int i = 0; i < C; ++i)
            if (live[i]) s += sir[i][perm[i]];
          if (p == 0 || s > best_v) { best = p; best_v = s; }
        }
        nth_perm(C, best, perm);
        for (int i = 0; i < C; ++i)
          if (live[i]) {
            o_sdr += sdr[i][perm[i]];
            o_sir += sir[i][perm[i]];
            o_sar += sar[perm[i]];
            o_imp += sdr[i][perm[i]] - base[i];
          }
        const double nl = (double)n_live;
        o_sdr /= nl; o_sir /= nl; o_sar /= nl; o_imp /= nl;
      }
      double* out = per_utt + 4 * (int64_t)(b0 + b);
      out[0] = o_sdr; out[1] = o_sir; out[2] = o_sar; out[3] = o_imp;
      perm_idx[b0 + b] = best;
      flags[b0 + b] = flag | (n_live == 0 ? 2 : 0);
    }
  }
  if (b0 + B != B_all) return;
  __threadfence_block();
  __syncthreads();                                             /* this call's rows are visible to the workgroup */
  double s[4] = {0.0, 0.0, 0.0, 0.0}, cnt = 0.0;
  for (int b = tid; b < B_all; b += kFinThreads)
    if (flags[b] == 0) {
      for (int k = 0; k < 4; ++k) s[k] += per_utt[4 * (int64_t)b + k];
      cnt += 1.0;
    }
  const double tn = fin_block_sum(cnt, part);
  for (int k = 0; k < 4; ++k) {
    const double ts = fin_block_sum(s[k], part);
    if (tid == 0) mean4[k] = tn > 0.0 ? ts / tn : 0.0;
  }
}

extern "C" int danet_bss_finalize(void* stream, int B, int C, int L, const double* R, const double* D,
                                  const double* ee, const double* Xg, const double* Xs, const int32_t* fg,
                                  const int32_t* fs, int b0, int B_all, double* per_utt, int32_t* perm_idx,
                                  int32_t* flags, double* mean4) {
  CHECK_SHAPE("finalize");
  CHECK_ARG(b0 >= 0 && B_all <= DANET_BSS_MAX_BATCH && (int64_t)b0 + B <= B_all,
            "finalize: need b0 >= 0 and b0 + B <= B_all <= %d (got b0 = %d, B = %d, B_all = %d)", DANET_BSS_MAX_BATCH,
            b0, B, B_all);
  CHECK_ARG(R && D && ee && Xg && Xs && fg && fs && per_utt && perm_idx && flags && mean4, "finalize: null pointer");
  CHECK_ARG(aligned(R, 8) && aligned(D, 8) && aligned(ee, 8) && aligned(Xg, 8) && aligned(Xs, 8) &&
                aligned(per_utt, 8) && aligned(mean4, 8) && aligned(fg, 4) && aligned(fs, 4) && aligned(perm_idx, 4) &&
                aligned(flags, 4),
            "finalize: misaligned pointer (fg, fs, perm_idx, flags 4-byte; all else 8-byte)");
  bss_finalize_kernel<<<dim3(1), kFinThreads, 0, (hipStream_t)stream>>>(B, C, L, R, D, ee, Xg, Xs, fg, fs, b0, B_all,
                                                                       per_utt, perm_idx, flags, mean4);
  CHECK_LAUNCH();
  return DANET_BSS_OK;
}
