/*
 * libdanet_stoi_hip.so (include/danet_stoi_hip.h): STOI and ESTOI of `valid` / `test` -- the synthesised waveforms
 * resampled to 10 kHz, the silent frames of every reference removed, one-third-octave band magnitudes of the
 * compacted frames, the 30-frame segment correlations, and the permutation search.  gfx950, wave64.
 *
 * danet_stoi_resample.  A thread per output; the table and the input span of up to 256 outputs in LDS.
 * danet_stoi_frames.    A workgroup per reference row: a wave per frame energy, then a ballot prefix scan.
 * danet_stoi_bands.     A wave per frame, four frames a workgroup: gather, 512-point real FFT in LDS (float64), bands.
 * danet_stoi_segments.  A workgroup per (utterance, reference, other signal), a thread per segment.
 * danet_stoi_finalize.  One workgroup, a thread per utterance for the search, then the batch means.
 */
#include <hip/hip_runtime.h>

#include "danet_stoi_hip.h"
#define DANET_EXT stoi
#define DANET_EXT_UPPER STOI
#include "ext_core.h"

static const int kThreads = 256, kWaves = kThreads / 64;
static const int kMaxC = DANET_STOI_MAX_C;
static const int kFrame = DANET_STOI_FRAME, kHop = DANET_STOI_HOP, kBands = DANET_STOI_BANDS, kSeg = DANET_STOI_SEG;
static const int kHalf = kFrame;                   /* points of the complex FFT behind the 512-point real one */
static const int kPitch = kHalf + 1;               /* 257 bins; odd: consecutive frames start on different banks */
static const int kSpanMax = 20480;                 /* floats of staged input a workgroup of the resampler holds */
static const double kClip = 6.623413251903491;     /* 1 + 10^(15/20) */
static const double kDyn = 1e-4;                   /* 40 dB */

static inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
static inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int gcd_of(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

static inline int half_len(int U, int D) { return (U == 1 && D == 1) ? 0 : 10 * (U > D ? U : D); }

static inline bool rate_ok(int U, int D) {
  if (U < 1 || D < 1 || U > DANET_STOI_MAX_TABLE || D > DANET_STOI_MAX_TABLE) return false;
  return gcd_of(U, D) == 1 && 2 * half_len(U, D) + 1 <= DANET_STOI_MAX_TABLE;
}

static inline int64_t frames_of(int64_t L10) { return L10 >= kFrame ? (L10 - kFrame) / kHop + 1 : 0; }

static inline bool batch_ok(int B, int C) { return B >= 1 && B <= DANET_STOI_MAX_BATCH && C >= 1 && C <= kMaxC; }
static inline bool len_ok(int64_t L) { return L >= 1 && L < ((int64_t)1 << 31); }

#define CHECK_BATCH(what)                                                                                       \
  CHECK_ARG(batch_ok(B, C), what ": need 1 <= B <= %d and 1 <= C <= %d (got %d, %d)", DANET_STOI_MAX_BATCH, kMaxC, \
            B, C)
#define CHECK_RATE(what)                                                                                        \
  CHECK_ARG(rate_ok(U, D), what ": U and D must be coprime positive integers with 20 max(U, D) + 1 <= %d "      \
            "(got %d, %d)", DANET_STOI_MAX_TABLE, U, D)

extern "C" size_t danet_stoi_workspace_bytes(int B, int C, int64_t Ls, int U, int D) {
  if (!batch_ok(B, C) || !rate_ok(U, D) || !len_ok(Ls) || !len_ok((Ls * U + D - 1) / D)) {
    set_error("workspace_bytes: need 1 <= B <= %d, 1 <= C <= %d, Ls and ceil(Ls U / D) in [1, 2^31), U and D coprime "
              "with 20 max(U, D) + 1 <= %d (got %d, %d, %lld, %d, %d)", DANET_STOI_MAX_BATCH, kMaxC,
              DANET_STOI_MAX_TABLE, B, C, (long long)Ls, U, D);
    return (size_t)-1;
  }
  const size_t L10 = (size_t)((Ls * U + D - 1) / D), nf = (size_t)frames_of((int64_t)L10), nfp = nf ? nf : 1;
  const size_t b = (size_t)B, c = (size_t)C, d = sizeof(double), w = sizeof(int32_t);
  return round256(b * (2 * c + 1) * L10 * sizeof(float)) + round256(b * c * nfp * d) + round256(b * c * nfp * w) +
         round256(b * c * nfp * w) + round256(b * c * w) + round256(b * c * d) +
         round256(b * c * (c + 2) * kBands * nfp * d) + round256(b * c * (c + 1) * 2 * d) + round256(b * 4 * d) +
         round256(b * w) + round256(b * w) + round256(4 * d) + round256(w);
}

/* ----------------------------------------------------------------------------------------- resample */
struct ResArgs {
  const float* wav;
  const float* h;
  float* sig;
  int64_t Ls, L10;
  int C, U, D, H, ntab, tile;
};

__global__ __launch_bounds__(kThreads) void stoi_resample_kernel(ResArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* tab = reinterpret_cast<float*>(smem);                 /* [ntab], padded to a multiple of 4 */
  float* xs = tab + ((a.ntab + 3) & ~3);                       /* the staged span                   */
  const int tid = threadIdx.x, r = blockIdx.y, b = blockIdx.z, C = a.C;
  const int64_t U = a.U, D = a.D, H = a.H, Ls = a.Ls;
  const int64_t n0 = (int64_t)blockIdx.x * a.tile;
  const int64_t n1 = n0 + a.tile < a.L10 ? n0 + a.tile : a.L10;
  const f32x4* hv = reinterpret_cast<const f32x4*>(a.h);
  for (int q = tid; q < a.ntab / 4; q += kThreads) *reinterpret_cast<f32x4*>(tab + 4 * q) = hv[q];
  for (int q = (a.ntab & ~3) + tid; q < a.ntab; q += kThreads) tab[q] = a.h[q];

  /* the samples k the outputs n0 .. n1 - 1 reach: 0 <= n D + H - k U <= 2H, inside [0, Ls) */
  const int64_t lo = n0 * D - H;
  const int64_t first = lo <= 0 ? 0 : (lo + U - 1) / U;
  int64_t last = ((n1 - 1) * D + H) / U;
  if (last > Ls - 1) last = Ls - 1;
  const bool mix = r == 2 * C;
  const float* x0 = a.wav + ((int64_t)b * 2 * C + (mix ? 0 : r)) * Ls;
  /* xs[0] is sample `start`: the 16-byte aligned address at or below sample `first` */
  const int64_t start = first - (int64_t)((((uintptr_t)x0 >> 2) + (uint64_t)first) & 3);
  const int nvec = last >= first ? (int)((last - start) / 4 + 1) : 0;
  const bool vec_ok = !mix || (Ls & 3) == 0;                   /* the rows of a mixture share one alignment */
  for (int v = tid; v < nvec; v += kThreads) {
    const int64_t i = start + 4 * (int64_t)v;
    f32x4 x;
    if (vec_ok && i >= 0 && i + 4 <= Ls) {
      x = *reinterpret_cast<const f32x4*>(x0 + i);
      if (mix)
        for (int c = 1; c < C; ++c) x += *reinterpret_cast<const f32x4*>(x0 + (int64_t)c * Ls + i);
    } else {
      for (int k = 0; k < 4; ++k) {
        float s = 0.0f;
        if (i + k >= 0 && i + k < Ls) {
          s = x0[i + k];
          if (mix)
            for (int c = 1; c < C; ++c) s += x0[(int64_t)c * Ls + i + k];
        }
        x[k] = s;
      }
    }
    *reinterpret_cast<f32x4*>(xs + 4 * v) = x;
  }
  __syncthreads();
  for (int64_t n = n0 + tid; n < n1; n += kThreads) {
    const int64_t c = n * D + H;                               /* the table index at k = 0 */
    const int64_t klo = c - 2 * H <= 0 ? 0 : (c - 2 * H + U - 1) / U;
    int64_t khi = c / U;
    if (khi > Ls - 1) khi = Ls - 1;
    const float* xp = xs + (klo - start);
    int ti = (int)(c - klo * U);
    double acc = 0.0;
    for (int64_t k = klo; k <= khi; ++k, ti -= (int)U, ++xp) acc += (double)tab[ti] * (double)*xp;
    a.sig[((int64_t)b * (2 * C + 1) + r) * a.L10 + n] = (float)acc;
  }
}

/* floats of staged input `tile` outputs can reach: their samples, 3 of alignment shift, rounded up to 16 bytes */
static inline int64_t span_cap(int64_t tile, int U, int D, int H) {
  return ((((tile - 1) * D + 2 * (int64_t)H) / U + 1 + 3 + 3) & ~(int64_t)3) + 4;
}

extern "C" int danet_stoi_resample(void* stream, int B, int C, int64_t Ls, int U, int D, const float* wav,
                                   const float* h, float* sig) {
  CHECK_BATCH("resample");
  CHECK_RATE("resample");
  CHECK_ARG(len_ok(Ls) && len_ok((Ls * U + D - 1) / D),
            "resample: Ls and ceil(Ls U / D) must be in [1, 2^31) (got Ls = %lld)", (long long)Ls);
  CHECK_ARG(wav && h && sig, "resample: null pointer");
  CHECK_ARG(aligned(wav, 4) && aligned(sig, 4) && aligned(h, 16),
            "resample: misaligned pointer (wav, sig 4-byte; h 16-byte)");
  ResArgs a;
  a.wav = wav; a.h = h; a.sig = sig; a.Ls = Ls; a.L10 = (Ls * U + D - 1) / D;
  a.C = C; a.U = U; a.D = D; a.H = half_len(U, D); a.ntab = 2 * a.H + 1;
  int tile = kThreads;
  while (tile > 1 && span_cap(tile, U, D, a.H) > kSpanMax) tile >>= 1;
  a.tile = tile;
  const size_t lds = ((size_t)((a.ntab + 3) & ~3) + (size_t)span_cap(tile, U, D, a.H)) * sizeof(float);
  const int64_t tiles = (a.L10 + tile - 1) / tile;
  CHECK_ARG(tiles < ((int64_t)1 << 31), "resample: too many tiles");
  if (lds > 64 * 1024) {     /* a long table: above the default dynamic-LDS limit, inside the CU's 160 KiB */
    static thread_local int lds_dev = -1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
      (void)hipGetLastError();
      set_error("resample: no HIP device");
      return DANET_STOI_ERR_LAUNCH;
    }
    if (dev != lds_dev) {
      const size_t most = ((size_t)DANET_STOI_MAX_TABLE + kSpanMax) * sizeof(float);
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(stoi_resample_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("resample: cannot reserve %zu bytes of LDS: %s", most, hipGetErrorString(e));
        return DANET_STOI_ERR_LAUNCH;
      }
      lds_dev = dev;
    }
  }
  stoi_resample_kernel<<<dim3((unsigned)tiles, 2 * C + 1, B), kThreads, lds, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_STOI_OK;
}

/* ------------------------------------------------------------------------------------------- frames */
__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void stoi_frames_kernel(int C, int64_t L10, int nf, int nfp,
                                                               const float* __restrict__ sig,
                                                               const float* __restrict__ w, double* E, int32_t* mask,
                                                               int32_t* kidx, int32_t* Mout, double* Emax) {
  __shared__ float ws[kFrame];
  __shared__ double wmax[kWaves];
  __shared__ int wcnt[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = blockIdx.x, b = blockIdx.y;
  const float* x = sig + ((int64_t)b * (2 * C + 1) + i) * L10;
  const int64_t row = (int64_t)b * C + i;
  double* e = E + row * nfp;
  int32_t* mk = mask + row * nfp;
  int32_t* kk = kidx + row * nfp;
  ws[tid] = w[tid];
  __syncthreads();
  double mx = 0.0;
  for (int f = wave; f < nf; f += kWaves) {
    const float* xf = x + (int64_t)f * kHop;
    const double v0 = (double)ws[lane] * (double)xf[lane], v1 = (double)ws[lane + 64] * (double)xf[lane + 64];
    const double v2 = (double)ws[lane + 128] * (double)xf[lane + 128];
    const double v3 = (double)ws[lane + 192] * (double)xf[lane + 192];
    const double s = wave_sum((v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3));
    if (lane == 0) e[f] = s;
    mx = s > mx ? s : mx;
  }
  if (lane == 0) wmax[wave] = mx;
  __threadfence_block();
  __syncthreads();                                             /* the energies are visible to the workgroup */
  double emax = wmax[0];
  for (int v = 1; v < kWaves; ++v) emax = wmax[v] > emax ? wmax[v] : emax;
  const double thr = kDyn * emax;
  int run = 0;                                                 /* kept frames in front of this chunk */
  for (int f0 = 0; f0 < nf; f0 += kThreads) {
    const int f = f0 + tid;
    const bool keep = f < nf && e[f] > thr;
    const unsigned long long bal = __ballot(keep);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();                                           /* the counts of the chunk before are read */
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = run;
    for (int v = 0; v < kWaves; ++v) {
      if (v < wave) off += wcnt[v];
      run += wcnt[v];
    }
    if (f < nf) mk[f] = keep ? 1 : 0;
    if (keep) kk[off + below] = f;
  }
  for (int q = run + tid; q < nfp; q += kThreads) kk[q] = 0;
  if (nf == 0 && tid == 0) { e[0] = 0.0; mk[0] = 0; }
  if (tid == 0) { Mout[row] = run; Emax[row] = emax; }
}

extern "C" int danet_stoi_frames(void* stream, int B, int C, int64_t L10, const float* sig, const float* w,
                                 double* E, int32_t* mask, int32_t* kidx, int32_t* M, double* Emax) {
  CHECK_BATCH("frames");
  CHECK_ARG(len_ok(L10), "frames: L10 must be in [1, 2^31) (got %lld)", (long long)L10);
  CHECK_ARG(sig && w && E && mask && kidx && M && Emax, "frames: null pointer");
  CHECK_ARG(aligned(sig, 4) && aligned(w, 4) && aligned(mask, 4) && aligned(kidx, 4) && aligned(M, 4) &&
                aligned(E, 8) && aligned(Emax, 8),
            "frames: misaligned pointer (sig, w, mask, kidx, M 4-byte; E, Emax 8-byte)");
  const int nf = (int)frames_of(L10);
  stoi_frames_kernel<<<dim3(C, B), kThreads, 0, (hipStream_t)stream>>>(C, L10, nf, nf ? nf : 1, sig, w, E, mask,
                                                                       kidx, M, Emax);
  CHECK_LAUNCH();
  return DANET_STOI_OK;
}

/* -------------------------------------------------------------------------------------------- bands */
struct BandArgs {
  const float* sig;
  const float* w;
  const double2* tw;
  const int32_t* kidx;
  const int32_t* M;
  double* T;
  int64_t L10;
  int C, nf;
  int lo[kBands], hi[kBands];
};

__device__ __forceinline__ int bitrev8(int x) { return (int)(__brev((unsigned)x) >> 24); }
__device__ __forceinline__ double2 cmul(double2 a, double2 w) {
  return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kThreads) void stoi_bands_kernel(BandArgs a) {
  __shared__ double2 tw[kHalf];                                /* exp(-2 pi i k / 512) */
  __shared__ double2 zb[kWaves * kPitch];
  __shared__ float ws[kFrame];
  __shared__ int blo[kBands], bhi[kBands];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int C = a.C, nf = a.nf, s = blockIdx.y, row = blockIdx.z;
  const int b = row / C, i = row - b * C;
  const int q = (int)blockIdx.x * kWaves + wave;               /* the compacted frame of this wave */
  const int M = clampi(a.M[row], 0, nf);
  const bool valid = q < M;
  const int sr = s == 0 ? i : (s <= C ? C + s - 1 : 2 * C);    /* the row of sig behind signal s */
  const float* x = a.sig + ((int64_t)b * (2 * C + 1) + sr) * a.L10;
  tw[tid] = a.tw[tid];
  ws[tid] = a.w[tid];
  if (tid < kBands) { blo[tid] = a.lo[tid]; bhi[tid] = a.hi[tid]; }
  __syncthreads();

  /* z[j] = c[2j] w[2j] + i c[2j + 1] w[2j + 1] for j < 128, zero padding behind, bit-reversed */
  double2* z = zb + wave * kPitch;
  const int32_t* kk = a.kidx + (int64_t)row * nf;
  const bool hp = valid && q > 0, hn = valid && q < M - 1;
  const float* x0 = x + (int64_t)kHop * (valid ? clampi(kk[q], 0, nf - 1) : 0);
  const float* xp = x + (int64_t)kHop * (hp ? clampi(kk[q - 1], 0, nf - 1) : 0);
  const float* xn = x + (int64_t)kHop * (hn ? clampi(kk[q + 1], 0, nf - 1) : 0);
  for (int jj = 0; jj < 4; ++jj) {
    const int j = lane + 64 * jj;
    double2 v = make_double2(0.0, 0.0);
    if (valid && j < kHop) {
      double c[2];
      for (int t = 0; t < 2; ++t) {
        const int n = 2 * j + t;
        double cv = (double)ws[n] * (double)x0[n];
        if (n < kHop) {
          if (hp) cv += (double)ws[n + kHop] * (double)xp[n + kHop];
        } else {
          if (hn) cv += (double)ws[n - kHop] * (double)xn[n - kHop];
        }
        c[t] = (double)ws[n] * cv;
      }
      v = make_double2(c[0], c[1]);
    }
    z[bitrev8(j)] = v;
  }
  /* eight radix-2 stages, fused in pairs: 64 items a pass, one per lane */
  for (int st = 1; st <= 8; st += 2) {
    __syncthreads();
    const int half = 1 << (st - 1);
    const int grp = lane >> (st - 1), pos = lane & (half - 1);
    double2* p = z + (grp << (st + 1)) + pos;
    /* the 256-point twiddle exp(-2 pi i p / 256) is entry 2p of the table */
    const double2 w1 = tw[2 * (pos << (8 - st))];
    const double2 w2 = tw[2 * (pos << (8 - st - 1))];
    const double2 w3 = tw[2 * ((pos + half) << (8 - st - 1))];
    double2 v0 = p[0], v1 = p[half], v2 = p[2 * half], v3 = p[3 * half];
    v1 = cmul(v1, w1);
    v3 = cmul(v3, w1);
    const double2 b0 = cadd(v0, v1), b1 = csub(v0, v1);
    double2 b2 = cadd(v2, v3), b3 = csub(v2, v3);
    b2 = cmul(b2, w2);
    b3 = cmul(b3, w3);
    p[0] = cadd(b0, b2);
    p[2 * half] = csub(b0, b2);
    p[half] = cadd(b1, b3);
    p[3 * half] = csub(b1, b3);
  }
  __syncthreads();
  /* split: X[k] = E[k] + exp(-2 pi i k / 512) O[k]; item k owns slots k and 256 - k (k = 0: 0, 256 and 128) */
  for (int k = lane; k < kHalf / 2; k += 64) {
    if (k == 0) {
      const double2 z0 = z[0], zh = z[kHalf / 2];
      z[0] = make_double2(z0.x + z0.y, 0.0);
      z[kHalf] = make_double2(z0.x - z0.y, 0.0);
      z[kHalf / 2] = make_double2(zh.x, -zh.y);
      continue;
    }
    const double2 p = z[k], r = z[kHalf - k];
    const double2 wk = tw[k], wm = tw[kHalf - k];
    const double2 Ek = make_double2(0.5 * (p.x + r.x), 0.5 * (p.y - r.y));
    const double2 Ok = make_double2(0.5 * (p.y + r.y), 0.5 * (r.x - p.x));
    const double2 Em = make_double2(Ek.x, -Ek.y);
    const double2 Om = make_double2(Ok.x, -Ok.y);
    z[k] = cadd(Ek, cmul(Ok, wk));
    z[kHalf - k] = cadd(Em, cmul(Om, wm));
  }
  __syncthreads();
  if (lane < kBands && q < nf) {
    double sum = 0.0;
    if (valid)
      for (int k = blo[lane]; k < bhi[lane]; ++k) sum += z[k].x * z[k].x + z[k].y * z[k].y;
    a.T[((((int64_t)row * (C + 2) + s) * kBands) + lane) * nf + q] = __dsqrt_rn(sum);
  }
}

extern "C" int danet_stoi_bands(void* stream, int B, int C, int64_t L10, const float* sig, const float* w,
                                const double* tw, const int32_t* bands, const int32_t* kidx, const int32_t* M,
                                double* T) {
  CHECK_BATCH("bands");
  CHECK_ARG(len_ok(L10), "bands: L10 must be in [1, 2^31) (got %lld)", (long long)L10);
  CHECK_ARG(sig && w && tw && bands && kidx && M && T, "bands: null pointer");
  CHECK_ARG(aligned(sig, 4) && aligned(w, 4) && aligned(kidx, 4) && aligned(M, 4) && aligned(bands, 4) &&
                aligned(tw, 16) && aligned(T, 8),
            "bands: misaligned pointer (sig, w, bands, kidx, M 4-byte; tw 16-byte; T 8-byte)");
  BandArgs a;
  for (int b = 0; b < kBands; ++b) {
    a.lo[b] = bands[2 * b];
    a.hi[b] = bands[2 * b + 1];
    CHECK_ARG(a.lo[b] >= 0 && a.lo[b] <= a.hi[b] && a.hi[b] <= kHalf + 1,
              "bands: band %d must have 0 <= lo <= hi <= %d (got %d, %d)", b, kHalf + 1, a.lo[b], a.hi[b]);
  }
  const int nf = (int)frames_of(L10);
  if (nf == 0) return DANET_STOI_OK;
  a.sig = sig; a.w = w; a.tw = reinterpret_cast<const double2*>(tw); a.kidx = kidx; a.M = M; a.T = T;
  a.L10 = L10; a.C = C; a.nf = nf;
  stoi_bands_kernel<<<dim3((nf + kWaves - 1) / kWaves, C + 2, B * C), kThreads, 0, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_STOI_OK;
}

/* ----------------------------------------------------------------------------------------- segments */
/* the four waves' butterflies joined as (p0 + p1) + (p2 + p3); every thread gets the sum */
__device__ __forceinline__ double block_sum(double v, double* part) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

/* d of STOI of the 15 x 30 blocks at X and Y (row pitch `ld`) */
__device__ double seg_stoi(const double* __restrict__ X, const double* __restrict__ Y, int ld) {
  double acc = 0.0;
  for (int bd = 0; bd < kBands; ++bd) {
    const double* x = X + (int64_t)bd * ld;
    const double* y = Y + (int64_t)bd * ld;
    double sx = 0.0, sxx = 0.0, syy = 0.0;
    for (int m = 0; m < kSeg; ++m) {
      sx += x[m];
      sxx += x[m] * x[m];
      syy += y[m] * y[m];
    }
    if (!(syy > 0.0)) continue;
    const double alpha = __dsqrt_rn(sxx) / __dsqrt_rn(syy);
    double sy = 0.0;
    for (int m = 0; m < kSeg; ++m) sy += fmin(alpha * y[m], kClip * x[m]);
    const double mx = sx / kSeg, my = sy / kSeg;
    double nxx = 0.0, nyy = 0.0, nxy = 0.0;
    for (int m = 0; m < kSeg; ++m) {
      const double dx = x[m] - mx, dy = fmin(alpha * y[m], kClip * x[m]) - my;
      nxx += dx * dx;
      nyy += dy * dy;
      nxy += dx * dy;
    }
    const double den = __dsqrt_rn(nxx) * __dsqrt_rn(nyy);
    if (den > 0.0) acc += nxy / den;
  }
  return acc / kBands;
}

/* mean and norm (after the mean is taken off) of the 15 rows of a block */
__device__ __forceinline__ void row_stats(const double* __restrict__ A, int ld, double (&mu)[kBands],
                                          double (&nr)[kBands]) {
#pragma unroll
  for (int bd = 0; bd < kBands; ++bd) {
    const double* x = A + (int64_t)bd * ld;
    double s = 0.0, ss = 0.0;
    for (int m = 0; m < kSeg; ++m) s += x[m];
    s /= kSeg;
    for (int m = 0; m < kSeg; ++m) ss += (x[m] - s) * (x[m] - s);
    mu[bd] = s;
    nr[bd] = __dsqrt_rn(ss);
  }
}

/* d of ESTOI of the same blocks */
__device__ double seg_estoi(const double* __restrict__ X, const double* __restrict__ Y, int ld) {
  double mx[kBands], nx[kBands], my[kBands], ny[kBands];
  row_stats(X, ld, mx, nx);
  row_stats(Y, ld, my, ny);
  double acc = 0.0;
  for (int m = 0; m < kSeg; ++m) {
    double xc[kBands], yc[kBands], sx = 0.0, sy = 0.0;
#pragma unroll
    for (int bd = 0; bd < kBands; ++bd) {
      xc[bd] = nx[bd] > 0.0 ? (X[(int64_t)bd * ld + m] - mx[bd]) / nx[bd] : 0.0;
      yc[bd] = ny[bd] > 0.0 ? (Y[(int64_t)bd * ld + m] - my[bd]) / ny[bd] : 0.0;
      sx += xc[bd];
      sy += yc[bd];
    }
    sx /= kBands;
    sy /= kBands;
    double cxx = 0.0, cyy = 0.0, cxy = 0.0;
#pragma unroll
    for (int bd = 0; bd < kBands; ++bd) {
      const double dx = xc[bd] - sx, dy = yc[bd] - sy;
      cxx += dx * dx;
      cyy += dy * dy;
      cxy += dx * dy;
    }
    const double den = __dsqrt_rn(cxx) * __dsqrt_rn(cyy);
    if (den > 0.0) acc += cxy / den;
  }
  return acc / kSeg;
}

__global__ __launch_bounds__(kThreads) void stoi_segments_kernel(int C, int nf, int nfp, const double* __restrict__ T,
                                                                 const int32_t* __restrict__ Mv,
                                                                 double* __restrict__ d) {
  __shared__ double part[kWaves];
  const int tid = threadIdx.x, j = blockIdx.x, i = blockIdx.y, b = blockIdx.z;
  const int64_t row = (int64_t)b * C + i;
  const int M = clampi(Mv[row], 0, nf);
  const double* X = T + row * (C + 2) * kBands * nfp;
  const double* Y = X + (int64_t)(1 + j) * kBands * nfp;
  double s1 = 0.0, s2 = 0.0;
  for (int q = kSeg - 1 + tid; q < M; q += kThreads) {
    s1 += seg_stoi(X + (q - (kSeg - 1)), Y + (q - (kSeg - 1)), nfp);
    s2 += seg_estoi(X + (q - (kSeg - 1)), Y + (q - (kSeg - 1)), nfp);
  }
  s1 = block_sum(s1, part);
  s2 = block_sum(s2, part);
  if (tid == 0) {
    const double n = (double)(M - (kSeg - 1));
    double* out = d + (row * (C + 1) + j) * 2;
    out[0] = M >= kSeg ? s1 / n : 0.0;
    out[1] = M >= kSeg ? s2 / n : 0.0;
  }
}

extern "C" int danet_stoi_segments(void* stream, int B, int C, int nf, const double* T, const int32_t* M, double* d) {
  CHECK_BATCH("segments");
  CHECK_ARG(nf >= 0 && nf < (1 << 24), "segments: nf must be in [0, 2^24) (got %d)", nf);
  CHECK_ARG(T && M && d, "segments: null pointer");
  CHECK_ARG(aligned(T, 8) && aligned(d, 8) && aligned(M, 4), "segments: misaligned pointer (M 4-byte; T, d 8-byte)");
  stoi_segments_kernel<<<dim3(C + 1, C, B), kThreads, 0, (hipStream_t)stream>>>(C, nf, nf ? nf : 1, T, M, d);
  CHECK_LAUNCH();
  return DANET_STOI_OK;
}

/* ----------------------------------------------------------------------------------------- finalize */
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

__global__ __launch_bounds__(kThreads) void stoi_finalize_kernel(int B, int C, int nf, const double* __restrict__ d,
                                                                 const int32_t* __restrict__ Mv,
                                                                 const double* __restrict__ Emax, int b0, int B_all,
                                                                 double* per_utt, int32_t* perm_idx, int32_t* flags,
                                                                 double* __restrict__ mean4,
                                                                 int32_t* __restrict__ count) {
  __shared__ double part[kWaves];
  const int tid = threadIdx.x;
  for (int u = tid; u < B; u += kThreads) {
    const double* du = d + (int64_t)u * C * (C + 1) * 2;
    bool live[kMaxC];
    int n_live = 0, flag = 0;
    for (int i = 0; i < C; ++i) {
      live[i] = nf == 0 || Emax[(int64_t)u * C + i] > 0.0;
      n_live += live[i] ? 1 : 0;
      if (live[i] && clampi(Mv[(int64_t)u * C + i], 0, nf) < kSeg) flag = 1;
    }
    double o[4] = {0.0, 0.0, 0.0, 0.0};
    int best = 0;
    if (flag == 0 && n_live > 0) {
      int nperm = 1;
      for (int i = 2; i <= C; ++i) nperm *= i;
      double best_v = 0.0;
      int perm[kMaxC];
      for (int p = 0; p < nperm; ++p) {
        nth_perm(C, p, perm);
        double s = 0.0;
        for (int i = 0; i < C; ++i)
          if (live[i]) s += du[(i * (C + 1) + perm[i]) * 2];
        if (p == 0 || s > best_v) { best = p; best_v = s; }
      }
      nth_perm(C, best, perm);
      for (int i = 0; i < C; ++i)
        if (live[i]) {
          const double* pe = du + (i * (C + 1) + perm[i]) * 2;
          const double* pm = du + (i * (C + 1) + C) * 2;
          o[0] += pe[0];
          o[1] += pe[1];
          o[2] += pe[0] - pm[0];
          o[3] += pe[1] - pm[1];
        }
      for (int k = 0; k < 4; ++k) o[k] /= (double)n_live;
    }
    double* out = per_utt + 4 * (int64_t)(b0 + u);
    for (int k = 0; k < 4; ++k) out[k] = o[k];
    perm_idx[b0 + u] = best;
    flags[b0 + u] = flag | (n_live == 0 ? 2 : 0);
  }
  if (b0 + B != B_all) return;
  __threadfence_block();
  __syncthreads();                                             /* this call's rows are visible to the workgroup */
  double s[4] = {0.0, 0.0, 0.0, 0.0}, cnt = 0.0;
  for (int u = tid; u < B_all; u += kThreads)
    if (flags[u] == 0) {
      for (int k = 0; k < 4; ++k) s[k] += per_utt[4 * (int64_t)u + k];
      cnt += 1.0;
    }
  const double tn = block_sum(cnt, part);
  for (int k = 0; k < 4; ++k) {
    const double ts = block_sum(s[k], part);
    if (tid == 0) mean4[k] = tn > 0.0 ? ts / tn : 0.0;
  }
  if (tid == 0) *count = (int32_t)tn;
}

extern "C" int danet_stoi_finalize(void* stream, int B, int C, int nf, const double* d, const int32_t* M,
                                   const double* Emax, int b0, int B_all, double* per_utt, int32_t* perm_idx,
                                   int32_t* flags, double* mean4, int32_t* count) {
  CHECK_BATCH("finalize");
  CHECK_ARG(nf >= 0 && nf < (1 << 24), "finalize: nf must be in [0, 2^24) (got %d)", nf);
  CHECK_ARG(b0 >= 0 && B_all <= DANET_STOI_MAX_BATCH && (int64_t)b0 + B <= B_all,
            "finalize: need b0 >= 0 and b0 + B <= B_all <= %d (got b0 = %d, B = %d, B_all = %d)",
            DANET_STOI_MAX_BATCH, b0, B, B_all);
  CHECK_ARG(d && M && Emax && per_utt && perm_idx && flags && mean4 && count, "finalize: null pointer");
  CHECK_ARG(aligned(d, 8) && aligned(Emax, 8) && aligned(per_utt, 8) && aligned(mean4, 8) && aligned(M, 4) &&
                aligned(perm_idx, 4) && aligned(flags, 4) && aligned(count, 4),
            "finalize: misaligned pointer (M, perm_idx, flags, count 4-byte; all else 8-byte)");
  stoi_finalize_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(B, C, nf, d, M, Emax, b0, B_all, per_utt,
                                                                     perm_idx, flags, mean4, count);
  CHECK_LAUNCH();
  return DANET_STOI_OK;
}
