/*
 * libdanet_prep_hip.so (include/danet_prep_hip.h): STFT of a ragged batch of device-resident
 * waveforms, written straight into the zero-padded, optionally cropped batch.  gfx950.
 *
 * Geometry.  One workgroup of 256 threads owns `fpw` CONSECUTIVE frames of ONE utterance on the
 * output time axis (fpw = 16 / 8 / 4 / 2 for N <= 128 / 256 / 2048 / 4096); the grid is the flat
 * product n_utt * ceil(t_count / fpw), so no dimension carries a 65535 ceiling.
 *   1. the (fpw-1)*S + N samples its frames cover are staged in LDS ONCE (zero outside the
 *      utterance): a sample is fetched from global memory once per workgroup, not N/S times;
 *   2. the twiddle table exp(-2 pi i k / N) and 1/sum(window) come from the plan
 *      (danet_prep_stft_plan), nothing is recomputed per launch;
 *   3. a frame of N real samples is transformed as an N/2-point COMPLEX FFT of
 *      z[j] = x[2j] w[2j] + i x[2j+1] w[2j+1] (bit-reversed load, radix-2 butterflies fused in pairs
 *      so that two stages cost one LDS pass and one barrier) plus the split pass
 *      X[k] = E[k] + exp(-2 pi i k / N) O[k];
 *   4. the fpw x F results sit in LDS at pitch F, i.e. exactly as the output rows lie in memory when
 *      ld_out == F: the workgroup streams them out as one span of 16-byte stores (an 8-byte head or
 *      tail where the span does not start or end on 16 bytes; F is odd).  Padding frames are
 *      literal +0.0 written by the same stores -- no memset, every element written once.
 * A frame's arithmetic is the same instruction sequence whatever its slot in the workgroup and
 * whatever else the launch computes, so a cropped launch equals a slice of the full one bit for bit.
 * What bounds it: LDS passes ((log2(N/2)+1)/2 + 2 per frame) and the store stream; per workgroup
 * 4N + 8 fpw (N/2+1) + 4((fpw-1)S + N) bytes of LDS (12.4 KB at N = 256, S = 64).
 * No atomics, no host round trip, plain HIP C++.
 */
#include <hip/hip_runtime.h>

#include "danet_prep_hip.h"
#define DANET_EXT prep
#define DANET_EXT_UPPER PREP
#include "ext_core.h"

static const int kThreads = 256;

static int ilog2_exact(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return ((1 << l) == n) ? l : -1;
}

static bool valid_fft_size(int N) {
  if (N < 64 || N > 4096) return false;
  return ilog2_exact(N) >= 0;
}

/* frames of an Ls-sample waveform (scipy: boundary='zeros', padded=True); Ls >= N */
__host__ __device__ __forceinline__ int64_t frames_of(int64_t Ls, int N, int S) {
  const int64_t nadd = ((-Ls) % S + S) % S % N;      /* ext - N = Ls */
  return (Ls + nadd) / S + 1;
}

extern "C" int danet_prep_num_frames(int64_t Ls, int N, int S) {
  if (N <= 0 || S <= 0 || S > N || Ls < N) {
    set_error("num_frames: need 0 < S <= N <= Ls (Ls=%lld, N=%d, S=%d)", (long long)Ls, N, S);
    return DANET_PREP_ERR_ARG;
  }
  const int64_t T = frames_of(Ls, N, S);
  if (T > 0x7fffffff) {
    set_error("num_frames: frame count does not fit an int");
    return DANET_PREP_ERR_ARG;
  }
  return (int)T;
}

/* plan layout: float2 tw[N/2] | float scale | pad to 16 bytes */
extern "C" size_t danet_prep_workspace_bytes(int N) {
  if (!valid_fft_size(N)) {
    set_error("workspace_bytes: N must be a power of two in [64, 4096] (got %d)", N);
    return (size_t)-1;
  }
  return (size_t)N * 4 + 16;
}

__global__ __launch_bounds__(kThreads) void prep_plan_kernel(int N, const float* __restrict__ window,
                                                             float2* __restrict__ tw,
                                                             float* __restrict__ scale) {
  __shared__ double part[kThreads];
  for (int k = threadIdx.x; k < N / 2; k += kThreads) {
    float sn, cs;
    sincospif(-2.0f * (float)k / (float)N, &sn, &cs);
    tw[k] = make_float2(cs, sn);
  }
  /* sum(window) in float64 like scipy's win.sum() on the float32 window (fixed order) */
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += kThreads) s += (double)window[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *scale = (float)(1.0 / part[0]);
}

extern "C" int danet_prep_stft_plan(void* stream, int N, const float* window, void* plan_ws,
                                    size_t plan_bytes) {
  CHECK_ARG(valid_fft_size(N), "stft_plan: N must be a power of two in [64, 4096] (got %d)", N);
  CHECK_ARG(window != nullptr && plan_ws != nullptr, "stft_plan: null pointer");
  CHECK_ARG(((uintptr_t)window & 3) == 0 && ((uintptr_t)plan_ws & 15) == 0,
            "stft_plan: window must be 4-byte and plan_ws 16-byte aligned");
  CHECK_ARG(plan_bytes >= danet_prep_workspace_bytes(N), "stft_plan: workspace too small (%zu < %zu)",
            plan_bytes, danet_prep_workspace_bytes(N));
  float2* tw = (float2*)plan_ws;
  float* scale = (float*)((char*)plan_ws + (size_t)N * 4);
  prep_plan_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(N, window, tw, scale);
  CHECK_LAUNCH();
  return DANET_PREP_OK;
}

struct PrepArgs {
  const float* pool;
  int64_t pool_len;
  const danet_prep_utt_t* desc;
  const float* window;
  const float2* tw;
  const float* scale;
  float2* out;
  int64_t ld_out;
  int n_chunks;              /* ceil(t_count / fpw) */
  int t_begin, t_count;
  int N, logM, S, fpw;
};

__device__ __forceinline__ int bitrev(int x, int bits) { return (int)(__brev((unsigned)x) >> (32 - bits)); }

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

/* n complex elements src (LDS; ZERO: literal +0.0 instead) -> dst (global, 8-byte aligned): 16-byte
 * stores over the 16-byte aligned middle, an 8-byte store at a misaligned head / odd tail */
template <bool ZERO>
__device__ __forceinline__ void store_span(float2* __restrict__ dst, const float2* src, int n) {
  const int head = (int)(((uintptr_t)dst >> 3) & 1);
  const int npair = (n - head) >> 1;
  for (int p = threadIdx.x; p < npair; p += kThreads) {
    const int e = head + 2 * p;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!ZERO) {
      const float2 a = src[e], b = src[e + 1];
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
    *reinterpret_cast<f32x4*>(dst + e) = v;
  }
  if (threadIdx.x == kThreads - 1) {
    if (head) dst[0] = ZERO ? make_float2(0.f, 0.f) : src[0];
    if ((n - head) & 1) dst[n - 1] = ZERO ? make_float2(0.f, 0.f) : src[n - 1];
  }
}

__global__ __launch_bounds__(kThreads) void prep_stft_batch_kernel(PrepArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int N = a.N, M = N >> 1, P = M + 1, S = a.S, logM = a.logM, fpw = a.fpw;
  float2* tw = reinterpret_cast<float2*>(smem);           /* [M]       exp(-2 pi i k / N) */
  float2* zb = tw + M;                                    /* [fpw][P]  frames, then the output rows */
  float* stg = reinterpret_cast<float*>(zb + fpw * P);    /* [(fpw-1) S + N] staged samples */
  const int tid = threadIdx.x;
  const int u = (int)(blockIdx.x / (unsigned)a.n_chunks);
  const int c = (int)(blockIdx.x - (unsigned)u * (unsigned)a.n_chunks);
  const int r0 = c * fpw;                                 /* first output row of this workgroup */
  const int nrows = min(fpw, a.t_count - r0);

  /* the descriptor is clamped, never trusted */
  int64_t off = a.desc[u].offset, len = a.desc[u].length;
  const int pad_left = a.desc[u].pad_left;
  if (len < 0) len = 0;
  if (off < 0) { len += off; off = 0; }
  if (off > a.pool_len) off = a.pool_len;
  if (len > a.pool_len - off) len = a.pool_len - off;
  const int64_t Tu = len >= N ? frames_of(len, N, S) : 0;
  const int64_t tu0 = (int64_t)a.t_begin + r0 - (int64_t)pad_left;   /* own frame index of row r0 */
  const bool any = Tu > 0 && tu0 + nrows > 0 && tu0 < Tu;

  float2* dst = a.out + ((int64_t)u * a.t_count + r0) * a.ld_out;
  if (!any) {                                             /* (uniform) nothing but padding here */
    if (a.ld_out == P) {
      store_span<true>(dst, nullptr, nrows * P);
    } else {
      for (int f = 0; f < nrows; ++f) store_span<true>(dst + (int64_t)f * a.ld_out, nullptr, P);
    }
    return;
  }

  const float* xs = a.pool + off;
  const int64_t base = tu0 * S - M;                       /* sample index of stg[0] */
  const int nstg = (nrows - 1) * S + N;
  for (int i = tid; i < nstg; i += kThreads) {
    const int64_t pos = base + i;
    stg[i] = (pos >= 0 && pos < len) ? xs[pos] : 0.f;
  }
  for (int k = tid; k < M; k += kThreads) tw[k] = a.tw[k];
  const float scale = *a.scale;
  __syncthreads();

  /* z[j] = x[2j] w[2j] + i x[2j+1] w[2j+1], bit-reversed */
  for (int idx = tid; idx < nrows * M; idx += kThreads) {
    const int f = idx >> logM, j = idx & (M - 1);
    const int64_t tu = tu0 + f;
    if (tu < 0 || tu >= Tu) continue;
    const float* s = stg + f * S + 2 * j;
    zb[f * P + bitrev(j, logM)] = make_float2(s[0] * a.window[2 * j], s[1] * a.window[2 * j + 1]);
  }
  __syncthreads();

  int s = 1;
  if (logM & 1) {                                         /* odd stage count: one plain radix-2 stage */
    for (int idx = tid; idx < nrows * (M >> 1); idx += kThreads) {
      const int f = idx >> (logM - 1), i = idx & ((M >> 1) - 1);
      const int64_t tu = tu0 + f;
      if (tu < 0 || tu >= Tu) continue;
      float2* z = zb + f * P + 2 * i;
      const float2 p = z[0], q = z[1];
      z[0] = cadd(p, q);
      z[1] = csub(p, q);
    }
    __syncthreads();
    s = 2;
  }
  for (; s <= logM; s += 2) {                             /* stages s and s+1 in one pass */
    const int half = 1 << (s - 1);
    for (int idx = tid; idx < nrows * (M >> 2); idx += kThreads) {
      const int f = idx >> (logM - 2), q = idx & ((M >> 2) - 1);
      const int64_t tu = tu0 + f;
      if (tu < 0 || tu >= Tu) continue;
      const int grp = q >> (s - 1), pos = q & (half - 1);
      float2* z = zb + f * P + (grp << (s + 1)) + pos;
      /* the N/2-point twiddle exp(-2 pi i p / (N/2)) is entry 2p of the table */
      const float2 w1 = tw[2 * (pos << (logM - s))];
      const float2 w2 = tw[2 * (pos << (logM - s - 1))];
      const float2 w3 = tw[2 * ((pos + half) << (logM - s - 1))];
      float2 v0 = z[0], v1 = z[half], v2 = z[2 * half], v3 = z[3 * half];
      v1 = cmul(v1, w1);
      v3 = cmul(v3, w1);
      const float2 b0 = cadd(v0, v1), b1 = csub(v0, v1);
      float2 b2 = cadd(v2, v3), b3 = csub(v2, v3);
      b2 = cmul(b2, w2);
      b3 = cmul(b3, w3);
      z[0] = cadd(b0, b2);
      z[2 * half] = csub(b0, b2);
      z[half] = cadd(b1, b3);
      z[3 * half] = csub(b1, b3);
    }
    __syncthreads();
  }

  /* split: X[k] = E[k] + exp(-2 pi i k / N) O[k], E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2i;
   * item k owns slots k and M-k of its frame (k = 0: slots 0, M and the self-paired M/2), in place */
  const int H = M >> 1;
  for (int idx = tid; idx < nrows * H; idx += kThreads) {
    const int f = idx >> (logM - 1), k = idx & (H - 1);
    const int64_t tu = tu0 + f;
    float2* z = zb + f * P;
    if (tu < 0 || tu >= Tu) {
      const float2 zero = make_float2(0.f, 0.f);
      if (k == 0) { z[0] = zero; z[M] = zero; z[H] = zero; }
      else { z[k] = zero; z[M - k] = zero; }
      continue;
    }
    if (k == 0) {
      const float2 z0 = z[0], zh = z[H];
      z[0] = make_float2((z0.x + z0.y) * scale, 0.f);
      z[M] = make_float2((z0.x - z0.y) * scale, 0.f);
      z[H] = make_float2(zh.x * scale, -zh.y * scale);
      continue;
    }
    const float2 p = z[k], q = z[M - k];
    const float2 wk = tw[k], wm = tw[M - k];
    /* E = ((p.x + q.x)/2, (p.y - q.y)/2), O = ((p.y + q.y)/2, (q.x - p.x)/2); for M-k swap p and q */
    const float2 Ek = make_float2(0.5f * (p.x + q.x), 0.5f * (p.y - q.y));
    const float2 Ok = make_float2(0.5f * (p.y + q.y), 0.5f * (q.x - p.x));
    const float2 Em = make_float2(Ek.x, -Ek.y);
    const float2 Om = make_float2(Ok.x, -Ok.y);
    const float2 xk = cadd(Ek, cmul(Ok, wk));
    const float2 xm = cadd(Em, cmul(Om, wm));
    z[k] = make_float2(xk.x * scale, xk.y * scale);
    z[M - k] = make_float2(xm.x * scale, xm.y * scale);
  }
  __syncthreads();

  if (a.ld_out == P) {
    store_span<false>(dst, zb, nrows * P);
  } else {
    for (int f = 0; f < nrows; ++f) store_span<false>(dst + (int64_t)f * a.ld_out, zb + f * P, P);
  }
}

/* LDS of the largest launch: N = S = 4096, two frames per workgroup */
static const size_t kMaxLds = (size_t)4096 * 4 + (size_t)2 * 2049 * 8 + ((size_t)4096 + 4096) * 4;

static int frames_per_workgroup(int N) { return N <= 128 ? 16 : (N <= 256 ? 8 : (N <= 2048 ? 4 : 2)); }

extern "C" int danet_prep_stft_batch(void* stream, int n_utt, const float* pool, int64_t pool_len,
                                     const danet_prep_utt_t* desc, int T_out, int t_begin, int t_count, int N,
                                     int S, const float* window, const void* plan_ws, float* out_c64,
                                     int64_t ld_out) {
  CHECK_ARG(valid_fft_size(N), "stft_batch: N must be a power of two in [64, 4096] (got %d)", N);
  CHECK_ARG(S > 0 && S <= N, "stft_batch: stride must be in (0, N] (got %d)", S);
  CHECK_ARG(n_utt >= 1, "stft_batch: n_utt must be >= 1 (got %d)", n_utt);
  CHECK_ARG(pool && desc && window && plan_ws && out_c64, "stft_batch: null pointer");
  CHECK_ARG(pool_len >= 0, "stft_batch: pool_len must be >= 0");
  CHECK_ARG(T_out >= 1 && t_begin >= 0 && t_count >= 1 && (int64_t)t_begin + t_count <= T_out,
            "stft_batch: need 0 <= t_begin, 1 <= t_count, t_begin + t_count <= T_out (got %d, %d, %d)",
            t_begin, t_count, T_out);
  const int F = N / 2 + 1;
  CHECK_ARG(ld_out >= F, "stft_batch: ld_out must be >= F (%lld < %d)", (long long)ld_out, F);
  CHECK_ARG(ld_out < ((int64_t)1 << 40), "stft_batch: ld_out too large");
  CHECK_ARG(((uintptr_t)pool & 3) == 0 && ((uintptr_t)window & 3) == 0 && ((uintptr_t)desc & 7) == 0 &&
                ((uintptr_t)out_c64 & 7) == 0 && ((uintptr_t)plan_ws & 15) == 0,
            "stft_batch: misaligned pointer (pool, window 4-byte; desc, out 8-byte; plan_ws 16-byte)");
  const int fpw = frames_per_workgroup(N);
  const int64_t n_chunks = ((int64_t)t_count + fpw - 1) / fpw;
  CHECK_ARG(n_chunks * n_utt < ((int64_t)1 << 31), "stft_batch: n_utt * ceil(t_count / %d) must be < 2^31",
            fpw);
  PrepArgs a;
  a.pool = pool; a.pool_len = pool_len; a.desc = desc; a.window = window;
  a.tw = (const float2*)plan_ws;
  a.scale = (const float*)((const char*)plan_ws + (size_t)N * 4);
  a.out = (float2*)out_c64; a.ld_out = ld_out;
  a.n_chunks = (int)n_chunks; a.t_begin = t_begin; a.t_count = t_count;
  a.N = N; a.logM = ilog2_exact(N) - 1; a.S = S; a.fpw = fpw;
  const size_t lds = (size_t)N * 4 + (size_t)fpw * F * 8 + ((size_t)(fpw - 1) * S + N) * 4;
  if (lds > 64 * 1024) {     /* N >= 2048: above the default dynamic-LDS limit, inside the CU's 160 KiB */
    /* asked for ONCE per host thread and device, sized for the largest launch of the envelope */
    static thread_local int lds_dev = -1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
      (void)hipGetLastError();
      set_error("stft_batch: no HIP device");
      return DANET_PREP_ERR_LAUNCH;
    }
    if (dev != lds_dev) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(prep_stft_batch_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("stft_batch: cannot reserve %zu bytes of LDS: %s", kMaxLds, hipGetErrorString(e));
        return DANET_PREP_ERR_LAUNCH;
      }
      lds_dev = dev;
    }
  }
  prep_stft_batch_kernel<<<dim3((unsigned)(n_chunks * n_utt)), kThreads, lds, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_PREP_OK;
}
