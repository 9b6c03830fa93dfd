/*
 * libdanet_speed_hip.so (include/danet_speed_hip.h): every utterance of a ragged batch resampled by its
 * own factor p / 512 through a 32-tap polyphase filter whose table is an input.  gfx950, wave64.
 *
 * One persistent launch: min(compute units, an upper bound of the tiles) workgroups of 512 threads.  A
 * workgroup that has work copies the 64 KB table into LDS once, at a row pitch of 36 floats (144 bytes,
 * still 16-byte aligned: the bank of a 16-byte read is (address / 4) mod 64 and 36 * phi mod 64 takes 16
 * values four banks apart, so lanes at different phases spread over the whole bank row where the dense
 * pitch of 32 would leave them two slots; lanes at the SAME phase, p = 512, read one address, a
 * broadcast).  It then walks the descriptor rows in order with a running tile count -- every workgroup
 * reads every row, 40 bytes of uniform loads each -- and takes the tiles whose running index is its own
 * modulo the grid: no list is built, no atomic is used, the split is a pure function of the table.
 *
 * A tile is 1024 consecutive outputs of one utterance.  Their inputs are the span
 * [(n0 * p) div Q - 15, ((n1 - 1) * p) div Q + 16], at most 1311 floats; it is staged in LDS starting at
 * the 16-byte aligned address at or below its first sample: whole vectors inside the utterance as 16-byte
 * loads, the vectors across its ends sample by sample, everything outside it as zeros.  Thread t then
 * computes outputs n0 + t and n0 + t + 512: neighbouring lanes read neighbouring staged samples and
 * store neighbouring outputs.  Each output is one chain of 32 fused multiply-adds, j ascending, from +0.
 */
#include <hip/hip_runtime.h>

#include "danet_speed_hip.h"
#define DANET_EXT speed
#define DANET_EXT_UPPER SPEED
#include "ext_core.h"
#include "ragged_rows.h"

static const int kQ = DANET_SPEED_PHASES;
static const int kQShift = 9;
static const int kTaps = DANET_SPEED_TAPS;
static const int kZ = kTaps / 2;
static const int kThreads = 512;
static const int kTile = 1024;                /* outputs per tile: two per thread */
static const int kPitch = kTaps + 4;          /* floats per table row in LDS      */
/* floats of a staged span: 1023 * 640 / 512 rounded up + 32 taps, + 3 in front (alignment) and up to the
 * next multiple of 4 behind */
static const int kSpan = 1320;
static const int64_t kMaxLen = kMaxSpan;      /* 2^40: what cut_span cuts to */

static_assert((1 << kQShift) == kQ, "Q is 2^kQShift");
static_assert(((kTile - 1) * DANET_SPEED_P_MAX + kQ - 1) / kQ + kTaps + 3 + 3 <= kSpan, "staged span");
static_assert(kTile == 2 * kThreads && kQ * kTaps / 4 == 8 * kThreads, "tile and table copy geometry");

extern "C" int64_t danet_speed_out_len(int64_t L, int p) {
  if (L < 1 || L > kMaxLen || p < DANET_SPEED_P_MIN || p > DANET_SPEED_P_MAX) {
    set_error("out_len: need 1 <= L <= 2^40 and %d <= p <= %d (got %lld, %d)", DANET_SPEED_P_MIN,
              DANET_SPEED_P_MAX, (long long)L, p);
    return -1;
  }
  return (L - 1) * kQ / p + 1;
}

struct SpeedArgs {
  const float* src;
  int64_t src_len;
  const danet_speed_utt_t* desc;
  const float* table;
  float* dst;
  int64_t dst_len;
  int n_utt;
};

/* a row as the kernel uses it: sample i of the utterance is src[so + i] for lo <= i < hi and zero
 * elsewhere; output n is written to dst[dof + n] for nlo <= n < nhi */
struct Row {
  int64_t so, lo, hi, dof, nlo, nhi;
  int p;
};

__device__ __forceinline__ Row load_row(const SpeedArgs& a, int u) {
  const danet_speed_utt_t d = a.desc[u];
  Row r;
  r.so = d.src_offset;
  r.dof = d.dst_offset;
  cut_span(d.src_offset, d.src_length, a.src_len, r.lo, r.hi);
  cut_span(d.dst_offset, d.dst_length, a.dst_len, r.nlo, r.nhi);
  r.p = d.p < DANET_SPEED_P_MIN ? DANET_SPEED_P_MIN : (d.p > DANET_SPEED_P_MAX ? DANET_SPEED_P_MAX : d.p);
  return r;
}

__global__ __launch_bounds__(kThreads) void speed_resample_kernel(SpeedArgs a) {
  __shared__ __attribute__((aligned(16))) float tab[kQ * kPitch];
  __shared__ __attribute__((aligned(16))) float xs[kSpan];
  const int tid = threadIdx.x;
  const int64_t G = gridDim.x, b = blockIdx.x;
  bool have_table = false;
  int64_t g0 = 0;                                     /* tiles of the rows in front of row u */
  for (int u = 0; u < a.n_utt; ++u) {
    const Row r = load_row(a, u);
    const int64_t nt = (r.nhi + kTile - 1) / kTile;   /* outputs below nlo are computed and not stored */
    for (int64_t t = (b + G - g0 % G) % G; t < nt; t += G) {
      if (!have_table) {                              /* (uniform) once per workgroup */
        const f32x4* tv = reinterpret_cast<const f32x4*>(a.table);
        for (int q = tid; q < kQ * kTaps / 4; q += kThreads)
          *reinterpret_cast<f32x4*>(tab + (q >> 3) * kPitch + (q & 7) * 4) = tv[q];
        have_table = true;
      }
      const int64_t n0 = t * kTile;
      const int64_t n1 = n0 + kTile < r.nhi ? n0 + kTile : r.nhi;
      const int64_t first = ((n0 * r.p) >> kQShift) - (kZ - 1);          /* first sample of the span */
      const int64_t last = (((n1 - 1) * r.p) >> kQShift) + kZ;           /* its last                 */
      /* xs[0] is sample `start`: the 16-byte aligned address at or below sample `first` */
      const int64_t start = first - (int64_t)((((uintptr_t)a.src >> 2) + (uint64_t)r.so + (uint64_t)first) & 3);
      const int nvec = (int)((last - start) / 4 + 1);                    /* <= kSpan / 4 */
      __syncthreads();                                                   /* the tile before is read */
      for (int v = tid; v < nvec; v += kThreads) {
        const int64_t i = start + 4 * (int64_t)v;
        f32x4 x;
        if (i >= r.lo && i + 4 <= r.hi) {
          x = *reinterpret_cast<const f32x4*>(a.src + r.so + i);
        } else {
          for (int k = 0; k < 4; ++k) x[k] = (i + k >= r.lo && i + k < r.hi) ? a.src[r.so + i + k] : 0.0f;
        }
        *reinterpret_cast<f32x4*>(xs + 4 * v) = x;
      }
      __syncthreads();
      for (int k = 0; k < kTile / kThreads; ++k) {
        const int64_t n = n0 + tid + k * kThreads;
        if (n >= n1) break;
        const int64_t np = n * r.p;
        const float* w = tab + (int)(np & (kQ - 1)) * kPitch;
        const float* x = xs + (int)((np >> kQShift) - (kZ - 1) - start);
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < kTaps; j += 4) {
          const f32x4 c = *reinterpret_cast<const f32x4*>(w + j);
          acc = __builtin_fmaf(c[0], x[j], acc);
          acc = __builtin_fmaf(c[1], x[j + 1], acc);
          acc = __builtin_fmaf(c[2], x[j + 2], acc);
          acc = __builtin_fmaf(c[3], x[j + 3], acc);
        }
        if (n >= r.nlo) a.dst[r.dof + n] = acc;
      }
    }
    g0 += nt;
  }
}

/* compute units of the current device, asked once per device and thread */
static int compute_units(void) {
  static thread_local int cached_dev = -1, cached_cus = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev != cached_dev) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cached_dev = dev;
    cached_cus = cus;
  }
  return cached_cus;
}

extern "C" int danet_speed_resample(void* stream, int n_utt, const float* src_pool, int64_t src_len,
                                    const danet_speed_utt_t* desc, const float* table, float* dst,
                                    int64_t dst_len) {
  CHECK_ARG(n_utt >= 1, "resample: n_utt must be >= 1 (got %d)", n_utt);
  CHECK_ARG(src_pool && desc && table && dst, "resample: null pointer");
  CHECK_ARG(src_len >= 0 && src_len <= kMaxLen && dst_len >= 0 && dst_len <= kMaxLen,
            "resample: src_len and dst_len must be in [0, 2^40] (got %lld, %lld)", (long long)src_len,
            (long long)dst_len);
  CHECK_ARG(((uintptr_t)src_pool & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)desc & 7) == 0 &&
                ((uintptr_t)table & 15) == 0,
            "resample: misaligned pointer (src_pool, dst 4-byte; desc 8-byte; table 16-byte)");
  const int cus = compute_units();
  if (cus < 1) {
    set_error("resample: no device (%s:%d)", __FILE__, __LINE__);
    return DANET_SPEED_ERR_LAUNCH;
  }
  /* no row has more than ceil(its span inside dst / 1024) tiles: with disjoint spans this bounds the sum */
  const int64_t bound = dst_len / kTile + n_utt;
  SpeedArgs a;
  a.src = src_pool; a.src_len = src_len; a.desc = desc; a.table = table; a.dst = dst; a.dst_len = dst_len;
  a.n_utt = n_utt;
  speed_resample_kernel<<<dim3((unsigned)(bound < cus ? bound : cus)), kThreads, 0, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_SPEED_OK;
}
