/*
 * libdanet_level_hip.so (include/danet_level_hip.h): per utterance of a ragged pool and per threshold, the
 * number of samples the P.56 activity detector calls active.  gfx950, wave64.
 *
 * The two-stage envelope p[n] = g p[n-1] + k |x[n]|, q[n] = g q[n-1] + k p[n] is a serial recurrence over a
 * whole file, and the hangover couples a sample to the last I samples before it.  Both are cut into tiles of
 * kTile = 1024 samples, one THREAD per (row, tile) -- a lane-serial run: a lane's 200-odd operations per
 * sample (two float64 fma, then a compare, two selects, a subtract, a compare and an add for each of 16
 * thresholds, all in registers) outweigh its one 4-byte load by far, so the loads are plain dword loads at
 * any offset residue (a lane's tile is 4 KiB of its own; the 64 lines of a wave stay in the vector L1 for
 * the 32 samples each serves), and a pool of hundreds of millions of samples is hundreds of thousands of
 * independent lanes.  Four launches:
 *   level_state_kernel    (row, tile) -> ws.state: the tile's end state (p, q) from a zero start
 *   level_carry_kernel    row         -> ws.state, in place: the state ENTERING every tile, in tile order
 *   level_count_kernel    (row, tile) -> ws.rec: the recurrence again from the carried state; per threshold
 *                                        the count with no hangover coming in, first and last index at or above
 *   level_rows_kernel     (row, thr)  -> counts: the tiles in order, adding what the hangover of earlier
 *                                        tiles covers in front of a tile's first own hit
 * Stream order is the only synchronisation; every word of ws that is read was written by the launch before;
 * there is no read-modify-write on memory.  Plain vector stores only.
 *
 * hipcc 7.x, -O3, gfx950: level_count_kernel 127 VGPRs (4 waves per SIMD), level_state_kernel 32, no scratch in any of the four
 * (checked with -Rpass-analysis=kernel-resource-usage; tools/bench_level.py has the timings).
 */
#include <hip/hip_runtime.h>

#include "danet_level_hip.h"
#define DANET_EXT level
#define DANET_EXT_UPPER LEVEL
#include "ext_core.h"
#include "ragged_rows.h"

static const int kThreads = 256;
static const int kThr = DANET_LEVEL_THRESHOLDS;
static const int kTile = DANET_LEVEL_TILE;
static const int kTileLog2 = 10;
static_assert((1 << kTileLog2) == kTile, "G = g^kTile is formed by kTileLog2 squarings");
static const int64_t kMaxLen = (int64_t)1 << 31;
static const int64_t kMaxHang = (int64_t)1 << 40;
static const int kNoHit = -(1 << 30);      /* `last` of a threshold nothing has reached yet */

/* per tile: the state (2 doubles), then count / first / last of every threshold (3 x 16 int32) */
static const size_t kStateBytes = 2 * sizeof(double);
static const size_t kRecInts = 3 * kThr;

static int64_t tiles_of(int64_t max_len) {
  const int64_t t = (max_len + kTile - 1) / kTile;
  return t < 1 ? 1 : t;
}

extern "C" size_t danet_level_workspace_bytes(int n_utt, int64_t max_len) {
  if (n_utt < 1 || max_len < 0 || max_len > kMaxLen || (int64_t)n_utt * tiles_of(max_len) >= ((int64_t)1 << 31)) {
    set_error("workspace_bytes: need n_utt >= 1, 0 <= max_len <= 2^31 and n_utt * tiles per row < 2^31 "
              "(got %d, %lld)", n_utt, (long long)max_len);
    return (size_t)-1;
  }
  return (size_t)n_utt * (size_t)tiles_of(max_len) * (kStateBytes + kRecInts * sizeof(int));
}

struct LevelArgs : RowTable {
  int n_utt;
  int tiles;             /* tiles of a max_len row, >= 1 */
  double g, k;           /* k = 1 - g                    */
  double G, K;           /* g^kTile, k kTile g^kTile     */
  int64_t hang;
  const double* thr;     /* [n_utt][kThr]                */
  int64_t* counts;       /* [n_utt][kThr]                */
  double2* state;        /* [n_utt][tiles]               */
  int* rec;              /* [n_utt][tiles][3][kThr]      */
};

/* thread -> (row u, tile t, its samples x[0..m)); false: no such tile in this row */
__device__ __forceinline__ bool tile_of_thread(const LevelArgs& a, int& u, int& t, const float*& x, int& m) {
  const int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (id >= (int64_t)a.n_utt * a.tiles) return false;
  u = (int)(id / a.tiles);
  t = (int)(id - (int64_t)u * a.tiles);
  int64_t off, len;
  clamp_row(a, u, off, len);
  const int64_t start = (int64_t)t * kTile;
  if (start >= len) return false;
  m = (int)min((int64_t)kTile, len - start);
  x = a.pool + off + start;
  return true;
}

__global__ __launch_bounds__(kThreads) void level_state_kernel(LevelArgs a) {
  int u, t, m;
  const float* x;
  if (!tile_of_thread(a, u, t, x, m)) return;
  double p = 0.0, q = 0.0;
#pragma unroll 8
  for (int i = 0; i < m; ++i) {
    p = fma(a.g, p, a.k * fabs((double)x[i]));
    q = fma(a.g, q, a.k * p);
  }
  a.state[(int64_t)u * a.tiles + t] = make_double2(p, q);
}

__global__ __launch_bounds__(kThreads) void level_carry_kernel(LevelArgs a) {
  const int u = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
  if (u >= a.n_utt) return;
  int64_t off, len;
  clamp_row(a, u, off, len);
  const int nt = (int)((len + kTile - 1) / kTile);      /* the tiles the first launch wrote */
  double2* st = a.state + (int64_t)u * a.tiles;
  double p = 0.0, q = 0.0;
  for (int t = 0; t < nt; ++t) {
    const double2 loc = st[t];            /* (only a row's last tile is short, and its end state enters nothing) */
    st[t] = make_double2(p, q);
    q = loc.y + (a.G * q + a.K * p);
    p = loc.x + a.G * p;
  }
}

__global__ __launch_bounds__(kThreads) void level_count_kernel(LevelArgs a) {
  int u, t, m;
  const float* x;
  if (!tile_of_thread(a, u, t, x, m)) return;
  const int64_t tile = (int64_t)u * a.tiles + t;
  const double2 in = a.state[tile];
  double p = in.x, q = in.y;
  const int hang = (int)min(a.hang, (int64_t)kTile);      /* inside a tile no distance exceeds kTile - 1 */
  double c[kThr];
  int cnt[kThr], first[kThr], last[kThr];
#pragma unroll
  for (int j = 0; j < kThr; ++j) {
    c[j] = a.thr[(int64_t)u * kThr + j];
    cnt[j] = 0;
    first[j] = m;
    last[j] = kNoHit;
  }
#pragma unroll 2
  for (int i = 0; i < m; ++i) {
    p = fma(a.g, p, a.k * fabs((double)x[i]));
    q = fma(a.g, q, a.k * p);
#pragma unroll
    for (int j = 0; j < kThr; ++j) {
      const bool hit = q >= c[j];
      last[j] = hit ? i : last[j];
      first[j] = min(first[j], hit ? i : m);
      cnt[j] += (i - last[j] <= hang) ? 1 : 0;
    }
  }
  int4* out = reinterpret_cast<int4*>(a.rec + tile * (int64_t)kRecInts);      /* 192-byte records: 16-byte aligned */
#pragma unroll
  for (int j = 0; j < kThr; j += 4) {
    out[j / 4] = make_int4(cnt[j], cnt[j + 1], cnt[j + 2], cnt[j + 3]);
    out[kThr / 4 + j / 4] = make_int4(first[j], first[j + 1], first[j + 2], first[j + 3]);
    out[2 * (kThr / 4) + j / 4] = make_int4(max(last[j], -1), max(last[j + 1], -1), max(last[j + 2], -1),
                                            max(last[j + 3], -1));
  }
}

__global__ __launch_bounds__(kThreads) void level_rows_kernel(LevelArgs a) {
  const int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (id >= (int64_t)a.n_utt * kThr) return;
  const int u = (int)(id / kThr), j = (int)(id % kThr);
  int64_t off, len;
  clamp_row(a, u, off, len);
  const int nt = (int)((len + kTile - 1) / kTile);      /* the tiles the third launch wrote */
  const int* rec = a.rec + (int64_t)u * a.tiles * (int64_t)kRecInts + j;
  int64_t total = 0, prev_last = -a.hang - 1;           /* nothing before the row: its cover ends at -1 */
  for (int t = 0; t < nt; ++t, rec += kRecInts) {
    const int64_t start = (int64_t)t * kTile;
    const int cnt = rec[0], first = rec[kThr], last = rec[2 * kThr];
    const int64_t covered = min(prev_last + a.hang + 1, start + first) - start;
    total += cnt + max(covered, (int64_t)0);
    if (last >= 0) prev_last = start + last;
  }
  a.counts[id] = total;
}

extern "C" int danet_level_activity(void* stream, int n_utt, const float* pool, int64_t pool_len,
                                    const int64_t* offsets, const int64_t* lengths, int64_t max_len, double g,
                                    int64_t hang, const double* thr, int64_t* counts, void* ws, size_t ws_bytes) {
  CHECK_ARG(n_utt >= 1, "activity: n_utt must be >= 1 (got %d)", n_utt);
  CHECK_ARG(pool_len >= 0, "activity: pool_len must be >= 0");
  CHECK_ARG(max_len >= 0 && max_len <= kMaxLen, "activity: max_len must be in [0, 2^31] (got %lld)",
            (long long)max_len);
  CHECK_ARG(g > 0.0 && g < 1.0, "activity: g must be inside (0, 1) (got %g)", g);      /* (a NaN fails both) */
  CHECK_ARG(hang >= 0 && hang <= kMaxHang, "activity: hang must be in [0, 2^40] (got %lld)", (long long)hang);
  CHECK_ARG(pool && offsets && lengths && thr && counts && ws, "activity: null pointer");
  CHECK_ARG(((uintptr_t)pool & 3) == 0 && ((uintptr_t)offsets & 7) == 0 && ((uintptr_t)lengths & 7) == 0 &&
                ((uintptr_t)thr & 7) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)ws & 15) == 0,
            "activity: misaligned pointer (pool 4-byte; offsets, lengths, thr, counts 8-byte; ws 16-byte)");
  const int64_t tiles = tiles_of(max_len);
  CHECK_ARG((int64_t)n_utt * tiles < ((int64_t)1 << 31), "activity: n_utt * tiles per row must be < 2^31");
  const size_t need = danet_level_workspace_bytes(n_utt, max_len);
  CHECK_ARG(ws_bytes >= need, "activity: workspace too small (%zu < %zu)", ws_bytes, need);
  LevelArgs a;
  a.pool = pool; a.pool_len = pool_len; a.offsets = offsets; a.lengths = lengths; a.max_len = max_len;
  a.n_utt = n_utt; a.tiles = (int)tiles; a.g = g; a.k = 1.0 - g; a.hang = hang; a.thr = thr; a.counts = counts;
  double G = g;
  for (int s = 0; s < kTileLog2; ++s) G *= G;
  a.G = G;
  a.K = a.k * (double)kTile * G;
  /* the states first (16-byte records), the 192-byte int32 records behind them: both 16-byte aligned, as ws is */
  a.state = (double2*)ws;
  a.rec = (int*)((char*)ws + (size_t)n_utt * (size_t)tiles * kStateBytes);
  const unsigned per_tile = (unsigned)(((int64_t)n_utt * tiles + kThreads - 1) / kThreads);
  const hipStream_t s = (hipStream_t)stream;
  level_state_kernel<<<dim3(per_tile), kThreads, 0, s>>>(a);
  CHECK_LAUNCH();
  level_carry_kernel<<<dim3((unsigned)((n_utt + kThreads - 1) / kThreads)), kThreads, 0, s>>>(a);
  CHECK_LAUNCH();
  level_count_kernel<<<dim3(per_tile), kThreads, 0, s>>>(a);
  CHECK_LAUNCH();
  level_rows_kernel<<<dim3((unsigned)(((int64_t)n_utt * kThr + kThreads - 1) / kThreads)), kThreads, 0, s>>>(a);
  CHECK_LAUNCH();
  return DANET_LEVEL_OK;
}
