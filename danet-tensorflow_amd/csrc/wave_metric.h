/*
 * The waveform SI-SDR core, once: what libdanet_metric_hip.so (csrc/metric), libdanet_neval_hip.so (csrc/neval)
 * and libdanet_wavloss_hip.so (csrc/wavloss) all compute.  Every result of the three is pinned bit for bit, so the
 * numerics live here and the libraries keep their entry points, their thin __global__ wrappers and what only they
 * add.  gfx950, wave64, workgroups of 256 threads.
 *
 * synth_tile.  One workgroup per (signal, tile of `hops` consecutive hops).  LDS: N/2 twiddles e^(+2 pi i j / N)
 * (sincospif, once per workgroup) and up to `max_frames` frames of N floats.
 *   split:  frame t, bin k < N/2:  Z[k] = E + i O with E = (X[k] + conj(X[N/2-k])) / N and
 *           O = (X[k] - conj(X[N/2-k])) / N * e^(+2 pi i k / N)  (the imaginary parts of X[0] and X[N/2]
 *           read as 0), stored at the bit-reversed index of k; a bin goes through the caller's load functor first;
 *   fft:    radix2_stages: log2(N/2) in-place radix-2 stages over all frames of the tile at once, one barrier per
 *           stage; z[m] = x[2m] + i x[2m+1], so the float view of the frame IS the real frame.  The sign of the
 *           transform is that of the twiddle table the caller filled (danet_wavloss_bwd fills e^(-2 pi i j / N));
 *   gather: thread -> output sample n of the tile; its frames in ascending t.
 * gram_pair.  One workgroup per (utterance, i <= j): nothing to share between workgroups, so no scratch and no
 * second launch; the waveforms of one batch sit in L2.
 * pit_search.  A thread per utterance: the sdr table, the live mask and the 24-permutation search in float64.  The
 * tables are indexed by constants alone (loops unrolled to kMaxC, a drawn column picked by comparison, a
 * permutation packed four bits a place), so they stay in registers: no scratch.
 */
#ifndef DANET_WAVE_METRIC_H
#define DANET_WAVE_METRIC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

static const int kThreads = 256;
static const int kWaves = kThreads / 64;
static const int kMaxC = 4;               /* MAXC of csrc/pit_common.h: DANET_{METRIC,NEVAL,WAVLOSS}_MAX_C */

/* ------------------------------------------------------------------------------------ synthesis */
static const int kLdsFloats = 16384;      /* 64 KiB: the twiddles (N floats) + the frames of a tile */
static const int kMaxFrames = 32;

struct Tiling {
  int max_frames;   /* frames a tile may hold in LDS                        */
  int hops;         /* hops (S output samples each) per tile, >= 1          */
  int tiles;        /* tiles per signal                                     */
};

static inline bool synth_shape_ok(int B, int C, int T, int N, int S) {
  return B >= 1 && C >= 1 && T >= 2 && N >= 64 && N <= 1024 && (N & (N - 1)) == 0 && 2 * S <= N && 8 * S >= N;
}

/* a tile of h hops starting at hop h0 covers the samples [h0 S, (h0 + h) S) and needs the frames
 * floor((h0 S - N/2) / S) + 1 .. floor(((h0 + h) S - 1 + N/2) / S): with N/2 = q S + r that is h + 2q - 1
 * frames when r = 0 and h + 2q + 1 otherwise (q <= 4, and q = 4 only with r = 0: at most h + 7) */
static inline Tiling tiling_of(int T, int N, int S) {
  Tiling g;
  g.max_frames = kLdsFloats / N - 1;
  if (g.max_frames > kMaxFrames) g.max_frames = kMaxFrames;
  const int q = (N / 2) / S, r = (N / 2) % S;
  const int extra = r == 0 ? 2 * q - 1 : 2 * q + 1;
  g.hops = g.max_frames - extra;            /* >= 15 - 7 */
  if (g.hops > T - 1) g.hops = T - 1;
  g.tiles = (T - 1 + g.hops - 1) / g.hops;
  return g;
}

static inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

static inline int log2_half(int N) {      /* log2(N/2), N a power of two */
  int l = 0;
  while ((2 << l) < N) ++l;
  return l;
}

/* what a synthesis launch of any number of rows per utterance shares */
struct SynthArgs {
  const float* window;
  float* wav;
  int C, T, N, S;
  int log2_half;     /* log2(N/2) */
  int hops, tiles, max_frames;
};

static inline SynthArgs synth_args(int C, int T, int N, int S, const float* window, float* wav) {
  const Tiling g = tiling_of(T, N, S);
  SynthArgs a;
  a.window = window; a.wav = wav;
  a.C = C; a.T = T; a.N = N; a.S = S;
  a.log2_half = log2_half(N);
  a.hops = g.hops; a.tiles = g.tiles; a.max_frames = g.max_frames;
  return a;
}

static inline size_t synth_lds_bytes(const SynthArgs& a) {     /* <= 64 KiB */
  return (size_t)(a.max_frames + 1) * a.N * sizeof(float);
}

__device__ __forceinline__ int floor_div(int a, int b) {      /* b > 0 */
  const int q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

/* in-place radix-2 transform (decimation in time) of the nfr frames of N floats at `frames`, whose N/2 complex
 * inputs sit at their bit-reversed indices; tw[j] = e^(+-2 pi i j / N), j < N/2, complete before the call */
__device__ __forceinline__ void radix2_stages(float* frames, const float2* tw, int nfr, int N, int log2_half) {
  const int half_m = N >> 2;
  for (int lh = 0; lh < log2_half; ++lh) {
    const int h = 1 << lh;
    for (int idx = threadIdx.x; idx < nfr * half_m; idx += kThreads) {
      const int f = idx >> (log2_half - 1), j = idx & (half_m - 1);
      const int pos = j & (h - 1);
      const int i0 = ((j >> lh) << (lh + 1)) + pos;
      float2* z = reinterpret_cast<float2*>(frames + f * N);
      const float2 w = tw[pos << (log2_half - lh)];             /* e^(+-2 pi i pos / 2h) */
      const float2 u = z[i0], v = z[i0 + h];
      const float vr = v.x * w.x - v.y * w.y, vi = v.x * w.y + v.y * w.x;
      z[i0] = make_float2(u.x + vr, u.y + vi);
      z[i0 + h] = make_float2(u.x - vr, u.y - vi);
    }
    __syncthreads();
  }
}

struct LoadBin {                                               /* a bin as it is stored */
  __device__ __forceinline__ float operator()(float x) const { return x; }
};

/* tile `tile` of the signal whose T frames of N/2 + 1 bins start at X -> the samples of that tile in row `sig` of
 * a.wav; both parts of every bin read go through load() */
template <class Load>
__device__ __forceinline__ void synth_tile(const SynthArgs& a, const float2* X, int sig, int tile, Load load) {
  extern __shared__ __align__(16) float lds[];                 /* (viewed as float2 below) */
  const int N = a.N, S = a.S, T = a.T, M = N >> 1, F = M + 1;
  float2* tw = reinterpret_cast<float2*>(lds);                 /* [M]              */
  float* frames = lds + N;                                     /* [max_frames][N]  */
  const int tid = threadIdx.x;
  const int Ls = (T - 1) * S;
  const int n0 = tile * a.hops * S;
  const int n1 = min(n0 + a.hops * S, Ls);
  const int t_first = max(floor_div(n0 - M, S) + 1, 0);
  const int t_last = min(floor_div(n1 - 1 + M, S), T - 1);
  const int nfr = min(t_last - t_first + 1, a.max_frames);     /* (the host sized the tile: never cut) */

  for (int j = tid; j < M; j += kThreads) {
    float s, c;
    sincospif((float)(2 * j) / (float)N, &s, &c);
    tw[j] = make_float2(c, s);
  }
  __syncthreads();

  /* split step: bins -> the N/2 complex inputs of the half-size transform, bit-reversed */
  const float inv_n = 1.0f / (float)N;
  const int shift = 32 - a.log2_half;
  for (int idx = tid; idx < nfr * M; idx += kThreads) {
    const int f = idx >> a.log2_half, k = idx & (M - 1);
    const float2* row = X + (int64_t)(t_first + f) * F;
    float2 p = row[k], q = row[M - k];
    p.x = load(p.x); p.y = load(p.y);
    q.x = load(q.x); q.y = load(q.y);
    if (k == 0) { p.y = 0.f; q.y = 0.f; }                      /* bins 0 and N/2: imaginary parts ignored */
    const float er = (p.x + q.x) * inv_n, ei = (p.y - q.y) * inv_n;
    const float dr = (p.x - q.x) * inv_n, di = (p.y + q.y) * inv_n;
    const float2 w = tw[k];
    const float o_r = dr * w.x - di * w.y, o_i = dr * w.y + di * w.x;
    const int rk = (int)(__brev((unsigned)k) >> shift);
    reinterpret_cast<float2*>(frames + f * N)[rk] = make_float2(er - o_i, ei + o_r);      /* E + i O */
  }
  __syncthreads();

  /* the inverse transform of every frame of the tile */
  radix2_stages(frames, tw, nfr, N, a.log2_half);

  /* gather: every output sample of the tile sums its frames, ascending t */
  float* y = a.wav + (int64_t)sig * Ls;
  for (int n = n0 + tid; n < n1; n += kThreads) {
    const int ta = max(floor_div(n - M, S) + 1, t_first);
    const int tb = min(floor_div(n + M, S), t_first + nfr - 1);
    float acc = 0.f, wsum = 0.f;
    for (int t = ta; t <= tb; ++t) {
      const int k = n - t * S + M;                              /* 0 <= k < N by the choice of ta, tb */
      const float w = a.window[k];
      acc += w * frames[(t - t_first) * N + k];
      wsum += w * w;
    }
    y[n] = wsum > 0.f ? acc / wsum : 0.f;
  }
}

/* ----------------------------------------------------------------------------------------- Gram */
/* every lane: the sum over the workgroup, (w0 + w1) + (w2 + w3) of the waves' butterflies */
__device__ __forceinline__ double block_sum_f64(double v, double* part) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();                                             /* (part may still be read from a call before) */
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

/* workgroup blockIdx.x = b * n_pairs + (pair i <= j of the upper triangle): G[b][i][j] = G[b][j][i] = the float64
 * inner product of rows i and j of wav [.][M][Ls]; part: kWaves doubles of LDS */
__device__ __forceinline__ void gram_pair(int M, int n_pairs, int64_t Ls, const float* wav, double* G,
                                          double* part) {
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)n_pairs);
  int p = (int)(blockIdx.x - (unsigned)b * (unsigned)n_pairs);
  int i = 0;
  while (p >= M - i) { p -= M - i; ++i; }                      /* row i of the upper triangle has M - i pairs */
  const int j = i + p;
  const float* x = wav + ((int64_t)b * M + i) * Ls;
  const float* y = wav + ((int64_t)b * M + j) * Ls;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t n = tid;
  for (; n + 3 * kThreads < Ls; n += 4 * kThreads) {
    const float x0 = x[n], x1 = x[n + kThreads], x2 = x[n + 2 * kThreads], x3 = x[n + 3 * kThreads];
    const float y0 = y[n], y1 = y[n + kThreads], y2 = y[n + 2 * kThreads], y3 = y[n + 3 * kThreads];
    a0 += (double)x0 * (double)y0;
    a1 += (double)x1 * (double)y1;
    a2 += (double)x2 * (double)y2;
    a3 += (double)x3 * (double)y3;
  }
  if (n < Ls) a0 += (double)x[n] * (double)y[n];
  if (n + kThreads < Ls) a1 += (double)x[n + kThreads] * (double)y[n + kThreads];
  if (n + 2 * kThreads < Ls) a2 += (double)x[n + 2 * kThreads] * (double)y[n + 2 * kThreads];
  const double r = block_sum_f64((a0 + a1) + (a2 + a3), part);
  if (tid == 0) {
    double* g = G + (int64_t)b * M * M;
    g[i * M + j] = r;
    g[j * M + i] = r;
  }
}

/* ------------------------------------------------------------------------------------- finalize */
/* sdr(i, j) from a = <s_i, s_i>, b = <y_j, y_j>, c = <s_i, y_j>, clamped to +-100 dB; *clamped (if asked for): the
 * value is one of the rule's clamps (its gradient is 0) */
__device__ __forceinline__ double sdr_db(double a, double b, double c, bool* clamped = nullptr) {
  const double t = c * c / a, r = b - t;
  if (clamped) *clamped = true;
  if (!(t > 0.0)) return -100.0;
  if (!(r > 0.0)) return 100.0;
  const double d = 10.0 * log10(t / r);
  if (clamped) *clamped = !(d > -100.0 && d < 100.0);
  return d < -100.0 ? -100.0 : (d > 100.0 ? 100.0 : d);
}

/* the p-th permutation of range(C) in itertools.permutations order (csrc/pit_common.h), four bits per position
 * (position i in bits 4i..4i+3); the values still to be placed are kept packed in the same way */
__device__ __forceinline__ unsigned nth_perm(int C, int p) {
  unsigned avail = 0x3210u, out = 0u;
  int fact = 1;
  for (int i = 2; i < C; ++i) fact *= i;
  int n = C;
  for (int i = 0; i < C; ++i) {
    const int q = p / fact;
    p -= q * fact;
    out |= ((avail >> (4 * q)) & 15u) << (4 * i);
    const unsigned low = avail & ((1u << (4 * q)) - 1u);          /* drop nibble q */
    avail = low | ((avail >> (4 * (q + 1))) << (4 * q));
    --n;
    if (n > 1) fact /= n;
  }
  return out;
}

__device__ __forceinline__ int perm_at(unsigned perm, int i) { return (int)((perm >> (4 * i)) & 15u); }

__device__ __forceinline__ double pick4(const double (&r)[kMaxC], int j) {
  return j == 0 ? r[0] : (j == 1 ? r[1] : (j == 2 ? r[2] : r[3]));
}

struct PitSearch {
  double sdr[kMaxC][kMaxC];   /* sdr[i][j]: reference i against estimate j; 0 where i is not live */
  double base[kMaxC];         /* the caller's baseline of reference i; 0 where i is not live      */
  bool live[kMaxC];           /* reference i has energy (and i < C)                               */
  int n_live;
  int best;                   /* the first permutation of the largest sum; 0 when n_live == 0     */
  double best_v;              /* its sum over the live references                                 */
};

struct NoBase {
  __device__ __forceinline__ double operator()(int, double) const { return 0.0; }
};

/* one utterance: g its Gram matrix of row length M, references in rows 0..C-1, estimates in rows C..2C-1;
 * base(i, <s_i, s_i>): the baseline of a live reference, taken while its row of the table is made.  Sums run over
 * i ascending and over live references only; a later permutation wins only when strictly greater. */
template <class Base>
__device__ __forceinline__ void pit_search(const double* g, int M, int C, PitSearch& s, Base base) {
  int nperm = 1;
  for (int i = 2; i <= C; ++i) nperm *= i;
  s.n_live = 0;
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) {
    s.live[i] = false;
    s.base[i] = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxC; ++j) s.sdr[i][j] = 0.0;
    if (i < C) {
      const double a = g[i * M + i];
      s.live[i] = a != 0.0;
      if (s.live[i]) {
        ++s.n_live;
#pragma unroll
        for (int j = 0; j < kMaxC; ++j)
          if (j < C) s.sdr[i][j] = sdr_db(a, g[(C + j) * M + (C + j)], g[i * M + (C + j)]);
        s.base[i] = base(i, a);
      }
    }
  }
  s.best = 0;
  s.best_v = 0.0;
  if (s.n_live == 0) return;
  for (int p = 0; p < nperm; ++p) {
    const unsigned perm = nth_perm(C, p);
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < kMaxC; ++i)
      if (s.live[i]) v += pick4(s.sdr[i], perm_at(perm, i));
    if (p == 0 || v > s.best_v) { s.best = p; s.best_v = v; }
  }
}

/* sum over the live references, i ascending, of sdr(i, best(i)) - base(i) */
__device__ __forceinline__ double pit_improvement(const PitSearch& s, int C) {
  const unsigned perm = nth_perm(C, s.best);
  double imp = 0.0;
#pragma unroll
  for (int i = 0; i < kMaxC; ++i)
    if (s.live[i]) imp += pick4(s.sdr[i], perm_at(perm, i)) - s.base[i];
  return imp;
}

#endif
