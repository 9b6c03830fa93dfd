/*
 * libdanet_phase_hip.so (include/danet_phase_hip.h): MISI phase refinement of the separated spectra in three
 * small kernels -- a pointwise start (magnitudes, copy, mixture sum), the overlap-add synthesis of the mixture or
 * of the current iterate, and the projection back onto the magnitudes.  gfx950, wave64.
 *
 * The synthesis and the radix-2 stages are those of csrc/wave_metric.h, which libdanet_metric_hip.so runs too; this
 * file adds the entry points, the choice of rows and the projection kernel.
 * danet_phase_init.  A thread per element of est0; then synth_tile over the mixture sum into row C of wav.
 * danet_phase_synth.  synth_tile over the C rows of every utterance into rows 0..C-1 of wav.
 * danet_phase_project.  One workgroup of 256 threads per (signal, tile of frames).  LDS: N/2 twiddles
 * e^(-2 pi i j / N) (sincospif, once per workgroup), the tile's span of z, and the tile's frames of N floats.
 *   stage:  z[n] = x_c[n] + (y[n] - sum_c' x_c'[n]) / C in float32, 0 outside [0, Ls);
 *   frames: v[m] = w[2m] z[.. + 2m] + i w[2m+1] z[.. + 2m + 1], stored at the bit-reversed index of m;
 *   fft:    radix2_stages over all frames of the tile: with these twiddles, the forward transform;
 *   split:  Z[k] = E - i e^(-2 pi i k / N) O with E = (V[k] + conj(V[N/2-k])) / 2, O = (V[k] - conj(V[N/2-k])) / 2;
 *           bins 0 and N/2 are Re V[0] +- Im V[0]; then X = A Z / |Z| where |Z|^2 > 0 and finite, the old X elsewhere.
 */
#include <hip/hip_runtime.h>

#include "danet_phase_hip.h"
#define DANET_EXT phase
#define DANET_EXT_UPPER PHASE
#include "ext_core.h"
#include "wave_metric.h"

static_assert(kMaxC == DANET_PHASE_MAX_C, "csrc/wave_metric.h and include/danet_phase_hip.h disagree");

/* ------------------------------------------------------------------------------------ workspace */
struct Layout {
  size_t a, mix, wav, total;   /* byte offsets of the three parts, and the size */
};

static inline Layout layout_of(int B, int C, int T, int N, int S) {
  const size_t F = (size_t)N / 2 + 1, Ls = (size_t)(T - 1) * (size_t)S;
  Layout l;
  l.a = 0;
  l.mix = l.a + round256((size_t)B * C * T * F * sizeof(float));
  l.wav = l.mix + round256((size_t)B * T * F * sizeof(float2));
  l.total = l.wav + round256((size_t)B * (C + 1) * Ls * sizeof(float));
  return l;
}

/* the envelope of THE RULE; Cm = 1 where an entry point has no mixture rows */
static bool envelope_ok(const char* who, int B, int C, int Cm, int T, int N, int S) {
  if (!synth_shape_ok(B, C, T, N, S) || C > kMaxC || Cm < 1 || Cm > kMaxC) {
    set_error("%s: need B >= 1, 1 <= C <= %d, 1 <= Cm <= %d, T >= 2, N a power of two in 64..1024 and "
              "N/8 <= S <= N/2 (got B = %d, C = %d, Cm = %d, T = %d, N = %d, S = %d)", who, kMaxC, kMaxC, B, C, Cm, T, N, S);
    return false;
  }
  const int64_t F = N / 2 + 1, Ls = (int64_t)(T - 1) * S, two31 = (int64_t)1 << 31;
  /* (products of at most 2^31 * 2^31 would overflow: each factor is checked on the way) */
  const int64_t tf = (int64_t)T * F, rows = (int64_t)B * (C > Cm ? C : Cm), wrows = (int64_t)B * (C + 1);
  if (tf >= two31 || rows * tf >= two31 || Ls >= two31 || wrows * Ls >= two31) {
    set_error("%s: B * max(C, Cm) * T * F and B * (C + 1) * (T - 1) * S must be < 2^31", who);
    return false;
  }
  return true;
}

extern "C" size_t danet_phase_workspace_bytes(int B, int C, int T, int N, int S) {
  if (!envelope_ok("workspace_bytes", B, C, 1, T, N, S)) return (size_t)-1;
  return layout_of(B, C, T, N, S).total;
}

/* ---------------------------------------------------------------------------------------- start */
__global__ __launch_bounds__(kThreads) void phase_start_kernel(int64_t n_est, int64_t n_mix, int64_t TF, int Cm,
                                                              const float2* est0, const float2* mixrows,
                                                              float* __restrict__ A, float2* __restrict__ mix,
                                                              float2* x) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_est) return;
  const float2 e = est0[i];                                    /* (x may be est0: read before the store) */
  /* the hypot form without its float32 rounding steps: the squares are exact in float64 and cannot overflow */
  A[i] = (float)sqrt((double)e.x * (double)e.x + (double)e.y * (double)e.y);
  x[i] = e;
  if (i < n_mix) {
    const int64_t b = i / TF, r = i - b * TF;
    const float2* row = mixrows + b * Cm * TF + r;
    float2 s = row[0];
    for (int c = 1; c < Cm; ++c) {
      const float2 v = row[(int64_t)c * TF];
      s.x += v.x;
      s.y += v.y;
    }
    mix[i] = s;
  }
}

/* ------------------------------------------------------------------------------------ synthesis */
struct PhaseSynthArgs {
  const float2* X;   /* [B][rows][T][F] */
  int rows;          /* signals per utterance synthesised: 1 (the mixture sum) or C */
  int row0;          /* their first row of wav [B][C + 1][Ls]: C or 0               */
  SynthArgs s;
};

__global__ __launch_bounds__(kThreads) void phase_synth_kernel(PhaseSynthArgs a) {
  const int T = a.s.T, F = (a.s.N >> 1) + 1;
  const int u = (int)(blockIdx.x / (unsigned)a.s.tiles);       /* b * rows + r */
  const int tile = (int)(blockIdx.x - (unsigned)u * (unsigned)a.s.tiles);
  const int b = u / a.rows, r = u - b * a.rows;
  synth_tile(a.s, a.X + (int64_t)u * T * F, b * (a.s.C + 1) + a.row0 + r, tile, LoadBin());
}

/* the launch of `rows` signals per utterance; blocks <= B * C * T < 2^31 by the envelope */
static inline void launch_synth(hipStream_t stream, int B, int C, int T, int N, int S, const float2* X, int rows, int row0,
                                const float* window, float* wav) {
  const PhaseSynthArgs a = {X, rows, row0, synth_args(C, T, N, S, window, wav)};
  const int64_t blocks = (int64_t)B * rows * a.s.tiles;
  phase_synth_kernel<<<dim3((unsigned)blocks), kThreads, synth_lds_bytes(a.s), stream>>>(a);
}

extern "C" int danet_phase_init(void* stream, int B, int C, int Cm, int T, int N, int S, const float* est0,
                                const float* mixrows, const float* window, void* ws, float* x) {
  if (!envelope_ok("init", B, C, Cm, T, N, S)) return DANET_PHASE_ERR_ARG;
  CHECK_ARG(est0 && mixrows && window && ws && x, "init: null pointer");
  CHECK_ARG(((uintptr_t)est0 & 7) == 0 && ((uintptr_t)mixrows & 7) == 0 && ((uintptr_t)x & 7) == 0 &&
                ((uintptr_t)ws & 7) == 0 && ((uintptr_t)window & 3) == 0,
            "init: misaligned pointer (est0, mixrows, x, ws 8-byte; window 4-byte)");
  const Layout l = layout_of(B, C, T, N, S);
  char* base = (char*)ws;
  const int64_t TF = (int64_t)T * (N / 2 + 1), n_est = (int64_t)B * C * TF, n_mix = (int64_t)B * TF;
  phase_start_kernel<<<dim3((unsigned)((n_est + kThreads - 1) / kThreads)), kThreads, 0, (hipStream_t)stream>>>(
      n_est, n_mix, TF, Cm, (const float2*)est0, (const float2*)mixrows, (float*)(base + l.a), (float2*)(base + l.mix),
      (float2*)x);
  CHECK_LAUNCH();
  launch_synth((hipStream_t)stream, B, C, T, N, S, (const float2*)(base + l.mix), 1, C, window, (float*)(base + l.wav));
  CHECK_LAUNCH();
  return DANET_PHASE_OK;
}

extern "C" int danet_phase_synth(void* stream, int B, int C, int T, int N, int S, const float* x, const float* window,
                                 void* ws) {
  if (!envelope_ok("synth", B, C, 1, T, N, S)) return DANET_PHASE_ERR_ARG;
  CHECK_ARG(x && window && ws, "synth: null pointer");
  CHECK_ARG(((uintptr_t)x & 7) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)window & 3) == 0,
            "synth: misaligned pointer (x, ws 8-byte; window 4-byte)");
  const Layout l = layout_of(B, C, T, N, S);
  launch_synth((hipStream_t)stream, B, C, T, N, S, (const float2*)x, C, 0, window, (float*)((char*)ws + l.wav));
  CHECK_LAUNCH();
  return DANET_PHASE_OK;
}

/* ----------------------------------------------------------------------------------- projection */
struct ProjectArgs {
  const float* wav;     /* [B][C + 1][Ls] */
  const float* A;       /* [B][C][T][F]   */
  const float* window;
  float2* x;            /* [B][C][T][F], in place */
  float2* z_out;        /* null or [B][C][T][F]   */
  int C, T, N, S;
  int log2_half;        /* log2(N/2) */
  int frames, tiles;    /* frames per tile, tiles per signal */
};

__global__ __launch_bounds__(kThreads) void phase_project_kernel(ProjectArgs a) {
  extern __shared__ __align__(16) float lds[];                 /* (viewed as float2 below) */
  const int N = a.N, S = a.S, T = a.T, C = a.C, M = N >> 1, F = M + 1;
  const int tid = threadIdx.x;
  const int sig = (int)(blockIdx.x / (unsigned)a.tiles);       /* b * C + c */
  const int tile = (int)(blockIdx.x - (unsigned)sig * (unsigned)a.tiles);
  const int b = sig / C, c = sig - b * C;
  const int t0 = tile * a.frames;
  const int nfr = min(a.frames, T - t0);                       /* >= 1: tiles = ceil(T / frames) */
  const int Ls = (T - 1) * S;
  const int span = (nfr - 1) * S + N;                          /* samples [n_lo, n_lo + span) */
  const int n_lo = t0 * S - M;
  float2* tw = reinterpret_cast<float2*>(lds);                 /* [M]                        */
  float* frames = lds + N;                                     /* [a.frames][N]              */
  float* z = frames + a.frames * N;                            /* [(a.frames - 1) * S + N]   */
  const int64_t row = ((int64_t)sig * T + t0) * F;             /* first element of the tile  */

  for (int k = tid; k < M; k += kThreads) {
    float s, co;
    sincospif((float)(2 * k) / (float)N, &s, &co);
    tw[k] = make_float2(co, -s);
  }
  /* stage z: the C rows of the utterance in ascending order, this signal's own selected among them, and y */
  const float* rows = a.wav + (int64_t)b * (C + 1) * Ls;
  const float* y = rows + (int64_t)C * Ls;
  const float fc = (float)C;
  for (int i = tid; i < span; i += kThreads) {
    const int n = n_lo + i;
    float v = 0.f;
    if (n >= 0 && n < Ls) {
      float sum = rows[n], own = sum;
      for (int c2 = 1; c2 < C; ++c2) {
        const float r = rows[(int64_t)c2 * Ls + n];
        sum += r;
        own = c2 == c ? r : own;
      }
      v = own + (y[n] - sum) / fc;
    }
    z[i] = v;
  }
  __syncthreads();

  /* windowed frames -> the N/2 complex inputs of the half-size transform, bit-reversed */
  const int shift = 32 - a.log2_half;
  for (int idx = tid; idx < nfr * M; idx += kThreads) {
    const int f = idx >> a.log2_half, m = idx & (M - 1);
    const float* src = z + f * S + 2 * m;
    const int rm = (int)(__brev((unsigned)m) >> shift);
    reinterpret_cast<float2*>(frames + f * N)[rm] = make_float2(a.window[2 * m] * src[0], a.window[2 * m + 1] * src[1]);
  }
  __syncthreads();

  /* the forward transform of every frame of the tile */
  radix2_stages(frames, tw, nfr, N, a.log2_half);

  /* split step, normalise, write: output bin idx = f * F + k of the tile per thread and turn */
  for (int idx = tid; idx < nfr * F; idx += kThreads) {
    const int f = idx / F, k = idx - f * F;
    const float2* v = reinterpret_cast<const float2*>(frames + f * N);
    float zr, zi;
    if (k == 0 || k == M) {
      const float2 v0 = v[0];
      zr = k == 0 ? v0.x + v0.y : v0.x - v0.y;
      zi = 0.f;
    } else {
      const float2 p = v[k], q = v[M - k];
      const float er = p.x + q.x, ei = p.y - q.y;               /* 2 E = V[k] + conj(V[M-k]) */
      const float dr = p.x - q.x, di = p.y + q.y;               /* 2 O = V[k] - conj(V[M-k]) */
      const float2 w = tw[k];
      const float pr = w.x * dr - w.y * di, pi = w.x * di + w.y * dr;
      zr = 0.5f * (er + pi);                                    /* E - i w O */
      zi = 0.5f * (ei - pr);
    }
    const float mag = a.A[row + idx];
    float2 out = a.x[row + idx];                                /* the old value of this thread's own bin */
    const float m2 = zr * zr + zi * zi;
    if (m2 > 0.f && m2 <= 3.402823466e+38f) {
      const float r = sqrtf(m2);
      out = mag == 0.f ? make_float2(0.f, 0.f) : make_float2(mag * (zr / r), mag * (zi / r));
    }
    a.x[row + idx] = out;
    if (a.z_out) a.z_out[row + idx] = make_float2(zr, zi);
  }
}

extern "C" int danet_phase_project(void* stream, int B, int C, int T, int N, int S, const float* window, void* ws,
                                   float* x, float* z_out) {
  if (!envelope_ok("project", B, C, 1, T, N, S)) return DANET_PHASE_ERR_ARG;
  CHECK_ARG(window && ws && x, "project: null pointer");
  CHECK_ARG(((uintptr_t)x & 7) == 0 && ((uintptr_t)z_out & 7) == 0 && ((uintptr_t)ws & 7) == 0 &&
                ((uintptr_t)window & 3) == 0,
            "project: misaligned pointer (x, z_out, ws 8-byte; window 4-byte)");
  CHECK_ARG(x != z_out, "project: z_out must not be x");
  const Layout l = layout_of(B, C, T, N, S);
  const int frames = DANET_PHASE_TILE_FRAMES(N);
  const int tiles = (T + frames - 1) / frames;
  const int64_t blocks = (int64_t)B * C * tiles;                /* <= B * C * T < 2^31 by the envelope */
  ProjectArgs a;
  a.wav = (const float*)((char*)ws + l.wav); a.A = (const float*)((char*)ws + l.a); a.window = window;
  a.x = (float2*)x; a.z_out = (float2*)z_out;
  a.C = C; a.T = T; a.N = N; a.S = S;
  a.log2_half = log2_half(N);
  a.frames = frames; a.tiles = tiles;
  /* twiddles N + frames * N + span (frames - 1) * S + N floats: <= 3N/2 (1 + frames) <= 16384 at S = N/2 */
  const size_t lds_bytes = ((size_t)N + (size_t)frames * N + (size_t)(frames - 1) * S + N) * sizeof(float);
  phase_project_kernel<<<dim3((unsigned)blocks), kThreads, lds_bytes, (hipStream_t)stream>>>(a);
  CHECK_LAUNCH();
  return DANET_PHASE_OK;
}
