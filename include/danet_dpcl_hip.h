/*
 * libdanet_dpcl_hip.so -- C ABI of the deep-clustering auxiliary loss (DPCL_WEIGHT): the weighted affinity loss
 * || W^1/2 (V V^T - Y Y^T) W^1/2 ||_F^2 of the embedding against the ideal binary mask, computed from E x (E + C)
 * weighted Gram matrices per utterance -- the N x N affinity matrices never exist -- and its gradient.  Three
 * launches: a stats pass over the embedding, a finalize step, and one backward pass.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other twelve libraries stay as they are.
 * Same conventions as include/danet_gclip_hip.h: caller-owned DEVICE pointers, fp32 / float64, `stream` a
 * hipStream_t passed as void*, 0 = DANET_DPCL_OK and negative = error with a thread-local message in
 * danet_dpcl_last_error(), asynchronous launches, no process environment read, no allocation, no atomics: repeated
 * calls agree bit for bit, and every address is a function of the host-visible arguments.
 *
 * THE RULE.  Per utterance b, with N = T * F rows:
 *     v_i        row i of the embedding [B][N][E], float32 as the encoder writes it (no normalisation)
 *     S_ci       src_pwr[b][c][i], the front end's |src| of the clean sources ([B][C][N], float32)
 *     y_i        = the lowest c with S_ci = max_c' S_c'i      (the ideal binary mask; an exact float32 comparison,
 *                                                              so a tie and an all-zero bin go to the lowest c)
 *     s_i        = sum_c S_ci                                  (added in the order c = 0, 1, ...)
 *     w_i        = s_i / sum_j s_j                             (magnitude-ratio weights: sum_i w_i = 1)
 *     A          = sum_i w_i v_i v_i^T                         (E x E)
 *     Bm         = sum_i w_i v_i e_{y_i}^T                     (E x C)
 *     c_k        = sum_{i: y_i = k} w_i
 *     L_b        = ||A||_F^2 - 2 ||Bm||_F^2 + sum_k c_k^2      (= sum_ij w_i w_j (v_i.v_j - [y_i = y_j])^2)
 *     silent     sum_j s_j = 0: A = Bm = c = 0, L_b = 0 and a zero gradient
 *     dpcl       = (1 / B) sum_b L_b
 *     total      = main + alpha * dpcl                         (main: a given scalar, 0 when absent)
 *     d total / d v_i = dloss * (alpha / B) * 4 w_i (A v_i - Bm[:, y_i])
 *
 * Arithmetic.  The stats pass cuts the N rows of an utterance into chunks(N) chunks of chunk_rows(N) rows,
 *     chunk_rows(N) = 128 * ceil(ceil(N / DANET_DPCL_MAX_CHUNKS) / 128),   chunks(N) = ceil(N / chunk_rows(N)),
 * a function of N alone, and writes per chunk the UNNORMALISED float32 sums  sum s_i v_i v_i^T,
 * sum_{y_i = k} s_i v_i, sum_{y_i = k} s_i and sum s_i  as one (E + 1) x (E + C + 1) matrix G = P^T Q with
 * P_i = [s_i v_i | s_i] and Q_i = [v_i | 1 | e_{y_i}]: G[e][f] = sum s v_e v_f, G[e][E + 1 + k] = sum_{y = k} s v_e, G[E][E] = sum s,
 * G[E][E + 1 + k] = sum_{y = k} s (and G[e][E] = G[E][e] = sum s v_e, which nothing reads).  Inside a chunk the rows are taken in tiles of 128; a tile's
 * products are added in float32 in a fixed order (below), the tiles of a chunk in float64 in tile order, rounded to
 * float32 once.  Finalize adds the chunks in float64 in chunk order, divides by sum s in float64 and forms L_b, dpcl
 * and total in float64.  Backward is float32 throughout.
 */
#ifndef DANET_DPCL_HIP_H
#define DANET_DPCL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/dpcl/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_DPCL_ABI_VERSION 1

#define DANET_DPCL_OK 0
#define DANET_DPCL_ERR_ARG (-1)     /* bad size / null or misaligned pointer / workspace too small / bad alpha */
#define DANET_DPCL_ERR_LAUNCH (-2)  /* hipLaunch failure                                                      */

#define DANET_DPCL_MAX_E 64
#define DANET_DPCL_MAX_C 4
#define DANET_DPCL_MAX_N ((int64_t)1 << 31)
#define DANET_DPCL_MAX_B 65535
#define DANET_DPCL_MAX_CHUNKS 16
#define DANET_DPCL_TILE_ROWS 128

int danet_dpcl_abi_version(void);
const char* danet_dpcl_last_error(void);

/* chunks(N) of THE RULE, a pure function; 0 (and a message) for N outside 1..DANET_DPCL_MAX_N. */
int danet_dpcl_chunks(int64_t N);

/* Bytes of the workspace danet_dpcl_stats writes and danet_dpcl_finalize reads:
 * B * chunks(N) * (E + 1) * (E + C + 1) float32, utterance-major, then chunk, then the matrix G row-major.
 * (size_t)-1 (and a message) outside the envelope 1 <= B <= DANET_DPCL_MAX_B, 1 <= N <= DANET_DPCL_MAX_N,
 * 1 <= E <= DANET_DPCL_MAX_E, 1 <= C <= DANET_DPCL_MAX_C.  The caller owns the workspace; nothing else is needed. */
size_t danet_dpcl_workspace_bytes(int B, int64_t N, int E, int C);

/* The stats pass, ONE launch of chunks(N) x B workgroups of 256 threads.  embed float32 [B][N][E], src_pwr float32
 * [B][C][N] -> workspace (the layout above), every element of it written with ordinary vector stores.
 * Every output element is one thread's own sum, or the sum of g = floor(256 / tiles) threads' sums in the order of
 * the threads (tiles = ceil((E + 1) / 4) * ceil((E + C + 1) / 4) register tiles of 4 x 4 outputs; thread group j
 * takes the rows j, j + g, ... of a tile of 128 rows).  An utterance's partials depend on its own rows, N, E and C
 * and on nothing else: not on B, not on its place in the batch.
 * embed 16-byte aligned with N * E a multiple of 4: 16-byte loads; otherwise (embed 4-byte aligned) a slower path
 * of 4-byte loads with the same arithmetic and the same result bit for bit -- never an error.
 * Envelope as danet_dpcl_workspace_bytes; no null pointer; embed, src_pwr, workspace 4-byte aligned;
 * workspace_bytes >= danet_dpcl_workspace_bytes(B, N, E, C).  A violation returns DANET_DPCL_ERR_ARG and
 * launches nothing.                                                                                          */
int danet_dpcl_stats(void* stream, int B, int64_t N, int E, int C, const float* embed, const float* src_pwr,
                     void* workspace, size_t workspace_bytes);

/* Finalize, ONE launch of one workgroup.  Reads the workspace of danet_dpcl_stats with the same (B, N, E, C) and
 * writes
 *     per_utt_f64 [B]            L_b
 *     dpcl_f32    [1]            dpcl
 *     total_f32   [1]            (float)((double)main + (double)alpha * dpcl); main_f32 a DEVICE scalar, NULL = 0.
 *                                alpha = 0 gives main back bit for bit
 *     tables_f32  [B][E][E + C]  row e: A[e][0..E) then Bm[e][0..C), already divided by sum s (NOT times 4)
 *     cs_f32      [B][C + 1]     c_0 .. c_{C-1}, then sum_j s_j (unnormalised)
 * alpha: a HOST scalar, finite and >= 0.  per_utt 8-byte, the rest 4-byte aligned; main_f32 may be NULL, nothing
 * else.  A violation returns DANET_DPCL_ERR_ARG and launches nothing.                                         */
int danet_dpcl_finalize(void* stream, int B, int64_t N, int E, int C, const void* workspace, size_t workspace_bytes,
                        const float* main_f32, float alpha, double* per_utt_f64, float* dpcl_f32, float* total_f32,
                        float* tables_f32, float* cs_f32);

/* Backward, ONE launch of ceil(N / 1024) x B workgroups of 256 threads, one row per thread at a time with the row
 * in registers and A, Bm in LDS:
 *     dembed[b][i][:] = (dloss * scale) * 4 * (s_i * (1 / sum s)) * (A v_i - Bm[:, y_i])
 * with y_i and s_i recomputed from src_pwr (C loads per row), dloss_f32 a DEVICE scalar (NULL = 1) and scale the
 * HOST scalar alpha / B (finite).  dembed float32 [B][N][E], every element written with an ordinary vector store;
 * a silent utterance (sum s = 0) gets zeros.  16-byte accesses when embed and dembed are 16-byte aligned and E is
 * one of 4, 8, 20, 40, 64 (the instantiated row sizes), 4-byte accesses otherwise, the same result.  tables_f32 and cs_f32 as danet_dpcl_finalize wrote
 * them.  No null pointer but dloss_f32; 4-byte alignment.  A violation returns DANET_DPCL_ERR_ARG and launches
 * nothing.                                                                                                    */
int danet_dpcl_bwd(void* stream, int B, int64_t N, int E, int C, const float* embed, const float* src_pwr,
                   const float* tables_f32, const float* cs_f32, const float* dloss_f32, float scale,
                   float* dembed);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_DPCL_HIP_H */
