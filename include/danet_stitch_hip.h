/*
 * libdanet_stitch_hip.so -- C ABI of chunked inference (INFER_CHUNK_LEN): a long recording is separated in
 * overlapping chunks, and this library puts the chunks' outputs back together -- it aligns the output channels of
 * neighbouring chunks (mask-based separation is permutation-free per chunk), cross-fades the overlaps and re-attaches
 * the mixture phase -- in three small kernels whose outputs can each be read back: affinity partials, permutation
 * chain, merged spectra.  gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other fourteen libraries stay as they are.
 * Same conventions as include/danet_metric_hip.h: caller-owned DEVICE pointers, fp32 / interleaved complex64 /
 * float64 / int32, `stream` a hipStream_t passed as void*, 0 = DANET_STITCH_OK and negative = error with a
 * thread-local message in danet_stitch_last_error(), asynchronous launches, no process environment read, no
 * allocation, no atomics, no transcendental math.
 *
 * THE RULE.
 *
 * Plan.  Integers only; a pure function of (T, L, V): T frames of the recording, L frames per chunk, V frames of
 * cross-fade, H = L - V.  T <= L: one chunk, and the chunked route is not taken at all.  Otherwise
 *     n   = 1 + ceil((T - L) / H)                 chunks,
 *     s_i = i * H  for i < n - 1,   s_{n-1} = T - L,     e_i = s_i + L.
 * The last chunk is slid back to end at the recording's end; it is NOT zero-padded (an unweighted attractor estimate
 * would average the padding in).  The last hop s_{n-1} - s_{n-2} is in [1, H].  Chunks i and i + 1 overlap on
 * O_i = [s_{i+1}, e_i): V frames for a regular pair, between V and L - 1 for the last pair.  They cross-fade on the
 * last V frames of chunk i, F_i = [e_i - V, e_i), which chunk i + 1 covers because every hop is <= H.  The fades are
 * disjoint because H >= V, so every output frame has at most two contributing chunks, even where three chunks overlap
 * it.
 *
 * Affinity.  m_i[c][t][f]: the separated magnitudes of chunk i, before phase re-attachment, float32 mags[n][C][L][F].
 *     S_i[c][c'] = sum over t in O_i and f of  m_i[c][t - s_i][f] * m_{i+1}[c'][t - s_{i+1}][f],
 * products (exact: float32 x float32) and sums in float64 over a fixed tree, no atomics: two launches agree bit for
 * bit.  Both factors of an overlap are CONTIGUOUS runs of |O_i| * F floats (rows hop .. L - 1 of m_i[c], rows
 * 0 .. |O_i| - 1 of m_{i+1}[c']).
 *
 * Assignment.  pi_i = the permutation p of range(C) that maximises sum_c S_i[c][p[c]] (added in ascending c), the
 * permutations taken in itertools.permutations order, the first winning a tie: an all-zero overlap gives the
 * identity.  Chain: P_0 = identity, P_{i+1}[c] = pi_i[P_i[c]].  Output channel c is chunk i's channel P_i[c].
 *
 * Merge.  For output frame t the owner is the smallest i with t < e_i.  If i < n - 1 and t >= e_i - V (a fade):
 *     k = t - (e_i - V),  a = m_i[P_i[c]][t - s_i][f],  b = m_{i+1}[P_{i+1}[c]][t - s_{i+1}][f],
 *     mag = fma(w_k, fl(b - a), a)            in float32: b == a returns exactly a,
 * otherwise mag = m_i[P_i[c]][t - s_i][f] exactly.  w_k = (k + 1) / (V + 1), k < V: the caller computes the table in
 * float64, rounds it once to float32 and hands it in (`fade`).  Output: complex64 out[C][T][F] =
 * (fl(mag * ph.re), fl(mag * ph.im)), ph the mixture phasor at (t, f) taken from the OWNER chunk's row of
 * phasor[n][L][F][2].  The front end that writes the phasor (danet_frontend_fwd) is pointwise in (t, f) -- one thread
 * per bin reads that bin of the sources and writes that bin of every output, with no reduction over t or f -- so every
 * chunk that covers a frame holds the same bits for it, and the owner's row is as good as any (checked by
 * tests/test_gpu_stitch.py on the model's own chunks).
 *
 * Envelope of the three device entry points: 1 <= C <= DANET_STITCH_MAX_C, F >= 1, 2 <= L, 1 <= V <= L / 2, T > L,
 * n <= DANET_STITCH_MAX_CHUNKS, L * F < 2^31, T * F < 2^40.
 */
#ifndef DANET_STITCH_HIP_H
#define DANET_STITCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/stitch/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_STITCH_ABI_VERSION 1

#define DANET_STITCH_OK 0
#define DANET_STITCH_ERR_ARG (-1)     /* bad shape / null or misaligned pointer / workspace too small */
#define DANET_STITCH_ERR_LAUNCH (-2)  /* hipLaunch failure                                            */

#define DANET_STITCH_MAX_C 4           /* 24 permutations at the most, as in include/danet_metric_hip.h */
#define DANET_STITCH_MAX_CHUNKS 65536
#define DANET_STITCH_TILE 8192         /* floats of an overlap run that one workgroup of the affinity pass sums */

int danet_stitch_abi_version(void);
const char* danet_stitch_last_error(void);

/* n of THE RULE (1 when T <= L); a pure host function.  Negative (and a message) unless T >= 1, L >= 2 and
 * 1 <= V <= L / 2.  n may exceed DANET_STITCH_MAX_CHUNKS here: the device entry points refuse such a plan.     */
int danet_stitch_chunks(int T, int L, int V);

/* Bytes of the workspace danet_stitch_affinity writes and danet_stitch_assign reads: float64
 * [n - 1][tiles][C][C] with tiles = ceil(L * F / DANET_STITCH_TILE), the same for every pair.  (size_t)-1 (and a
 * message) outside the envelope.                                                                              */
size_t danet_stitch_workspace_bytes(int T, int L, int V, int C, int F);

/* The per-pair, per-tile partial sums of S (THE RULE) into ws, ONE launch: one workgroup of 256 threads per (tile,
 * pair) sums the products of floats [tile * TILE, (tile + 1) * TILE) of the pair's overlap run for all C x C channel
 * pairs at once.  A thread takes the groups of four consecutive floats tid, tid + 256, ... of the tile in order (the
 * four products added one after the other), the 64 lanes of a wave meet in a fixed butterfly and the four waves as
 * (w0 + w1) + (w2 + w3).  A tile behind the end of its pair's run writes zeros, so every byte of the workspace is
 * written.  The runs are read with 16-byte loads where the address allows (mags 16-byte aligned, L * F a multiple of
 * 4 and, for chunk i's run, hop * F too) and with 4-byte loads to the same bits otherwise: never an error.
 * mags 4-byte, ws 8-byte aligned; ws_bytes >= danet_stitch_workspace_bytes.  A violation returns
 * DANET_STITCH_ERR_ARG and launches nothing.                                                                   */
int danet_stitch_affinity(void* stream, int T, int L, int V, int C, int F, const float* mags, void* ws,
                          size_t ws_bytes);

/* S, the local permutations and their chain, ONE launch of ONE workgroup, so the route has no host wait: thread
 * tid takes the pairs tid, tid + 256, ...; for each it adds the tiles of every entry in ascending order into
 * S_out float64 [n - 1][C][C] and searches the C! permutations; then one thread composes the chain into perm_out
 * int32 [n][C] (perm_out[i][c] = P_i[c]; it reads the local permutations eight pairs ahead of the composition).
 * ws, S_out 8-byte, perm_out 4-byte aligned.  A violation returns DANET_STITCH_ERR_ARG and launches nothing.    */
int danet_stitch_assign(void* stream, int T, int L, int V, int C, int F, const void* ws, size_t ws_bytes,
                        double* S_out, int32_t* perm_out);

/* The merge of THE RULE into out complex64 [C][T][F], ONE launch, the gather form: every output element reads its
 * one or two sources.  A thread takes two consecutive elements of the flat index t * F + f of one channel, so loads
 * and stores are coalesced whatever F is, and writes them with one 16-byte store (two 8-byte stores when out is only
 * 8-byte aligned, and for an odd last element).  phasor float32 [n][L][F][2], fade float32 [V], perm int32 [n][C] as
 * danet_stitch_assign wrote it.  Entries of perm are read from device memory and clamped to [0, C): no read or write
 * leaves a buffer whatever the table holds.
 * mags, fade, perm 4-byte, phasor, out 8-byte aligned.  A violation returns DANET_STITCH_ERR_ARG and launches
 * nothing.                                                                                                     */
int danet_stitch_merge(void* stream, int T, int L, int V, int C, int F, const float* mags, const float* phasor,
                       const float* fade, const int32_t* perm, float* out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_STITCH_HIP_H */
