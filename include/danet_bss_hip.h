/*
 * libdanet_bss_hip.so -- C ABI of the BSS-eval figures of `valid` / `test` (EVAL_BSS_SDR): SDR, SIR, SAR and the
 * SDR improvement over the unprocessed mixture, as BSS-eval v3 `bss_eval_sources` defines them (projection of every
 * estimate onto the references filtered by an L-tap distortion filter), in five stages whose outputs can each be
 * read back: lagged correlations, the block-Toeplitz systems, a batched blocked Cholesky solve, decibels.
 * gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other fifteen libraries stay as they are.
 * Same conventions as include/danet_metric_hip.h: caller-owned DEVICE pointers, fp32 / float64 / int32, `stream`
 * a hipStream_t passed as void*, 0 = DANET_BSS_OK and negative = error with a thread-local message in
 * danet_bss_last_error(), asynchronous launches, no process environment read, no allocation; every argument
 * error returns before any launch; nothing the device alone can see (the values of the waveforms, a failing
 * pivot) moves a read or a write; every value is written with ordinary vector stores.
 *
 * THE RULE.
 *
 * Signals.  wav[b] of danet_metric_synth: float32 [2C][Ls], the C references s_i first, then the C UNPERMUTED
 * estimates e_j, each Ls = (T - 1) * S samples and zero outside [0, Ls).  L is the filter length, 1 <= L <= 512.
 *
 * Correlations.  Products are float64 and exact; sums are float64 over a fixed tree that depends on Ls alone (so
 * on (Ls, L) alone): a sum runs over all n in [0, Ls) -- a factor outside its signal reads as 0 -- term n goes
 * to accumulator n mod 4 in ascending n, and the four join as (a0 + a1) + (a2 + a3).
 *     R_ik[tau] = sum_n s_i[n] s_k[n + tau],  |tau| < L.   Computed for i <= k only (for i = k, tau >= 0 only) and
 *                 mirrored, R_ki[tau] = R_ik[-tau]: R_ii is symmetric bit for bit by construction.
 *     D_ji[tau] = sum_n e_j[n] s_i[n - tau],  0 <= tau < L.
 *     ee_j      = sum_n e_j[n]^2.
 *
 * Systems.  G[(i, t1), (k, t2)] = R_ik[t1 - t2], CL x CL, block-Toeplitz; its diagonal blocks G_ii are L x L
 * Toeplitz.  A reference with R_ii[0] = 0 is silent: its rows and columns of G (and its G_ii) are replaced by the
 * identity and its right-hand sides by 0; it takes no part in any mean or permutation.
 *
 * Per estimate j.  pall_j = D_j^T G^-1 D_j (D_j the CL-vector of the D_ji), st_ij = D_ji^T G_ii^-1 D_ji, and with
 *     q(a, b) = -100 when a <= 0;  +100 when b <= 0 (and a > 0);  else 10 log10(a / b) clamped to [-100, 100]:
 *     SDR(i, j) = q(st_ij, ee_j - st_ij),   SIR(i, j) = q(st_ij, pall_j - st_ij),   SAR(j) = q(pall_j, ee_j - pall_j).
 * These are the energies of bss_eval_sources: s_target is the projection onto the L delays of one reference,
 * s_target + e_interf the projection onto the delays of all of them, and orthogonality turns every energy into a
 * quadratic form.
 *
 * Permutation.  As in BSS-eval v3, p maximises sum_i SIR(i, p(i)) over the live references (added in ascending
 * i); ties go to the first permutation in itertools.permutations(range(C)) order.
 *
 * Baseline.  The mixture m = sum_k s_k taken as the estimate of every reference.  By linearity
 * D_mi[tau] = sum_k R_ik[tau] (ascending k, from 0.0) and mm = sum_i sum_k R_ik[0] (row by row), so the baseline
 * is one more right-hand side per G_ii: base_i = q(st_mi, mm - st_mi).
 *
 * Per utterance.  (SDR, SIR, SAR, SDRi) = the means over the live references of SDR(i, p(i)), SIR(i, p(i)),
 * SAR(p(i)) and SDR(i, p(i)) - base_i; (0, 0, 0, 0) and perm_idx 0 when no reference is live.
 *
 * Flagged utterances.  A pivot of the Cholesky factorisation of any of an utterance's matrices that is not a
 * positive finite number sets that utterance's flag.  A flagged utterance reports (0, 0, 0, 0), perm_idx 0, and
 * is left out of the batch means.  Unlike mir_eval there is NO least-squares fallback for a singular system.
 * flags[b]: bit 0 = a pivot failed, bit 1 = no reference is live.
 *
 * Per batch.  mean4 = the means over the utterances with flags = 0, or 0 if there is none.
 */
#ifndef DANET_BSS_HIP_H
#define DANET_BSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/bss/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                */
#pragma GCC visibility push(default)

#define DANET_BSS_ABI_VERSION 1

#define DANET_BSS_OK 0
#define DANET_BSS_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_BSS_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_BSS_MAX_C 4          /* 24 permutations at the most                          */
#define DANET_BSS_MAX_L 512        /* the filter length of bss_eval_sources                */
#define DANET_BSS_MAX_N 2048       /* the largest system: DANET_BSS_MAX_C * DANET_BSS_MAX_L */
#define DANET_BSS_MAX_RHS 16
#define DANET_BSS_MAX_BATCH 65535  /* utterances (matrices) of one call                     */
#define DANET_BSS_BLOCK 64         /* the block of the Cholesky factorisation              */

int danet_bss_abi_version(void);
const char* danet_bss_last_error(void);

/* Bytes of one buffer that holds everything the entry points write for B utterances, each part at a multiple of
 * 256 bytes, in this order (n = C * L):
 *     R        float64 [B][C][C][2L - 1]    R[b][i][k][tau + L - 1] = R_ik[tau]
 *     D        float64 [B][C][C][L]         D[b][j][i][tau] = D_ji[tau]
 *     ee       float64 [B][C]
 *     G        float64 [B][n][n]
 *     Gs       float64 [B][C][L][L]         the diagonal blocks G_ii
 *     Xg       float64 [B][C][n]            right-hand sides / solutions of G: row j is D_j
 *     Xs       float64 [B][C][C + 1][L]     of G_ii: rows j < C are D_ji, row C is the baseline D_mi
 *     fg       int32   [B]                  flags of the factorisations of G
 *     fs       int32   [B][C]               and of the G_ii
 *     per_utt  float64 [B][4]
 *     perm_idx int32   [B]
 *     flags    int32   [B]
 *     mean4    float64 [4]
 * (size_t)-1 for B outside 1..DANET_BSS_MAX_BATCH, C outside 1..DANET_BSS_MAX_C or L outside 1..DANET_BSS_MAX_L. */
size_t danet_bss_workspace_bytes(int B, int C, int L);

/* The correlations of THE RULE from wav float32 [B][2C][Ls], ONE launch.
 *
 * Geometry: a workgroup of 256 threads takes one pair of signals of one utterance and 256 consecutive lags, one
 * lag per lane.  It runs over the samples in tiles of 1024: a tile of the first signal and the 1024 + 256 samples
 * of the second that the 256 lags reach are staged in LDS as float64 (zero outside the signal), and every lane
 * runs over the tile with four accumulators in rotation.  No atomics: two launches agree bit for bit.  The
 * mirrored halves of R are written by the lane that computed the value.
 * B in 1..DANET_BSS_MAX_BATCH; C in 1..DANET_BSS_MAX_C; 1 <= Ls < 2^31; L in 1..DANET_BSS_MAX_L (L > Ls is
 * allowed: the lags beyond the signal are 0); wav 4-byte, R, D, ee 8-byte aligned.  A violation returns
 * DANET_BSS_ERR_ARG and launches nothing.                                                                      */
int danet_bss_xcorr(void* stream, int B, int C, int64_t Ls, int L, const float* wav, double* R, double* D,
                    double* ee);

/* G, Gs, Xg and Xs of THE RULE from R and D, ONE launch: copies and the ascending-k sums of the baseline row, the
 * identity rows and columns and the zero right-hand sides of a silent reference included.  Same envelope as
 * danet_bss_workspace_bytes; every pointer 8-byte aligned.                                                    */
int danet_bss_systems(void* stream, int B, int C, int L, const double* R, const double* D, double* G, double* Gs,
                      double* Xg, double* Xs);

/* Batched float64 Cholesky solve, in place, no pivoting: for every m < nmat, A[m] (n x n, row-major, symmetric
 * positive definite; only its lower triangle is read) is overwritten by its factor -- L in the lower triangle, and
 * L^T of every finished panel in the rows above it -- and the nrhs rows of X[m] ([nrhs][n], one right-hand side
 * per row) by the solutions of A[m] x = b.  flags[m] = 1 when a pivot was not a positive finite number (the rest
 * of that matrix is then meaningless, and no other matrix is touched by it), else 0.
 *
 * Geometry: right-looking, blocked by DANET_BSS_BLOCK = 64 columns.  Per panel three launches over ALL matrices of
 * the batch: the 64 x 64 diagonal block is factored in LDS by one workgroup per matrix; the rows below it are
 * solved against it, one wave per (matrix, 64 rows), which also stores the transposed copy; the trailing update
 * A_ij -= L_ik L_jk^T runs on one workgroup per (matrix, 64 x 64 tile of the lower triangle) with
 * v_mfma_f64_16x16x4_f64, the two 64 x 32 panel slabs staged in LDS -- so the update of the whole batch is
 * spread over the whole GPU.  A last panel narrower than 64 and tiles that reach beyond n are handled by zero
 * fill on load and a bound on store.  Then ONE launch, a workgroup per (matrix, right-hand side), does the two
 * triangular solves block by block: a 256-thread coalesced sweep over the finished part, the four partial sums
 * joined as (p0 + p1) + (p2 + p3), and a 64-lane substitution through the diagonal block.
 * 1 <= nmat <= DANET_BSS_MAX_BATCH; 1 <= n <= DANET_BSS_MAX_N; 1 <= nrhs <= DANET_BSS_MAX_RHS; A, X 8-byte,
 * flags 4-byte aligned.  A violation returns DANET_BSS_ERR_ARG and launches nothing.                           */
int danet_bss_chol_solve(void* stream, int nmat, int n, int nrhs, double* A, double* X, int32_t* flags);

/* The decibels of THE RULE, ONE launch of one workgroup of 1024 threads: from the correlations, the right-hand
 * sides D, the solutions Xg, Xs and the factorisation flags fg, fs of B utterances it writes rows b0 .. b0 + B - 1
 * of per_utt [B_all][4], perm_idx [B_all] and flags [B_all]; when b0 + B = B_all it then writes mean4 from ALL
 * B_all rows (the rows of the groups before were written by earlier calls on the same stream), so the batch
 * means do not depend on how the batch was cut into groups.  A dot product is taken by one wave: lane l adds the
 * terms l, l + 64, ... in order, the lanes join in a fixed butterfly.  The batch sums: thread t adds the
 * utterances t, t + 1024, ... in order, the same butterfly, and the sixteen waves join pairwise in order.
 * B >= 1, b0 >= 0, b0 + B <= B_all <= DANET_BSS_MAX_BATCH; C, L as above; fg, fs, perm_idx, flags 4-byte, all
 * else 8-byte aligned.  A violation returns DANET_BSS_ERR_ARG and launches nothing.                            */
int danet_bss_finalize(void* stream, int B, int C, int L, const double* R, const double* D, const double* ee,
                       const double* Xg, const double* Xs, const int32_t* fg, const int32_t* fs, int b0, int B_all,
                       double* per_utt, int32_t* perm_idx, int32_t* flags, double* mean4);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_BSS_HIP_H */
