/*
 * libdanet_stoi_hip.so -- C ABI of the intelligibility figures of `valid` / `test` (EVAL_STOI): STOI, its extended
 * form ESTOI, and the improvement of each over the unprocessed mixture, in five stages whose outputs can each be
 * read back: resampling to 10 kHz, silent frames, one-third-octave band magnitudes, 30-frame segments, finalize.
 * gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the ABIs of the other sixteen libraries stay as they are.
 * Same conventions as include/danet_bss_hip.h: caller-owned DEVICE pointers (one HOST pointer, named below),
 * fp32 / float64 / int32, `stream` a hipStream_t passed as void*, 0 = DANET_STOI_OK and negative = error with a
 * thread-local message in danet_stoi_last_error(), asynchronous launches, no process environment read, no
 * allocation; every argument error returns before any launch; what the device alone can see (the frame counts M and
 * the frame indices k) is clamped before it moves a read or a write; every value is written with ordinary vector
 * stores; no atomics, so two calls agree bit for bit and an utterance's figures do not depend on its company.  The
 * library holds no transcendental math: the resampling table, the window, the twiddle factors and the band bins are
 * inputs, and 1 + 10^(15/20) is written out below.
 *
 * THE RULE.
 *
 * Signals.  wav[b] of danet_metric_synth: float32 [2C][Ls], the C references s_i first, then the C UNPERMUTED
 * estimates e_j, each Ls = (T - 1) * S samples.  A last row is the mixture m[n] = s_0[n] + s_1[n] + ..., summed in
 * float32 in that order.
 *
 * 1. Resample to 10 kHz.  g = gcd(10000, SMPRATE), U = 10000 / g, D = SMPRATE / g, H = 10 max(U, D),
 *    h = U * firwin(2H + 1, 1 / max(U, D), window = ('kaiser', 5.0)) rounded once to float32, L10 = ceil(Ls U / D),
 *        y[n] = sum_k h[n D + H - k U] x[k]   over the k with 0 <= k < Ls and 0 <= n D + H - k U <= 2H,
 *    which is scipy.signal.resample_poly(x, U, D).  Products are float64 and exact, the sum is float64 in ascending
 *    k, y[n] is rounded once to float32.  With U = D = 1 the stage is a copy: H = 0 and h = {1}.
 *
 * 2. Silent frames, per reference i.  Frames of 256 samples, hop 128: nf = floor((L10 - 256) / 128) + 1, none when
 *    L10 < 256.  w = hanning(258)[1:-1] as float32.  E_f = sum_n (w[n] x[128 f + n])^2, products and sums float64
 *    over a fixed tree (lane l of a wave adds (v_l^2 + v_(l+64)^2) + (v_(l+128)^2 + v_(l+192)^2), the 64 lanes join
 *    in a butterfly).  Frame f is kept iff E_f > 1e-4 * max_f E_f (40 dB under the loudest frame);
 *    k(0) < k(1) < ... < k(M - 1) are the kept frames.  M belongs to reference i and is applied to every signal
 *    paired with it.
 *
 * 3. Compaction and bands.  For every signal z paired with reference i -- s_i itself, every e_j, and m --
 *    compacted frame q is c_q[n] = w[n] z[128 k(q) + n] plus the overlapping halves of its neighbours:
 *    w[n + 128] z[128 k(q - 1) + n + 128] for n < 128 when q > 0, and w[n - 128] z[128 k(q + 1) + n - 128] for
 *    n >= 128 when q < M - 1: the overlap-add of the kept windowed frames re-framed at the same hop, as a gather.
 *    Z_q = FFT_512(w * c_q zero-padded), 257 bins, float64.  Fifteen one-third-octave bands from 150 Hz: band b sums
 *    |Z_q|^2 over the bins [lo_b, hi_b) in ascending order, lo_b / hi_b the bins nearest to 150 * 2^((2b - 1) / 6)
 *    and 150 * 2^((2b + 1) / 6) on the grid 10000 k / 512:
 *        {7, 9} {9, 11} {11, 14} {14, 17} {17, 22} {22, 27} {27, 34} {34, 43} {43, 55} {55, 69} {69, 87} {87, 109}
 *        {109, 138} {138, 174} {174, 219}
 *    and T[b, q] = sqrt(sum).
 *
 * 4. Segments.  For q = 29 .. M - 1, X and Y are the 15 x 30 blocks of the reference and of the other signal that
 *    end at frame q.
 *    STOI: per band row, alpha = |X_b| / |Y_b|, Y'_b = min(alpha Y_b, 6.623413251903491 X_b) (= 1 + 10^(15/20)),
 *    d_q = the mean over the 15 rows of the correlation coefficient of X_b and Y'_b.
 *    ESTOI: both blocks have every row mean-removed and scaled to unit norm, then every column mean-removed over the
 *    15 bands and scaled to unit norm; d_q = (1 / 30) sum X Y.
 *    A zero norm anywhere makes that row or column contribute 0; there is no epsilon.  The figure of a pair is the
 *    mean of d_q over its M - 29 segments, all in float64: thread t adds the segments t, t + 256, ... in order, the
 *    lanes of a wave join in a butterfly and the four waves as (p0 + p1) + (p2 + p3).
 *
 * 5. Finalize.  A reference whose frames all have E_f = 0 (nf >= 1) is silent and takes no part.  An utterance in
 *    which some live reference has M < 30 is flagged: it reports (0, 0, 0, 0), perm_idx 0, and is left out of the
 *    batch means.  flags[b]: bit 0 = a live reference has M < 30, bit 1 = no reference is live.  The permutation p
 *    maximises sum_i STOI(i, p(i)) over the live references (added in ascending i); ties go to the first in
 *    itertools.permutations(range(C)) order; ESTOI is reported under that same pairing.  Per utterance
 *    (STOI, ESTOI, STOIi, ESTOIi) = the means over the live references of STOI(i, p(i)), ESTOI(i, p(i)),
 *    STOI(i, p(i)) - STOI(i, m) and ESTOI(i, p(i)) - ESTOI(i, m), m the mixture taken as the estimate.  Per batch:
 *    the means over the utterances with flags = 0 (0 if there is none) and their count.
 */
#ifndef DANET_STOI_HIP_H
#define DANET_STOI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/stoi/exports.map: exactly the entry
 * points declared between this push and the pop are exported.                                 */
#pragma GCC visibility push(default)

#define DANET_STOI_ABI_VERSION 1

#define DANET_STOI_OK 0
#define DANET_STOI_ERR_ARG (-1)     /* bad shape / null or misaligned pointer */
#define DANET_STOI_ERR_LAUNCH (-2)  /* hipLaunch failure                      */

#define DANET_STOI_MAX_C 4          /* 24 permutations at the most                              */
#define DANET_STOI_MAX_BATCH 16383  /* utterances of one call                                   */
#define DANET_STOI_MAX_TABLE 16384  /* entries of the resampling table: 2H + 1 <= this          */
#define DANET_STOI_FRAME 256
#define DANET_STOI_HOP 128
#define DANET_STOI_BANDS 15
#define DANET_STOI_SEG 30

int danet_stoi_abi_version(void);
const char* danet_stoi_last_error(void);

/* Bytes of one buffer that holds everything the entry points write for B utterances, each part at a multiple of
 * 256 bytes, in this order (L10 = ceil(Ls U / D), nf as in THE RULE, nfp = max(nf, 1)):
 *     sig      float32 [B][2C + 1][L10]        the 10 kHz rows: references, estimates, mixture
 *     E        float64 [B][C][nfp]             frame energies of the references
 *     mask     int32   [B][C][nfp]             1 = kept
 *     kidx     int32   [B][C][nfp]             k(q) for q < M, 0 behind
 *     M        int32   [B][C]
 *     Emax     float64 [B][C]                  max_f E_f (0 without a frame)
 *     T        float64 [B][C][C + 2][15][nfp]  band magnitudes; signal 0 = s_i, 1 + j = e_j, C + 1 = m; 0 for q >= M
 *     d        float64 [B][C][C + 1][2]        (STOI, ESTOI) of reference i against e_j (j < C) and m (j = C)
 *     per_utt  float64 [B][4]
 *     perm_idx int32   [B]
 *     flags    int32   [B]
 *     mean4    float64 [4]
 *     count    int32   [1]
 * (size_t)-1 for B outside 1..DANET_STOI_MAX_BATCH, C outside 1..DANET_STOI_MAX_C, Ls or L10 outside [1, 2^31), or
 * (U, D) not coprime positive integers with 2H + 1 <= DANET_STOI_MAX_TABLE.                                    */
size_t danet_stoi_workspace_bytes(int B, int C, int64_t Ls, int U, int D);

/* Stage 1, ONE launch: wav float32 [B][2C][Ls] -> sig float32 [B][2C + 1][L10], the mixture row formed while its
 * span is loaded.  h: float32 [2H + 1] (H = 10 max(U, D); U = D = 1: H = 0, one entry).
 *
 * Geometry: a workgroup of 256 threads takes up to 256 consecutive outputs of one row.  The whole table and the
 * input span those outputs reach are staged in LDS -- the span with 16-byte loads wherever the row is 16-byte
 * aligned and inside [0, Ls), zero outside -- then a thread per output runs over its taps.  Fewer outputs per
 * workgroup where 256 of them would reach beyond 80 KiB of staged input.
 * Envelope as danet_stoi_workspace_bytes; wav, sig 4-byte, h 16-byte aligned.  A violation returns
 * DANET_STOI_ERR_ARG and launches nothing.                                                                    */
int danet_stoi_resample(void* stream, int B, int C, int64_t Ls, int U, int D, const float* wav, const float* h,
                        float* sig);

/* Stage 2, ONE launch, a workgroup per reference row: E, mask, kidx, M and Emax of THE RULE from sig.  A wave per
 * frame for the energies; the compaction is a prefix scan over 256 frames at a time (ballot inside a wave, the four
 * waves' counts through LDS).  w: float32 [256].
 * B, C as above; 1 <= L10 < 2^31; sig, w, mask, kidx, M 4-byte, E, Emax 8-byte aligned.                         */
int danet_stoi_frames(void* stream, int B, int C, int64_t L10, const float* sig, const float* w, double* E,
                      int32_t* mask, int32_t* kidx, int32_t* M, double* Emax);

/* Stage 3, ONE launch over the frames of all (b, i, signal): gather, window, 512-point FFT in LDS, 15 band
 * magnitudes -> T.  A wave per frame, four frames per workgroup: the frame is transformed as a 256-point complex
 * FFT of z[j] = c[2j] + i c[2j + 1] (bit-reversed load, four passes of two fused radix-2 stages, one item per lane)
 * plus the split pass, in float64 at an odd LDS pitch of 257; lane b < 15 then sums band b.  tw: float64 [256][2],
 * tw[k] = exp(-2 pi i k / 512).  bands: a HOST pointer to int32 [15][2], {lo_b, hi_b} with 0 <= lo_b <= hi_b <=
 * 257, read before the launch.  M and kidx are clamped to [0, nf] and [0, nf - 1] on the device.  Nothing is
 * launched when L10 < 256.
 * sig, w, kidx, M 4-byte; tw 16-byte; T 8-byte aligned.                                                         */
int danet_stoi_bands(void* stream, int B, int C, int64_t L10, const float* sig, const float* w, const double* tw,
                     const int32_t* bands, const int32_t* kidx, const int32_t* M, double* T);

/* Stage 4, ONE launch, a workgroup per (b, i, j): d of THE RULE from T [B][C][C + 2][15][max(nf, 1)] and M
 * (clamped to [0, nf]); (0, 0) where M < 30.
 * 0 <= nf < 2^24; M 4-byte; T, d 8-byte aligned.                                                                */
int danet_stoi_segments(void* stream, int B, int C, int nf, const double* T, const int32_t* M, double* d);

/* Stage 5, ONE launch of one workgroup of 256 threads: from d, M and Emax of B utterances it writes rows b0 ..
 * b0 + B - 1 of per_utt [B_all][4], perm_idx [B_all] and flags [B_all]; when b0 + B = B_all it then writes mean4
 * and count from ALL B_all rows (the rows of the groups before were written by earlier calls on the same stream),
 * so the batch means do not depend on how the batch was cut into groups.  The batch sums: thread t adds the
 * utterances t, t + 256, ... in order, the lanes of a wave join in a butterfly, the four waves pairwise in order.
 * B >= 1, b0 >= 0, b0 + B <= B_all <= DANET_STOI_MAX_BATCH; M, perm_idx, flags, count 4-byte, all else 8-byte
 * aligned.                                                                                                      */
int danet_stoi_finalize(void* stream, int B, int C, int nf, const double* d, const int32_t* M, const double* Emax,
                        int b0, int B_all, double* per_utt, int32_t* perm_idx, int32_t* flags, double* mean4,
                        int32_t* count);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_STOI_HIP_H */
