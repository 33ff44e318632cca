/* eaqhm_swipe.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the error
 * codes): the three stages of the SWIPE' pitch estimator on the device.  The host forms every small table
 * (eaqhm_amd/pitch.py: swipe_plan) with the NumPy expressions of swipe.py; the kernels do the work per frame, per
 * candidate and per instant.  No atomics, every word has one writer, every reduction has a fixed order: the same bits on
 * every launch.  The entry points do not read the device arrays: finite values are the CALLER'S contract.           */
#ifndef EAQHM_SWIPE_H
#define EAQHM_SWIPE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define EAQHM_SWIPE_WMAX 8192      /* largest window, samples */
#define EAQHM_SWIPE_EMAX 1024      /* ERB points at most */
#define EAQHM_SWIPE_WINDOWS 8      /* window sizes of one pick at most */
#define EAQHM_SWIPE_FINE 64        /* points of a candidate's fine grid at most */

/* SWIPE' (additions under ABI 6) ------------------------------------------------------------------------
 * eaqhm_swipe_loudness: the normalised square-root ERB spectrum of every frame of one window size.
 *   x          double[n]          the signal; frame m is the w samples starting at m hop - pad, and a sample outside
 *                                 [0, n) is an exact zero (no padded copy exists)
 *   w          a power of two, 8 <= w <= 8192; 1 <= hop <= w; 0 <= pad < 2^31; 1 <= nframes < 2^31
 *   window     double[w]          multiplied onto the frame before the transform
 *   fs, sumw2  the one-sided density is |X_k|^2 (x 2 except at DC and Nyquist) / fs / sumw2
 *   lo         int32[nE]          lower bin of ERB point e, clamped by the kernel to [0, w/2 - 1]; the upper is lo + 1
 *   xlo, df    double[nE]         f_e - f[lo] and f[lo + 1] - f[lo]: value = ((P[lo + 1] - P[lo]) / df) xlo + P[lo], each
 *                                 operation rounded once (SciPy's interp1d arithmetic)
 *   L          double[nframes][ld], ld >= nE, 1 <= nE <= 1024: sqrt(max(0, value)) divided by the row's 2-norm; a row
 *                                 whose norm is 0 is exactly zero.  Columns nE .. ld - 1 are not written.
 *   The transform is an in-place radix-4 (last stage radix-2) complex FFT in LDS with the imaginary part zero and twiddles
 *   from FP64 sincospi; one block per frame for w > 256, one wave per frame (four frames a block) below.
 * eaqhm_swipe_scores: Si[cand][nframes] = K[cand][ldk] . L[nframes][ldl]^T over the first nE columns, on
 *   v_mfma_f64_16x16x4_f64, k ascending, one accumulator per output; 1 <= cand <= 4096, 1 <= nE <= 65536,
 *   1 <= nframes < 2^31, ldk >= nE, ldl >= nE; none needs to be a multiple of 4, 16 or 64 (zeros in LDS).
 * eaqhm_swipe_pick: per instant t[i], S_c = sum over the windows covering candidate c of mu (slope (t - ts[lo]) + y[lo])
 *   (windows in index order, each operation rounded once), the FIRST maximum over c, and the parabolic refinement.
 *   Si, mu, tshift   HOST arrays [nwin] of device pointers: Si_v double[ncand_v][nframes_v], mu_v double[ncand_v],
 *                    tshift_v double[nframes_v] ascending
 *   j0, ncand, nframes  HOST arrays [nwin]: window v covers candidates j0_v .. j0_v + ncand_v - 1 of the npc; nframes_v >= 2
 *   t          double[T]          the instants, 1 <= T < 2^31;  3 <= npc <= 65536, 1 <= nwin <= 8
 *   pc0        the pitch returned where the maximum lies on candidate 0 or npc - 1 (with s = S there)
 *   ntc        double[npc][3]     the abscissae of the three neighbouring candidates of c
 *   nftc, ptab double[npc][nfmax] the fine grid of c and the pitch of each of its points; nf int32[npc] its length,
 *                                 clamped by the kernel to [1, nfmax]; 1 <= nfmax <= 64
 *   p, s       double[T]          pitch (READ from ptab at the first maximum of the quadratic on the fine grid) and strength
 *   S          double[npc][T] or NULL: the combined strengths, written only when asked for
 * EAQHM_EINVAL, nothing launched, no output touched, for null pointers and sizes outside the ranges above.            */
int eaqhm_swipe_loudness(eaqhm_ctx* ctx, const double* x, int64_t n, int32_t w, int32_t hop, int64_t pad, int64_t nframes,
                         const double* window, double fs, double sumw2, const int32_t* lo, const double* xlo,
                         const double* df, int32_t nE, double* L, int64_t ld);
int eaqhm_swipe_scores(eaqhm_ctx* ctx, const double* K, int32_t cand, int64_t ldk, const double* L, int64_t nframes,
                       int64_t ldl, int32_t nE, double* Si);
int eaqhm_swipe_pick(eaqhm_ctx* ctx, int32_t nwin, const double* const* Si, const int32_t* j0, const int32_t* ncand,
                     const int64_t* nframes, const double* const* mu, const double* const* tshift, const double* t,
                     int64_t T, int32_t npc, double pc0, const double* ntc, const double* nftc, const double* ptab,
                     const int32_t* nf, int32_t nfmax, double* p, double* s, double* S);

#ifdef __cplusplus
}
#endif
#endif
