/* eaqhm_onset.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the error
 * codes): the three stages of the transient onset detector on the device.  The host forms the window and
 * the band edges (eaqhm_amd/transient.py: onset_plan) and runs the `wait` rule over the flagged frames; the kernels do the
 * work per frame.  No atomics, every word has one writer, every reduction has a fixed order: the same bits on every
 * launch.  The entry points do not read the device arrays: finite values are the CALLER'S contract.                    */
#ifndef EAQHM_ONSET_H
#define EAQHM_ONSET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define EAQHM_ONSET_WMIN 32        /* smallest window, samples */
#define EAQHM_ONSET_WMAX 2048      /* largest window, samples */
#define EAQHM_ONSET_HOP 4096       /* largest hop, samples */
#define EAQHM_ONSET_BANDS 64       /* bands at most */
#define EAQHM_ONSET_LAG 16         /* largest lag of the flux, frames */
#define EAQHM_ONSET_SPAN 64        /* largest pre_max, post_max, pre_avg, post_avg, frames */

/* Transient onsets (additions under ABI 6) ---------------------------------------------------------------
 * eaqhm_onset_bands: the log band energies of every frame.
 *   x          double[n]          the signal, n >= 1; frame m is the w samples m hop - w/2 .. m hop + w/2 - 1, and a
 *                                 sample outside [0, n) is an exact zero (no padded copy exists)
 *   w          a power of two, 32 <= w <= 2048; 1 <= hop <= 4096; 1 <= nframes < 2^31
 *   window     double[w]          multiplied onto the frame before the transform
 *   inv_sumw2  P_k = (Re X_k^2 + Im X_k^2) inv_sumw2, finite and > 0: the host passes 1 / (sum of the window)^2
 *   k          int32[B + 1]       HOST array, 1 <= B <= 64: band b holds the bins k[b] .. k[b + 1] - 1;
 *                                 0 <= k[0], k[b] < k[b + 1], k[B] <= w/2 + 1
 *   floor      finite and > 0
 *   L          double[nframes][ld], ld >= B: L[m][b] = ln(E + floor), E the sum of P_k over the band with k ascending,
 *                                 one addition after the other from an exact 0.  Columns B .. ld - 1 are not written.
 *   The transform is an in-place radix-4 (last stage radix-2) complex FFT in LDS with the imaginary part zero and twiddles
 *   from FP64 sincospi; one block per frame for w > 256, one wave per frame (four frames a block) below.  A frame's
 *   row depends on its w samples alone, not on its place in the launch.
 * eaqhm_onset_flux: d[m] = (sum over b ascending of max(0, L[m][b] - L[m - lag][b])) / B, one addition after the other
 *   from an exact 0, where m >= lag and whole_lo <= m - lag, m <= whole_hi; an exact 0 elsewhere (an empty range
 *   whole_lo > whole_hi: everywhere).  L double[nframes][ld], ld >= B, 1 <= B <= 64, 1 <= lag <= 16,
 *   1 <= nframes < 2^31; d double[nframes].
 * eaqhm_onset_peaks: flag[m] = 1 where d[m] > 0, no d[j] >= d[m] for j in [m - pre_max, m), no d[j] > d[m] for j in
 *   (m, m + post_max], and d[m] >= s / count + delta with s the sum of d[m - pre_avg .. m + post_avg] in ascending frame
 *   order, one addition after the other from an exact 0; every window is cut at 0 and nframes - 1; 0 elsewhere.
 *   d double[nframes], flag uint8[nframes], 1 <= nframes < 2^31; the four spans in [0, 64]; delta finite and >= 0.
 * EAQHM_EINVAL, nothing launched, no output touched, for null pointers and sizes outside the ranges above.            */
int eaqhm_onset_bands(eaqhm_ctx* ctx, const double* x, int64_t n, int32_t w, int32_t hop, int64_t nframes,
                      const double* window, double inv_sumw2, const int32_t* k, int32_t B, double floor, double* L,
                      int64_t ld);
int eaqhm_onset_flux(eaqhm_ctx* ctx, const double* L, int64_t nframes, int64_t ld, int32_t B, int32_t lag,
                     int64_t whole_lo, int64_t whole_hi, double* d);
int eaqhm_onset_peaks(eaqhm_ctx* ctx, const double* d, int64_t nframes, int32_t pre_max, int32_t post_max,
                      int32_t pre_avg, int32_t post_avg, double delta, uint8_t* flag);

#ifdef __cplusplus
}
#endif
#endif
