/* eaqhm_viterbi.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the error
 * codes): the continuous pitch track, a Viterbi decode over the SWIPE' strengths with an optional unvoiced state, and the
 * parabolic refinement along the decoded path.  The recurrence has no product: a maximum, one
 * subtraction and one addition per state and step, every tie decided by rule, so the path is the same bits as a float64
 * restatement on any finite input.  No atomics, every word has one writer, every reduction has a fixed order.  The
 * entry points allocate nothing and do not read the device arrays: finite values are the CALLER'S contract.          */
#ifndef EAQHM_VITERBI_H
#define EAQHM_VITERBI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define EAQHM_VITERBI_TILE 8       /* instants of a time tile: one staged block of S, one row of tilemap */
#define EAQHM_VITERBI_NPC 1024     /* candidates at most */
#define EAQHM_VITERBI_JUMP 256     /* W, the widest step in candidates, at most */

/* The continuous pitch track (additions under ABI 6) -------------------------------------------------
 * States: candidate c in [0, npc), and npc, "unvoiced", which exists only with unvoiced != 0.
 *   D[c, 0] = S[c, 0], U[0] = uv;  for t >= 1
 *   best[c] = max over |c - c'| <= W, 0 <= c' < npc of D[c', t-1] - cost[|c - c'|]: on equal values the smaller |c - c'|,
 *             then the lower c'; with the unvoiced state alt = U[t-1] - vcost replaces it only if alt > best[c]
 *   D[c, t] = best[c] + S[c, t]
 *   U[t]    = ((D[m, t-1] - vcost) > U[t-1] ? D[m, t-1] - vcost : U[t-1]) + uv, m the first maximum of D[., t-1]
 * eaqhm_viterbi_forward: one block walks the T steps.
 *   S          double[npc][T]     3 <= npc <= 1024, 1 <= T < 2^31
 *   cost       double[W + 1]      DEVICE array, finite and >= 0; 0 <= W <= min(npc - 1, 256)
 *   unvoiced   0: no unvoiced state (uv and vcost are not looked at); otherwise uv finite, vcost finite and >= 0
 *   bp         int16[T][npc + 1]  the predecessor of every state at every step; row 0 holds the state itself, and
 *                                 without the unvoiced state column npc holds npc
 *   tilemap    int16[ntiles][npc + 1], ntiles = ceil(T / EAQHM_VITERBI_TILE): the state at instant k TILE from which
 *                                 the state at instant min((k + 1) TILE, T - 1) descends
 *   last       double[npc + 1]    D[., T-1] and U[T-1] (-inf without the unvoiced state)
 * eaqhm_viterbi_backtrack: the end state is the first maximum of last[0 .. npc), or npc if last[npc] is strictly
 *   larger; one lane walks the tile maps and writes q at every tile boundary, then one lane per tile fills its tile
 *   from bp.    q  int32[T], values in [0, npc]
 * eaqhm_viterbi_refine: per instant, c = q[t]: c == npc gives p = s = 0; c == 0 or npc - 1 gives p = pc[c], s = S[c, t];
 *   otherwise eaqhm_swipe_pick's refinement of candidate c (the quadratic through S[c-1 .. c+1, t] on ntc[c], Horner on
 *   nftc[c], the first maximum k, p = ptab[c][k], s that value).  pc double[npc]; ntc, nftc, ptab, nf, nfmax as in
 *   eaqhm_swipe_pick; 1 <= nfmax <= 64; a q outside [0, npc] is read as npc.   p, s  double[T]
 * EAQHM_EINVAL, nothing launched, no output touched, for null pointers and sizes outside the ranges above.            */
int eaqhm_viterbi_forward(eaqhm_ctx* ctx, const double* S, int32_t npc, int64_t T, const double* cost, int32_t W,
                          int32_t unvoiced, double uv, double vcost, int16_t* bp, int16_t* tilemap, double* last);
int eaqhm_viterbi_backtrack(eaqhm_ctx* ctx, const int16_t* bp, const int16_t* tilemap, const double* last, int32_t npc,
                            int64_t T, int32_t* q);
int eaqhm_viterbi_refine(eaqhm_ctx* ctx, const double* S, const int32_t* q, int32_t npc, int64_t T, const double* pc,
                         const double* ntc, const double* nftc, const double* ptab, const int32_t* nf, int32_t nfmax,
                         double* p, double* s);

#ifdef __cplusplus
}
#endif
#endif
