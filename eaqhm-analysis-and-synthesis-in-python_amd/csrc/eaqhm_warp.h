// eaqhm_warp.h — the piecewise-linear formant warp: a strictly increasing map W through
// (0, 0) and the breakpoints (x_j, y_j), j = 0..B-1, B <= WARP_BMAX, continued past the last one with the last slope.
// The kernels read its inverse V = W^-1 at an output frequency q:
//   b = min(#{j : y_j <= q}, B - 1),   V(q) = x_{b-1} + (q - y_{b-1}) * ((x_b - x_{b-1}) / (y_b - y_{b-1})),
// x_{-1} = y_{-1} = 0, in exactly this order of operations (tests/formant_warp_ref.py has the same).
// One wave serves one instant / frame, so the row is wave-uniform: warp_stage puts its y_j and the B slope ratios into
// the wave's 2 x WARP_BMAX doubles of LDS once; x is the same for every row and is staged once per block.
// Monotone rows are the caller's contract: a bad row gives wrong numbers (the scan is bounded by B, every index by
// B - 1), never an access outside the tables.
#pragma once

namespace eaqhm {

constexpr int WARP_BMAX = 16;

struct WarpRow {
  const double* wx;   // x_j            [B]  LDS, shared by the block
  const double* wy;   // y_j            [B]  LDS, this wave's
  const double* ws;   // slope ratios   [B]  LDS, this wave's
  int B;
  bool ident;         // the row is x bit for bit: V(q) = q, no arithmetic
};

// the block's copy of x: threads 0..B-1; visible after the next barrier
__device__ inline void warp_stage_x(const double* __restrict__ x, int B, int tid, double* wx) {
  if (tid < B) wx[tid] = x[tid];
}

// the wave's copy of its row and the ratios: lanes 0..B-1; visible after the next barrier.  Returns (wave-uniform)
// whether the row equals x bit for bit (every value is finite and > 0, so == is the comparison of the bits).
__device__ inline bool warp_stage(const double* __restrict__ x, const double* __restrict__ yrow, int B, int lane,
                                  double* wy, double* ws) {
  bool differs = false;
  if (lane < B) {
    const double xl = x[lane], yl = yrow[lane];
    const double xp = lane ? x[lane - 1] : 0.0, yp = lane ? yrow[lane - 1] : 0.0;
    wy[lane] = yl;
    ws[lane] = (xl - xp) / (yl - yp);
    differs = xl != yl;
  }
  return __ballot(differs) == 0ull;
}

__device__ inline double warp_inverse(const WarpRow& W, double q) {
#pragma clang fp contract(off)   // the model's three roundings: no fused multiply-add
  if (W.ident) return q;
  int b = 0;
  for (int j = 0; j < W.B; ++j) b += (W.wy[j] <= q) ? 1 : 0;   // one LDS address for the wave: a broadcast
  b = min(b, W.B - 1);
  const double xp = b ? W.wx[b - 1] : 0.0, yp = b ? W.wy[b - 1] : 0.0;
  return xp + (q - yp) * W.ws[b];
}

}  // namespace eaqhm
