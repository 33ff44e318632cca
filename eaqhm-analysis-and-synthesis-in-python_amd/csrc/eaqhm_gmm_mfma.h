// eaqhm_gmm_mfma.h — what the mixture's kernels (eaqhm_gmm.hip) and the conditional E-step of the trajectory refinement
// (eaqhm_mlpg_em.hip) share: the 64-row tile, the LDS stride rules and the FP64 MFMA with its 16-lane sum.  gfx950 only.
//
// The MFMA's lane maps (tools/mfma_f64_probe.hip): lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register
// r of lane l is D[(l >> 4) + 4 r][l & 15].
#pragma once
#include "eaqhm_common.h"
#include "eaqhm_gmm_chunks.h"

namespace eaqhm {

typedef double gd4 __attribute__((ext_vector_type(4)));

// LDS row strides in doubles.  "rowk": the 16 lanes of a quarter wave read 16 rows at the same k, the quarters k..k+3:
// a stride = 2 (mod 32) spreads a half wave (the unit of a 64-bit LDS read) over all 64 banks.  "krow": the 16 lanes
// read 16 consecutive doubles of one row, the quarters four consecutive rows: a stride = 16 (mod 32) does the same.
__host__ __device__ inline int gmm_stride_rowk(int d) { return ((d + 31) & ~31) + 2; }
__host__ __device__ inline int gmm_stride_krow(int dp16) { return (dp16 & 16) ? dp16 : dp16 + 16; }
__host__ __device__ inline int gmm_pad16(int d) { return (d + 15) & ~15; }

__device__ inline gd4 gmm_mfma(double a, double b, gd4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// sum over the 16 lanes that share lane >> 4
__device__ inline double gmm_sum16(double x) {
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 8);
  return x;
}
}  // namespace eaqhm
