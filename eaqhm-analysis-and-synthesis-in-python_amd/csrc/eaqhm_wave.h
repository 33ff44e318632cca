// eaqhm_wave.h — what the lanes of one wave (64) hand each other in registers: the one definition of each primitive
// outside the LS headers.  A function whose arithmetic the host models follow rounding by rounding says so itself
// (#pragma clang fp contract(off) at the start of its body, as warp_inverse does in eaqhm_warp.h): it must come out the
// same in a unit that contracts and in one that does not.
#pragma once

namespace eaqhm {

// the sum over the wave in every lane: partner lane ^ 32, 16, .. 1
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// x of lane src, src the same on every lane: two v_readlane, the value lands in scalar registers
__device__ __forceinline__ double wave_lane(double x, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
  return __hiloint2double(hi, lo);
}

// the larger value, the lower index on equal values, over the wave; every lane returns lane 0's answer
__device__ inline void wave_first_max(double& v, int& i) {
  for (int d = 1; d < 64; d <<= 1) {
    const double ov = __shfl_xor(v, d);
    const int oi = __shfl_xor(i, d);
    const bool take = ov > v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
  }
  v = __shfl(v, 0);
  i = __shfl(i, 0);
}

// A(z) of reflection coefficients: lane i holds k_i in kk (lanes 1..p); a_j comes back on lane j (a_0 = 1).  The
// model's step-up operation by operation: a_j += k_i a_{i-j}, j = 1..i, from the old values.
__device__ __forceinline__ double stepup_lanes(double kk, int p, int lane) {
#pragma clang fp contract(off)
  double a = lane == 0 ? 1.0 : 0.0;
  for (int i = 1; i <= p; ++i) {
    const double k = __shfl(kk, i, 64);
    const double ar = __shfl(a, (i - lane) & 63, 64);
    if (lane >= 1 && lane <= i) a += k * ar;
  }
  return a;
}

// The Levinson-Durbin recursion on r[l] of lane l (r[0] > 0): a_j on lane j (a_0 = 1), the reversed vectors by a
// cross-lane read, the sum by a wave reduction.  Leaves k_lane in kk (lanes 1..p; 0 from the stage it stopped at) and
// returns E.  Inflate = false leaves r[0] as it is: the -90 dB white floor that steadies an analysed frame would be the
// whole error of the exact way back from a cepstrum.
template <bool Inflate = true>
__device__ __forceinline__ double levinson_lanes(double r, int p, int lane, double& kk) {
#pragma clang fp contract(off)
  if (Inflate && lane == 0) r *= (1.0 + 1e-9);
  double E = __shfl(r, 0, 64);
  double a = lane == 0 ? 1.0 : 0.0;
  for (int i = 1; i <= p; ++i) {
    const int src = (i - lane) & 63;
    const double rr = __shfl(r, src, 64);
    const double acc = __shfl(wave_sum(lane < i ? a * rr : 0.0), 0, 64);
    const double k = -acc / E;
    if (!(fabs(k) < 1.0)) break;
    const double ar = __shfl(a, src, 64);
    if (lane >= 1 && lane <= i) a += k * ar;      // lane i: 0 + k a_0
    if (lane == i) kk = k;
    E *= (1.0 - k * k);
  }
  return E;
}

}  // namespace eaqhm
