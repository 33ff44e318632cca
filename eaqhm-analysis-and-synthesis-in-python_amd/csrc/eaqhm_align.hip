// eaqhm_align.hip — time alignment of two models: banded DTW over their cepstral rows.  gfx950 (MI355X)
// only, FP64.
//
//   eaqhm_cepstrum_cost_kernel  the local cost d(i, j) of every cell of the band, +inf outside the table
//   eaqhm_dtw_tile_kernel       one wave per 64 x 64 tile of the (i, j) table: the recursion D and the back-pointers
//   eaqhm_dtw_backtrack_kernel  one wave: lane 0 walks the back-pointers, the wave moves the path to the front
//
// The band (§9.6): half-width r rows of B around the scaled diagonal, centre c_i = (2 i (nB-1) + (nA-1)) / (2 (nA-1))
// (64-bit integer division; 0 when nA = 1); cell (i, j) is stored at [i][j - c_i + r], W = 2 r + 1 columns per row.
// The forward pass is one launch per tile anti-diagonal I + J = t on the context's stream: a tile reads what the tiles
// above, left and above-left of it wrote, and those ran in earlier launches.  No workgroup waits on another.
#include "eaqhm_common.h"
#include "eaqhm_wave.h"

namespace eaqhm {

typedef long long i64;

__host__ __device__ inline i64 band_centre(i64 i, int nA, int nB) {
  return nA > 1 ? (2 * i * (i64)(nB - 1) + (i64)(nA - 1)) / (2 * (i64)(nA - 1)) : 0;
}

// ------------------------------------------------------------------------------------------------
// The local cost.  d(i, j) = c0_weight dC_0^2 + 2 sum_{p=1..P} dC_p^2 with dC = CA[i] - CB[j], the differences formed
// directly (every term is >= 0: nothing cancels).  A row whose c_0 is -inf is empty: d = 0 between two empty rows,
// empty_cost between an empty row and any other.
// A block owns COST_ROWS rows of A (in LDS) and walks the B rows its band covers in chunks of 64 (staged in LDS at an
// odd stride, so that the 64 lanes of a wave, one B row each, read 64 different banks at the same p).  Wave w owns
// COST_ROWS / 4 of the A rows: a B value is read once for all of them, the A values are LDS broadcasts.  A chunk's cells
// land in 64 consecutive doubles of a band row.  Chunks are dealt out over gridDim.y.
constexpr int COST_ROWS = 16;
constexpr int COST_Q = COST_ROWS / 4;   // A rows per wave
constexpr int COST_PMAX = 63;

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_cepstrum_cost_kernel(const double* __restrict__ cepsA, int nA, const double* __restrict__ cepsB, int nB, int P,
                               double c0_weight, double empty_cost, int r, double* __restrict__ band) {
  __shared__ double As[COST_ROWS * (COST_PMAX + 1)];
  __shared__ double Bs[64 * (COST_PMAX + 2)];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = P + 1, LS = n | 1;
  const int i0 = blockIdx.x * COST_ROWS;
  const int rows = min(COST_ROWS, nA - i0);
  const i64 W = 2 * (i64)r + 1;
  for (int k = threadIdx.x; k < rows * n; k += 256) As[(k / n) * (COST_PMAX + 1) + k % n] = cepsA[(size_t)i0 * n + k];
  i64 ci[COST_Q];
  bool ea[COST_Q];
  for (int q = 0; q < COST_Q; ++q) ci[q] = band_centre(min(i0 + w * COST_Q + q, nA - 1), nA, nB);
  const i64 jlo = band_centre(i0, nA, nB) - r, jhi = band_centre(i0 + rows - 1, nA, nB) + r;   // the block's B rows
  __syncthreads();
  for (int q = 0; q < COST_Q; ++q) ea[q] = As[(w * COST_Q + q) * (COST_PMAX + 1)] == -INFINITY;
  for (i64 jc = jlo + 64 * (i64)blockIdx.y; jc <= jhi; jc += 64 * (i64)gridDim.y) {
    // rows jc .. jc + 63 of B, those inside the table: one contiguous piece of cepsB
    const i64 b0 = max(jc, (i64)0), b1 = min(jc + 64, (i64)nB);
    for (i64 k = threadIdx.x; k < (b1 - b0) * n; k += 256)
      Bs[(int)(b0 - jc + k / n) * LS + (int)(k % n)] = cepsB[(size_t)b0 * n + k];
    __syncthreads();
    const i64 j = jc + lane;
    const bool inside = j >= 0 && j < nB;
    double acc[COST_Q] = {}, d0[COST_Q];
    if (inside) {
      const double* b = Bs + lane * LS;
      const double bz = b[0];
      for (int q = 0; q < COST_Q; ++q) {
        acc[q] = 0.0;
        d0[q] = As[(w * COST_Q + q) * (COST_PMAX + 1)] - bz;
      }
      for (int p = 1; p <= P; ++p) {
        const double bp = b[p];
        for (int q = 0; q < COST_Q; ++q) {
          const double d = As[(w * COST_Q + q) * (COST_PMAX + 1) + p] - bp;
          acc[q] += d * d;
        }
      }
      const bool eb = bz == -INFINITY;
      for (int q = 0; q < COST_Q; ++q) {
        const double d = c0_weight * (d0[q] * d0[q]) + 2.0 * acc[q];
        acc[q] = ea[q] && eb ? 0.0 : ea[q] || eb ? empty_cost : d;
      }
    }
    for (int q = 0; q < COST_Q; ++q) {
      const int i = i0 + w * COST_Q + q;
      const i64 col = j - ci[q] + r;
      if (i < nA && col >= 0 && col < W) band[(size_t)i * (size_t)W + (size_t)col] = inside ? acc[q] : INFINITY;
    }
    __syncthreads();   // Bs is staged again
  }
}

// ------------------------------------------------------------------------------------------------
// The recursion.  D(0,0) = d(0,0); D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)), predecessors outside the
// table or the band count +inf.  Codes: 0 diagonal, 1 from (i-1,j), 2 from (i,j-1), 3 the start; on equal values the
// lower code wins (a later candidate replaces the current one only when strictly smaller).
//
// One wave per tile (block = one wave).  The tile's d go to LDS (cells outside the band or the table: +inf, which the
// recursion carries without a special case: inf + x = inf for x >= 0).  Lane l owns tile row l and sweeps the 127
// anti-diagonals: at step s it is at column s - l.  Its left neighbour value is its own last result; the value above
// is lane l-1's last result, shifted in by DPP; the diagonal one is the value above of the step before.  Lane 0 reads
// the row above the tile (loaded one value per lane) by v_readlane at the step's index; the column left of the tile
// seeds `left` and, shifted by one lane, `diag`.  LDS row stride 64 doubles: on an anti-diagonal lane l is at
// l * 64 + (s - l) = 63 l + s, an odd stride, so the 64 lanes hit different banks.
__device__ inline double lane_shr1(double x) {   // lane l gets lane l-1's x; lane 0 keeps its own
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

struct BandView {
  int nA, nB, r;
  i64 W;
  // the band index of cell (i, j) with centre c = c_i, or -1 outside the table or the band
  __device__ i64 at(i64 i, i64 j, i64 c) const {
    const i64 col = j - c + r;
    return i >= 0 && i < nA && j >= 0 && j < nB && col >= 0 && col < W ? i * W + col : -1;
  }
};

extern "C" __global__ void __launch_bounds__(64)
    eaqhm_dtw_tile_kernel(double* __restrict__ band, int nA, int nB, int r, int t, int I_first,
                          unsigned char* __restrict__ ptr) {
  __shared__ double Ds[64 * 64];
  __shared__ unsigned char Ps[64 * 64];
  __shared__ i64 cs[64];
  const int lane = threadIdx.x;
  const int I = I_first + blockIdx.x, J = t - I;
  const int i0 = I * 64;
  const i64 j0 = (i64)J * 64;
  const BandView V{nA, nB, r, 2 * (i64)r + 1};
  // a tile wholly outside the band: the rows' intervals [c_i - r, c_i + r] overlap (r admits a path), so their union
  // is [c_first - r, c_last + r]
  const int i_last = min(i0 + 63, nA - 1);
  if (band_centre(i_last, nA, nB) + r < j0 || band_centre(i0, nA, nB) - r > j0 + 63) return;   // block-uniform
  const i64 c_own = band_centre(min(i0 + lane, nA - 1), nA, nB);
  cs[lane] = c_own;
  __syncthreads();
  for (int a = 0; a < 64; ++a) {
    const i64 k = V.at(i0 + a, j0 + lane, cs[a]);
    Ds[a * 64 + lane] = k >= 0 ? band[k] : INFINITY;
  }
  // the row above, the column to the left, the corner
  i64 k = I > 0 ? V.at(i0 - 1, j0 + lane, band_centre(i0 - 1, nA, nB)) : -1;
  const double top = k >= 0 ? band[k] : INFINITY;
  k = J > 0 ? V.at(i0 + lane, j0 - 1, c_own) : -1;
  const double leftcol = k >= 0 ? band[k] : INFINITY;
  k = I > 0 && J > 0 ? V.at(i0 - 1, j0 - 1, band_centre(i0 - 1, nA, nB)) : -1;
  const double corner = I == 0 && J == 0 ? 0.0 : k >= 0 ? band[k] : INFINITY;   // 0 ahead of the start: D(0,0) = d + 0
  __syncthreads();

  double left = leftcol, diag = lane_shr1(leftcol), prev = INFINITY;
  if (lane == 0) diag = corner;
  for (int s = 0; s < 127; ++s) {
    double up = lane_shr1(prev);
    const double t_s = wave_lane(top, s & 63);
    if (lane == 0) up = s < 64 ? t_s : INFINITY;
    const int jj = s - lane;
    if (jj >= 0 && jj < 64) {
      const double d = Ds[lane * 64 + jj];
      double best = diag;
      int code = 0;
      if (up < best) { best = up; code = 1; }
      if (left < best) { best = left; code = 2; }
      const double v = d + best;
      if (i0 + lane == 0 && j0 + jj == 0) code = 3;
      Ds[lane * 64 + jj] = v;
      Ps[lane * 64 + jj] = (unsigned char)code;
      left = v;
      diag = up;
      prev = v;
    }
  }
  __syncthreads();
  for (int a = 0; a < 64; ++a) {   // only cells of the band inside the table are written
    const i64 q = V.at(i0 + a, j0 + lane, cs[a]);
    if (q >= 0) {
      band[q] = Ds[a * 64 + lane];
      ptr[q] = Ps[a * 64 + lane];
    }
  }
}

// The backtrack: lane 0 walks from (nA-1, nB-1) to (0, 0), at most nA + nB - 1 cells, and writes them from the end of
// `path` backwards; then the wave moves the L pairs to the front, 64 at a time (the destination lies below the source,
// and a chunk's loads are complete before its stores are issued).  A walk that leaves the band or does not end at the
// start gives path_len = -1.
extern "C" __global__ void __launch_bounds__(64)
    eaqhm_dtw_backtrack_kernel(const double* __restrict__ band, int nA, int nB, int r,
                               const unsigned char* __restrict__ ptr, int* __restrict__ path, int* __restrict__ path_len,
                               double* __restrict__ total) {
  __shared__ int len_s;
  const int lane = threadIdx.x;
  const BandView V{nA, nB, r, 2 * (i64)r + 1};
  const i64 cap = (i64)nA + nB - 1;
  if (lane == 0) {
    i64 i = nA - 1, j = nB - 1, n = 0;
    bool ok = false;
    const i64 kend = V.at(i, j, band_centre(i, nA, nB));
    *total = kend >= 0 ? band[kend] : INFINITY;
    while (n < cap) {
      const i64 k = V.at(i, j, band_centre(i, nA, nB));
      if (k < 0) break;
      ++n;
      path[2 * (cap - n)] = (int)i;
      path[2 * (cap - n) + 1] = (int)j;
      if (i == 0 && j == 0) { ok = true; break; }
      const int code = ptr[k];
      if (code == 0) { --i; --j; }
      else if (code == 1) --i;
      else if (code == 2) --j;
      else break;
    }
    len_s = ok ? (int)n : -1;
    *path_len = len_s;
  }
  __syncthreads();
  const i64 L = len_s, off = cap - L;
  if (L < 0 || off == 0) return;
  const int2* src = reinterpret_cast<const int2*>(path) + off;
  int2* dst = reinterpret_cast<int2*>(path);
  for (i64 k0 = 0; k0 < L; k0 += 64) {
    int2 v = make_int2(0, 0);
    if (k0 + lane < L) v = src[k0 + lane];
    __syncthreads();   // every load of the chunk has returned
    if (k0 + lane < L) dst[k0 + lane] = v;
    __syncthreads();
  }
}
}  // namespace eaqhm

using namespace eaqhm;

static const int ALIGN_NMAX = 1 << 30;   // nA + nB - 1 and 2 r + 1 stay below 2^31

// the smallest half-width that admits a path
static i64 band_min_radius(int nA, int nB) {
  return nA == 1 ? (i64)nB - 1 : ((i64)nB - 1 + (nA - 2)) / ((i64)nA - 1);
}

static bool band_ok(int nA, int nB, int r) {
  return nA >= 1 && nB >= 1 && nA <= ALIGN_NMAX && nB <= ALIGN_NMAX && r >= 0 && r < ALIGN_NMAX &&
         (i64)r >= band_min_radius(nA, nB);
}

extern "C" int eaqhm_cepstrum_cost(eaqhm_ctx* ctx, const double* cepsA, int32_t nA, const double* cepsB, int32_t nB,
                                   int32_t order, double c0_weight, double empty_cost, int32_t r, double* band_out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!cepsA || !cepsB || !band_out) return ctx->fail(EAQHM_EINVAL, "eaqhm_cepstrum_cost: bad argument");
  if (order < 1 || order > COST_PMAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_cepstrum_cost: need 1 <= order <= 63");
  if (!std::isfinite(c0_weight) || c0_weight < 0.0 || !std::isfinite(empty_cost) || empty_cost < 0.0)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_cepstrum_cost: c0_weight and empty_cost must be finite and >= 0");
  if (!band_ok(nA, nB, r))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_cepstrum_cost: need nA, nB >= 1 and a half-width r that admits a path");
  const unsigned tiles = (unsigned)((nA + COST_ROWS - 1) / COST_ROWS);
  // chunks of 64 B rows a block walks: its band rows span at most W + the centres' advance over its A rows
  const i64 span = 2 * (i64)r + 1 + (COST_ROWS - 1) * (band_min_radius(nA, nB) + 1);
  const i64 chunks = (span + 63) / 64;
  const i64 want = (1024 + tiles - 1) / tiles;   // about four blocks per CU where the table is short and wide
  const unsigned gy = (unsigned)std::max<i64>(1, std::min<i64>(std::min<i64>(chunks, want), 65535));
  hipLaunchKernelGGL(eaqhm_cepstrum_cost_kernel, dim3(tiles, gy), dim3(256), 0, ctx->stream, cepsA, (int)nA, cepsB,
                     (int)nB, (int)order, c0_weight, empty_cost, (int)r, band_out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_dtw(eaqhm_ctx* ctx, double* band, int32_t nA, int32_t nB, int32_t r, uint8_t* ptr, int32_t* path,
                         int32_t* path_len, double* total) {
  if (!ctx) return EAQHM_EINVAL;
  if (!band || !ptr || !path || !path_len || !total) return ctx->fail(EAQHM_EINVAL, "eaqhm_dtw: bad argument");
  if (!band_ok(nA, nB, r))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_dtw: need nA, nB >= 1 and a half-width r that admits a path");
  const int TI = (nA + 63) / 64, TJ = (nB + 63) / 64;
  // tile (I, t - I) meets the band iff c_last(I) + r >= 64 (t - I) and c_first(I) - r <= 64 (t - I) + 63.  Both left
  // sides minus their right sides grow with I, so the tiles of an anti-diagonal that meet the band are one run of I.
  auto reaches = [&](int I, int t) {
    return band_centre(std::min(64 * (i64)I + 63, (i64)nA - 1), nA, nB) + r >= 64 * (i64)(t - I);
  };
  auto not_past = [&](int I, int t) { return band_centre(64 * (i64)I, nA, nB) - r <= 64 * (i64)(t - I) + 63; };
  for (int t = 0; t < TI + TJ - 1 && ctx->dtw_phases != 2; ++t) {   // stream order is the only order between tiles
    int lo = std::max(0, t - (TJ - 1)), hi = std::min(t, TI - 1);
    int a = lo, b = hi + 1;   // the first I that reaches the band
    while (a < b) {
      const int m = a + (b - a) / 2;
      if (reaches(m, t)) b = m; else a = m + 1;
    }
    const int I_first = a;
    a = lo - 1, b = hi;       // the last I not past it
    while (a < b) {
      const int m = a + (b - a + 1) / 2;
      if (not_past(m, t)) a = m; else b = m - 1;
    }
    const int I_last = a;
    if (I_first > I_last) continue;
    hipLaunchKernelGGL(eaqhm_dtw_tile_kernel, dim3((unsigned)(I_last - I_first + 1)), dim3(64), 0, ctx->stream, band,
                       (int)nA, (int)nB, (int)r, t, I_first, ptr);
  }
  if (ctx->dtw_phases != 1)
    hipLaunchKernelGGL(eaqhm_dtw_backtrack_kernel, dim3(1), dim3(64), 0, ctx->stream, band, (int)nA, (int)nB, (int)r,
                       ptr, path, path_len, total);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
