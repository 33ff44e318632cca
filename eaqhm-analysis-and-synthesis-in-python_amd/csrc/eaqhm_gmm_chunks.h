// eaqhm_gmm_chunks.h — the row chunks of the mixture's M-step, shared with the k-means update (eaqhm_gmm.hip,
// eaqhm_kmeans.hip): a function of N alone, so that sums over chunks come out in the same order on every device.
#pragma once

namespace eaqhm {

typedef long long i64;

constexpr int GMM_ROWS = 64;     // rows of a block's tile: four waves, one 16-row MFMA tile each
constexpr int GMM_CHUNK_MIN = 512;    // rows of an M-step chunk at least
constexpr int GMM_CHUNKS_MAX = 128;   // chunks at most: N = 10^6, M = 64, D = 128 needs 128 x 64 x 45 tiles = 755 MB

// the M-step's chunking: a function of N only (and through the tile count of (D, M) for the size of `work`)
__host__ __device__ inline i64 gmm_chunk_rows(i64 N) {
  const i64 per = (N + GMM_CHUNKS_MAX - 1) / GMM_CHUNKS_MAX;
  const i64 r = (per + GMM_ROWS - 1) / GMM_ROWS * GMM_ROWS;
  return r > GMM_CHUNK_MIN ? r : GMM_CHUNK_MIN;
}
}  // namespace eaqhm
