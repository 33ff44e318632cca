// eaqhm_cepstrum_fit.inc — the body of eaqhm_model_cepstrum_kernel and of its warped sibling (DESIGN.md §9.5, §9.8),
// included once by each with CEP_WARPED 0 or 1: the warped kernel has one more argument, cep_a, and stages its nodes at
// Omega_a(w_n).  Text inclusion and not a template: the compiler places a shared inlined body differently, and the
// unwarped kernel keeps its machine code this way (tools/isa_diff.py).
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * CEP_WAVES + w);   // one wave per instant: scalar
  if (i >= No_ti) return;   // the waves of a block share no data: no block barrier below
  const int n = P + 1, LS = cep_stride(P);
  double* sw = lds + (size_t)w * cep_wave_doubles(K, P);
  double* sv = sw + K;
  double* T = sv + K;
  double* A = T + (2 * P + 2);
  const double* row = records + (size_t)i * (3 * K + 1);
  double* out = ceps + (size_t)i * n;

  // ---- 1. the nodes: the active slots (am != 0, f > 0) in slot order
  int nn = 0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    const bool act = k < K && row[k] != 0.0 && row[K + k] > 0.0;
    const unsigned long long m = __ballot(act);
    if (act) {
      const int p = nn + __popcll(m & ((1ull << lane) - 1ull));
#if CEP_WARPED
      sw[p] = cep_omega(cep_a, ((2.0 * M_PI) * row[K + k]) / fs);
#else
      sw[p] = ((2.0 * M_PI) * row[K + k]) / fs;
#endif
      sv[p] = log(row[k]);
    }
    nn += __popcll(m);
  }
  if (nn == 0) {   // an empty instant: -inf, 0, .., 0
    if (lane < n) out[lane] = lane == 0 ? -INFINITY : 0.0;
    return;
  }
  __builtin_amdgcn_wave_barrier();

  // ---- 2. T_d = sum_n cos(d w_n), d = 0..2P, and b_p = sum_n v_n m_p(w_n), p = 0..P: lanes over d, every lane walks
  // the nodes (one LDS address for the wave: a broadcast).  Each cosine is taken at d w_n itself, so there is no
  // phasor to drift.  d <= P <= 63 falls in the first round: b_r ends up in lane r, the owner of row r.
  double b = 0.0;
  for (int d = lane; d <= 2 * P; d += 64) {
    const double dd = (double)d;
    double t = 0.0, bv = 0.0;
    for (int q = 0; q < nn; ++q) {
      const double c = cos(dd * sw[q]);
      t += c;
      bv += sv[q] * c;
    }
    T[d] = t;
    if (d <= P) b = d == 0 ? bv : 2.0 * bv;
  }
  __builtin_amdgcn_wave_barrier();

  // ---- 3. Cholesky G = L L^T, column by column (left-looking): lane r >= j forms G_rj - sum_{k<j} L_rk L_jk from its
  // own row and row j (a broadcast); the pivot comes from lane j.  A pivot that is not finite or not > 0 ends the fit
  // with a NaN row.
  const int r = lane;
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    if (r >= j && r < n) {
      s = cep_gram(T, r, j, lam);
      for (int k = 0; k < j; ++k) s -= A[r * LS + k] * A[j * LS + k];
    }
    const double piv = cep_lane(s, j);
    if (!(piv > 0.0) || !(piv < INFINITY)) { bad = true; break; }   // wave-uniform
    const double dj = sqrt(piv);
    if (r >= j && r < n) A[r * LS + j] = r == j ? dj : s / dj;
    __builtin_amdgcn_wave_barrier();
  }
  if (bad) {
    if (r < n) out[r] = NAN;
    return;
  }
  // forward: L y = b, column by column; lane j keeps y_j
  double y = b;
  for (int j = 0; j < n; ++j) {
    const double yj = cep_lane(y, j) / A[j * LS + j];
    if (r == j) y = yj;
    else if (r > j && r < n) y -= A[r * LS + j] * yj;
  }
  // backward: L^T c = y; lane r < j reads L_jr along row j (consecutive addresses)
  for (int j = n - 1; j >= 0; --j) {
    const double cj = cep_lane(y, j) / A[j * LS + j];
    if (r == j) y = cj;
    else if (r < j) y -= A[j * LS + r] * cj;
  }
  if (r < n) out[r] = y;
