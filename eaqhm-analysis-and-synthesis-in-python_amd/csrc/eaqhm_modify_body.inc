// eaqhm_modify_body.inc — the eval kernel body of eaqhm_modify.hip, compiled four times: EAQHM_MODIFY_CURVE 0 gives
// eaqhm_modify_eval_kernel (DESIGN.md §9), 1 gives eaqhm_modify_eval_curve_kernel (§9.1); with EAQHM_MODIFY_SHAPE 1
// they become eaqhm_modify_eval_shape_kernel and eaqhm_modify_eval_curve_shape_kernel (§11).  The time map enters the
// body through the MAP_* macros and the shape-invariant phase term through the SHAPE_* macros (empty without it) that
// eaqhm_modify.hip defines for each variant.  The body is shared as text rather than as an inlined device template
// because inlining reorders the scalar kernel's code and costs it an occupancy step (§9.1).
// No include guard: included once per variant.

// ------------------------------------------------------------------------------------------------
// Block of TBS consecutive output samples x all slots.
//   stage 0  per sample: interval j and offset r (LDS); the shape kernels also the fundamental's phase advance s(n') in
//            cycles (§11).
//   stage 1  one thread per (interval, slot) touching the block: the interval's local phase
//            Psi(u) = R_j + sum_{v=1..u} w(v) - sum_{v=0..u} sin(pi v/D) er, u = 0..D, in the eval kernel's summation
//            order; at each of the block's samples in the interval the phase P0 + beta rho ((1-fr) Psi(u0) + fr Psi(u0+1))
//            goes to X[k][s].  A run's last knot (tau = c_b) is the end u = D of its last interval.  The shape kernels
//            weigh Psi by 1 (§11).
//   stage 2  one thread per (sample, slot group): amplitude, A cos(phase), isolated knots (the shape kernels first add
//            2 pi (k+1) s(n') to the phases of their cells); then one thread per sample adds the slots in slot order
//            and the a0 spline.
#if EAQHM_MODIFY_CURVE && EAQHM_MODIFY_SHAPE
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_modify_eval_curve_shape_kernel(MEvalArgs E, MCurve Cu, MShape Sh, int TBS, int NR) {
#elif EAQHM_MODIFY_SHAPE
extern "C" __global__ void __launch_bounds__(256) eaqhm_modify_eval_shape_kernel(MEvalArgs E, MShape Sh, int TBS, int NR) {
#elif EAQHM_MODIFY_CURVE
extern "C" __global__ void __launch_bounds__(256) eaqhm_modify_eval_curve_kernel(MEvalArgs E, MCurve Cu, int TBS, int NR) {
#else
extern "C" __global__ void __launch_bounds__(256) eaqhm_modify_eval_kernel(MEvalArgs E, int TBS, int NR) {
#endif
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const ModArgs& A = E.M;
  const int D = A.step, K = A.Kmax, TP = TBS + 1;
  double* ft = lds;                                   // D+1
  double* X = lds + ((D + 1 + 1) & ~1);               // [K][TP]
  double* sr = X + (size_t)K * TP;                    // [TBS] r of each sample
  double* crec = sr + TBS;                            // [NR][3K+1]
  double* cmom = crec + (size_t)NR * (3 * K + 1);     // [NR][K+1]
  int* sj = (int*)(cmom + (size_t)NR * (K + 1));      // [TBS] interval of each sample
  unsigned char* ccode = (unsigned char*)(sj + ((TBS + 1) & ~1));   // [NR][K]
  const int tid = threadIdx.x;
  const long long t0 = E.t_lo + (long long)blockIdx.x * TBS;
  const long long t1 = (t0 + TBS < E.t_hi) ? (t0 + TBS) : E.t_hi;
  const int ns = (int)(t1 - t0);
  MAP_INIT
  SHAPE_INIT
  int jfirst, jlast;
  double rdummy;
  MAP_LOCATE(t0, jfirst, rdummy);
  MAP_LOCATE(t1 - 1, jlast, rdummy);
  MAP_BOUND
  // intervals met by the block: one before the first sample's (a run's last knot) up to the last sample's
  const int jlo = max(0, jfirst - 1), jhi = min(A.No_ti - 2, jlast);
  MCache C;
  {
    C.r0 = max(0, jlo - 1);
    C.r1 = min(A.No_ti - 1, jhi + 2);
    if (C.r1 > C.r0 + NR - 1) C.r1 = C.r0 + NR - 1;
    if (C.r1 < C.r0) C.r1 = C.r0 - 1;
    C.rec = crec; C.mom = cmom; C.code = ccode;
    const int nrow = C.r1 - C.r0 + 1, RS = 3 * K + 1;
    for (int q = tid; q < nrow * RS; q += blockDim.x) crec[q] = A.records[(size_t)C.r0 * RS + q];
    for (int q = tid; q < nrow * (K + 1); q += blockDim.x) cmom[q] = A.mom[(size_t)C.r0 * (K + 1) + q];
    for (int q = tid; q < nrow * K; q += blockDim.x) ccode[q] = A.code[(size_t)C.r0 * K + q];
    MAP_STAGE
  }
  for (int u = tid; u <= D; u += blockDim.x) ft[u] = sin(M_PI * (double)u / (double)D);
  for (int s = tid; s < ns; s += blockDim.x) {
    int j; double r;
    MAP_LOCATE(t0 + s, j, r);
    sj[s] = j; sr[s] = r;
    SHAPE_SAMPLE
  }
  __syncthreads();
  MAP_BLOCK_WEIGHT
  // ---- stage 1
  if (jhi >= jlo) {
    const int nint = jhi - jlo + 1;
    const double scale = 2.0 * M_PI / A.fs;
    double S = 0.0;   // sum_{v=0..D} sin(pi v/D), in order
    for (int u = 0; u <= D; ++u) S += ft[u];
    for (int p = tid; p < nint * K; p += blockDim.x) {
      const int jj = p / K, k = p - jj * K, j = jlo + jj;
      CSlot Sl{A, C, k};
      const int cj = Sl.code(j);
      if (cj == 0 || Sl.code(j + 1) == 0) continue;
      // the block's samples in this interval: [sa, sb), plus the run's last knot when j+1 ends the run
      int sa = 0, hi = ns;
      while (sa < hi) { const int mid = (sa + hi) >> 1; if (sj[mid] < j) sa = mid + 1; else hi = mid; }
      int sb = sa;
      while (sb < ns && sj[sb] == j) ++sb;
      const bool ends = Sl.code(j + 2) == 0;
      const int sl = (ends && sb < ns && sj[sb] == j + 1 && sr[sb] == 0.0) ? sb : -1;
      if (sa == sb && sl < 0) continue;
      const FmPiece P = make_piece(Sl, j, cj);
      double w0, acc, emis, Mr;
      interval_close(Sl, P, j, D, scale, w0, acc, emis, Mr);
      // a run's last interval closes its mismatch completely: the model's phase at that knot is the integrated one
      const double er = ends ? emis / S : M_PI * emis / (2.0 * (double)D);
      const double Rj = E.R[(size_t)j * K + k], ph0 = E.P0[(size_t)j * K + k];
      MAP_INTERVAL_WEIGHT
      acc = w0;
      double c = ft[0] * er;
      double prev = MAP_PSI((acc - w0) - c);
      int q = sa;
      // u = 0: samples on the knot itself
      while (q < sb && sr[q] == 0.0) { X[(size_t)k * TP + q] = MAP_OFF + br * prev; ++q; }
      for (int u = 1; u <= D; ++u) {
        acc += scale * P(u);
        c += ft[u] * er;
        const double psi = MAP_PSI((acc - w0) - c);
        while (q < sb) {
          const double rq = sr[q], u0 = floor(rq), fr = rq - u0;
          if ((int)u0 == u - 1 && fr > 0.0) X[(size_t)k * TP + q] = MAP_OFF + br * ((1.0 - fr) * prev + fr * psi);
          else if ((int)u0 == u && fr == 0.0) X[(size_t)k * TP + q] = MAP_OFF + br * psi;
          else break;
          ++q;
        }
        prev = psi;
      }
      if (sl >= 0) X[(size_t)k * TP + sl] = MAP_OFF + br * prev;
    }
  }
  __syncthreads();
  // ---- stage 2
  const int s = tid % TBS, g = tid / TBS, G = blockDim.x / TBS;
  const bool live = s < ns;
  const long long n = t0 + s;
  if (live) {
    const int j = sj[s];
    const double r = sr[s];
    MAP_ISO_RANGE
    SHAPE_ADD
    for (int k = g; k < K; k += G) {
      CSlot Sl{A, C, k};
      auto inrun = [&](int q) { return q >= 0 && q <= A.No_ti - 2 && Sl.code(q) != 0 && Sl.code(q + 1) != 0; };
      double cell = 0.0;
      int jj = -1;
      double rr = r;
      if (inrun(j)) jj = j;
      else if (r == 0.0 && inrun(j - 1)) { jj = j - 1; rr = (double)D; }
      if (jj >= 0) {
        const double a0v = E.amp[(size_t)jj * K + k], a1v = E.amp[(size_t)(jj + 1) * K + k];
        const double Av = ((a1v - a0v) / (double)D) * rr + a0v;
        cell = (Av != 0.0) ? Av * cos(X[(size_t)k * TP + s]) : 0.0;
      }
      for (int i = ilo; i <= ihi; ++i) {   // isolated accepted knots land on the output sample nearest to their image
        if (Sl.code(i) == 1 && MAP_ISO_AT(i))
          cell += E.amp[(size_t)i * K + k] * cos(Sl.ph(i));
      }
      X[(size_t)k * TP + s] = cell;   // this thread is the only reader of the cell
    }
  }
  __syncthreads();
  if (tid < TBS && live) {
    double synth = 0.0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) synth += X[(size_t)k * TP + s];
    const double tau = MAP_TAU;
    int ia = sj[s];
    if (ia > A.No_ti - 2) ia = A.No_ti - 2;
    if (ia < 0) ia = 0;
    CSlot S0{A, C, K};   // column K of mom = the a0 spline; its knots are the last record column
    const int RS = 3 * K + 1;
    const double a0v = spline_piece(S0.recv(ia, RS - 1), S0.recv(ia + 1, RS - 1), S0.mom(ia), S0.mom(ia + 1),
                                    tau - (double)ia * (double)D, (double)D);
    E.out[n] = a0v + 2.0 * synth;
  }
}
