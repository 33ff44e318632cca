// eaqhm_cepstrum_build.inc — the body of eaqhm_model_build_kernel and of its warped sibling (DESIGN.md §9.7, §9.8),
// included once by each with CEP_WARPED 0 or 1 (see eaqhm_cepstrum_fit.inc): the warped kernel has one more argument,
// cep_a, and takes the cell's angle through the rational map and the recurrence in Reinsch's form (cep_axis_angle).
  __shared__ double sc[CEP_WAVES][CEP_PMAX + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * CEP_WAVES + w);   // one wave per instant: scalar
  if (i >= n) return;
  double* c = sc[w];
  if (lane <= P) c[lane] = ceps[(size_t)i * (P + 1) + lane];
  __builtin_amdgcn_wave_barrier();
  const bool rowlive = voiced[i] != 0 && c[0] != -INFINITY;
  const double fi = f0[i], th = theta[i], half = 0.5 * fs;
  double* row = records + (size_t)i * (3 * (size_t)Kmax + 1);
  for (int k0 = 0; k0 < Kmax; k0 += 64) {
    const int k = k0 + lane;
    if (k >= Kmax) break;
    const double h = (double)(k + 1);
    const double fm = __dmul_rn(h, fi);
    double a = 0.0, f = 0.0, ph = 0.0;
    if (rowlive && k < Kcap && fm < half) {
#if CEP_WARPED
      double b1, d1;
      const CepAngle A = cep_axis_angle(cep_axis(cep_a), (M_PI * fm) / fs);
      const double sn = A.sn;
      cep_recur_reinsch(c, P, A, b1, d1);
      a = exp(2.0 * (0.5 * A.dl * b1 + A.sg * d1) + c[0]);
#else
      double sn, cs, b1, b2;
      sincos(((2.0 * M_PI) * fm) / fs, &sn, &cs);
      const double cw2 = 2.0 * cs;
      cep_recur(c, P, cw2, b1, b2);
      a = exp(2.0 * (0.5 * cw2 * b1 - b2) + c[0]);
#endif
      if (a != 0.0) {
        const double hs = __dmul_rn(h, th);           // the product rounded as the definition rounds it, then frac
        double x = __dmul_rn(2.0 * M_PI, hs - floor(hs));
        if (!zero_phase) x += -2.0 * (b1 * sn);
        ph = x - (2.0 * M_PI) * ceil((x - M_PI) / (2.0 * M_PI));   // into (-pi, pi]
        f = fm;
      }
    }
    row[k] = a;
    row[Kmax + k] = f;
    row[2 * Kmax + k] = ph;
  }
  if (lane == 0) row[3 * (size_t)Kmax] = a0[i];
