// eaqhm_noise_from_cepstrum.inc — the body of eaqhm_noise_from_cepstrum_kernel and of its warped sibling (DESIGN.md
// §10.4, §9.8), included once by each with CEP_WARPED 0 or 1; text inclusion keeps the unwarped kernel's machine code as
// it was (tools/isa_diff.py).  The warped kernel has one more argument, cep_a: its row lies on the all-pass warped axis,
// so Clenshaw runs from cos Omega_a(w_t) = (v - u)(v + u) / (u^2 + v^2), u = (1 + a) sin(w_t / 2), v = (1 - a) cos(w_t / 2),
// taken at the half angle itself (one sincospi per cell beside the Q steps of the recurrence: the table's cos w_t would
// lose the stretched band to cancellation at |a| near 0.9).  The lag sums and the recursion read the table as before.
  __shared__ double tab[NW_M + 1];
  __shared__ double Pw[NW_WAVES][NW_M + 2];
  __shared__ double cw[NW_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NW_WAVES + wave;
  const bool live = m < Nf;
  for (int j = threadIdx.x; j <= NW_M; j += 64 * NW_WAVES) tab[j] = cospi((double)j / (double)NW_M);
  const double cl = (live && lane <= Q) ? ceps[(size_t)m * (Q + 1) + lane] : 0.0;
  double* c = cw[wave];
  double* P = Pw[wave];
  c[lane] = cl;
  const double c0 = __shfl(cl, 0, 64);
  const bool work = live && c0 != -INFINITY;       // uniform over the wave
  __syncthreads();
  if (work) {
    for (int t = lane; t <= NW_M; t += 64) {
#if CEP_WARPED
      double sh, ch;
      sincospi((double)t / (double)(2 * NW_M), &sh, &ch);
      const double u = (1.0 + cep_a) * sh, v = (1.0 - cep_a) * ch;
      const double cw2 = 2.0 * (((v - u) * (v + u)) / (u * u + v * v));
#else
      const double cw2 = 2.0 * tab[t];
#endif
      double b1 = 0.0, b2 = 0.0;
      for (int q = Q; q >= 1; --q) {               // one LDS address for the wave: a broadcast
        const double b0 = c[q] + (cw2 * b1 - b2);
        b2 = b1;
        b1 = b0;
      }
      P[t] = exp(4.0 * (0.5 * cw2 * b1 - b2));
    }
  }
  __syncthreads();
  if (!live) return;
  if (!work) {
    if (lane == 0) sigma_out[m] = 0.0;
    if (lane >= 1 && lane <= p) refl_out[(size_t)m * p + (lane - 1)] = 0.0;
    return;
  }

  // r[l] on lane l, as in noise_warp_frame
  auto ct = [&](int t) {
    const int idx = (lane * t) & (2 * NW_M - 1);
    return tab[idx > NW_M ? 2 * NW_M - idx : idx];
  };
  double r0 = 0.5 * P[0], r1 = 0.0, r2 = 0.0, r3 = ((lane & 1) ? -0.5 : 0.5) * P[NW_M];
  for (int t = 1; t + 3 < NW_M; t += 4) {
    r0 = fma(P[t], ct(t), r0);
    r1 = fma(P[t + 1], ct(t + 1), r1);
    r2 = fma(P[t + 2], ct(t + 2), r2);
    r3 = fma(P[t + 3], ct(t + 3), r3);
  }
  r0 = fma(P[NW_M - 3], ct(NW_M - 3), r0);
  r1 = fma(P[NW_M - 2], ct(NW_M - 2), r1);
  r2 = fma(P[NW_M - 1], ct(NW_M - 1), r2);
  const double r = ((r0 + r1) + (r2 + r3)) / (double)NW_M;

  double kk = 0.0;
  const double E = levinson_lanes<false>(r, p, lane, kk);
  if (lane == 0) sigma_out[m] = exp(c0) * sqrt(E);
  if (lane >= 1 && lane <= p) refl_out[(size_t)m * p + (lane - 1)] = kk;
