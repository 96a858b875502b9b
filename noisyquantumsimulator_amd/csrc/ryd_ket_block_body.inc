// ryd_ket_block_body.inc -- the body of ket_block_kernel and of its summary-only twin,
// included textually by both (so that ket_block_kernel compiles exactly as it did when this
// was its own body).  The including kernel provides PROTO, KD, the kernel parameters and
// STATE (false: the amplitude rows are not stored; `st` is NULL and `lds` unread).
  const int64_t gi = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (gi >= n) return;
  const int64_t i = gi;
  const PointP q = load_point<PROTO>(prm, ldp, i);
  const bool valid = point_valid<PROTO>(q, n_steps);
  // |01> block (c01, c0r) and the |11> symmetric block (c11, c+, crr), complex
  double b2r[2] = {1.0, 0.0}, b2i[2] = {0.0, 0.0};
  double b3r[3] = {1.0, 0.0, 0.0}, b3i[3] = {0.0, 0.0, 0.0};
  KetBlocks K;
  K.a = K.dl = K.dt = -1.0;                  // nothing built yet
  bool over_cap = false;
  int nseg_used = 0, nbuild = 0;
  const int nseg = n_segments<PROTO>(n_steps);
  for (int s = 0; s < nseg && valid; ++s) {
    double a, c, sn, dl, dt;
    ket_seg_polar<PROTO>(q, s, n_steps, shape, a, c, sn, dl, dt);
    if (!(dt > 0.0)) continue;               // empty / padding segment: identity
    {                                        // the ket_cheb_kernel's step cap, same bound
      Seg g;
      g.om_re = a;
      g.om_im = 0.0;
      g.dl = dl;
      g.dt = dt;
      double emin, emax;
      h_bounds(g, q.V, q.d1, emin, emax);
      if (!(0.5 * (emax - emin) * dt <= X_CAP)) {
        over_cap = true;
        continue;
      }
    }
    if (!(a == K.a && dl == K.dl && dt == K.dt)) {
      ket_blocks_build(K, a, dl, dt, q.d1, q.V);
      ++nbuild;
    }
    ++nseg_used;
    // frame: w = D^dag b, w <- U w, b = D w  (D = diag(1, e^{i phi}[, e^{2 i phi}]))
    const double c2 = fma(c, c, -sn * sn), s2 = 2.0 * c * sn;
    {
      const double xr = CMUL_RE(b2r[1], b2i[1], c, -sn), xi = CMUL_IM(b2r[1], b2i[1], c, -sn);
      const double yr = CMUL_RE(K.u2[0][0], K.u2[0][1], b2r[0], b2i[0]) +
                        CMUL_RE(K.u2[1][0], K.u2[1][1], xr, xi);
      const double yi = CMUL_IM(K.u2[0][0], K.u2[0][1], b2r[0], b2i[0]) +
                        CMUL_IM(K.u2[1][0], K.u2[1][1], xr, xi);
      const double zr = CMUL_RE(K.u2[1][0], K.u2[1][1], b2r[0], b2i[0]) +
                        CMUL_RE(K.u2[2][0], K.u2[2][1], xr, xi);
      const double zi = CMUL_IM(K.u2[1][0], K.u2[1][1], b2r[0], b2i[0]) +
                        CMUL_IM(K.u2[2][0], K.u2[2][1], xr, xi);
      b2r[0] = yr;
      b2i[0] = yi;
      b2r[1] = CMUL_RE(zr, zi, c, sn);
      b2i[1] = CMUL_IM(zr, zi, c, sn);
    }
    {
      const double wr[3] = {b3r[0], CMUL_RE(b3r[1], b3i[1], c, -sn), CMUL_RE(b3r[2], b3i[2], c2, -s2)};
      const double wi[3] = {b3i[0], CMUL_IM(b3r[1], b3i[1], c, -sn), CMUL_IM(b3r[2], b3i[2], c2, -s2)};
      const int U[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
      double yr[3], yi[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double accr = 0.0, acci = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const double ur = K.u3[U[r][m]][0], ui = K.u3[U[r][m]][1];
          accr = fma(ur, wr[m], fma(-ui, wi[m], accr));
          acci = fma(ur, wi[m], fma(ui, wr[m], acci));
        }
        yr[r] = accr;
        yi[r] = acci;
      }
      b3r[0] = yr[0];
      b3i[0] = yi[0];
      b3r[1] = CMUL_RE(yr[1], yi[1], c, sn);
      b3i[1] = CMUL_IM(yr[1], yi[1], c, sn);
      b3r[2] = CMUL_RE(yr[2], yi[2], c2, s2);
      b3i[2] = CMUL_IM(yr[2], yi[2], c2, s2);
    }
  }
  // rows of the ket layout (2 D doubles per input, D = KD^2, basis KD*a1 + a2; |r-> rows
  // of dim 4 stay zero): input x = 4 i + k
  constexpr int D = KD * KD;
  const double h = 0.70710678118654752440;
  // (input k, basis b) -> amplitude; every other entry is an exact zero
  const double c1r = h * b3r[1], c1i = h * b3i[1];
  if constexpr (STATE) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const int a1 = b / KD, a2 = b % KD;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double re = 0.0, im = 0.0;
        if (k == 0 && b == 0) re = 1.0;                                        // |00>
        if (k == 1 && a1 == 0 && a2 == 1) { re = b2r[0]; im = b2i[0]; }        // |01> -> c01 |01>
        if (k == 1 && a1 == 0 && a2 == 2) { re = b2r[1]; im = b2i[1]; }        //        + c0r |0r>
        if (k == 2 && a1 == 1 && a2 == 0) { re = b2r[0]; im = b2i[0]; }        // |10>: atom-swap mirror
        if (k == 2 && a1 == 2 && a2 == 0) { re = b2r[1]; im = b2i[1]; }
        if (k == 3 && a1 == 1 && a2 == 1) { re = b3r[0]; im = b3i[0]; }        // |11> -> c11 |11>
        if (k == 3 && ((a1 == 1 && a2 == 2) || (a1 == 2 && a2 == 1))) { re = c1r; im = c1i; }   // c+ |+>
        if (k == 3 && a1 == 2 && a2 == 2) { re = b3r[2]; im = b3i[2]; }        //  + crr |rr>
        st[(int64_t)(2 * b) * lds + 4 * i + k] = re;
        st[(int64_t)(2 * b + 1) * lds + 4 * i + k] = im;
      }
    }
  }
  uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
  if (over_cap) stat |= RYD_STATUS_STEP_CAP;
  bool fin = true;
#pragma unroll
  for (int e = 0; e < 2; ++e) fin = fin && isfinite(b2r[e]) && isfinite(b2i[e]);
#pragma unroll
  for (int e = 0; e < 3; ++e) fin = fin && isfinite(b3r[e]) && isfinite(b3i[e]);
  if (!fin) stat |= RYD_STATUS_NONFINITE;
  // compute_CZ_fidelity pure branch (RG/simulation.py:483-631), as ket_cheb_kernel
  const double orr[4] = {1.0, b2r[0], b2r[0], b3r[0]}, oii[4] = {0.0, b2i[0], b2i[0], b3i[0]};
  double p[4], ph[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    p[x] = orr[x] * orr[x] + oii[x] * oii[x];
    ph[x] = atan2(oii[x], orr[x]);
  }
  double cp = ph[3] - ph[1] - ph[2] + ph[0];
  cp = cp + M_PI;
  cp = cp - 2.0 * M_PI * floor(cp / (2.0 * M_PI));
  cp = cp - M_PI;
  const double err = fmin(fabs(cp - M_PI), fabs(cp + M_PI));
  const double cerr = cos(err / 2);
  const double pen = cerr * cerr;
  const double avgp = 0.25 * (p[0] + p[1] + p[2] + p[3]);
  const double avgf = 0.25 * (p[0] + p[1] + p[2] + p[3] * pen);
  double nrm11 = 0.0;
#pragma unroll
  for (int e = 0; e < 3; ++e) nrm11 += b3r[e] * b3r[e] + b3i[e] * b3i[e];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    sm[(int64_t)(RYD_S_POP0 + x) * ldm + i] = p[x];
    sm[(int64_t)(RYD_S_OV_RE0 + x) * ldm + i] = orr[x];
    sm[(int64_t)(RYD_S_OV_IM0 + x) * ldm + i] = oii[x];
  }
  sm[(int64_t)RYD_S_AVG_POP * ldm + i] = avgp;
  sm[(int64_t)RYD_S_CTRL_PHASE * ldm + i] = cp;
  sm[(int64_t)RYD_S_PENALTY * ldm + i] = pen;
  sm[(int64_t)RYD_S_AVG_F * ldm + i] = avgf;
  sm[(int64_t)RYD_S_NMV_USEFUL * ldm + i] = (double)nseg_used;     // block segment applications
  sm[(int64_t)RYD_S_NMV_EXEC * ldm + i] = (double)nseg_used;
  sm[(int64_t)RYD_S_TRACE11 * ldm + i] = nrm11;
  sm[(int64_t)RYD_S_NSQUARE * ldm + i] = (double)nbuild;           // propagator builds
  status[i] = stat;
