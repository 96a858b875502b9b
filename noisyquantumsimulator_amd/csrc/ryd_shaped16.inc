// ryd_shaped16.inc -- LP shaped (RG/simulation.py:2099-2231, evolve_shaped_pulse), identical
// atoms, on 16-lane DPP rows (round 5).  Included by ryd_engine.hip after ryd_sym16.inc and
// ryd_coh_prop.inc (row_newbcast helpers, cp_wsync).
//
// A shaped pulse changes its amplitude every one of its 2 x 499 segments, so no propagator
// is reused and the state itself is carried through each segment's Chebyshev series
// (x = omega dt ~ 1-10 per segment: ~15-35 terms).  lindblad_cheb_kernel does that with one
// lane per (point, basis input) on the full 25-vector: the stationary |00>, the 5-coordinate
// |01> and |10> and the 15-coordinate |11> triangle all cost 162 FMAs per term, and a C2-sized
// batch fills only 625 waves.  Here one 16-lane row holds a point:
//   lane c < 15 carries |11>'s triangle coordinate c (sym16's layout), lanes c < 5 also
//   |01>'s single-atom coordinate c (|10> is its mirror, |00> stationary);
//   per segment lane m builds column m of the segment's generator (apply_Lsym on e_m; the
//   5 x 5 single-atom block likewise) and one LDS transpose gives lane c row c;
//   a Chebyshev term is then b_c <- a_k v_c + sum_m Y[c][m] bcast_m(b) + b2_c: 15 (+5) DPP
//   row_newbcast FMAs per lane accumulated onto b itself (three chains for the triangle).
// The laser phase is constant within each pulse (0, then arg xi): the state is carried in the
// pulse's frame (the (ex, ey) rotation of ryd_coh_prop.inc / ryd_dim4_prop.inc), so every
// generator has a real Rabi frequency.

#ifndef RYD_SH16_OCC
#define RYD_SH16_OCC 3
#endif
#ifndef RYD_SH16_CHAINS
#define RYD_SH16_CHAINS 1
#endif
constexpr int SH_BLOCK = 64;                   // one wave, 4 points
constexpr int SH_CHAINS = RYD_SH16_CHAINS;     // accumulation chains of a term's 15 broadcasts
constexpr int SH_PPW = 4;
constexpr int SH_BUF = NS * 16 + 5 * 5;        // >= 4 x 25 (outputs) and 2 x 20 (frame stage)
constexpr int SH_KMAX = 64;
constexpr double SH_XSUB = 20.0;               // largest series argument per (sub-)step: cheb_terms <= 46                    // series terms per segment (x <= ~40; beyond: the
                                               // generic kernel -- see batch_path())

// coordinate s of Q R Q^T on the 15-coordinate triangle (Q rotates (ex, ey) = (3, 4) of each
// atom: x' = c x + sn y, y' = -sn x + c y), read from the stage u
__device__ __forceinline__ double sh_frame_at(const double* u, int s, double c, double sn) {
  int i = 0, b = s;
  while (b >= 5 - i) {                         // row of triangle index s (i <= j)
    b -= 5 - i;
    ++i;
  }
  const int j = i + b;
  const bool ri = i == 3 || i == 4, rj = j == 3 || j == 4;
  const double qi3 = i == 3 ? c : -sn, qi4 = i == 3 ? sn : c;
  const double qj3 = j == 3 ? c : -sn, qj4 = j == 3 ? sn : c;
  if (!ri && !rj) return u[s];
  if (ri && !rj) return fma(qi3, u[tri(3, j)], qi4 * u[tri(4, j)]);
  if (!ri && rj) return fma(qj3, u[tri(i, 3)], qj4 * u[tri(i, 4)]);
  return fma(qi3, fma(qj3, u[tri(3, 3)], qj4 * u[tri(3, 4)]), qi4 * fma(qj3, u[tri(4, 3)], qj4 * u[tri(4, 4)]));
}
__device__ __forceinline__ double sh_vframe_at(const double* u, int k, double c, double sn) {
  if (k == 3) return fma(c, u[3], sn * u[4]);
  if (k == 4) return fma(-sn, u[3], c * u[4]);
  return u[k];
}

// sin(pi u) for u in [0, 1] (the envelope's midpoints): folded to pi u' with u' <= 1/2 and a
// Taylor polynomial in (pi u')^2 to degree 23 (truncation < 1e-20 at pi / 2); no library
// call, whose range reduction was ~90 instructions per segment
__device__ __forceinline__ double sh_sinpi(double u) {
  const double uf = u > 0.5 ? 1.0 - u : u;
  const double x = M_PI * uf, x2 = x * x;
  double p = -1.0 / 25852016738884976640000.0;                 // -1/23!
  p = fma(p, x2, 1.0 / 51090942171709440000.0);                // 1/21!
  p = fma(p, x2, -1.0 / 121645100408832000.0);                 // -1/19!
  p = fma(p, x2, 1.0 / 355687428096000.0);                     // 1/17!
  p = fma(p, x2, -1.0 / 1307674368000.0);                      // -1/15!
  p = fma(p, x2, 1.0 / 6227020800.0);                          // 1/13!
  p = fma(p, x2, -1.0 / 39916800.0);                           // -1/11!
  p = fma(p, x2, 1.0 / 362880.0);                              // 1/9!
  p = fma(p, x2, -1.0 / 5040.0);                               // -1/7!
  p = fma(p, x2, 1.0 / 120.0);                                 // 1/5!
  p = fma(p, x2, -1.0 / 6.0);                                  // -1/3!
  return fma(x * x2, p, x);
}

// signed 4-bit field f of c (one v_bfe_i32)
__device__ __forceinline__ int sh_code(uint32_t c, int f) { return (int)(c << (28 - 4 * f)) >> 28; }

// acc += bcast_M(x) * w (NOP: x may have been written just before -- 2 wait states)
template <int M, bool NOP>
__device__ __forceinline__ void sh_fmac(double& acc, double x, double w) {
  if constexpr (NOP)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(x), "v"(w), "i"(M));
  else
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(x), "v"(w), "i"(M));
}

// one Clenshaw step on both blocks, in place:
//   b <- ck t + b + sum_m bcast_m(a) y[m]   (15 triangle products: b itself and two more chains)
//   c <- ck sg + c + sum_m bcast_m(ca) w[m] (5 single-atom products, interleaved)
// a and ca were written just before: the first broadcast of each waits 2 states
__device__ __forceinline__ void sh_step(double& b, double t, double a, const double (&y)[NS], double& c,
                                        double sg, double ca, const double (&w)[5], double ck) {
  // (the a_k v terms as asm too: a compiler-emitted FMA feeding the broadcast chain's
  // accumulator made it pad each step with s_nops for the unknown asm that reads it)
  asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(b) : "v"(ck), "v"(t));
  asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(c) : "v"(ck), "v"(sg));
  double b1 = 0.0, b2 = 0.0;
  static_for<NS>([&](auto MM) {
    constexpr int m = decltype(MM)::value;
    constexpr int ch = m % SH_CHAINS;
    if constexpr (ch == 0) sh_fmac<m, m == 0>(b, a, y[m]);
    else if constexpr (ch == 1) sh_fmac<m, m == 1>(b1, a, y[m]);
    else sh_fmac<m, m == 2>(b2, a, y[m]);
    if constexpr (m < 5) sh_fmac<m, m == 0>(c, ca, w[m]);
  });
  if constexpr (SH_CHAINS == 3) b += b1 + b2;
  else if constexpr (SH_CHAINS == 2) b += b1;
}

// The point a row computes with: its own when valid, else a neutral one (unit Rabi frequency,
// xi = 1, everything else 0).  An invalid row is inactive (sc = 0) but its generator rows, its
// bound and its amplitudes are still formed, and 0 * inf or 0 * NaN from a non-finite column
// would reach its state through the identity steps; with finite constants the row keeps its
// inputs exactly.  A valid row's values pass through unchanged, and each selected value is
// opaque to the compiler, as a loaded one is: the arithmetic that follows is then formed (and
// contracted into FMAs) as it is without the selection, so a valid row keeps its bits.
__device__ __forceinline__ double sh_pick(bool valid, double x, double neutral) {
  double r = valid ? x : neutral;
  asm volatile("" : "+v"(r));
  return r;
}
__device__ __forceinline__ PointP sh_point_or_neutral(const PointP& q, bool valid) {
  PointP r = q;
  r.Om = sh_pick(valid, q.Om, 1.0);
  r.Dl = sh_pick(valid, q.Dl, 0.0);
  r.V = sh_pick(valid, q.V, 0.0);
  r.d1 = sh_pick(valid, q.d1, 0.0);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    r.gA[c] = sh_pick(valid, q.gA[c], 0.0);
    r.gB[c] = sh_pick(valid, q.gB[c], 0.0);
  }
  r.tau = sh_pick(valid, q.tau, 0.0);
  r.xr = sh_pick(valid, q.xr, 1.0);
  r.xi = sh_pick(valid, q.xi, 0.0);
  r.corr = sh_pick(valid, q.corr, 1.0);
  return r;
}

template <int PROTO>
__global__ __launch_bounds__(SH_BLOCK) __attribute__((amdgpu_waves_per_eu(RYD_SH16_OCC, 8))) void
lindblad_shaped16_kernel(const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st,
                         int64_t lds, double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status,
                         int n_steps, int shape) {
  // one scratch area per row, used in turn: the generator's columns (m * 16 + k, then the
  // single-atom block's at 15 * 16) while the rows are built, the frame rotations' stage,
  // the output block at the end
  __shared__ double s_buf[SH_PPW][SH_BUF];
  __shared__ double s_cf[SH_PPW][SH_KMAX + 2];   // the point's normalised Chebyshev coefficients
  __shared__ double s_cfid[SH_KMAX + 2];         // the identity's: 1, 0, 0, ...
  for (int k = threadIdx.x; k < SH_KMAX + 2; k += SH_BLOCK) s_cfid[k] = k == 0 ? 1.0 : 0.0;
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  const int64_t gi = xcd_block(blockIdx.x, gridDim.x) * SH_PPW + row;
  const bool live = gi < n;
  const int64_t i = live ? gi : n - 1;
  const PointP qin = load_point<PROTO>(prm, ldp, i);
  const bool valid = live && point_valid<PROTO>(qin, n_steps);
  const PointP q0 = sh_point_or_neutral(qin, valid);
  double* Lc = s_buf[row];
  double* Mc = s_buf[row] + NS * 16;
  double* stg = s_buf[row];
  const bool tl = l < NS, vl = l < 5;
  // |11> = e11 (x) e11: triangle coordinate sym_index(1, 1) = 5; |01>: single-atom e11 (1)
  double t = l == sym_index(1, 1) ? 1.0 : 0.0, sg = l == 1 ? 1.0 : 0.0;
  double rsum = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) rsum += fabs(q0.gA[c]) + fabs(q0.gB[c]);
  double fc = 1.0, fs = 0.0;                   // the frame e^{i phi} the state is carried in
  double nuse = 0.0;
  bool over_cap = false;
  const int nseg = n_segments<PROTO>(n_steps);
  // One Chebyshev scale for the whole pulse pair: the Gershgorin bound at the largest
  // amplitude (|Omega| corr max(1, |xi|); the envelopes peak at 1) bounds every segment, and
  // x = omega dt is then the same for all segments (dt = tau / n_steps), so the Bessel
  // coefficients are computed once per point (Miller's recurrence as cheb_segment) and read
  // from LDS per term.  omega is dominated by V (the |rr> level), so the few extra terms of the
  // low-amplitude segments are ~nothing.
  const double dt = q0.tau / (double)n_steps;
  double omega, x;
  {
    Seg gp;
    gp.om_re = q0.Om * q0.corr * fmax(1.0, sqrt(q0.xr * q0.xr + q0.xi * q0.xi));
    gp.om_im = 0.0;
    gp.dl = q0.Dl;
    gp.dt = dt;
    double emin, emax;
    h_bounds(gp, q0.V, q0.d1, emin, emax);
    omega = (emax - emin) + rsum;
    x = omega * dt;
  }
  const bool capped = valid && !(x <= X_CAP);
  const bool active = valid && !capped && x > X_SKIP;
  over_cap = capped;
  const double sc = active ? 2.0 / omega : 0.0;
  // a coarse schedule (x > SH_XSUB per segment) takes each segment in nsub equal sub-steps;
  // a row with fewer than its wave's count idles through the rest (c_0 = 1, c_k = 0: exact
  // identity), so its result does not depend on its neighbours
  const int nsub = active && x > SH_XSUB ? (int)ceil(x / SH_XSUB) : 1;
  if (nsub > 1) x /= (double)nsub;
  const int nsw = __builtin_amdgcn_readfirstlane(wave_max(nsub));
  const int kt = active ? cheb_terms(x) : -1;
  if (kt > SH_KMAX) over_cap = true;           // (x <= SH_XSUB keeps kt below SH_KMAX)
  const int kcut = (__builtin_amdgcn_readfirstlane(wave_max(kt < SH_KMAX ? kt : SH_KMAX)) + 1) & ~1;
  {
    // normalised coefficients c_0 = J_0 / S, c_k = 2 J_k / S (k <= kt; 0 above the point's
    // own cut, so its result does not depend on its wave neighbours)
    const int ks = active ? kt + MILLER_MARGIN : -1;
    const int kstart = (__builtin_amdgcn_readfirstlane(wave_max(ks)) + 1) & ~1;
    const double i2x = active ? 2.0 / x : 0.0;
    double Jp1 = 0.0, Jp2 = 0.0, S = 0.0;
    for (int k = kstart; k >= 0; --k) {
      const double Jk = (k == 0 ? fma(i2x, Jp1, -Jp2) : fma(i2x * (double)(k + 1), Jp1, -Jp2)) +
                        (k == ks ? MILLER_SEED : 0.0);
      Jp2 = Jp1;
      Jp1 = Jk;
      S = k == 0 ? S + Jk : ((k & 1) ? S : fma(2.0, Jk, S));   // J_0 + 2 sum J_2k = 1
      if (l == 0 && k <= kcut) s_cf[row][k] = (k <= kt) ? (k == 0 ? Jk : 2.0 * Jk) : 0.0;
    }
    cp_wsync();
    if (l == 0) {
      const double inv = active ? 1.0 / S : 0.0;
      for (int k = 0; k <= kcut; ++k) s_cf[row][k] *= inv;
      if (!active) s_cf[row][0] = 1.0;          // an inactive point keeps its state
    }
    cp_wsync();
    if (active) nuse = (double)nseg * (double)nsub * (double)(kt + 1);
  }
  const double* cf = s_cf[row];
  // ---- the generator's rows, once per point.  In the pulse's frame the Rabi frequency is
  // real and the segment generator is L0 + hx L1 (make_gen: hx = sc w / 2 the only entry that
  // depends on the amplitude w), where L1 -- the Rabi part at hx = 1 -- has small integer
  // entries (+-1, +-2, +-4).  Lane m builds column m of L0 and of L1 by applying them to e_m
  // (apply_Lsym, mrow), one LDS transpose gives lane c row c; L0's row stays in registers,
  // L1's as 4-bit codes: a segment's row is then one FMA per entry. ----
  double y0[NS], m0[5];
  uint32_t yc0 = 0u, yc1 = 0u, mcd = 0u;
  {
    Seg gz;
    gz.om_re = 0.0;
    gz.om_im = 0.0;
    gz.dl = q0.Dl;
    gz.dt = dt;
    const Gen A0 = make_gen(gz, q0.d1, q0.gA, sc);
    Gen A1;
    A1.g0 = A1.g1 = A1.mg01 = A1.hy = A1.hy2 = A1.hz2 = A1.G = 0.0;
    A1.hx = 1.0;
    A1.hx2 = 2.0;
    const auto rows = [&](const Gen& A, double vs, double (&yr)[NS], double (&mr)[5]) {
      double e[NS], o[NS], ov[5];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        e[k] = k == l ? 1.0 : 0.0;
        o[k] = 0.0;
      }
      apply_Lsym(A, vs, e, o);
#pragma unroll
      for (int r = 0; r < 5; ++r) ov[r] = mrow(A, r, e[1], e[2], e[3], e[4], 0.0);
      cp_wsync();
      if (tl) {
#pragma unroll
        for (int k = 0; k < NS; ++k) Lc[l * 16 + k] = o[k];
      }
      if (vl) {
#pragma unroll
        for (int r = 0; r < 5; ++r) Mc[l * 5 + r] = ov[r];
      }
      cp_wsync();
#pragma unroll
      for (int m = 0; m < NS; ++m) yr[m] = tl ? Lc[m * 16 + l] : 0.0;
#pragma unroll
      for (int m = 0; m < 5; ++m) mr[m] = vl ? Mc[m * 5 + l] : 0.0;
      cp_wsync();
    };
    {
      double y1[NS], m1[5];
      rows(A1, 0.0, y1, m1);
#pragma unroll
      for (int m = 0; m < NS; ++m) {
        const uint32_t c = (uint32_t)(int)y1[m] & 15u;   // exact small integers
        if (m < 8) yc0 |= c << (4 * m);
        else yc1 |= c << (4 * (m - 8));
      }
#pragma unroll
      for (int m = 0; m < 5; ++m) mcd |= ((uint32_t)(int)m1[m] & 15u) << (4 * m);
    }
    rows(A0, sc * 0.5 * q0.V, y0, m0);
  }
  // ---- the schedule (segment<LP_SHAPED>, ryd_engine.hip): segment j of a pulse has amplitude
  // Omega corr env_j, env_j = sin^2(pi tm_j / tau) with tm_j / tau = (j + 1/2) / (n_steps - 1)
  // for the cosine shape (1 otherwise).  The laser phase is constant within a pulse (0, then
  // arg xi), so the frame changes at most at s = 0 and s = n_steps - 1. ----
  const int mseg = n_steps - 1;
  const bool cosine = shape == RYD_SHAPE_COSINE;
  const double amp = q0.Om * q0.corr;
  const double xabs = sqrt(q0.xr * q0.xr + q0.xi * q0.xi);
  const double hsc = 0.5 * sc;
  for (int s = 0; s < nseg; ++s) {
    const int pulse = s >= mseg ? 1 : 0;
    const int j = s - pulse * mseg;
    double env = 1.0;
    if (cosine) {
      const double sn = sh_sinpi(((double)j + 0.5) / (double)mseg);
      env = sn * sn;
    }
    const double a = amp * env;
    const double w = fabs(a) * (pulse ? xabs : 1.0);
    if (s == 0 || s == mseg) {
      // ---- a phase change: rotate the carried state into the new frame (a change below
      // 1e-15 is not one) ----
      double uc = fc, us = fs;
      if (w > 0.0) {
        const double sg1 = a < 0.0 ? -1.0 : 1.0;
        uc = pulse ? sg1 * q0.xr / xabs : sg1;
        us = pulse ? sg1 * q0.xi / xabs : 0.0;
      }
      if (__ballot(valid && fabs(uc - fc) + fabs(us - fs) > 1e-15)) {
        const double dc = fma(uc, fc, us * fs), ds = fma(us, fc, -uc * fs);   // e^{i (phi - phi_prev)}
        cp_wsync();
        if (tl) stg[l] = t;
        if (vl) stg[NS + l] = sg;
        cp_wsync();
        const double nt = tl ? sh_frame_at(stg, l, dc, -ds) : 0.0;
        const double nv = vl ? sh_vframe_at(stg + NS, l, dc, -ds) : 0.0;
        cp_wsync();
        if (valid) {
          t = nt;
          sg = nv;
          fc = uc;
          fs = us;
        }
      }
    }
    // ---- the segment's 2Y = (2 / omega) (L0 + hx L1), hx = w / 2 (pre-scaled by sc) ----
    const double hx = hsc * w;
    // (opaque per trip: hoisted out of the loop, the decoded codes would hold 40 registers)
    asm volatile("" : "+v"(yc0), "+v"(yc1), "+v"(mcd));
    double yrow[NS], mrw[5];
#pragma unroll
    for (int m = 0; m < NS; ++m)
      yrow[m] = fma(hx, (double)sh_code(m < 8 ? yc0 : yc1, m & 7), y0[m]);
#pragma unroll
    for (int m = 0; m < 5; ++m) mrw[m] = fma(hx, (double)sh_code(mcd, m), m0[m]);
    // ---- Clenshaw: b_k = c_k v + 2Y b_{k+1} + b_{k+2} on (t, sg), coefficients from LDS ----
    for (int sub = 0; sub < nsw; ++sub) {
      const double* cp = sub < nsub ? cf : s_cfid;   // s_cfid: this row's identity sub-step
      double bA = 0.0, bB = 0.0, cA = 0.0, cB = 0.0;
      // (the next pair of coefficients is read one trip ahead: its LDS latency hides behind
      // the trip's 40 broadcast FMAs)
      double ck = cp[kcut], ck1 = cp[kcut > 0 ? kcut - 1 : 0];
      for (int k = kcut; k >= 2; k -= 2) {
        const double nk = cp[k - 2], nk1 = cp[k > 2 ? k - 3 : 0];
        sh_step(bB, t, bA, yrow, cB, sg, cA, mrw, ck);
        sh_step(bA, t, bB, yrow, cA, sg, cB, mrw, ck1);
        ck = nk;
        ck1 = nk1;
      }
      sh_step(bB, t, 0.5 * bA, yrow, cB, sg, 0.5 * cA, mrw, ck);
      t = bB;
      sg = cB;
    }
  }
  // ---- back to the lab frame; the four inputs' 25-coordinate states ----
  cp_wsync();
  if (tl) stg[l] = t;
  if (vl) stg[NS + l] = sg;
  cp_wsync();
  const double ot = tl ? sh_frame_at(stg, l, fc, fs) : 0.0;
  const double ov = vl ? sh_vframe_at(stg + NS, l, fc, fs) : 0.0;
  double* so = s_buf[row];
  cp_wsync();
#pragma unroll 1
  for (int e = l; e < 4 * 25; e += 16) so[e] = 0.0;
  cp_wsync();
  if (l == 0) so[0] = 1.0;                                         // |00>
  if (vl) {
    so[25 + l] = ov;                                               // |01>: R[0][k]
    so[50 + 5 * l] = ov;                                           // |10>: R[k][0]
  }
  if (tl) {                                                        // |11>: both triangle halves
    int ii = 0, b = l;
    while (b >= 5 - ii) {
      b -= 5 - ii;
      ++ii;
    }
    so[75 + 5 * ii + (ii + b)] = ot;
    so[75 + 5 * (ii + b) + ii] = ot;
  }
  cp_wsync();
  bool fin = true;
#pragma unroll 1
  for (int e = l; e < 4 * 25; e += 16) {
    const double v = so[e];
    fin = fin && isfinite(v);
    if (live) st[(int64_t)(e % 25) * lds + 4 * i + e / 25] = v;
  }
  const uint64_t rowm = 0xFFFFull << (16 * row);
  const bool any_nonfin = (__ballot(!fin) & rowm) != 0ull;
  const bool any_cap = (__ballot(over_cap) & rowm) != 0ull;
  if (live && l == 0) {
    const double p[4] = {so[0], so[25 + 1], so[50 + 5], so[75 + 6]};
    double tr = 0.0;                                               // |11>'s trace over the 9 levels
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
#pragma unroll
      for (int jj = 0; jj < 3; ++jj) tr += so[75 + 5 * ii + jj];
    const double avg = 0.25 * (p[0] + p[1] + p[2] + p[3]);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      sm[(int64_t)(RYD_S_POP0 + x) * ldm + i] = p[x];
      sm[(int64_t)(RYD_S_OV_RE0 + x) * ldm + i] = nan;
      sm[(int64_t)(RYD_S_OV_IM0 + x) * ldm + i] = nan;
    }
    sm[(int64_t)RYD_S_AVG_POP * ldm + i] = avg;
    sm[(int64_t)RYD_S_CTRL_PHASE * ldm + i] = nan;
    sm[(int64_t)RYD_S_PENALTY * ldm + i] = nan;
    sm[(int64_t)RYD_S_AVG_F * ldm + i] = avg;
    // work counters: the series terms of the point (each term: one triangle and one 5-vector
    // generator application; bench.py FLOP_PER_SHAPED16_TERM)
    sm[(int64_t)RYD_S_NMV_USEFUL * ldm + i] = nuse;
    sm[(int64_t)RYD_S_NMV_EXEC * ldm + i] = nuse;
    sm[(int64_t)RYD_S_TRACE11 * ldm + i] = tr;
    sm[(int64_t)RYD_S_NSQUARE * ldm + i] = 0.0;
    uint32_t stt = valid ? 0u : RYD_STATUS_BAD_INPUT;
    if (any_cap) stt |= RYD_STATUS_STEP_CAP;
    if (any_nonfin) stt |= RYD_STATUS_NONFINITE;
    status[i] = stt;
  }
}
