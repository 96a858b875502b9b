// ryd_traj_eig.inc -- the C5 quantum-jump kernel with exact jump times (included by
// ryd_engine.hip after ryd_traj_sym.inc, whose adapted basis, block layout, jump and
// reduction helpers it uses).  Selected by ladder_levels = RYD_T_EXACT (0).
//
// The ladder kernels place a jump at the end of the dt / 2^L quantum that contains the
// crossing ||psi(t)||^2 = r, found by a binary walk of ~1.5 L dependent ladder steps per
// jump.  Here each adapted block of H_eff (complex symmetric, <= 4 x 4; ryd_traj_sym.inc)
// is diagonalised once per (|Omega|, Delta) by complex-orthogonal Jacobi rotations,
// H_B = W_B diag(lam_B) W_B^T with W_B^T W_B = I, so the no-jump ket at any time t is
//     psi(t) = W diag(exp(-i lam t)) W^T psi(0),
// and ||psi(t)||^2 and its derivative -<psi(t)| sum_k L_k^dag L_k |psi(t)> (the decay
// operator is diagonal in the adapted basis) cost 12 complex exponentials (one per
// distinct eigenvalue) and the 66-MAC block product.  The jump time is the root of
// ||psi(t)||^2 = r, by Newton from the average-decay guess through the segment-end norm
// (which the no-jump test computes anyway), safeguarded by the bracket it keeps
// (bisection when a step leaves it).  It converges to the rounding level of the norm in
// 3-5 evaluations (tools/proto_eig_jumps.py measured 3.9 on the C5 grid with Newton on
// log n; Newton on n itself saves the logarithms and was 2 % faster here), and the jump
// times match the oracle's root-finding on expm (oracle/three_atom_oracle.py
// mc_trajectory) to ~1e-12 of the segment instead of to the ladder quantum.
//
// Work mapping, random streams, the classify pass, the batched jumps of parked lanes
// and the on-chip reduction are those of traj3s_kernel; every lane evaluates one time
// per loop trip, so lanes in different phases (segment-end test, Newton, parked) stay
// converged.  No ladder: ~0.8 KB of LDS per point besides the reduction tile.

constexpr int TE_NL = 12;                        // eigenvalues over the 5 block types
constexpr int TE_NW = 34;                        // eigenvector entries (sum of D^2)
#ifndef RYD_T_EIG_WAVES
#define RYD_T_EIG_WAVES 1
#endif

__host__ __device__ constexpr int te_loff(int B) { return B == 0 ? 0 : B == 1 ? 2 : B == 2 ? 5 : B == 3 ? 6 : 10; }
__host__ __device__ constexpr int te_woff(int B) { return B == 0 ? 0 : B == 1 ? 4 : B == 2 ? 13 : B == 3 ? 14 : 30; }
// atoms in {1, r} of adapted component j (the decay operator is 2 (hgr n_r + hgs (k - n_r)))
__host__ __device__ constexpr int te_k(int j) { return j == 0 ? 0 : j < 7 ? 1 : j < 19 ? 2 : 3; }

__device__ __forceinline__ double2 te_mul(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
// 1/x from the hardware estimate and two Newton steps (the Jacobi rotations are a chain of
// dependent reciprocals; the IEEE division sequence is several times longer)
__device__ __forceinline__ double te_inv(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}
__device__ __forceinline__ double2 te_rcp(double2 a) {
  const double s = fmax(fabs(a.x), fabs(a.y));
  const double is = te_inv(s);
  const double ar = a.x * is, ai = a.y * is;
  const double d = te_inv(s * fma(ar, ar, ai * ai));
  return make_double2(ar * d, -ai * d);
}
// (|z| as sqrt(x^2 + y^2) without hypot's scaling: the rotation arguments 1 + th^2 and
// 1 + t^2 stay far inside the double range -- |th| < 1e20 after te_rot's small-coupling exit)
__device__ __forceinline__ double2 te_sqrt(double2 z) {          // principal branch
  const double m = sqrt(fma(z.x, z.x, z.y * z.y));
  if (m == 0.0) return make_double2(0.0, 0.0);
  if (z.x >= 0.0) {
    const double t = sqrt(0.5 * (m + z.x));
    return make_double2(t, 0.5 * z.y * te_inv(t));
  }
  const double t = sqrt(0.5 * (m - z.x));
  return make_double2(0.5 * fabs(z.y) * te_inv(t), copysign(t, z.y));
}

// One Jacobi rotation on (p, q): A <- G^T A G, W <- W G, G = [[c, s], [-s, c]], c^2 + s^2 = 1
// (complex), chosen to zero A[p][q] with the smaller of the two rotation angles.
template <int D, int p, int q>
__device__ __forceinline__ void te_rot(double2 (&A)[D][D], double2 (&W)[D][D]) {
  const double2 apq = A[p][q];
  const double mag = fabs(apq.x) + fabs(apq.y);
  if (mag == 0.0) return;
  if (mag <= 1e-20 * (fabs(A[p][p].x) + fabs(A[p][p].y) + fabs(A[q][q].x) + fabs(A[q][q].y))) {
    A[p][q] = A[q][p] = make_double2(0.0, 0.0);                   // below any effect on the spectrum
    return;
  }
  const double2 th = te_mul(make_double2(A[q][q].x - A[p][p].x, A[q][q].y - A[p][p].y),
                            te_rcp(make_double2(2.0 * apq.x, 2.0 * apq.y)));
  const double2 th2 = te_mul(th, th);
  const double2 sq = te_sqrt(make_double2(1.0 + th2.x, th2.y));
  const bool plus = fma(th.x, sq.x, th.y * sq.y) >= 0.0;
  const double2 t = te_rcp(plus ? make_double2(th.x + sq.x, th.y + sq.y) : make_double2(th.x - sq.x, th.y - sq.y));
  const double2 t2 = te_mul(t, t);
  const double2 c = te_rcp(te_sqrt(make_double2(1.0 + t2.x, t2.y)));
  const double2 s = te_mul(t, c);
  const double2 tapq = te_mul(t, apq);
  const double2 app = make_double2(A[p][p].x - tapq.x, A[p][p].y - tapq.y);
  const double2 aqq = make_double2(A[q][q].x + tapq.x, A[q][q].y + tapq.y);
  static_for<D>([&](auto RR) {
    constexpr int r = decltype(RR)::value;
    if constexpr (r != p && r != q) {
      const double2 arp = A[r][p], arq = A[r][q];
      const double2 ca = te_mul(c, arp), sb = te_mul(s, arq), sa = te_mul(s, arp), cb = te_mul(c, arq);
      A[r][p] = A[p][r] = make_double2(ca.x - sb.x, ca.y - sb.y);
      A[r][q] = A[q][r] = make_double2(sa.x + cb.x, sa.y + cb.y);
    }
    const double2 wp = W[r][p], wq = W[r][q];
    const double2 cw = te_mul(c, wp), sw = te_mul(s, wq), sp = te_mul(s, wp), cq = te_mul(c, wq);
    W[r][p] = make_double2(cw.x - sw.x, cw.y - sw.y);
    W[r][q] = make_double2(sp.x + cq.x, sp.y + cq.y);
  });
  A[p][p] = app;
  A[q][q] = aqq;
  A[p][q] = A[q][p] = make_double2(0.0, 0.0);
}

// Lanes blk = 0..4 diagonalise block types 0..4 at once: each block sits in the top-left corner of
// a 4 x 4 (zero couplings to the padding, so its rotations are skipped), and all lanes run
// the same cyclic sweeps until their own off-diagonal part is negligible.  Writes lam at
// te_loff(B), W row-major D x D at te_woff(B) (the columns are the eigenvectors); returns
// the sweeps this lane took.
__device__ __forceinline__ int te_build_inl(double2* lam, double2* Wl, int blk, double w, double dl, double d1,
                                            double V, const TRates& R) {
  const int B = blk < TS_NBLK ? blk : 0;
  const int D = ts_dim(B);
  double2 A[4][4], W[4][4];
  static_for<4>([&](auto RR) {
    constexpr int r = decltype(RR)::value;
    static_for<4>([&](auto CC) {
      constexpr int c = decltype(CC)::value;
      A[r][c] = (r < D && c < D) ? ts_heff(B, r < c ? r : c, r < c ? c : r, w, dl, d1, V, R) : make_double2(0.0, 0.0);
      W[r][c] = make_double2(r == c ? 1.0 : 0.0, 0.0);
    });
  });
  int ns = 0;
  for (int sw = 0; sw < 16; ++sw) {
    double off = 0.0, dia = 0.0;
    static_for<4>([&](auto PP) {
      constexpr int p = decltype(PP)::value;
      dia += fabs(A[p][p].x) + fabs(A[p][p].y);
      static_for<4>([&](auto QQ) {
        constexpr int q = decltype(QQ)::value;
        if constexpr (q > p) off += fabs(A[p][q].x) + fabs(A[p][q].y);
      });
    });
    if (!(off > 1e-18 * dia)) break;
    ++ns;
    static_for<4>([&](auto PP) {
      constexpr int p = decltype(PP)::value;
      static_for<4>([&](auto QQ) {
        constexpr int q = decltype(QQ)::value;
        if constexpr (q > p) te_rot<4, p, q>(A, W);
      });
    });
  }
  if (blk < TS_NBLK) {
    static_for<4>([&](auto RR) {
      constexpr int r = decltype(RR)::value;
      if (r < D) lam[te_loff(B) + r] = A[r][r];
      static_for<4>([&](auto CC) {
        constexpr int c = decltype(CC)::value;
        if (r < D && c < D) Wl[te_woff(B) + r * D + c] = W[r][c];
      });
    });
  }
  return blk < TS_NBLK ? ns : 0;
}
// The same decomposition from the blocks' tridiagonal form (ts_heff: complex diagonal a_k,
// real couplings b_k -- each adapted block is a ladder in its number of atoms in |r>): the
// eigenvalues are the roots of det(T - z) by Aberth-Ehrlich iteration (all D roots at once,
// started at the diagonal entries, moved off each other by the largest coupling), each
// eigenvector by the three-term recurrence of (T - lam) v = 0 from v_0 = 1, scaled to
// v^T v = 1.  Returns 16 (the Jacobi build's "not converged") when the iteration cap is
// reached; an ill-conditioned basis is caught by the caller's ||W||_F test as before.
__device__ __forceinline__ int te_build_tri(double2* lam, double2* Wl, int blk, double w, double dl, double d1,
                                            double V, const TRates& R) {
  const int B = blk < TS_NBLK ? blk : 0;
  const int D = ts_dim(B);
  double2 a[4];
  double b[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = k < D ? ts_heff(B, k, k, w, dl, d1, V, R) : make_double2(0.0, 0.0);
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = k + 1 < D ? ts_heff(B, k, k + 1, w, dl, d1, V, R).x : 0.0;
  double bmax = 0.0, amax = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) bmax = fmax(bmax, fabs(b[k]));
#pragma unroll
  for (int k = 0; k < 4; ++k) amax = fmax(amax, fabs(a[k].x) + fabs(a[k].y));
  const bool coupled = bmax > 0.0;
  // starting points: the diagonal, each moved by 0.6 bmax in its own direction
  double2 z[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double ang = 0.7 + 1.9 * k;
    z[k] = make_double2(a[k].x + 0.6 * bmax * cos(ang), a[k].y + 0.6 * bmax * sin(ang));
    if (!coupled) z[k] = a[k];
  }
  int it = 0;
  bool done = !coupled || D < 2;
  for (; it < 40; ++it) {
    if (__ballot(!done) == 0ull) break;
    double2 nz[4];
    double dmax = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      nz[i] = z[i];
      if (i >= D) continue;
      // q = det(T_k - z) and q' by the recurrence
      double2 q0 = make_double2(1.0, 0.0), q1 = make_double2(a[0].x - z[i].x, a[0].y - z[i].y);
      double2 d0 = make_double2(0.0, 0.0), d1q = make_double2(-1.0, 0.0);
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        if (k >= D) break;
        const double2 am = make_double2(a[k].x - z[i].x, a[k].y - z[i].y);
        const double bb = b[k - 1] * b[k - 1];
        const double2 q2 = make_double2(fma(am.x, q1.x, -am.y * q1.y) - bb * q0.x, fma(am.x, q1.y, am.y * q1.x) - bb * q0.y);
        const double2 d2 = make_double2(fma(am.x, d1q.x, -am.y * d1q.y) - bb * d0.x - q1.x,
                                        fma(am.x, d1q.y, am.y * d1q.x) - bb * d0.y - q1.y);
        q0 = q1;
        q1 = q2;
        d0 = d1q;
        d1q = d2;
      }
      const double2 wi = te_mul(q1, te_rcp(d1q));                    // Newton step p / p'
      double2 sum = make_double2(0.0, 0.0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j == i || j >= D) continue;
        const double2 r = te_rcp(make_double2(z[i].x - z[j].x, z[i].y - z[j].y));
        sum.x += r.x;
        sum.y += r.y;
      }
      const double2 ws = te_mul(wi, sum);
      const double2 step = te_mul(wi, te_rcp(make_double2(1.0 - ws.x, -ws.y)));
      nz[i] = make_double2(z[i].x - step.x, z[i].y - step.y);
      dmax = fmax(dmax, fabs(step.x) + fabs(step.y));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = nz[i];
    if (!done && !(dmax > 1e-15 * amax)) done = true;   // (NaN: runs to the cap, then the guard)
  }
  const int ns = done ? (it > 15 ? 15 : it) : 16;
  if (blk < TS_NBLK) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= D) continue;
      const double2 zc = z[c];
      double2 v[4];
      if (coupled) {
        // twisted recurrence: the rows above the twist index tw (the diagonal entry nearest
        // the eigenvalue, where the eigenvector peaks) from v_0 = 1 downwards, the rows below
        // it from v_{D-1} = 1 upwards, the two halves scaled to meet at tw -- each half grows
        // toward the peak, so neither loses digits to cancellation
        int tw = 0;
        double dm = fabs(zc.x - a[0].x) + fabs(zc.y - a[0].y);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
          const double dk = fabs(zc.x - a[k].x) + fabs(zc.y - a[k].y);
          if (k < D && dk < dm) {
            dm = dk;
            tw = k;
          }
        }
        double2 f[4], g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          f[k] = make_double2(k == 0 ? 1.0 : 0.0, 0.0);
          g[k] = make_double2(k == D - 1 ? 1.0 : 0.0, 0.0);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (k < tw) {
            const double2 t = te_mul(make_double2(zc.x - a[k].x, zc.y - a[k].y), f[k]);
            const double2 u = k == 0 ? make_double2(0.0, 0.0) : make_double2(b[k - 1] * f[k - 1].x, b[k - 1] * f[k - 1].y);
            const double ib = 1.0 / b[k];
            f[k + 1] = make_double2((t.x - u.x) * ib, (t.y - u.y) * ib);
          }
        }
#pragma unroll
        for (int k = 3; k >= 1; --k) {
          if (k < D && k > tw) {
            const double2 t = te_mul(make_double2(zc.x - a[k].x, zc.y - a[k].y), g[k]);
            const double2 u = k + 1 < D ? make_double2(b[k] * g[k + 1].x, b[k] * g[k + 1].y) : make_double2(0.0, 0.0);
            const double ib = 1.0 / b[k - 1];
            g[k - 1] = make_double2((t.x - u.x) * ib, (t.y - u.y) * ib);
          }
        }
        const double2 fr = tw == 0 ? f[0] : tw == 1 ? f[1] : tw == 2 ? f[2] : f[3];
        const double2 gr = tw == 0 ? g[0] : tw == 1 ? g[1] : tw == 2 ? g[2] : g[3];
        const double2 ifr = te_rcp(fr), igr = te_rcp(gr);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k <= tw ? te_mul(f[k], ifr) : te_mul(g[k], igr);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = make_double2(k == c ? 1.0 : 0.0, 0.0);
      }
      double2 nn = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < D) nn = make_double2(nn.x + (v[k].x * v[k].x - v[k].y * v[k].y), nn.y + 2.0 * v[k].x * v[k].y);
      const double2 is = te_rcp(te_sqrt(nn));
      lam[te_loff(B) + c] = zc;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < D) Wl[te_woff(B) + r * D + c] = te_mul(v[r], is);
    }
  }
  return blk < TS_NBLK ? ns : 0;
}

__device__ __attribute__((noinline)) int te_build(double2* lam, double2* Wl, int blk, double w, double dl, double d1,
                                                  double V, const TRates& R) {
#ifdef RYD_TE_TRIDIAG
  return te_build_tri(lam, Wl, blk, w, dl, d1, V, R);
#else
  return te_build_inl(lam, Wl, blk, w, dl, d1, V, R);
#endif
}

// c = W^T x, instance by instance (component 0, |000>, is its own eigenvector)
__device__ __forceinline__ void te_coeffs(const double2* __restrict__ Wl, const double (&x)[T_NV], double (&c)[T_NV]) {
  c[0] = x[0];
  c[1] = x[1];
  static_for<TS_NINST>([&](auto II) {
    constexpr int ii = decltype(II)::value;
    constexpr int B = ts_inst_block(ii), s0 = ts_inst_start(ii), D = ts_dim(B);
    static_for<D>([&](auto KK) {
      constexpr int k = decltype(KK)::value;
      double re = 0.0, im = 0.0;
      static_for<D>([&](auto RR) {
        constexpr int r = decltype(RR)::value;
        const double2 m = Wl[te_woff(B) + r * D + k];
        const double xr = x[2 * (s0 + r)], xi = x[2 * (s0 + r) + 1];
        re = fma(m.x, xr, fma(-m.y, xi, re));
        im = fma(m.x, xi, fma(m.y, xr, im));
      });
      c[2 * (s0 + k)] = re;
      c[2 * (s0 + k) + 1] = im;
    });
  });
}

// e^{a} (cos b, -sin b) for the evaluation: Cody-Waite reductions (ln 2 and pi/2 in two
// FMA parts) and Taylor polynomials to beyond double precision on the reduced ranges
// (|r| <= 0.35: degree 13; |x| <= pi/4: degree 17/18).  The arguments here are
// |lam t| <~ 1e5; the two-part reduction stays accurate to |b| ~ 1e15, and beyond that
// (a frequency times a duration no physical input reaches) the result is NaN, which the
// kernel reports as RYD_STATUS_NONFINITE.  No library call: a call site inside the walk
// loop would force its live kets to be saved around it.
__device__ __forceinline__ void te_expi(double a, double b, double& re, double& im) {
  const double n = rint(a * 1.4426950408889634074);
  double r = fma(-n, 6.9314718055994528623e-01, a);
  r = fma(-n, 2.3190468138462996154e-17, r);
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  const double m = a < -745.0 ? 0.0 : ldexp(p, (int)n);
  // branch-free (a divergent branch per exponential splits the evaluation into basic blocks
  // and the live kets spill around each)
  const bool ok = fabs(b) < 1.0e15;
  const double k = ok ? rint(b * 0.63661977236758134308) : 0.0;
  double x = fma(-k, 1.5707963267948966192, b);
  x = fma(-k, 6.1232339957367660359e-17, x);
  const double x2 = x * x;
  double s = 1.0 / 355687428096000.0;                         // 1/17!
  s = fma(s, x2, -1.0 / 1307674368000.0);
  s = fma(s, x2, 1.0 / 6227020800.0);
  s = fma(s, x2, -1.0 / 39916800.0);
  s = fma(s, x2, 1.0 / 362880.0);
  s = fma(s, x2, -1.0 / 5040.0);
  s = fma(s, x2, 1.0 / 120.0);
  s = fma(s, x2, -1.0 / 6.0);
  s = fma(s * x2, x, x);
  double c = -1.0 / 6402373705728000.0;                       // -1/18!
  c = fma(c, x2, 1.0 / 20922789888000.0);
  c = fma(c, x2, -1.0 / 87178291200.0);
  c = fma(c, x2, 1.0 / 479001600.0);
  c = fma(c, x2, -1.0 / 3628800.0);
  c = fma(c, x2, 1.0 / 40320.0);
  c = fma(c, x2, -1.0 / 720.0);
  c = fma(c, x2, 1.0 / 24.0);
  c = fma(c, x2, -0.5);
  c = fma(c, x2, 1.0);
  const int q = (int)((long long)k & 3);
  double sn = (q & 1) ? c : s;
  double cs = (q & 1) ? s : c;
  sn = (q & 2) ? -sn : sn;
  cs = ((q + 1) & 2) ? -cs : cs;
  if (!ok) sn = cs = __builtin_nan("");
  re = m * cs;
  im = -m * sn;
}

// instances of block type B (ts_inst_block order): 1-atom x3, 2-sym x3, 2-anti x3, 3-sym, 3-std x2
__host__ __device__ constexpr int te_ninst(int B) { return B == 3 ? 1 : B == 4 ? 2 : 3; }
__host__ __device__ constexpr int te_inst(int B, int m) {
  return B == 0 ? m : B == 1 ? 3 + 2 * m : B == 2 ? 4 + 2 * m : B == 3 ? 9 : 10 + m;
}

// y = W diag(exp(-i lam t)) c; returns ||y||^2 and sets dn = d||y||^2/dt = -<y|Gamma|y>.
// Block type by block type, so only one type's exponentials are live at a time.
__device__ __forceinline__ double te_eval(const double2* __restrict__ lam, const double2* __restrict__ Wl,
                                          const double (&c)[T_NV], double t, const TRates& R, double (&y)[T_NV],
                                          double& dn) {
  y[0] = c[0];
  y[1] = c[1];
  double n = fma(c[0], c[0], c[1] * c[1]);
  double gr = 0.0, gs = 0.0;                     // sum n_r |y|^2, sum (k - n_r) |y|^2
  static_for<TS_NBLK>([&](auto BB) {
    constexpr int B = decltype(BB)::value;
    constexpr int D = ts_dim(B);
    double er[D], ei[D];
    static_for<D>([&](auto KK) {
      constexpr int k = decltype(KK)::value;
      const double2 l = lam[te_loff(B) + k];
      te_expi(l.y * t, l.x * t, er[k], ei[k]);
    });
    static_for<te_ninst(B)>([&](auto MM) {
      constexpr int s0 = ts_inst_start(te_inst(B, decltype(MM)::value));
      double br[D], bi[D];
      static_for<D>([&](auto KK) {
        constexpr int k = decltype(KK)::value;
        const double xr = c[2 * (s0 + k)], xi = c[2 * (s0 + k) + 1];
        br[k] = fma(er[k], xr, -ei[k] * xi);
        bi[k] = fma(er[k], xi, ei[k] * xr);
      });
      static_for<D>([&](auto RR) {
        constexpr int r = decltype(RR)::value;
        double vr = 0.0, vi = 0.0;
        static_for<D>([&](auto KK) {
          constexpr int k = decltype(KK)::value;
          const double2 m = Wl[te_woff(B) + r * D + k];
          vr = fma(m.x, br[k], fma(-m.y, bi[k], vr));
          vi = fma(m.x, bi[k], fma(m.y, br[k], vi));
        });
        y[2 * (s0 + r)] = vr;
        y[2 * (s0 + r) + 1] = vi;
        const double p = fma(vr, vr, vi * vi);
        n += p;
        constexpr int nr = ts_nr(s0 + r), kk = te_k(s0 + r);
        if constexpr (nr > 0) gr = fma((double)nr, p, gr);
        if constexpr (kk - nr > 0) gs = fma((double)(kk - nr), p, gs);
      });
    });
  });
  dn = -2.0 * fma(R.hgr, gr, R.hgs * gs);
  return n;
}


// ts_reduce_round with the shifted sums, the element pairs and the shifts held in registers
// across the round's tiles (one read and one write of accg per round, not per tile).
// stage(tb, tn) fills stg with kets tb .. tb + tn - 1 of the round (between the barriers).
// kmask: the elements (lane + 64 k, bit k) this wave reduces -- all of them, except in the
// cooperative range merge, where the waves of a workgroup split them.
template <typename Stage>
__device__ __forceinline__ void te_reduce_tiles(double2* stg, double* accg, const double* s_phi, int lane, int l0,
                                                int nk, Stage stage, uint32_t kmask = 0x3Fu) {
  int pa[T_EPL], pb[T_EPL];
  double rr[T_EPL], ri[T_EPL], a0[T_EPL], a1[T_EPL], a2[T_EPL];
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {
    const int e = lane + k * T_WAVE;
    pa[k] = pb[k] = 0;
    rr[k] = ri[k] = a0[k] = a1[k] = a2[k] = 0.0;
    if (e < T_NPAIR && ((kmask >> k) & 1u)) {
      t_pair(e, pa[k], pb[k]);
      const double ar = s_phi[2 * pa[k]], ai = s_phi[2 * pa[k] + 1], br = s_phi[2 * pb[k]], bi = s_phi[2 * pb[k] + 1];
      rr[k] = fma(ar, br, ai * bi);
      ri[k] = fma(ai, br, -ar * bi);
      a0[k] = accg[3 * e];
      a1[k] = accg[3 * e + 1];
      a2[k] = accg[3 * e + 2];
    }
  }
  for (int tb = l0; tb < l0 + nk; tb += T_TILE) {
    const int tn = min(T_TILE, l0 + nk - tb);
    __syncthreads();
    stage(tb, tn);
    // a short tile is padded with the shift itself, whose terms are exactly zero (x = phi_a
    // phi_b^* - rr: the same two roundings): every tile is then a full, unrolled 8 kets --
    // with a break at the tile's end the loop was not unrolled where the registers are tight
    for (int e = lane; e < (T_TILE - tn) * T_NB; e += T_WAVE) {
      const int idx = e % T_NB;
      stg[tn * T_NB + e] = make_double2(s_phi[2 * idx], s_phi[2 * idx + 1]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < T_EPL; ++k) {
      if (lane + k * T_WAVE < T_NPAIR && ((kmask >> k) & 1u)) {
#pragma unroll
        for (int t = 0; t < T_TILE; ++t) {         // unrolled: the tile's LDS reads issue together
          const double2 u1 = stg[t * T_NB + pa[k]], u2 = stg[t * T_NB + pb[k]];
          const double xr = fma(u1.x, u2.x, u1.y * u2.y) - rr[k];
          const double xi = fma(u1.y, u2.x, -u1.x * u2.y) - ri[k];
          a0[k] += xr;
          a1[k] += xi;
          a2[k] = fma(xr, xr, fma(xi, xi, a2[k]));
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {
    const int e = lane + k * T_WAVE;
    if (e < T_NPAIR && ((kmask >> k) & 1u)) {
      accg[3 * e] = a0[k];
      accg[3 * e + 1] = a1[k];
      accg[3 * e + 2] = a2[k];
    }
  }
}

// a round of kets held by lanes l0 .. l0 + nk - 1
__device__ __forceinline__ void te_reduce_round(double2* stg, double* accg, const double* s_phi,
                                                const double (&z)[T_NV], bool act, int lane, int l0, int nk) {
  te_reduce_tiles(stg, accg, s_phi, lane, l0, nk, [&](int tb, int) {
    if (act && lane >= tb && lane < tb + T_TILE)
#pragma unroll
      for (int idx = 0; idx < T_NB; ++idx)
        stg[(lane - tb) * T_NB + idx] = make_double2(z[2 * idx], z[2 * idx + 1]);
  });
}
// the same round from kets in global scratch (the range merge): ket j of the round is row
// rows[j] of kets; a tile's 8 x 54 doubles are loaded by the whole wave, 7 independent
// loads per lane (prefetching the next tile into registers while one is reduced measured
// no faster: the merge is bound by the reduction, profiles/r05/c5_merge/)
__device__ __forceinline__ void te_reduce_global(double2* stg, double* accg, const double* s_phi,
                                                 const double* __restrict__ kets, const uint32_t* rows, int lane,
                                                 int nk, uint32_t kmask = 0x3Fu) {
  constexpr int NV = (T_TILE * T_NV + T_WAVE - 1) / T_WAVE;
  double* stgd = reinterpret_cast<double*>(stg);
  // the next tile's kets are loaded while this one is reduced (with the elements split over
  // a workgroup's waves the merge waits on these loads, not on the arithmetic)
  double v[NV];
  const auto load = [&](int tb, int tn) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int e = lane + k * T_WAVE;
      const int t = e / T_NV, c = e - t * T_NV;
      v[k] = t < tn ? kets[(size_t)rows[tb + t] * T_NV + c] : 0.0;
    }
  };
  load(0, min(T_TILE, nk));
  te_reduce_tiles(stg, accg, s_phi, lane, 0, nk, [&](int tb, int tn) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int e = lane + k * T_WAVE;
      if (e < tn * T_NV) stgd[e] = v[k];
    }
    const int nb = tb + T_TILE;
    if (nb < nk) load(nb, min(T_TILE, nk - nb));
  }, kmask);
}

// ts_write_moments with the rows assembled in LDS first: the mirrored triangle's elements
// are 27 complex apart in the row, so writing them straight from the pair lanes scatters
// the stores; from LDS both rows go out contiguously
__device__ __forceinline__ void te_write_moments(double* orho, double* ose, const double* accg, const double* s_phi,
                                                 int lane, double ntr, double& trl, double& qpl, double2* l_rho) {
  double sev[T_EPL];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {
    const int e = lane + k * T_WAVE;
    sev[k] = 0.0;
    if (e < T_NPAIR) {
      int pa, pb;
      t_pair(e, pa, pb);
      const double ar = s_phi[2 * pa], ai = s_phi[2 * pa + 1], br = s_phi[2 * pb], bi = s_phi[2 * pb + 1];
      const double dr = accg[3 * e] / ntr, di = accg[3 * e + 1] / ntr;
      const double mr = fma(ar, br, ai * bi) + dr, mi = fma(ai, br, -ar * bi) + di;
      const double var = accg[3 * e + 2] / ntr - (dr * dr + di * di);
      sev[k] = ntr > 1.0 ? sqrt(fmax(var, 0.0) / (ntr - 1.0)) : 0.0;
      l_rho[pa + T_NB * pb] = make_double2(mr, mi);
      l_rho[pb + T_NB * pa] = make_double2(mr, -mi);
      if (pa == pb) {
        trl += mr;
        if (t_qubit(pa)) qpl += mr;
      }
    }
  }
  __syncthreads();
  if ((reinterpret_cast<uintptr_t>(orho) & 15u) == 0u) {      // (ld_rho is the caller's: may be odd)
    double2* orho2 = reinterpret_cast<double2*>(orho);
    for (int e = lane; e < T_NB * T_NB; e += T_WAVE) orho2[e] = l_rho[e];
  } else {
    for (int e = lane; e < T_NB * T_NB; e += T_WAVE) {
      orho[2 * e] = l_rho[e].x;
      orho[2 * e + 1] = l_rho[e].y;
    }
  }
  __syncthreads();                                    // the standard errors through the same buffer
  double* l_se = reinterpret_cast<double*>(l_rho);
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {
    const int e = lane + k * T_WAVE;
    if (e < T_NPAIR) {
      int pa, pb;
      t_pair(e, pa, pb);
      l_se[pa + T_NB * pb] = sev[k];
      l_se[pb + T_NB * pa] = sev[k];
    }
  }
  __syncthreads();
  for (int e = lane; e < T_NB * T_NB; e += T_WAVE) ose[e] = l_se[e];
  __syncthreads();
}

// ---- the kernel: TE_P points per wave ----
// Per point the work is that of traj3s_kernel (no-jump branch, classify, walk the jumpers,
// shifted-sum reduction), but a wave owns TE_P points: pass 1 runs them side by side (lane
// group p = lanes 8p .. 8p + 7 diagonalises and evolves point p), and the jumpers of all
// TE_P points share the walk rounds (a C5 point has ~31 jumpers, so one point per wave
// left half the lanes idle and paid the slowest chain per point).  Each point's kets are
// still reduced in its own jumper order, so results do not depend on how points are
// grouped into waves (launch shape, range shards).  C5 kernel times (profiles/r03/c5eig/):
// 1 point per wave 0.95 ms, 2 points 0.54 ms, 4 points 0.60 ms, 8 points 0.86 ms -- past 2
// the waves (n / TE_P, one per SIMD at 480 registers) get too few to even out their work.
// Slot p of wave b is point b (p = 0) or its mirror 2 npair - 1 - b (p = 1; see pt below),
// so neighbouring grid points (similar jump counts) land in different waves and a cost-
// ordered launch pairs heavy with light.  Exact mode needs |Omega| and Delta
// constant over a point's segments (LP square, smooth JP, bang-bang): the eigen-data are
// built once per point.
#ifndef RYD_T_EIG_P
#define RYD_T_EIG_P 2
#endif
constexpr int TE_P = RYD_T_EIG_P;
static_assert(TE_P >= 1 && TE_P <= 8, "pass 1 uses lane groups of 8");
constexpr int TE_SLOT_SHIFT = 28;                // jumper entry: slot << 28 | trajectory (< 2^20)
constexpr double TE_COND_MAX = 1.0e4;            // ||W_B||_F^2 / D bound of an accepted eigenbasis
#ifndef RYD_TE_JB
#define RYD_TE_JB 16                             // lanes at jumps / boundaries that trigger a service pass
#endif
constexpr int TE_JB = RYD_TE_JB;                 // (8, as traj3s: +1 %; 4: +1 %; profiles/r04/c5_walk/)
constexpr int64_t TE_SIMDS = 1024;               // MI355X: 256 CUs x 4 SIMDs (when the query fails)
constexpr double TE_SCRATCH_MAX = 4.0 * (1ull << 30);   // merge scratch (kets) bound, bytes

// COOP (launches split into trajectory ranges): one workgroup per wave pair of points, its
// a.split <= TE_COOP_MAX waves the ranges.  Every wave runs pass 1 (the same values into the
// same LDS, as each range wave of the one-wave-per-range form did), walks its own range, and
// after one barrier the waves merge the kets together -- wave w the shifted-sum elements
// lane + 64 k for its share of k, each element summed over all of the point's jumpers in
// trajectory order: the additions of the one-wave form, so the rows are bit-identical to it
// and to the last-wave merge this replaces.  Barriers inside a range's walk are wave-local.
constexpr int TE_COOP_MAX = 4;
template <int PROTO, bool COOP = false>
__global__ __launch_bounds__(COOP ? TE_COOP_MAX * T_WAVE : T_WAVE) __attribute__((amdgpu_waves_per_eu(RYD_T_EIG_WAVES, 8))) void
traj3e_kernel(TrajArgs a) {
  double tp_start = T_CLK(), tp_pass1 = 0.0, tp_cls = 0.0, tp_walk = 0.0, tp_red = 0.0, tp_mark = 0.0, tp_jac = 0.0;
  const double tp_rt0 = T_RTC();
  (void)tp_start; (void)tp_jac; (void)tp_pass1; (void)tp_cls; (void)tp_walk; (void)tp_red; (void)tp_mark; (void)tp_rt0;
  __shared__ double2 e_lam[TE_P * TE_NL];
  __shared__ double2 e_W[TE_P * TE_NW];
  constexpr int NWG = COOP ? TE_COOP_MAX : 1;          // waves per workgroup
  __shared__ double2 stg_all[NWG * T_TILE * T_NB];     // each wave's reduction tile (8 kets)
  __shared__ uint32_t s_list_all[NWG * TE_P * T_CHUNK];  // each wave's jumper list
  __shared__ double s_wst[COOP ? TE_P : 1][NWG][8];    // COOP: each range's statistics
  __shared__ double s_psi0[T_NV];                      // adapted basis
  __shared__ double s_phi[TE_P * T_NV];                // atom basis (each point's reduction shift)
  __shared__ double s_surv[TE_P];
  __shared__ int s_ok[TE_P], s_nseg[TE_P];
  // the no-jump branch at the end of the first active segment A (its ket and norm) and
  // the norm at the end of the second, B, when B is the last (else -1): before its first
  // jump a trajectory needs no segment-end test there
  __shared__ double s_yA[TE_P][T_NV];
  __shared__ double s_nA[TE_P], s_nB[TE_P];
  __shared__ int s_sgA[TE_P], s_sgB[TE_P];
  __shared__ double2 l_rho[T_NB * T_NB];               // one point's output rows, assembled (rho, then se)
  __shared__ double s_tot[TE_P][3 * T_NPAIR];          // each point's shifted sums (LDS: no HBM read-modify-write)
  __shared__ int s_last[TE_P];
  // grid = npair x split: wave (b, kc) runs points b, b + npair, ... over trajectory range kc
  // (COOP: workgroup b, its wave kc)
  const int lane = COOP ? (int)(threadIdx.x & (T_WAVE - 1)) : (int)threadIdx.x;
  const int64_t nwv = a.npair;
  const int64_t bw = COOP ? (int64_t)blockIdx.x : (int64_t)blockIdx.x % nwv;
  const int kc = COOP ? (int)(threadIdx.x / T_WAVE) : (int)((int64_t)blockIdx.x / nwv);
  double2* const stg = stg_all + (COOP ? kc : 0) * (T_TILE * T_NB);
  uint32_t* const s_list = s_list_all + (COOP ? kc : 0) * (TE_P * T_CHUNK);
  // the sync of a range's own walk: the whole block in the one-wave form, the wave's LDS
  // operations (a wave's lanes run in lock step) in the cooperative one
  const auto range_sync = [&]() {
    if constexpr (COOP) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else __syncthreads();
  };
  const int ngrp = a.n_traj / T_WAVE;                  // 64-trajectory groups (n_traj % 64 == 0)
  const int r0 = T_WAVE * (kc * ngrp / a.split), r1 = T_WAVE * ((kc + 1) * ngrp / a.split);
  // slot p: row p of a TE_P x npair table laid boustrophedon (odd rows reversed), so a
  // wave's two points sit at mirrored positions of the launch: heavy with light when the
  // points are ordered by cost (both C5 orders keep the pulse length monotone)
  const auto pt = [&](int p) -> int64_t { return (int64_t)p * nwv + ((p & 1) ? nwv - 1 - bw : bw); };
  const int nseg = n_segments<PROTO>(a.n_steps);
  if (lane == 0) {
    double x[T_NV], y[T_NV];
#pragma unroll
    for (int e = 0; e < T_NV; ++e) x[e] = a.psi0[e];
    ts_to_adapted(x, y);
#pragma unroll
    for (int e = 0; e < T_NV; ++e) s_psi0[e] = y[e];
  }
  __syncthreads();

  // ---- pass 1, lane group ssl: validity, eigen-decomposition, no-jump branch ----
  const int ssl = lane >> 3, blk = lane & 7;
  double nsweep = 0.0;
  {
    const bool inb = ssl < TE_P && pt(ssl) < a.n;
    const int64_t ip = inb ? pt(ssl) : pt(0);
    const PointP q0 = load_point<PROTO>(a.prm, a.ld, ip);
    bool ok = inb && point_valid<PROTO>(q0, a.n_steps), konst = true;
    TRates R;
#pragma unroll
    for (int c = 0; c < 4; ++c) R.g[c] = q0.gA[c];
    R.hgr = 0.5 * (R.g[0] + R.g[1] + R.g[2]);
    R.hgs = 0.5 * R.g[3];
    double kw = -1.0, kdl = 0.0;
    for (int sg = 0; sg < nseg && ok && konst; ++sg) {
      const Seg g = segment<PROTO>(q0, sg, a.n_steps, a.shape);
      if (!(g.dt > 0.0)) continue;
      const double w = 0.5 * sqrt(g.om_re * g.om_re + g.om_im * g.om_im);
      if (kw < 0.0) {
        kw = w;
        kdl = g.dl;
      } else if (fabs(w - kw) > 1e-12 * kw || fabs(g.dl - kdl) > 1e-12 * fmax(fabs(kdl), kw)) {
        konst = false;                                 // not a constant-|Omega|, Delta schedule
      }                                                // (|Omega xi| = |Omega| only to rounding)
    }
    if (kw < 0.0) kw = 0.0;
    bool eig_bad = ok && !konst;                       // the ladder kernel takes such a point
    double2* lam = e_lam + (ssl < TE_P ? ssl : 0) * TE_NL;
    double2* Wl = e_W + (ssl < TE_P ? ssl : 0) * TE_NW;
    ok = ok && konst;
    if (ok) {
      nsweep = (double)te_build(lam, Wl, blk, kw, kdl, q0.d1, q0.V, R);
      eig_bad = blk < TS_NBLK && nsweep >= 16.0;      // the sweep cap reached: not converged
    }
    __syncthreads();
    tp_jac = T_CLK() - tp_start;
    if (ok && blk < TS_NBLK) {                        // conditioning of the block's eigenbasis
      const int D = ts_dim(blk);
      double f = 0.0;
      for (int e = 0; e < D * D; ++e) {
        const double2 w = Wl[te_woff(blk) + e];
        f = fma(w.x, w.x, fma(w.y, w.y, f));
      }
      eig_bad = eig_bad || !(f <= TE_COND_MAX * D);
    }
    // the point's lane group agrees: an unconverged or ill-conditioned block, or a schedule
    // without constant |Omega| and Delta, sends the whole point to the ladder kernel
    // (RYD_STATUS_EXACT_FALLBACK)
    const uint64_t badm = __ballot(eig_bad);
    const bool fallback = inb && ((badm >> (8 * ssl)) & 0xFFull) != 0ull;
    ok = ok && !fallback;
    double y[T_NV], c[T_NV];
#pragma unroll
    for (int e = 0; e < T_NV; ++e) y[e] = s_psi0[e];
    double surv = 1.0, phf = 0.0, nA = -1.0, nB = -1.0;
    int nseg_eff = 0, sgA = -1, sgB = -1;
    const bool wr = blk == 0 && ssl < TE_P;
    if (ok) {
      for (int sg = 0; sg < nseg; ++sg) {
        const Seg g = segment<PROTO>(q0, sg, a.n_steps, a.shape);
        if (!(g.dt > 0.0)) continue;
        const double ph = (g.om_re == 0.0 && g.om_im == 0.0) ? phf : atan2(g.om_im, g.om_re);
        if (ph != phf) {
          ts_rotate(y, phf - ph);
          phf = ph;
        }
        te_coeffs(Wl, y, c);
        double dn;
        surv = te_eval(lam, Wl, c, g.dt, R, y, dn);
        if (nseg_eff == 0) {
          nA = surv;
          sgA = sg;
          if (wr)
#pragma unroll
            for (int e = 0; e < T_NV; ++e) s_yA[ssl][e] = y[e];
        } else if (nseg_eff == 1) {
          nB = surv;
          sgB = sg;
        }
        ++nseg_eff;
      }
      ts_rotate(y, phf);
    }
    if (wr) {
      s_ok[ssl] = ok ? 1 : (fallback ? -1 : 0);     // -1: the ladder kernel takes the point
      s_surv[ssl] = surv;
      s_nseg[ssl] = nseg_eff;
      s_nA[ssl] = nA;
      s_nB[ssl] = nseg_eff == 2 ? nB : -1.0;
      s_sgA[ssl] = sgA;
      s_sgB[ssl] = sgB;
      if (ok) {
        ts_to_atom(y, c);
        const double inv = surv > 0.0 ? 1.0 / sqrt(surv) : 0.0;
#pragma unroll
        for (int e = 0; e < T_NV; ++e) s_phi[ssl * T_NV + e] = c[e] * inv;
      }
    }
  }
  __syncthreads();
  tp_pass1 = T_CLK() - tp_start;
  // rejected points (the first range's wave writes them): zero rows and BAD_INPUT, or
  // EXACT_FALLBACK for the ladder pass; accepted: their shifted sums start at 0
  for (int p = 0; p < TE_P && pt(p) < a.n; ++p) {
    const int64_t ip = pt(p);
    if (s_ok[p] == 1) {
      for (int e = lane; e < 3 * T_NPAIR; e += T_WAVE) s_tot[p][e] = 0.0;
    } else if (kc == 0) {
      double* orho = a.rho + (size_t)ip * a.ld_rho;
      double* ose = a.se + (size_t)ip * a.ld_se;
      for (int e = lane; e < RYD_T_RHO_WIDTH; e += T_WAVE) orho[e] = 0.0;
      for (int e = lane; e < RYD_T_SE_WIDTH; e += T_WAVE) ose[e] = 0.0;
      if (lane < RYD_T_NSUMMARY) a.summ[lane * a.ld_summ + ip] = 0.0;
      if (lane == 0) a.status[ip] = s_ok[p] < 0 ? RYD_STATUS_EXACT_FALLBACK : RYD_STATUS_BAD_INPUT;
    }
  }
  __syncthreads();
  double st_j[TE_P], st_hit[TE_P], st_max[TE_P], st_use[TE_P], st_exec[TE_P];
  uint32_t capm = 0u, nonfinm = 0u;                    // bit p: a trajectory of point p capped / non-finite
  static_for<TE_P>([&](auto PP) {
    constexpr int p = decltype(PP)::value;
    st_j[p] = st_hit[p] = st_max[p] = 0.0;
    st_use[p] = lane == 0 && kc == 0 ? (double)s_nseg[p] : 0.0;   // (every range repeats pass 1)
    st_exec[p] = lane == 0 ? 8.0 * s_nseg[p] : 0.0;    // its pass-1 lane group
  });

  for (int c0 = r0; c0 < r1; c0 += T_CHUNK) {
    const int cn = min(T_CHUNK, r1 - c0);
    tp_mark = T_CLK();
    int J = 0;
    for (int p = 0; p < TE_P; ++p) {
      if (s_ok[p] != 1) continue;
      const int64_t ip = pt(p);
      const uint64_t gpoint = (uint64_t)(a.point_offset + a.point_stride * ip);
      const double surv = s_surv[p];
      for (int t0 = 0; t0 < cn; t0 += T_WAVE) {
        const uint32_t traj = (uint32_t)(c0 + t0 + lane);
        double r, s;
        t_draw(traj, 0u, gpoint, a.seed, r, s);
        const bool jumps = !(surv > r);
        const uint64_t m = __ballot(jumps);
        const int pos = __popcll(m & ((1ull << lane) - 1ull));
        if (jumps) s_list[J + pos] = ((uint32_t)p << TE_SLOT_SHIFT) | traj;
        J += __popcll(m);
        if (!jumps && a.rec) {
          double* rec = a.rec + ((size_t)ip * a.n_traj + traj) * RYD_T_REC_WIDTH;
          for (int e = 0; e < T_NV; ++e) rec[e] = s_phi[p * T_NV + e];
          rec[RYD_T_REC_NJUMPS] = 0.0;
          for (int k = 0; k < 2 * RYD_T_REC_JUMPS; ++k) rec[RYD_T_REC_JUMP0 + k] = -1.0;
          rec[RYD_T_REC_ITERS] = (double)s_nseg[p];
        }
      }
    }
    range_sync();
    tp_cls += T_CLK() - tp_mark;
    for (int j0 = 0; j0 < J; j0 += T_WAVE) {
      tp_mark = T_CLK();
      const bool act = j0 + lane < J;
      const uint32_t ent = act ? s_list[j0 + lane] : 0u;
      const int p = (int)(ent >> TE_SLOT_SHIFT);
      const uint32_t traj = ent & ((1u << TE_SLOT_SHIFT) - 1u);
      const int64_t ip = pt(p);
      const uint64_t gpoint = (uint64_t)(a.point_offset + a.point_stride * ip);
      const double2* lam = e_lam + p * TE_NL;
      const double2* Wl = e_W + p * TE_NW;
      double* rec = (a.rec && act) ? a.rec + ((size_t)ip * a.n_traj + traj) * RYD_T_REC_WIDTH : nullptr;
      if (rec)
        for (int k = 0; k < 2 * RYD_T_REC_JUMPS; ++k) rec[RYD_T_REC_JUMP0 + k] = -1.0;
      TRates R;
      {
        const PointP q0 = load_point<PROTO>(a.prm, a.ld, ip);
#pragma unroll
        for (int c = 0; c < 4; ++c) R.g[c] = q0.gA[c];
        R.hgr = 0.5 * (R.g[0] + R.g[1] + R.g[2]);
        R.hgs = 0.5 * R.g[3];
      }
      double y[T_NV], c[T_NV];
#pragma unroll
      for (int e = 0; e < T_NV; ++e) y[e] = c[e] = s_psi0[e];
      double r, s;
      uint32_t cycle = 0;
      t_draw(traj, cycle, gpoint, a.seed, r, s);
      int nj = 0;
      bool cap = false;
      double iters = 0.0, phl = 0.0, t0 = 0.0, wsteps = 0.0;
      // Each lane walks its own segments (round 4; round 3 took the segments in lock step,
      // so a round waited at every boundary for its slowest lane).  mode 1: test the
      // segment end; 2: Newton on the crossing; 3: parked at a jump; 4: at a segment
      // boundary; 5: coefficients due; 0: done.  tc: the segment time c refers to; te: the
      // evaluation time after tc; n0 = ||c's ket||^2; gdt: the segment's length.  Jumps and
      // boundaries are served together, once TE_JB lanes wait or none evaluates.
      int mode = act ? 4 : 0, sg = -1;
      double gdt = 0.0, tc = 0.0, te = 0.0, lo = 0.0, hi = 0.0, n0 = 1.0;
      for (;;) {
        const bool run = (mode == 1 || mode == 2) && iters < T_ITER_CAP;
        if ((mode == 1 || mode == 2) && !run) {        // the evaluation cap
          cap = true;
          mode = 0;
        }
        if (__ballot(run)) wsteps += 1.0;
        if (run) {
          // an opaque offset per trip keeps the eigen-data loads next to their use (hoisted
          // out of the loop they would hold 92 registers across it)
          int o = 0;
          asm volatile("" : "+s"(o));
          double dn;
          const double nn = te_eval(lam + o, Wl + o, c, te, R, y, dn);
          iters += 1.0;
          if (mode == 1) {
            if (nn > r) {
              t0 += gdt;                               // no jump left in this segment: y is its end
              mode = 4;
            } else {
              lo = 0.0;
              hi = te;
              double tg = nn > 0.0 ? te * (log(n0 / r) / log(n0 / nn)) : 0.5 * te;
              if (!(tg > lo && tg < hi)) tg = 0.5 * (lo + hi);
              te = tg;
              mode = 2;
            }
          } else {
            if (nn > r) lo = te;
            else hi = te;
            if (fabs(nn - r) <= 2e-15 * r || hi - lo <= 4e-16 * hi) {
              mode = 3;                                // y: the ket at the crossing
            } else {
              double tn = dn < 0.0 ? te - (nn - r) / dn : lo - 1.0;
              if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
              te = tn;
            }
          }
        }
        const uint64_t sm = __ballot(mode == 3 || mode == 4);
        const uint64_t rm = __ballot(mode == 1 || mode == 2);
        if (!sm && !rm) break;
        if (sm && (!rm || __popcll(sm) >= TE_JB)) {
          if (mode == 3) {
            tc += te;
            double z[T_NV];
            ts_to_atom(y, z);
            const int ch = t_jump(z, s, R);
            const double nz = t_norm2(z);
            const double inv = nz > 0.0 ? 1.0 / sqrt(nz) : 0.0;
#pragma unroll
            for (int e = 0; e < T_NV; ++e) z[e] *= inv;
            ts_to_adapted(z, y);
            if (ch >= 0) {
              if (rec && nj < RYD_T_REC_JUMPS) {
                rec[RYD_T_REC_JUMP0 + 2 * nj] = t0 + tc;
                rec[RYD_T_REC_JUMP0 + 2 * nj + 1] = (double)ch;
              }
              ++nj;
            }
            ++cycle;
            if (nj >= T_MAX_JUMPS) {
              r = 0.0;
              cap = true;
            } else {
              t_draw(traj, cycle, gpoint, a.seed, r, s);
            }
            te = gdt - tc;
            mode = 5;
          }
          while (mode == 4) {                          // the next segment of positive length
            if (++sg >= nseg) {
              mode = 0;
              break;
            }
            const PointP q = load_point<PROTO>(a.prm, a.ld, ip);
            const Seg g = segment<PROTO>(q, sg, a.n_steps, a.shape);
            if (!(g.dt > 0.0)) continue;
            const double ph = (g.om_re == 0.0 && g.om_im == 0.0) ? phl : atan2(g.om_im, g.om_re);
            if (ph != phl) {
              ts_rotate(y, phl - ph);
              phl = ph;
            }
            gdt = g.dt;
            tc = 0.0;
            te = gdt;
            if (nj == 0 && sg == s_sgA[p] && s_nA[p] > r) {
              // before the first jump: no jump in segment A, whose end ket pass 1 has
#pragma unroll
              for (int e = 0; e < T_NV; ++e) y[e] = s_yA[p][e];
              t0 += gdt;
              continue;
            }
            mode = 5;
          }
          if (mode == 5) {
            te_coeffs(Wl, y, c);
            n0 = t_norm2(y);
            mode = 1;
            // before the first jump the segment-end norm of A (<= r here), or of a last B, is
            // pass 1's: straight to Newton
            const double kn = nj != 0 ? -1.0 : sg == s_sgA[p] ? s_nA[p] : sg == s_sgB[p] ? s_nB[p] : -1.0;
            if (kn >= 0.0) {
              lo = 0.0;
              hi = te;
              double tg = kn > 0.0 ? te * (log(n0 / r) / log(n0 / kn)) : 0.5 * te;
              if (!(tg > lo && tg < hi)) tg = 0.5 * (lo + hi);
              te = tg;
              mode = 2;
            }
          }
        }
      }
      ts_rotate(y, phl);
      double z[T_NV];
      ts_to_atom(y, z);
      const double nn = t_norm2(z);
      const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
      bool fin = nn > 0.0;
#pragma unroll
      for (int e = 0; e < T_NV; ++e) {
        z[e] *= inv;
        fin = fin && isfinite(z[e]);
      }
      if (rec) {
        for (int e = 0; e < T_NV; ++e) rec[e] = z[e];
        rec[RYD_T_REC_NJUMPS] = (double)nj;
        rec[RYD_T_REC_ITERS] = iters;
      }
      // this round's lane-iterations, shared out over the points of its active lanes
      const double share = 64.0 * wsteps / (double)max(__popcll(__ballot(act)), 1);
      if (act) {
        if (cap) capm |= 1u << p;
        if (!fin) nonfinm |= 1u << p;
        static_for<TE_P>([&](auto PP) {
          constexpr int pp = decltype(PP)::value;
          if (p == pp) {
            st_j[pp] += (double)nj;
            st_hit[pp] += nj > 0 ? 1.0 : 0.0;
            st_max[pp] = fmax(st_max[pp], (double)nj);
            st_use[pp] += iters;
            st_exec[pp] += share;
          }
        });
      }
      tp_walk += T_CLK() - tp_mark;
      tp_mark = T_CLK();
      if (!COOP && a.split == 1) {
        for (int pp = 0; pp < TE_P; ++pp) {             // each point's kets, in its jumper order
          const uint64_t m = __ballot(act && p == pp);
          if (!m) continue;
          te_reduce_round(stg, s_tot[pp], s_phi + pp * T_NV, z, act && p == pp, lane, (int)__builtin_ctzll(m),
                          __popcll(m));
        }
      } else if (act) {                                 // the merging wave reduces them in order
        double* kt = a.kets + ((size_t)ip * a.n_traj + traj) * T_NV;
#pragma unroll
        for (int e = 0; e < T_NV; ++e) kt[e] = z[e];
      }
      range_sync();
      tp_red += T_CLK() - tp_mark;
    }
  }
  tp_mark = T_CLK();
  const double ntr = (double)a.n_traj;
  // this wave's statistics of its points
  double sjv[TE_P], shv[TE_P], mjv[TE_P], suv[TE_P], sev[TE_P];
  bool capv[TE_P], nfv[TE_P];
  static_for<TE_P>([&](auto PP) {
    constexpr int p = decltype(PP)::value;
    sjv[p] = t_wave_sum(st_j[p]);
    shv[p] = t_wave_sum(st_hit[p]);
    mjv[p] = t_wave_max(st_max[p]);
    suv[p] = t_wave_sum(st_use[p]);
    sev[p] = t_wave_sum(st_exec[p]);
    capv[p] = __ballot((capm >> p) & 1u) != 0ull;
    nfv[p] = __ballot((nonfinm >> p) & 1u) != 0ull;
  });
  if constexpr (COOP) {
    // each range's statistics to LDS; the barrier also publishes every range's kets (global)
    // to the workgroup
    static_for<TE_P>([&](auto PP) {
      constexpr int p = decltype(PP)::value;
      if (lane == 0) {
        s_wst[p][kc][0] = sjv[p];
        s_wst[p][kc][1] = shv[p];
        s_wst[p][kc][2] = mjv[p];
        s_wst[p][kc][3] = suv[p];
        s_wst[p][kc][4] = sev[p];
        s_wst[p][kc][5] = capv[p] ? 1.0 : 0.0;
        s_wst[p][kc][6] = nfv[p] ? 1.0 : 0.0;
      }
    });
    __syncthreads();
  } else if (a.split > 1) {
    // ranges of a point in other waves: statistics to scratch, then the last wave of the
    // point to arrive merges (release: every lane's ket stores and these before the count;
    // acquire: the other waves' before the merge reads them)
    static_for<TE_P>([&](auto PP) {
      constexpr int p = decltype(PP)::value;
      if (lane == 0 && pt(p) < a.n && s_ok[p] == 1) {
        double* stt = a.stats + ((size_t)pt(p) * a.split + kc) * 8;
        stt[0] = sjv[p];
        stt[1] = shv[p];
        stt[2] = mjv[p];
        stt[3] = suv[p];
        stt[4] = sev[p];
        stt[5] = capv[p] ? 1.0 : 0.0;
        stt[6] = nfv[p] ? 1.0 : 0.0;
      }
    });
    __threadfence();
    __syncthreads();
    if (lane < TE_P) {
      const bool mine = pt(lane) < a.n && s_ok[lane] == 1;
      s_last[lane] = mine && atomicAdd(&a.arrive[pt(lane)], 1u) == (uint32_t)(a.split - 1) ? 1 : 0;
    }
    __syncthreads();
    bool anyl = false;
    for (int q = 0; q < TE_P; ++q) anyl = anyl || s_last[q] != 0;
    if (anyl) __threadfence();
  }
  double tp_arrive = 0.0, tp_merge = 0.0;
  (void)tp_arrive; (void)tp_merge;
  static_for<TE_P>([&](auto PP) {
    constexpr int p = decltype(PP)::value;
    const int64_t ip = pt(p);
    if (!(ip < a.n && s_ok[p] == 1)) return;
    double sjt = sjv[p], sht = shv[p], mjt = mjv[p], sut = suv[p], set = sev[p];
    bool any_cap = capv[p], any_nonfin = nfv[p];
    if (a.split > 1) {
      if (!COOP && !s_last[p]) return;
      double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (lane < a.split) {                            // lane k: range k's statistics
        if constexpr (COOP) {
#pragma unroll
          for (int e = 0; e < 7; ++e) v[e] = s_wst[p][lane][e];
        } else {
          const double* sk = a.stats + ((size_t)ip * a.split + lane) * 8;
#pragma unroll
          for (int e = 0; e < 7; ++e) v[e] = sk[e];
        }
      }
      sjt = t_wave_sum(v[0]);
      sht = t_wave_sum(v[1]);
      mjt = t_wave_max(v[2]);
      sut = t_wave_sum(v[3]);
      set = t_wave_sum(v[4]);
      any_cap = __ballot(v[5] != 0.0) != 0ull;
      any_nonfin = __ballot(v[6] != 0.0) != 0ull;
      // the point's kets in jumper (= trajectory) order -- the arithmetic of a one-wave
      // point: the jumper list again (up to TE_P * T_CHUNK at a time), then its kets 64 at a
      // time through te_reduce_round
      const uint64_t gpoint = (uint64_t)(a.point_offset + a.point_stride * ip);
      const double surv = s_surv[p];
      const double tp_m0 = T_CLK();
      (void)tp_m0;
      for (int c0 = 0; c0 < a.n_traj; c0 += TE_P * T_CHUNK) {
        const int cn = min(TE_P * T_CHUNK, a.n_traj - c0);
        int J = 0;
        const double tp_c0 = T_CLK();      // this chunk's jumper classification only
        (void)tp_c0;
        __syncthreads();
        for (int t0 = 0; t0 < cn; t0 += T_WAVE) {
          const uint32_t traj = (uint32_t)(c0 + t0 + lane);
          double r, sx;
          t_draw(traj, 0u, gpoint, a.seed, r, sx);
          const bool jumps = !(surv > r);
          const uint64_t m = __ballot(jumps);
          if (jumps) s_list[J + __popcll(m & ((1ull << lane) - 1ull))] = traj;
          J += __popcll(m);
        }
        __syncthreads();
        tp_arrive += T_CLK() - tp_c0;
        // (COOP: wave kc reduces its share of the elements, k in [6 kc / split, 6 (kc + 1) / split))
        const uint32_t kmask = COOP ? ((1u << (T_EPL * (kc + 1) / a.split)) - (1u << (T_EPL * kc / a.split))) : 0x3Fu;
        for (int j0 = 0; j0 < J; j0 += T_WAVE)
          te_reduce_global(stg, s_tot[p], s_phi + p * T_NV, a.kets + (size_t)ip * a.n_traj * T_NV, s_list + j0,
                           lane, min(T_WAVE, J - j0), kmask);
      }
      __syncthreads();
      tp_merge += T_CLK() - tp_m0;
    }
    double* orho = a.rho + (size_t)ip * a.ld_rho;
    double* ose = a.se + (size_t)ip * a.ld_se;
    double trl = 0.0, qpl = 0.0;
    te_write_moments(orho, ose, s_tot[p], s_phi + p * T_NV, lane, ntr, trl, qpl, l_rho);
    trl = t_wave_sum(trl);
    qpl = t_wave_sum(qpl);
    const double sw = t_wave_sum(ssl == p ? nsweep : 0.0);
    if (lane == 0) {
      double* sm = a.summ;
      const int64_t ldm = a.ld_summ;
      sm[RYD_TS_MEAN_JUMPS * ldm + ip] = sjt / ntr;
      sm[RYD_TS_FRAC_JUMPED * ldm + ip] = sht / ntr;
      sm[RYD_TS_MAX_JUMPS * ldm + ip] = mjt;
      sm[RYD_TS_TRACE * ldm + ip] = trl;
      sm[RYD_TS_QUBIT_POP * ldm + ip] = qpl;
      sm[RYD_TS_ITER_USEFUL * ldm + ip] = sut;         // evaluations of psi(t)
      sm[RYD_TS_ITER_EXEC * ldm + ip] = set;           // lane-evaluations issued for this point
      sm[RYD_TS_NLADDER * ldm + ip] = 1.0;             // eigen-decompositions
      sm[RYD_TS_NSQUARE * ldm + ip] = sw;              // Jacobi sweeps over the 5 block types
      sm[RYD_TS_RESERVED * ldm + ip] = 0.0;
      a.status[ip] = (any_cap ? RYD_STATUS_STEP_CAP : 0u) | (any_nonfin ? RYD_STATUS_NONFINITE : 0u);
#ifdef RYD_T_PROF
      sm[RYD_TS_MEAN_JUMPS * ldm + ip] = tp_pass1;
      sm[RYD_TS_FRAC_JUMPED * ldm + ip] = tp_cls;
      sm[RYD_TS_MAX_JUMPS * ldm + ip] = tp_walk;
      sm[RYD_TS_TRACE * ldm + ip] = tp_red;
      sm[RYD_TS_QUBIT_POP * ldm + ip] = T_CLK() - tp_mark;
      sm[RYD_TS_RESERVED * ldm + ip] = T_CLK() - tp_start;
      sm[RYD_TS_NLADDER * ldm + ip] = tp_rt0;          // the wave's start and end, 100 MHz clock
      sm[RYD_TS_NSQUARE * ldm + ip] = T_RTC();
      sm[RYD_TS_ITER_USEFUL * ldm + ip] = tp_jac;      // pass 1 through the eigen-decomposition
      sm[RYD_TS_ITER_EXEC * ldm + ip] = tp_merge;      // the merge (tp_arrive of it: its jumper lists)
#endif
    }
  });
}

// Trajectory ranges per point: enough waves to give every SIMD one (traj3e_kernel holds
// one wave per SIMD), each range whole 64-trajectory groups, the merge scratch (every
// trajectory's ket slot) bounded.  RYD_TE_SPLIT=k forces k (1: no split).
int te_split(int64_t n, int n_traj) {
  const int64_t npair = (n + TE_P - 1) / TE_P;
  int64_t simds = TE_SIMDS;                     // 4 SIMDs per CU of the current device
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      cus > 0)
    simds = 4 * (int64_t)cus;
  int k = (int)std::min<int64_t>(std::max<int64_t>(simds / std::max<int64_t>(npair, 1), 1), 64);
  const char* e = getenv("RYD_TE_SPLIT");
  if (e && e[0]) k = std::max(1, std::min(64, atoi(e)));
  k = std::min(k, std::max(1, n_traj / T_WAVE));
  if ((double)n * n_traj * T_NV * sizeof(double) > TE_SCRATCH_MAX) k = 1;
  return k;
}

template <int PROTO>
int te_launch_proto(const TrajArgs& ta, hipStream_t stream) {
  TrajArgs arg = ta;
  arg.npair = (ta.n + TE_P - 1) / TE_P;
  arg.split = te_split(ta.n, ta.n_traj);
  // split launches run cooperatively (one workgroup per wave pair, its ranges as its waves,
  // at most TE_COOP_MAX) unless RYD_TE_COOP=0 keeps the last-wave merge (the A/B; the
  // outputs are the same bits either way)
  const char* ce = getenv("RYD_TE_COOP");
  const bool coop_on = !(ce && ce[0] == '0');
  if (coop_on) arg.split = std::min(arg.split, TE_COOP_MAX);
  const bool coop = coop_on && arg.split > 1;
  if (arg.npair * arg.split > 0x7fffffffLL) return fail(RYD_ERR_INVALID, "batch too large for one launch");
  void* args[] = {(void*)&arg};
  void* buf = nullptr;
  hipError_t e = hipSuccess;
  if (arg.split > 1) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    hipMemPool_t pool = jp_pool(dev);
    if (!pool) return fail(RYD_ERR_ALLOC, "trajectory merge pool creation failed");
    const size_t nk = sizeof(double) * (size_t)ta.n * ta.n_traj * T_NV;
    // (the cooperative merge needs only the kets: statistics and arrival go through LDS)
    const size_t ns = coop ? 0 : sizeof(double) * (size_t)ta.n * arg.split * 8;
    const size_t na = coop ? 0 : sizeof(uint32_t) * (size_t)ta.n;
    HIPCHK(hipMallocFromPoolAsync(&buf, nk + ns + na, pool, stream));
    arg.kets = (double*)buf;
    arg.stats = coop ? nullptr : (double*)((char*)buf + nk);
    arg.arrive = coop ? nullptr : (uint32_t*)((char*)buf + nk + ns);
    if (!coop) e = hipMemsetAsync(arg.arrive, 0, na, stream);
  }
  if (e == hipSuccess && coop) {
    e = hipLaunchKernel((const void*)traj3e_kernel<PROTO, true>, dim3((unsigned)arg.npair),
                        dim3((unsigned)(T_WAVE * arg.split)), args, 0, stream);
  } else if (e == hipSuccess) {
    e = hipLaunchKernel((const void*)traj3e_kernel<PROTO>, dim3((unsigned)(arg.npair * arg.split)), dim3(T_WAVE), args,
                        0, stream);
  }
  const hipError_t ef = buf ? hipFreeAsync(buf, stream) : hipSuccess;   // on the error path too
  if (e != hipSuccess) return fail(RYD_ERR_HIP, std::string("traj3e launch: ") + hipGetErrorString(e));
  if (ef != hipSuccess) return fail(RYD_ERR_HIP, std::string("traj3e scratch free: ") + hipGetErrorString(ef));
  // points the exact kernel declined (RYD_STATUS_EXACT_FALLBACK): the L = 16 ladder walk
  TrajArgs fx = ta;
  fx.L = 16;
  fx.fix = 1;
  return ts_launch_proto<PROTO>(fx, stream);
}
