// ryd_coh4_prop.inc -- the process-map coherences for hilbert_space_dim = 4 (SURVEY.md §8
// a12 / f4).  Included by ryd_engine.hip after ryd_coh_prop.inc (cp_cheb, the DPP complex
// MACs, the quad sectors' phase-0 generator and frame) and ryd_dim4_prop.inc; the q = 0
// single-atom block is Gen4 / make_gen4's.
//
// With the mJ sublevels |r+>, |r-> the qubit matrix units still evolve in the excitation-
// number sectors of the dim-3 model (the comment above coherence_cheb_kernel), over
//   q = 0  factor: {e00, e11, e++, ex, ey, e--}     (Gen4's 6 x 6 real block)
//   q = -1 factor: {|0><1|, |0><r+|}                (|0><r-| is never reached: sigma+
//          drives |1> <-> |r+> only and the mJ jump |r-><r+| annihilates |0><r+|), the 2 x 2
//          block of make_cgen with |r+>'s decay raised by the mJ out-rate gm.
//   KIND 0 (0,-1): 12 complex coordinates k = 2 alpha + beta, KIND 1 (-1,0): k = 6 alpha + beta,
//   KIND 2 / 3 (-1,-1) / (-1,+1): 4 coordinates, as in dim 3.
// V P_R (x) P_R with P_R = P_r+ + P_r-: (V/2)(S (x) D + D (x) S), S on q = 0: e++, e-- -> 2x,
// ex, ey -> 1x; D: ex -> ey, ey -> -ex (apply4_V); on q = -1: S = diag(0, 1), D = i diag(0, 1).
// The output rows RYD_C_* are the dim-3 ones (the qubit block has the same support).
//
// coherence4_cheb_kernel: one lane per (point, input) and sector, a Chebyshev series per
// segment (LP shaped; RYD_COH_PROP=0): coherence_cheb_body (ryd_engine.hip) on Sector4, the
// description below, which also serves lindblad4_cheb_kernel.  coherence4_prop_kernel:
// coherence_prop_kernel's mapping -- one 16-lane DPP row per point, lane c < 12 builds column
// c of the (0,-1) phase-0 propagator, squarings in registers (the 2 columns with the q = 0
// atom in |0><0| feed only themselves: 124 complex products instead of 144), the quad sectors
// on quads 0 and 1 of the same row.  c4_sector repeats cp_sector's control flow (see DESIGN.md
// section 0 for why the two are not one body).

constexpr int C4_NMAX = 12;

__device__ __forceinline__ CGen make_cgen4(const Seg& g, double d1, const double* r, double gm, double s,
                                           bool conj) {
  CGen c = make_cgen(g, d1, r, s, conj);
  c.m11r = -0.5 * s * (r[0] + r[1] + r[2] + gm);
  return c;
}

// o[0..5] += M u[0..5] (apply4_one's rows) for one (re or im) component, stride-addressed.
// PH0: real Rabi frequency, the hy terms (exact zeros) left out.
template <int ST, bool PH0>
__device__ __forceinline__ void c4_m0_apply(const Gen4& a, const double* b, double* o) {
  const double u1 = b[1 * ST], u2 = b[2 * ST], u3 = b[3 * ST], u4 = b[4 * ST], u5 = b[5 * ST];
  const double u25 = u2 + u5;
  o[0] = fma(a.g0, u25, o[0]);
  if constexpr (PH0) {
    o[1 * ST] = fma(a.g1, u25, fma(-a.hx2, u4, o[1 * ST]));
    o[2 * ST] = fma(a.mg, u2, fma(a.hx2, u4, fma(a.gm, u5, o[2 * ST])));
    o[3 * ST] = fma(-a.G, u3, fma(a.hz2, u4, o[3 * ST]));
  } else {
    o[1 * ST] = fma(a.g1, u25, fma(a.hy2, u3, fma(-a.hx2, u4, o[1 * ST])));
    o[2 * ST] = fma(a.mg, u2, fma(-a.hy2, u3, fma(a.hx2, u4, fma(a.gm, u5, o[2 * ST]))));
    o[3 * ST] = fma(a.hy, u2 - u1, fma(-a.G, u3, fma(a.hz2, u4, o[3 * ST])));
  }
  o[4 * ST] = fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o[4 * ST])));
  o[5 * ST] = fma(a.gm, u2, fma(a.mg, u5, o[5 * ST]));
}

// (o0, o1) += m (z0, z1) on the q = -1 pair at doubles p0 (|0><1|) and p1 (|0><r+|)
template <bool PH0>
__device__ __forceinline__ void c4_cblock(const CGen& m, const double* b, double* o, int p0, int p1) {
  const double z0r = b[p0], z0i = b[p0 + 1], z1r = b[p1], z1i = b[p1 + 1];
  if constexpr (PH0) {
    cp_cblock(cp_cgen0(m), z0r, z0i, z1r, z1i, o[p0], o[p0 + 1], o[p1], o[p1 + 1]);
  } else {
    CMAC(o[p0], o[p0 + 1], m.m00r, m.m00i, z0r, z0i);
    CMAC(o[p0], o[p0 + 1], m.m01r, m.m01i, z1r, z1i);
    CMAC(o[p1], o[p1 + 1], m.m10r, m.m10i, z0r, z0i);
    CMAC(o[p1], o[p1 + 1], m.m11r, m.m11i, z1r, z1i);
  }
}

// o += 2Y b on the (0,-1) (KIND 0) or (-1,0) (KIND 1) sector, 24 doubles: Q0 the q = 0 atom's
// block (A for KIND 0, B for KIND 1), Qm the q = -1 atom's
template <int KIND, bool PH0>
__device__ __forceinline__ void apply4_coh(const Gen4& Q0, const CGen& Qm, double vs, const double* b, double* o) {
  // doubles: KIND 0 4 al + 2 be + c, KIND 1 12 al + 2 be + c
  constexpr int S0 = KIND == 0 ? 4 : 2;          // stride of the q = 0 index
  constexpr int S1 = KIND == 0 ? 2 : 12;         // stride of the q = -1 index
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c) c4_m0_apply<S0, PH0>(Q0, b + S1 * j + c, o + S1 * j + c);
#pragma unroll
  for (int a = 0; a < 6; ++a) c4_cblock<PH0>(Qm, b, o, S0 * a, S0 * a + S1);
  // V on the |0><r+| half: S (x) D (i x the S weight) and D (x) S (ex -> ey, ey -> -ex)
#pragma unroll
  for (int a = 2; a < 6; ++a) {
    const double sa = (a == 2 || a == 5) ? 2.0 * vs : vs;
    o[S0 * a + S1] = fma(-sa, b[S0 * a + S1 + 1], o[S0 * a + S1]);
    o[S0 * a + S1 + 1] = fma(sa, b[S0 * a + S1], o[S0 * a + S1 + 1]);
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    o[S0 * 4 + S1 + c] = fma(vs, b[S0 * 3 + S1 + c], o[S0 * 4 + S1 + c]);
    o[S0 * 3 + S1 + c] = fma(-vs, b[S0 * 4 + S1 + c], o[S0 * 3 + S1 + c]);
  }
}

// ---- hilbert_space_dim = 4 for the per-lane Chebyshev bodies (ryd_engine.hip) -----------
// Per-atom q = 0 block {e00, e11, e++, ex, ey, e--}, q = -1 block {|0><1|, |0><r+|}, the mJ
// mixing rates GMJ_A / GMJ_B as extra parameter columns.
struct Sector4 {
  static constexpr int NB = 6;                 // q = 0 block of one atom
  static constexpr int NS = NB * NB;           // the real (0,0) sector (state vector)
  static constexpr int NROW = 2 * NB;          // complex coordinates of a row sector
  struct Mj {                                  // the extra parameter columns
    double a, b;
  };
  __device__ static __forceinline__ Mj load_mj(const double* prm, int64_t ldp, int64_t i) {
    return {col(prm, RYD_P_GMJ_A, ldp, i), col(prm, RYD_P_GMJ_B, ldp, i)};
  }
  __device__ static __forceinline__ bool mj_valid(const Mj& m) { return gmj_valid(m.a, m.b); }
  __device__ static __forceinline__ bool mj_valid(bool ok, const Mj& m) { return gmj_valid(ok, m.a, m.b); }
  __device__ static __forceinline__ double rate_extra(const Mj& m) {           // their term of the rate sum
    return 2.0 * (fabs(m.a) + fabs(m.b));
  }
  __host__ __device__ static constexpr bool population(int a) { return a < 3 || a == 5; }   // e00, e11, e++, e--

  struct StateGen {
    Gen4 A, B;
  };
  // SYM (identical atoms): B is A
  template <bool SYM>
  __device__ static __forceinline__ StateGen state_gen(const Seg& g, const PointP& q, const Mj& m, double sc) {
    const Gen4 A = make_gen4(g, q.d1, q.gA, m.a, sc);
    return {A, SYM ? A : make_gen4(g, q.d1, q.gB, m.b, sc)};
  }
  template <bool SYM>
  __device__ static __forceinline__ void state_apply(const StateGen& G, double vs, const double (&b)[NS],
                                                     double (&o)[NS]) {
    apply4_one<6>(G.A, b, o);
    apply4_one<1>(G.B, b, o);
    apply4_V(vs, b, o);
  }

  // sector KIND's generator blocks: a row sector reads Q0 (the q = 0 atom: A for KIND 0, B for
  // KIND 1) and Qm (the other atom's q = -1 block), the quads Am and Bm (B's block conjugated
  // for KIND 3, the (-1,+1) sector)
  struct RowGen {
    Gen4 Q0;
    CGen Qm;
  };
  struct QuadGen {
    CGen Am, Bm;
  };
  template <int KIND>
  __device__ static __forceinline__ auto coh_gen(const Seg& g, const PointP& q, const Mj& m, double sc) {
    if constexpr (KIND == 0)
      return RowGen{make_gen4(g, q.d1, q.gA, m.a, sc), make_cgen4(g, q.d1, q.gB, m.b, sc, false)};
    else if constexpr (KIND == 1)
      return RowGen{make_gen4(g, q.d1, q.gB, m.b, sc), make_cgen4(g, q.d1, q.gA, m.a, sc, false)};
    else
      return QuadGen{make_cgen4(g, q.d1, q.gA, m.a, sc, false), make_cgen4(g, q.d1, q.gB, m.b, sc, KIND == 3)};
  }
  // the quads have no q = 0 factor: dim 3's apply with those blocks zero
  template <int KIND, typename G>
  __device__ static __forceinline__ void coh_apply(const G& c, double vs, const double* b, double* o) {
    if constexpr (KIND < 2) apply4_coh<KIND, false>(c.Q0, c.Qm, vs, b, o);
    else apply_coh<KIND>(Gen{}, Gen{}, c.Am, c.Bm, vs, b, o);
  }
};

// the four sectors in one launch, as coherence_cheb_kernel
template <int PROTO>
__global__ __launch_bounds__(BLOCK) void coherence4_cheb_kernel(const double* __restrict__ prm, int64_t n,
                                                                int64_t ldp, double* __restrict__ out, int64_t ldo,
                                                                uint32_t* __restrict__ status, int n_steps,
                                                                int shape, int64_t b0, int64_t b1, int64_t b2) {
  coherence_cheb_body<PROTO, Sector4>(prm, n, ldp, out, ldo, status, n_steps, shape, b0, b1, b2);
}

// ---- the propagator kernel -------------------------------------------------------------
// coordinates of the invariant block (the q = 0 atom in |0><0|)
template <int K>
__host__ __device__ constexpr bool c4_inv(int k) { return K == 0 ? k < 2 : (k % 6 == 0); }

// acc += column (lane) of v v for the (0,-1) / (-1,0) sector (12 complex coordinates)
template <int K>
__device__ __forceinline__ void c4_square_row(const double (&v)[24], double (&acc)[24]) {
  static_for<12>([&](auto MM) {
    constexpr int m = decltype(MM)::value;
    const double br = v[2 * m], bi = v[2 * m + 1];
    if constexpr (c4_inv<K>(m)) {            // feeds the invariant rows only
      constexpr int k0 = 0, k1 = K == 0 ? 1 : 6;
      cmac2_row<m, m == 0>(acc[2 * k0], acc[2 * k0 + 1], acc[2 * k1], acc[2 * k1 + 1], v[2 * k0], v[2 * k0 + 1],
                           v[2 * k1], v[2 * k1 + 1], br, bi);
    } else {
      static_for<6>([&](auto KK) {
        constexpr int k0 = 2 * decltype(KK)::value, k1 = k0 + 1;
        cmac2_row<m, false>(acc[2 * k0], acc[2 * k0 + 1], acc[2 * k1], acc[2 * k1 + 1], v[2 * k0], v[2 * k0 + 1],
                            v[2 * k1], v[2 * k1 + 1], br, bi);
      });
    }
  });
}

// coordinate k of R_th u on a row sector (cp_frame_at's roles: ex is index 3, ey index 4 of
// the q = 0 factor, e-- does not rotate; the q = -1 factor's |0><r+| carries e^{-i th})
template <int K>
__device__ __forceinline__ double2 c4_frame_at(const double2* u, int k, double c1, double s1) {
  const int a = K == 0 ? (k >> 1) : (k % 6);   // q = 0 index
  const int p = K == 0 ? (k & 1) : (k / 6);    // q = -1 index
  constexpr int d = K == 0 ? 2 : 1;
  double2 z = u[k];
  if (a == 3) {                                  // x' = c x + s y
    const double2 y = u[k + d];
    z = make_double2(fma(c1, z.x, s1 * y.x), fma(c1, z.y, s1 * y.y));
  } else if (a == 4) {                           // y' = -s x + c y
    const double2 x = u[k - d];
    z = make_double2(fma(c1, z.x, -s1 * x.x), fma(c1, z.y, -s1 * x.y));
  }
  const double pc = p == 1 ? c1 : 1.0, ps = p == 1 ? -s1 : 0.0;
  return make_double2(fma(pc, z.x, -ps * z.y), fma(pc, z.y, ps * z.x));
}

// One sector group of one row (cp_sector for dim 4).  K = 0 / 1: the 12-coordinate row
// sectors; K = 2: the quad pair.
template <int PROTO, int K>
__device__ __forceinline__ void c4_sector(const double* prm, int64_t ldp, bool valid, int n_steps, int shape, int l,
                                          double2* Ul, double2* stg, lds_zero_t* zl, double* __restrict__ out,
                                          int64_t ldo, int64_t i, bool live, bool mirror, uint32_t& stat) {
  constexpr bool QUAD = K == 2;
  constexpr int n = QUAD ? 4 : 12;
  constexpr int NV = 2 * n;
  constexpr int NIN = QUAD ? 1 : 2;
  const int qd = QUAD ? (l >> 2) : 0;            // quad of the row: 0 (-1,-1), 1 (-1,+1), 2-3 idle
  const bool k3 = QUAD && qd == 1;
  const int e = QUAD ? (l & 3) : l;
  const bool col_ = QUAD ? qd < 2 : l < n;       // this lane builds a column / carries a coordinate
  double2* U = Ul + (QUAD ? 16 * (qd & 1) : 0);  // U[c][k] at U[c * n + k]
  double2* sg = stg + (QUAD ? 4 * (qd & 1) : 0);
  auto frame = [&](const double2* u, int k, double c1, double s1) {
    if constexpr (QUAD) return cp_frame_at<2>(u, k, k3, c1, s1, c1 * c1 - s1 * s1, 2.0 * s1 * c1);
    else return c4_frame_at<K>(u, k, c1, s1);
  };
  double2 u[NIN];
#pragma unroll
  for (int s = 0; s < NIN; ++s) {
    const int k0 = s == 0 ? 0 : (K == 0 ? 2 : 1);
    u[s] = make_double2(col_ && e == k0 ? 1.0 : 0.0, 0.0);
  }
  double kw = -1.0, kdl = 0.0, kdt = -1.0;       // the propagator's key
  double fc = 1.0, fs = 0.0;                     // the frame e^{i phi} the inputs are carried in
  const int nseg = n_segments<PROTO>(n_steps);
  for (int sgi = 0; sgi < nseg; ++sgi) {
    // the point's parameters reloaded per segment (L2 hits) rather than held across the build
    const double* pq = prm;
    asm volatile("" : "+s"(pq));
    const PointP q = load_point<PROTO>(pq, ldp, i);
    const double gmA = col(pq, RYD_P_GMJ_A, ldp, i), gmB = col(pq, RYD_P_GMJ_B, ldp, i);
    const Seg g = segment<PROTO>(q, sgi, n_steps, shape);
    const bool act = valid && g.dt > 0.0;
    const double w = 0.5 * sqrt(g.om_re * g.om_re + g.om_im * g.om_im);
    const bool rebuild = act && (w != kw || g.dl != kdl || g.dt != kdt);
    double uc = fc, us = fs;
    if (w > 0.0) {
      const double m = 1.0 / (2.0 * w);
      uc = g.om_re * m;
      us = g.om_im * m;
    }
    if (rebuild) {
      kw = w;
      kdl = g.dl;
      kdt = g.dt;
    }
    if (__ballot(rebuild)) {
      // ---- U = exp(L(phase 0) dt): Chebyshev columns at dt / 2^s, then s squarings ----
      double rsum = 2.0 * (fabs(gmA) + fabs(gmB));
#pragma unroll
      for (int c = 0; c < 4; ++c) rsum += fabs(q.gA[c]) + fabs(q.gB[c]);
      Seg g0;
      g0.om_re = 2.0 * kw;
      g0.om_im = 0.0;
      g0.dl = kdl;
      g0.dt = kdt;
      double emin, emax;
      // V drops out of the (-1,+1) sector: its bound (and squaring count) leaves V out
      h_bounds(g0, (QUAD && k3) ? 0.0 : q.V, q.d1, emin, emax);
      const double omega = (emax - emin) + rsum;
      const double x = omega * kdt;
      const bool capped = rebuild && !(x <= X_CAP);
      if (capped) stat |= RYD_STATUS_STEP_CAP;
      const bool bld = rebuild && !capped && (!QUAD || qd < 2);
      const int s = (bld && x > CP_XS) ? (int)ceil(log2(x / CP_XS)) : 0;
      const double xs = ldexp(x, -s);
      const double sc = 2.0 / omega;
      const bool cact = bld && xs > X_SKIP;
      double v[NV];
      if constexpr (QUAD) {
        const CpCGen0 Am = cp_cgen0(make_cgen4(g0, q.d1, q.gA, gmA, sc, false));
        const CpCGen0 Bm = cp_cgen0(make_cgen4(g0, q.d1, q.gB, gmB, sc, k3));
        const double vs = k3 ? 0.0 : sc * 0.5 * q.V;
        const CpGen0 Z = {};
        cp_cheb<NV, true>(v, xs, cact,
                          [&](const double (&b)[NV], double (&o)[NV]) { cp_apply0<2>(Z, Z, Am, Bm, vs, b, o); });
      } else {
        const Gen4 Q0 = K == 0 ? make_gen4(g0, q.d1, q.gA, gmA, sc) : make_gen4(g0, q.d1, q.gB, gmB, sc);
        const CGen Qm = K == 0 ? make_cgen4(g0, q.d1, q.gB, gmB, sc, false)
                               : make_cgen4(g0, q.d1, q.gA, gmA, sc, false);
        const double vs = sc * 0.5 * q.V;
        cp_cheb<NV, false>(v, xs, cact,
                           [&](const double (&b)[NV], double (&o)[NV]) { apply4_coh<K, true>(Q0, Qm, vs, b, o); });
      }
      // squarings: U <- U U in registers; a row (a quad's bank) with fewer levels stops early
      const int smax = __builtin_amdgcn_readfirstlane(wave_max(s));
      const int smax1 = QUAD ? __builtin_amdgcn_readfirstlane(wave_max(k3 ? s : 0)) : 0;
      const int smax0 = QUAD ? __builtin_amdgcn_readfirstlane(wave_max(k3 ? 0 : s)) : 0;
      // ping-pong v -> w -> v; the accumulators are cleared by LDS reads of zero words
      auto square = [&](const double (&a)[NV], double (&o)[NV], int lvl) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          o[j] = zl[j];
          asm volatile("" ::: "memory");
        }
        if constexpr (QUAD) {
          if (lvl < smax0) cp_square_bank<0>(a, o);
          if (lvl < smax1) cp_square_bank<1>(a, o);
        } else {
          c4_square_row<K>(a, o);
        }
      };
      {
        double w2[NV];
        for (int qq = 0; qq < smax; qq += 2) {
          if (qq < s) square(v, w2, qq);       // uniform over a row (a bank)
          if (qq + 1 < s) {
            square(w2, v, qq + 1);
          } else if (qq < s) {
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] = w2[j];
          }
        }
      }
      cp_wsync();
      if (rebuild && col_) {
#pragma unroll
        for (int k = 0; k < n; ++k) U[e * n + k] = make_double2(v[2 * k], v[2 * k + 1]);
      }
      cp_wsync();
    }
    if (!act) continue;
    // ---- the segment: u <- U R_{-(phi - phi_prev)} u ----
    const double dc = fma(uc, fc, us * fs), ds = fma(us, fc, -uc * fs);   // e^{i Delta}
    fc = uc;
    fs = us;
    const double c1 = dc, s1 = -ds;                                     // R_{-Delta}
#pragma unroll
    for (int s = 0; s < NIN; ++s) {
      cp_wsync();
      if (col_) sg[s * C4_NMAX + e] = u[s];
    }
    cp_wsync();
    if (col_) {
      double2 acc[NIN];
#pragma unroll
      for (int s = 0; s < NIN; ++s) acc[s] = make_double2(0.0, 0.0);
#pragma unroll
      for (int c = 0; c < n; ++c) {
        const double2 a = U[c * n + e];          // U[e][c]
#pragma unroll
        for (int s = 0; s < NIN; ++s) {
          const double2 z = frame(sg + s * C4_NMAX, c, c1, s1);
          acc[s].x = fma(a.x, z.x, fma(-a.y, z.y, acc[s].x));
          acc[s].y = fma(a.x, z.y, fma(a.y, z.x, acc[s].y));
        }
      }
#pragma unroll
      for (int s = 0; s < NIN; ++s) u[s] = acc[s];
    }
  }
  // ---- back to the lab frame: v = R_phi u; the qubit images ----
#pragma unroll
  for (int s = 0; s < NIN; ++s) {
    cp_wsync();
    if (col_) sg[s * C4_NMAX + e] = u[s];
  }
  cp_wsync();
  double2 z[NIN];
#pragma unroll
  for (int s = 0; s < NIN; ++s) z[s] = col_ ? frame(sg + s * C4_NMAX, e, fc, fs) : make_double2(0.0, 0.0);
  bool fin = true;
#pragma unroll
  for (int s = 0; s < NIN; ++s) fin = fin && isfinite(z[s].x) && isfinite(z[s].y);
  if (col_ && !fin) stat |= RYD_STATUS_NONFINITE;
  if (!live) return;
  // K0 o0 = C[0][0] (coordinate 0), o1 = C[1][0] (2); K1 C[0][0] (0), C[0][1] (1); K2/K3 C[0][0].
  // mirror (K0, identical atoms): the (-1,0) sector's images are the same numbers
  if constexpr (!QUAD) {
    const int i1 = K == 0 ? 2 : 1;
#pragma unroll
    for (int s = 0; s < NIN; ++s) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t == 1 && !mirror) break;
        const int base = (t == 0 ? (K == 0 ? RYD_C_K0 : RYD_C_K1) : RYD_C_K1) + 4 * s;
        if (l == 0) {
          out[(int64_t)(base + 0) * ldo + i] = z[s].x;
          out[(int64_t)(base + 1) * ldo + i] = z[s].y;
        }
        if (l == i1) {
          out[(int64_t)(base + 2) * ldo + i] = z[s].x;
          out[(int64_t)(base + 3) * ldo + i] = z[s].y;
        }
      }
    }
  } else if (col_ && e == 0) {
    const int base = k3 ? RYD_C_K3 : RYD_C_K2;
    out[(int64_t)(base + 0) * ldo + i] = z[0].x;
    out[(int64_t)(base + 1) * ldo + i] = z[0].y;
  }
}

template <int PROTO>
__global__ __launch_bounds__(CP_BLOCK) __attribute__((amdgpu_waves_per_eu(RYD_CP_OCC, 8))) void coherence4_prop_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ out, int64_t ldo,
    uint32_t* __restrict__ status, int n_steps, int shape) {
  __shared__ double2 s_U[CP_NR][C4_NMAX * C4_NMAX];
  __shared__ double2 s_stg[CP_NR][2 * C4_NMAX];
  __shared__ double s_zero[2 * C4_NMAX];        // zero words: squaring accumulator clears
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  if (threadIdx.x < 2 * C4_NMAX) s_zero[threadIdx.x] = 0.0;   // one wave: ordered before the first read
  lds_zero_t* zl = (lds_zero_t*)s_zero;
  const int64_t gi = xcd_block(blockIdx.x, gridDim.x) * CP_NR + row;   // XCD-aware order (ryd_sym16.inc)
  const bool live = gi < n;
  const int64_t i = live ? gi : n - 1;
  bool valid, sym = true;
  {
    const PointP q = load_point<PROTO>(prm, ldp, i);
    const double gmA = col(prm, RYD_P_GMJ_A, ldp, i), gmB = col(prm, RYD_P_GMJ_B, ldp, i);
    valid = live && point_valid<PROTO>(q, n_steps) && gmj_valid(gmA, gmB);
#pragma unroll
    for (int c = 0; c < 4; ++c) sym = sym && q.gA[c] == q.gB[c];
    sym = sym && gmA == gmB;
  }
  uint32_t stat = 0u;
  double2* Ul = s_U[row];
  double2* stg = s_stg[row];
  // (-1,0) is the atom-swap mirror of (0,-1) when the atoms are identical; otherwise it is built
  c4_sector<PROTO, 0>(prm, ldp, valid, n_steps, shape, l, Ul, stg, zl, out, ldo, i, live, sym, stat);
  c4_sector<PROTO, 2>(prm, ldp, valid, n_steps, shape, l, Ul, stg, zl, out, ldo, i, live, false, stat);
  if (__ballot(!sym && live))
    c4_sector<PROTO, 1>(prm, ldp, valid, n_steps, shape, l, Ul, stg, zl, out, ldo, i, live && !sym, false, stat);
  uint32_t st = stat;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) st |= (uint32_t)__shfl_xor((int)st, o, 16);
  if (live && !valid) st |= RYD_STATUS_BAD_INPUT;
  if (live && l == 0) status[i] = st;
}
