// ryd_coh_sched.inc -- the process-map coherences of a custom pulse schedule
// (included by ryd_engine.hip after ryd_coh_prop.inc and ryd_sched_table.inc, whose building
// blocks it takes unchanged: cp_cheb, cp_apply0, cp_square_row / cp_square_bank, cp_frame_at,
// make_gen / make_cgen, the Gershgorin bound, CP_XS, X_CAP; SCHED_TABLE_VALID, SCHED_CHUNK_*,
// sched16_point_valid).  The last user of those macros: it drops them at its end.
//
// ryd_run_schedule_coherences[_device]: coherence_prop_kernel with the segments read from the
// caller's table instead of segment<PROTO>().  Lindblad, dim 3, identical atoms.
//
// Layout.  That of coherence_prop_kernel: one wave = 4 points, one 16-lane DPP row each, blocks
// in xcd_block order.  Sector (0,-1) is built on lanes 0-9 of the row (column c on lane c), the
// (-1,-1) / (-1,+1) pair on quads 0 and 1; the (-1,0) images are the atom-swap mirror of (0,-1)
// and are copied into the RYD_C_K1 rows.  The two sector groups run as two passes over the
// table (cs_sector<0>, then cs_sector<2>): a pass holds one sector's column, its squaring
// partner and the Chebyshev pair (80 doubles per lane for (0,-1)) at 2 waves per SIMD, and a
// fused loop would carry the other group's inputs, frame and key through that build.  The
// second pass reads the table again: L2 hits, 32 bytes per segment and point.
//
// Table.  Read by the protocol of ryd_sched_table.inc, with fast_sincos for the phase -- the
// function, and therefore the frame, of the state kernel, so that the states of
// ryd_run_schedule and these coherences join into one map.
//
// Memo.  A sector's propagator exp(L(phase 0) dt) depends on the key and the point's scalars
// only.  It is rebuilt when the segment's key differs (==, on the three products) from the key
// of the row's last build, so a key that returns to an earlier value builds again.  The wave
// enters the build when any row needs to; a row that does not need to runs it with inactive
// lanes and writes nothing, so its propagator in LDS stays bit for bit and a row's output never
// depends on its neighbours.  Before the first build the key is (0, 0, 0), which no segment of
// positive duration equals.  The chunk's five values per lane, the frame and the inputs are
// parked in LDS across a build (ryd_sched16.inc parks its states the same way).
//
// Segments.  A segment of duration zero (x / Omega == 0) is skipped and keeps the frame.
// a_s = 0 with x_s > 0 is free evolution: the generator has no drive, any frame is right, and
// the inputs are carried into the frame of the table's phi_s as the state kernel carries its
// states.
//
// Validity.  The pass of ryd_sched_table.inc.  An invalid row takes part in no segment and no
// build and writes the untouched inputs' images, E(|a><b|) = |a><b|, flagged
// BAD_INPUT (as coherence_prop_kernel does for a refused point).
//
// Step cap.  A build whose argument (the Gershgorin width plus the rates, times dt) exceeds X_CAP
// in either sector group -- both bounds are evaluated in both passes, so the passes agree -- sets
// STEP_CAP.  The row writes no propagator, takes part in nothing from then on and, like an
// invalid row, ends with the identity images: it never applies an LDS slice it has not written.

constexpr int CS_NPARK = 11;                   // per lane: the chunk's key (3), cos, sin; the frame; the inputs

// One sector group of one row over the whole table.  K = 0: (0,-1) and its mirror (-1,0);
// K = 2: the quad pair.  `valid` is the row's (by value: a capped row drops out of this pass,
// and the other pass finds the same cap itself).
template <int K>
__device__ __forceinline__ void cs_sector(const double* prm, int64_t ldp, bool valid,
                                          const double* __restrict__ tab, int n_seg, int l, double2* Ul,
                                          double2* stg, lds_zero_t* zl, double (*park)[CS_NPARK],
                                          double* __restrict__ out, int64_t ldo, int64_t i, bool live,
                                          uint32_t& stat) {
  constexpr bool QUAD = K == 2;
  constexpr int n = QUAD ? 4 : 10;
  constexpr int NV = 2 * n;
  constexpr int NIN = QUAD ? 1 : 2;              // inputs of this sector
  const int qd = QUAD ? (l >> 2) : 0;            // quad of the row: 0 (-1,-1), 1 (-1,+1), 2-3 idle
  const bool k3 = QUAD && qd == 1;
  const int e = QUAD ? (l & 3) : l;              // coordinate / column of this lane
  const bool col = QUAD ? qd < 2 : l < n;        // this lane builds a column / carries a coordinate
  double2* U = Ul + (QUAD ? 16 * (qd & 1) : 0);  // this lane's sector: U[c][k] at U[c * n + k]
  double2* sg = stg + (QUAD ? 4 * (qd & 1) : 0);
  // inputs: K0 C[0][0], C[1][0] (coordinates 0, 2); K2/K3 C[0][0]
  double2 u[NIN];
#pragma unroll
  for (int s = 0; s < NIN; ++s) u[s] = make_double2(col && e == 2 * s ? 1.0 : 0.0, 0.0);
  double La = 0.0, Ld = 0.0, Lt = 0.0;           // the key of the row's last build
  double fc = 1.0, fs = 0.0;                     // the frame e^{i phi} the inputs are carried in
  for (int s0 = 0; s0 < n_seg; s0 += 16) {
    // ---- the chunk: lane l's segment s0 + l (clamped), key and phase
    double Ka, Kd, Kt, Pc, Ps;
    {
      const double* pp = prm;
      asm volatile("" : "+s"(pp));               // re-read (a cache hit), not kept live through the builds
      const double Om = pp[(int64_t)RYD_P_OMEGA * ldp + i];
      SCHED_CHUNK_LOAD(tab, n_seg, s0, l, Om)
      if (!valid) {
        SCHED_CHUNK_NEUTRAL()
      }
    }
    const int cnt = min(16, n_seg - s0);
    for (int j = 0; j < cnt; ++j) {
      // segment s0 + j: lane 0 of the row after j rotations
      const double a = row_bcast<0>(Ka), dl = row_bcast<0>(Kd), dt = row_bcast<0>(Kt);
      const bool need = valid && dt != 0.0 && !(a == La && dl == Ld && dt == Lt);
      if (__ballot(need)) {
        // ---- U = exp(L(phase 0) dt): Chebyshev columns at dt / 2^s, then s squarings ----
        park[l][0] = Ka;
        park[l][1] = Kd;
        park[l][2] = Kt;
        park[l][3] = Pc;
        park[l][4] = Ps;
        park[l][5] = fc;
        park[l][6] = fs;
#pragma unroll
        for (int s2 = 0; s2 < NIN; ++s2) {
          park[l][7 + 2 * s2] = u[s2].x;
          park[l][8 + 2 * s2] = u[s2].y;
        }
        if (need) {
          La = a;
          Ld = dl;
          Lt = dt;
        }
        const double* pq = prm;
        asm volatile("" : "+s"(pq));
        const PointP q = load_point<RYD_PROTO_LP_SQUARE>(pq, ldp, i);
        double rsum = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) rsum += fabs(q.gA[c]) + fabs(q.gB[c]);
        Seg g0;
        g0.om_re = La;
        g0.om_im = 0.0;
        g0.dl = Ld;
        g0.dt = Lt;
        // V drops out of the (-1,+1) sector: its bound (and squaring count) leaves V out.  Both
        // bounds decide the cap, in both passes.
        double eminV, emaxV, emin0, emax0;
        h_bounds_w(0.5 * La, Ld, q.V, q.d1, eminV, emaxV);
        h_bounds_w(0.5 * La, Ld, 0.0, q.d1, emin0, emax0);
        const double omV = (emaxV - eminV) + rsum, om0 = (emax0 - emin0) + rsum;
        const bool capped = need && !(omV * Lt <= X_CAP && om0 * Lt <= X_CAP);
        const double omega = (QUAD && k3) ? om0 : omV;
        const double x = omega * Lt;
        const bool bld = need && !capped && (!QUAD || qd < 2);
        const int s = (bld && x > CP_XS) ? (int)ceil(log2(x / CP_XS)) : 0;
        const double xs = ldexp(x, -s);
        const double sc = omega > 0.0 ? 2.0 / omega : 0.0;
        const bool cact = bld && xs > X_SKIP;
        double v[NV];
        if constexpr (QUAD) {
          // both quads run cp_apply0<2>: quad 1's (-1,+1) generator is the conjugated B block and
          // no V term
          const CpCGen0 Am = cp_cgen0(make_cgen(g0, q.d1, q.gA, sc, false));
          const CpCGen0 Bm = cp_cgen0(make_cgen(g0, q.d1, q.gB, sc, k3));
          const double vs = k3 ? 0.0 : sc * 0.5 * q.V;
          const CpGen0 Z = {};
          cp_cheb<NV, true>(v, xs, cact,
                            [&](const double (&b)[NV], double (&o)[NV]) { cp_apply0<2>(Z, Z, Am, Bm, vs, b, o); });
        } else {
          const CpGen0 A0 = cp_gen0(make_gen(g0, q.d1, q.gA, sc));
          const CpGen0 B0 = cp_gen0(make_gen(g0, q.d1, q.gB, sc));
          const CpCGen0 Am = cp_cgen0(make_cgen(g0, q.d1, q.gA, sc, false));
          const CpCGen0 Bm = cp_cgen0(make_cgen(g0, q.d1, q.gB, sc, false));
          const double vs = sc * 0.5 * q.V;
          cp_cheb<NV, false>(v, xs, cact,
                             [&](const double (&b)[NV], double (&o)[NV]) { cp_apply0<K>(A0, B0, Am, Bm, vs, b, o); });
        }
        // squarings: U <- U U in registers; a row (a quad's bank) with fewer levels stops early,
        // and in the quad layout each bank's instructions stop at its own wave maximum
        const int smax = __builtin_amdgcn_readfirstlane(wave_max(s));
        const int smax1 = QUAD ? __builtin_amdgcn_readfirstlane(wave_max(k3 ? s : 0)) : 0;
        const int smax0 = QUAD ? __builtin_amdgcn_readfirstlane(wave_max(k3 ? 0 : s)) : 0;
        // ping-pong v -> w -> v; the accumulators are cleared by LDS reads of zero words
        auto square = [&](const double (&a2)[NV], double (&o)[NV], int lvl) {
          asm volatile("" ::: "memory");         // re-read the zero words every level
#pragma unroll
          for (int k = 0; k < NV; ++k) {
            o[k] = zl[k];
            asm volatile("" ::: "memory");
          }
          if constexpr (QUAD) {
            if (lvl < smax0) cp_square_bank<0>(a2, o);
            if (lvl < smax1) cp_square_bank<1>(a2, o);
          } else {
            cp_square_row<K>(a2, o);
          }
        };
        {
          double w[NV];
          for (int qq = 0; qq < smax; qq += 2) {
            if (qq < s) square(v, w, qq);        // uniform over a row (a bank): its lanes all take part
            if (qq + 1 < s) {
              square(w, v, qq + 1);
            } else if (qq < s) {
#pragma unroll
              for (int k = 0; k < NV; ++k) v[k] = w[k];
            }
          }
        }
        cp_wsync();
        if (bld && col) {                        // only a row that built: the others keep their slice
#pragma unroll
          for (int k = 0; k < n; ++k) U[e * n + k] = make_double2(v[2 * k], v[2 * k + 1]);
        }
        cp_wsync();
        Ka = park[l][0];
        Kd = park[l][1];
        Kt = park[l][2];
        Pc = park[l][3];
        Ps = park[l][4];
        fc = park[l][5];
        fs = park[l][6];
#pragma unroll
        for (int s2 = 0; s2 < NIN; ++s2) u[s2] = make_double2(park[l][7 + 2 * s2], park[l][8 + 2 * s2]);
        if (capped) {                            // row-uniform: out of this pass, identity images
          stat |= RYD_STATUS_STEP_CAP;
          valid = false;
#pragma unroll
          for (int s2 = 0; s2 < NIN; ++s2) u[s2] = make_double2(col && e == 2 * s2 ? 1.0 : 0.0, 0.0);
          fc = 1.0;
          fs = 0.0;
        }
      }
      if (valid && dt != 0.0) {
        // ---- the segment: u <- U R_{-(phi - phi_prev)} u (inputs carried in the current frame) ----
        const double uc = row_bcast<0>(Pc), us = row_bcast<0>(Ps);
        const double dc = fma(uc, fc, us * fs), ds = fma(us, fc, -uc * fs);   // e^{i Delta}
        fc = uc;
        fs = us;
        const double c1 = dc, s1 = -ds;                                     // R_{-Delta}
        const double c2 = c1 * c1 - s1 * s1, s2 = 2.0 * s1 * c1;
#pragma unroll
        for (int s = 0; s < NIN; ++s) {
          cp_wsync();
          if (col) sg[s * CP_NMAX + e] = u[s];
        }
        cp_wsync();
        if (col) {
          double2 acc[NIN];
#pragma unroll
          for (int s = 0; s < NIN; ++s) acc[s] = make_double2(0.0, 0.0);
#pragma unroll
          for (int c = 0; c < n; ++c) {
            const double2 am = U[c * n + e];       // U[e][c]
#pragma unroll
            for (int s = 0; s < NIN; ++s) {
              const double2 z = cp_frame_at<K>(sg + s * CP_NMAX, c, k3, c1, s1, c2, s2);
              acc[s].x = fma(am.x, z.x, fma(-am.y, z.y, acc[s].x));
              acc[s].y = fma(am.x, z.y, fma(am.y, z.x, acc[s].y));
            }
          }
#pragma unroll
          for (int s = 0; s < NIN; ++s) u[s] = acc[s];
        }
      }
      SCHED_CHUNK_ROL1()
    }
  }
  // ---- back to the lab frame: v = R_phi u; the qubit images ----
  const double c2 = fc * fc - fs * fs, s2 = 2.0 * fs * fc;
#pragma unroll
  for (int s = 0; s < NIN; ++s) {
    cp_wsync();
    if (col) sg[s * CP_NMAX + e] = u[s];
  }
  cp_wsync();
  double2 z[NIN];
#pragma unroll
  for (int s = 0; s < NIN; ++s)
    z[s] = col ? cp_frame_at<K>(sg + s * CP_NMAX, e, k3, fc, fs, c2, s2) : make_double2(0.0, 0.0);
  bool fin = true;
#pragma unroll
  for (int s = 0; s < NIN; ++s) fin = fin && isfinite(z[s].x) && isfinite(z[s].y);
  if (col && !fin) stat |= RYD_STATUS_NONFINITE;
  if (!live) return;
  // K0: o0 = C[0][0] (coordinate 0), o1 = C[1][0] (2), and the same numbers as the (-1,0)
  // sector's images (identical atoms); K2 / K3: C[0][0]
  if constexpr (!QUAD) {
#pragma unroll
    for (int s = 0; s < NIN; ++s) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int base = (t == 0 ? RYD_C_K0 : RYD_C_K1) + 4 * s;
        if (l == 0) {
          out[(int64_t)(base + 0) * ldo + i] = z[s].x;
          out[(int64_t)(base + 1) * ldo + i] = z[s].y;
        }
        if (l == 2) {
          out[(int64_t)(base + 2) * ldo + i] = z[s].x;
          out[(int64_t)(base + 3) * ldo + i] = z[s].y;
        }
      }
    }
  } else if (col && e == 0) {
    const int base = k3 ? RYD_C_K3 : RYD_C_K2;
    out[(int64_t)(base + 0) * ldo + i] = z[0].x;
    out[(int64_t)(base + 1) * ldo + i] = z[0].y;
  }
}

__global__ __launch_bounds__(CP_BLOCK) __attribute__((amdgpu_waves_per_eu(RYD_CP_OCC, 8))) void
coherence_sched_kernel(const double* __restrict__ prm, int64_t n, int64_t ldp, const double* __restrict__ sched,
                       int64_t ldsc, int n_seg, double* __restrict__ out, int64_t ldo,
                       uint32_t* __restrict__ status) {
  __shared__ double2 s_U[CP_NR][CP_NMAX * CP_NMAX];
  __shared__ double2 s_stg[CP_NR][2 * CP_NMAX];
  __shared__ double s_zero[2 * CP_NMAX];        // zero words: squaring accumulator clears
  __shared__ double s_park[CP_NR][16][CS_NPARK];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  if (threadIdx.x < 2 * CP_NMAX) s_zero[threadIdx.x] = 0.0;   // one wave: ordered before the first read
  lds_zero_t* zl = (lds_zero_t*)s_zero;
  const int64_t gi = xcd_block(blockIdx.x, gridDim.x) * CP_NR + row;
  const bool live = gi < n;
  const int64_t i = live ? gi : n - 1;           // a row past the batch reads point n - 1
  // the row's table: point i <= n - 1 (ldsc = 0: the shared row)
  const double* __restrict__ tab = sched + i * ldsc;
  bool valid;
  {
    const PointP q = load_point<RYD_PROTO_LP_SQUARE>(prm, ldp, i);
    valid = live && sched16_point_valid(q);
  }
  SCHED_TABLE_VALID(valid, tab, n_seg, l, row)
  uint32_t stat = 0u;
  cs_sector<0>(prm, ldp, valid, tab, n_seg, l, s_U[row], s_stg[row], zl, s_park[row], out, ldo, i, live, stat);
  cs_sector<2>(prm, ldp, valid, tab, n_seg, l, s_U[row], s_stg[row], zl, s_park[row], out, ldo, i, live, stat);
  // the row's flags (every lane of the wave reaches this)
  uint32_t st = stat;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) st |= (uint32_t)__shfl_xor((int)st, o, 16);
  if (live && !valid) st |= RYD_STATUS_BAD_INPUT;
  if (live && l == 0) status[i] = st;
}

#undef SCHED_TABLE_VALID
#undef SCHED_CHUNK_LOAD
#undef SCHED_CHUNK_NEUTRAL
#undef SCHED_CHUNK_ROL1
#undef SCHED_CHUNK_ROR1
#undef SCHED_CHUNK_TO_LANE15
