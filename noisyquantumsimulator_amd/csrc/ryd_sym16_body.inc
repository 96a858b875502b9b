// ryd_sym16_body.inc -- the body of lindblad_sym16_kernel, included by ryd_sym16.inc inside
// each of its two kernel templates (textually, so that the one-wave kernels compile exactly
// as they did when this was their own body).  The including function provides PROTO, the
// kernel parameters, STATE (false: the summary-only twins, whose epilogue stores no state rows) and
//   BAL = 0: one wave per workgroup, one job (the three one-wave kernels);
//   BAL = 1: a wave of the balanced form's workgroup (LP square; `gpc` groups per workgroup,
//            `nohandoff`, `wt`): every LDS array gets a copy per wave, the job comes from the role
//            table, and the first build may be split with a partner wave (build16<S16Handoff>);
//   BAL = 2: the same, with `p32`: the first parameter load is one instruction per wave
//            (load_point16_row).  Both take the branch-free validity test (point_valid_flat).
  constexpr int NW = BAL ? S16_BAL_MAXW : 1;
  __shared__ __attribute__((aligned(16))) double UtW[NW][S16_PPW][NS][16];   // transpose, then output staging
  static_assert(sizeof(UtW[0]) >= sizeof(double) * S16_PPW * 4 * NC, "output staging must fit in Ut");
#ifdef RYD_S16_PROF
  double s16_ts[16];
  s16_ts[8] = (double)__builtin_amdgcn_s_memrealtime();
  S16_MARK(0);
  s16_ts[10] = s16_ts[11] = 0.0;             // balanced form: role and handoff record
  s16_ts[12] = 0.0;                          // balanced form: roles known, the consumer's flag cleared
  int bal_polls = 0;
#endif
  __shared__ double ZlW[NW][16];             // zero words: squaring accumulator clears, lane 15's row
  const int wv = BAL ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  double (&Ut)[S16_PPW][NS][16] = UtW[wv];
  double (&Zl)[16] = ZlW[wv];
  const int l = BAL ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
  const int p = l >> 4, r = l & 15;
  if (l < 16) Zl[l] = 0.0;                   // same wave: ordered before the first squaring
  // balanced form: the handoff slots of the (at most two) split jobs, and this wave's role
  __shared__ double Hcols[2][NS][64];        // (never referenced by the one-wave kernels: not allocated there)
  __shared__ int Hcnt[2][S16_BAL_NCNT][64];
  __shared__ int Hflag[2];
  S16Role role = {S16_BAL_WHOLE, 0};
  int64_t job = 0;
  if constexpr (BAL != 0) {
    role = s16_bal_role(gpc, wv);
    job = s16_bal_job(blockIdx.x, nwg, role.off);
    // No workgroup barrier.  LDS keeps what the last workgroup left, so a consumer clears its
    // own flag before its first poll (same wave, same address: ordered) and the producer only
    // sets it.  A consumer then acts only on a flag this workgroup's producer set after the
    // clear; in every other interleaving (the producer's store came first and was cleared) it
    // exhausts its polls and runs the producer's part itself -- the same bits.  The barrier
    // this replaces waited for the workgroup's last-dispatched wave (profiles/sym16_entry/).
    if (role.role == S16_BAL_CONSUMER)
      __hip_atomic_store(&Hflag[role.off - (gpc & ~3)], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    S16_MARK(12);
    // a job past the batch: its producer and its consumer both leave here, by the same test
    if (job >= (n + S16_PPW - 1) / S16_PPW) return;
    if (role.role != S16_BAL_WHOLE) __builtin_amdgcn_s_setprio(3);   // both halves of a split job: see s16_phase_prio
  }
  // the wave's first point (uniform, 64-bit) and this lane's byte offset from it, clamped
  // to the batch: every parameter address is an SGPR base plus this 32-bit offset
  const int64_t b0 = (BAL ? job : xcd_block(blockIdx.x, gridDim.x)) * S16_PPW;
  const int64_t i0 = b0 < n ? b0 : n - 1;    // a wave past the batch (padded grid) reads point n-1
  const int64_t last = n - 1 - i0;           // >= 0
  const unsigned po8 = 8u * (unsigned)min(p, last < S16_PPW - 1 ? (int)last : S16_PPW - 1);
  // loaded and validated once; the segment-0 build takes its inputs from here
  PointP q0l;
  if constexpr (p32 != 0) {
    q0l = load_point16_row<PROTO>(prm, ldp, i0, po8, r);
  } else {
    q0l = load_point16<PROTO>(prm, ldp, i0, po8);
  }
  S16_MARK(13);
  if constexpr (BAL != 0) s16_in_hand(q0l);
  const PointP q0 = q0l;
#ifdef RYD_S16_PROF
  asm volatile("s_waitcnt vmcnt(0)" ::"v"(q0.Om), "v"(q0.xi) : "memory");   // the stamp of "values in hand"
  S16_MARK(14);
#endif
  bool valid;
  if constexpr (BAL != 0) valid = point_valid_flat<PROTO>(q0);
  else valid = point_valid<PROTO>(q0, n_steps);
  const bool frame_ok =
      !(PROTO == RYD_PROTO_LP_SQUARE) || !valid || fabs(q0.xr * q0.xr + q0.xi * q0.xi - 1.0) <= 1e-14;
  S16_MARK(1);
  if constexpr (BAL != 0) {
    if (role.role == S16_BAL_WHOLE) __builtin_amdgcn_s_setprio(3 - RYD_S16_BAL_PRIO_DROP);
  } else {
    S16_PRIO(3);
  }
#ifndef RYD_S16_TAIL_PRIO
#define RYD_S16_TAIL_PRIO 3                  // C3 -1.3 %, C4 unchanged (profiles/r02/ab14)
#endif
  // RYD_S16_TAIL_PRIO: in a launch with refill, the last-dispatched round of waves
  // runs at raised priority so the launch's tail waves finish sooner
  if (!BAL && RYD_S16_TAIL_PRIO && !s16_one_round() &&
      blockIdx.x + 256u * 4u * (unsigned)RYD_S16_WAVES >= gridDim.x)
    __builtin_amdgcn_s_setprio(RYD_S16_TAIL_PRIO);
  // states: |11> triangle coordinate r; |01> atom-B coordinate r (r < 5); |00> scalar
  double t = (r == sym_index(1, 1)) ? 1.0 : 0.0;
  double z = (r == 1) ? 1.0 : 0.0;
  double s00 = 1.0;
  double u[NS];                              // row r of the current propagator
  double cp = 1.0, sp = 0.0;                 // frame the states are in
  int nuse = 0, nexec = 0, nsq = 0;        // flop counters (series terms, squarings)
  bool over_cap = false;
  const int nseg = n_segments<PROTO>(n_steps);
  SegRot rw_out = {};                        // LP square: segment 1's lane weights serve the epilogue too

  if constexpr (PROTO == RYD_PROTO_SMOOTH_JP) {
    // one propagator (every segment has amplitude Omega and duration tau / n_steps),
    // then n_steps frame-rotated updates.  Phases: lane r computes segment s0 + r of
    // each 16-segment chunk, the update of segment s0 + j takes it from lane j (DPP).
    double ph_c, ph_s, dt;
    double th_c, th_s, dc, ds;               // cos/sin of lane r's modulation angle; chunk step
    {
      const PointP& q = q0;
      dt = q.tau / (double)n_steps;
      int rep0;
      int nrep0;
      build16(u, Ut, q, valid, valid, q.Om, q.Dl, dt, p, r, 0, rep0, nrep0, nuse, nexec, nsq, over_cap,
              (lds_zero_t*)Zl S16_PROF_PASS);
      // the modulation angle theta_s = w_mod (s dt + dt/2) - phi_off of segment s = s0 + r
      // (RG/simulation.py:1698-1731) advances by 16 w_mod dt per chunk: one rotation of
      // (cos, sin) per chunk instead of a sin/cos evaluation (~1e-15 drift over 19 chunks)
      fast_sincos(q.wmod * ((double)r * dt + dt / 2) - q.phoff, th_s, th_c);
      fast_sincos(16.0 * (q.wmod * dt), ds, dc);
    }
    const SegRow01 k1 = seg_row01(u, r);
    const SegRot rw = seg_rot(r);
    // RYD_JP_WTAB: weight table [point][segment][type 0..4] of (al, be) pairs in Ut; a lane's
    // type: 0 invariant (1, 0), 1/2 single angle (cr, +-sr), 3/4 double angle (C2, +-S2)
    d2v* wtab = reinterpret_cast<d2v*>(&Ut[0][0][0]);
    static_assert(sizeof(Ut) >= sizeof(d2v) * S16_PPW * 16 * 5, "weight table must fit in Ut");
    const bool th = r == 2 || r == 3 || r == 6 || r == 7 || r == 8 || r == 9;
    const int wtyp = th ? 1 + (r & 1) : (r == SEG_M || r == SEG_Q) ? 3 + (r & 1) : 0;
    if constexpr (RYD_JP_WTAB != 0) {
      wave_sync();                           // the build's transpose reads are done
      wtab[(p * 16 + r) * 5] = d2v{1.0, 0.0};
    }
    for (int s0 = 0; s0 < nseg; s0 += 16) {
      {
        const double* pp = prm;
        asm volatile("" : "+s"(pp));
        const PointP q = load_point16<PROTO>(pp, ldp, i0, po8);
        double cth = th_c;
        if (s0 + 16 > nseg) {                // last chunk: lanes past the end take segment nseg-1
          double st, ct;
          fast_sincos(q.wmod * ((double)(nseg - 1) * dt + dt / 2) - q.phoff, st, ct);
          if (s0 + r >= nseg) cth = ct;
        }
        fast_sincos(q.A * cth, ph_s, ph_c);
        const double tc = fma(th_c, dc, -th_s * ds);
        th_s = fma(th_s, dc, th_c * ds);
        th_c = tc;
      }
      // lane j: the rotation from segment s0+j-1's frame (lane j-1; lane 0: the frame the
      // state is in, cp/sp) to segment s0+j's, its double angle -- once per chunk
      double pc = row_shr1(ph_c), ps = row_shr1(ph_s);
      if (r == 0) {
        pc = cp;
        ps = sp;
      }
      const double cr = pc * ph_c + ps * ph_s, sr = ps * ph_c - pc * ph_s;
      const double C2 = fma(cr, cr, -sr * sr), S2 = 2.0 * (cr * sr);
      // the frame after this chunk: lane 15 (segment s0+15, or nseg-1 clamped)
      cp = row_bcast<15>(ph_c);
      sp = row_bcast<15>(ph_s);
      if constexpr (RYD_JP_WTAB != 0) {
        // the rotation weights (al, be) of every lane type for the chunk's 16 segments in
        // LDS (in Ut, free between the build and the epilogue): lane j writes segment j's
        // four signed pairs, then each segment costs one 16-byte LDS read per lane instead
        // of two weight inits and four DPP FMAs
        wave_sync();                         // the previous chunk's reads are done
        wtab[(p * 16 + r) * 5 + 1] = d2v{cr, sr};
        wtab[(p * 16 + r) * 5 + 2] = d2v{cr, -sr};
        wtab[(p * 16 + r) * 5 + 3] = d2v{C2, S2};
        wtab[(p * 16 + r) * 5 + 4] = d2v{C2, -S2};
        wave_sync();
      }
      static_for<16>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if (s0 + j < nseg) {
          double al, be;
          if constexpr (RYD_JP_WTAB != 0) {
            const d2v w = wtab[(p * 16 + j) * 5 + wtyp];
            al = w.x;
            be = w.y;
          } else {
            // al = wI + w2 C2_j + wT cr_j, be = b2 S2_j + bT sr_j: row_newbcast operands
            al = rw.wI;
            be = 0.0;
            fmac2_bcast<j>(al, C2, rw.w2, cr, rw.wT);
            fmac2_bcast<j>(be, S2, rw.b2, sr, rw.bT);
          }
          t = fma(al, t, be * quad_swap(t));
          z = fma(al, z, be * quad_swap(z));
          seg_apply<false>(u, k1, t, z, s00, (lds_zero_t*)Zl);
        }
      });
    }
    // |00>: the invariant coordinate is multiplied by the same U'_00 every segment, so
    // s00 = U'_00^nseg by binary powering (uniform nseg) instead of one multiply per segment
    {
      double b = k1.u00, acc = 1.0;
      for (int e = nseg; e > 0; e >>= 1) {
        if (e & 1) acc *= b;
        b *= b;
      }
      s00 = acc;
    }
  } else {
    // LP square (2 segments, one propagator when |xi| = 1) and bang-bang (a propagator
    // per segment).  The states and the frame are parked in LDS across an in-loop
    // build so that they hold no registers while the Chebyshev series runs.
    __shared__ double SvW[NW][S16_PPW][16][2];
    __shared__ double SpW[NW][S16_PPW][8];
    __shared__ int ScW[NW][S16_PPW][2];
    double (&Sv)[S16_PPW][16][2] = SvW[wv];
    double (&Sp)[S16_PPW][8] = SpW[wv];
    int (&Sc)[S16_PPW][2] = ScW[wv];
    constexpr int KEEP = PROTO == RYD_PROTO_LP_SQUARE ? RYD_LP_UNSQUARED : 0;
    int rep = 0, nrep = 0;                   // unsquared levels of the current propagator
    SegRow01 k1 = {};                        // the |01> row of the current propagator
    if (nseg > 0) {
      // Segment 0 always builds (an all-invalid wave builds identity rows).  The inputs
      // |11>, |01>, |00> are basis states that every frame rotation leaves alone, so the
      // first application of U' is a column read: t = U' e_(1,1) (segment-order lane 5),
      // z = column 1 of the |01> row, s00 = U'_00 -- what seg_apply gives on the unit
      // vectors (0 * x = 0 for finite rows) without its 20 DPP FMAs and the rotation.
      const PointP& q = q0;
      double a, c, sn, dl, dt;
      bool hold;
      seg_polar<PROTO>(q, 0, n_steps, frame_ok, a, c, sn, dl, dt, hold);
      if constexpr (BAL != 0) {
        int* pollp = nullptr;
#ifdef RYD_S16_PROF
        pollp = &bal_polls;
#endif
        const S16Handoff ho = {role.role, role.off - (gpc & ~3), nohandoff == 0, Hcols, Hcnt, Hflag, pollp};
        if (build16(u, Ut, q, valid, valid, a, dl, dt, p, r, KEEP, rep, nrep, nuse, nexec, nsq, over_cap,
                    (lds_zero_t*)Zl S16_PROF_PASS, ho))
          return;                            // a producer: its consumer has the job from here
      } else {
        build16(u, Ut, q, valid, valid, a, dl, dt, p, r, KEEP, rep, nrep, nuse, nexec, nsq, over_cap,
                (lds_zero_t*)Zl S16_PROF_PASS);
      }
      if constexpr (PROTO != RYD_PROTO_LP_SQUARE) {
        if (r == 0) {                        // segment the propagator was built for
          Sp[p][5] = a;
          Sp[p][6] = dt;
        }
      }
      k1 = seg_row01(u, r);
      t = u[sym_index(1, 1)];
      z = k1.o[1];
      s00 = k1.u00;
      for (int j = 1; j < (1 << nrep); ++j) {
        if (j < (1 << rep)) seg_apply(u, k1, t, z, s00);
      }
      if (!hold) {
        cp = c;
        sp = sn;
      }
      wave_sync();
    }
    for (int s = 1; s < nseg; ++s) {
      // re-read the segment's scalars (L1 hits) instead of keeping them live: the
      // Chebyshev phase needs the registers.  Only what seg_polar reads is loaded here
      // (LP square: amplitude, duration, xi); a rebuild loads the whole point itself.
      double a, c, sn, dl, dt;
      bool hold = false;
      // LP square with every xi of the wave on the unit circle (or its row invalid): the
      // segment has segment 0's amplitude and duration (valid: both finite), no rebuild, and
      // its phase is q0's xi, which stays in registers through the build (LP square has them
      // to spare: 122 VGPRs) -- no global load, no LDS exchange.  The general path (a non-unit
      // xi somewhere in the wave; bang-bang always) stays as it was.
      bool general = true;
      if constexpr (PROTO == RYD_PROTO_LP_SQUARE) {
        general = __builtin_amdgcn_ballot_w64(!frame_ok) != 0;
        c = q0.xr;
        sn = q0.xi;
      }
      if (general) {
        const double* pp = prm;
        asm volatile("" : "+s"(pp));
        const PointP q = load_point16<PROTO>(pp, ldp, i0, po8);
        seg_polar<PROTO>(q, s, n_steps, frame_ok, a, c, sn, dl, dt, hold);
        // LP square: segment 0 was built for (Omega, tau), the same loads
        const bool need = PROTO == RYD_PROTO_LP_SQUARE ? valid && !(a == q.Om && dt == q.tau)
                                                       : valid && !(a == Sp[p][5] && dt == Sp[p][6]);
        if (__builtin_amdgcn_ballot_w64(need) != 0) {
          // Every point of the wave rebuilds: a point whose segment did not change gets
          // the same propagator bit for bit (its series and squarings do not depend on
          // its neighbours), so the previous row need not stay live through the build.
          Sv[p][r][0] = t;
          Sv[p][r][1] = z;
          if (r == 0) {
            Sp[p][0] = s00;
            Sp[p][1] = cp;
            Sp[p][2] = sp;
            Sc[p][0] = nuse;
            Sc[p][1] = nsq;
          }
          int nu = 0, nq = 0;
          const double* pb = pp;               // bang-bang rebuilds every segment: the same loads
          if constexpr (PROTO == RYD_PROTO_LP_SQUARE) asm volatile("" : "+s"(pb));   // loaded on this path only
          const PointP qb = load_point16<PROTO>(pb, ldp, i0, po8);
          build16(u, Ut, qb, valid, need, a, dl, dt, p, r, KEEP, rep, nrep, nu, nexec, nq, over_cap,
                  (lds_zero_t*)Zl S16_PROF_PASS);
          t = Sv[p][r][0];
          z = Sv[p][r][1];
          s00 = Sp[p][0];
          cp = Sp[p][1];
          sp = Sp[p][2];
          nuse = Sc[p][0] + nu;
          nsq = Sc[p][1] + nq;
          wave_sync();
          if constexpr (PROTO != RYD_PROTO_LP_SQUARE) {   // LP square has no third segment to compare
            if (r == 0) {
              Sp[p][5] = a;
              Sp[p][6] = dt;
            }
            wave_sync();
          }
          const double* pq = prm;
          asm volatile("" : "+s"(pq));
          seg_polar<PROTO>(load_point16<PROTO>(pq, ldp, i0, po8), s, n_steps, frame_ok, a, c, sn, dl, dt, hold);
          k1 = seg_row01(u, r);                // the |01> row is not kept live across a build
        }
      }
      if (hold) {
        c = cp;
        sn = sp;
      }
      const double cr = cp * c + sp * sn, sr = sp * c - cp * sn;
      rw_out = seg_rot(r);                   // (rotation weights are not kept live across a build)
      rotate_state(t, z, cr, sr, rw_out);
      seg_apply(u, k1, t, z, s00);
      // the unsquared levels: 2^rep - 1 more applications of the built factor, frame fixed
      for (int j = 1; j < (1 << nrep); ++j) {
        if (j < (1 << rep)) seg_apply(u, k1, t, z, s00);
      }
      cp = c;
      sp = sn;
    }
  }
  S16_MARK(5);
  // ---- back to the lab frame Q(cp, sp).  The lane and point indices are recomputed
  // here (mbcnt, blockIdx) rather than kept live through the series.
  {
    const int lid = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    int pl = lid >> 4;
    asm volatile("" : "+v"(pl));
    const int64_t b2 = BAL ? job : xcd_block(blockIdx.x, gridDim.x);
    if constexpr (PROTO != RYD_PROTO_LP_SQUARE) rw_out = seg_rot(lid & 15);
#ifdef RYD_S16_PROF
    if constexpr (BAL != 0) {
      // columns AVG_POP and AVG_F of the PROF build: 1 + role + 4 * workgroup wave index + 64 *
      // polls (negative polls: the fallback ran); the producer's cycles to its handoff + 2^20 * its SIMD
      s16_ts[10] = (double)(1 + role.role + 4 * wv) + 64.0 * (double)bal_polls;
      if (bal_polls > 0) {
        const int s = role.off - (gpc & ~3);
        s16_ts[11] = (double)Hcnt[s][2][lid] + 1048576.0 * (double)((Hcnt[s][3][lid] >> 4) & 3);
      }
    }
#endif
    return sym16_epilogue<STATE>(t, z, s00, cp, sp, rw_out, valid, over_cap, nuse, nexec, nsq, lid, pl, b2, n, st, lds, sm,
                                 ldm, status, st32 != 0, wt, Ut S16_PROF_PASS);
  }
