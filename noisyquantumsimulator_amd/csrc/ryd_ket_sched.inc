// ryd_ket_sched.inc -- noise-free custom pulse schedules as kets, with the derivatives of the
// two diagonal overlaps with respect to every segment's phase (included by ryd_engine.hip after
// ryd_sched_table.inc and ryd_sched16.inc, inside the anonymous namespace).
//
// ryd_run_schedule_kets[_device]: the table of ryd_run_schedule (ryd_sched16.inc), dim 3,
// identical atoms, no rates.  The layout is the family's: four points per wave, one 16-lane
// DPP row each, xcd_block order.  Lane r < 10 of a row holds one real component of the point's
// two blocks (ryd_ket_block_body.inc): lanes 0..3 the |01> block (c01, c0r), lanes 4..9 the
// |11> symmetric block (c11, c+, crr), real part on the even lane, imaginary on the odd one.
// A segment is the block propagator of ket_blocks_build in real form: every lane holds its row
// of ten coefficients and takes the ten components from the row by row_newbcast FMAs
// (dot5_bcast).  The laser phase is a frame, D = diag(1, e^{i phi}[, e^{2 i phi}]), carried
// relatively from segment to segment as lindblad_sched16_kernel carries (cp, sp).
//
// Table.  Read by the protocol of ryd_sched_table.inc (SCHED_TABLE_VALID, SCHED_CHUNK_*), the
// point's Omega held in a register; the rate columns take part in sched16_point_valid and in
// nothing else.  The lane also forms its segment's step cap (h_bounds, X_CAP, as ket_block_kernel) and
// marks a capped segment with the duration -1, which no valid table holds.
// A chunk whose segments all run on every row's current propagator (a phase-only stretch) takes
// a shorter loop: the lanes form their segments' frame steps sixteen at once, and a segment is
// four broadcasts, the rotation and the ten FMAs, with no key, compare or ballot.  Both loops do
// the same arithmetic on the same numbers, so a row's bits do not depend on its wave's choice.
//
// Memo.  As ryd_sched16.inc: key (a Omega, delta Omega, x / Omega), ==, the wave builds when
// any row needs to, a row that does not need to rebuilds on its own last key; the lanes of a
// row build redundantly.  Before the first build the row holds the identity under (0, 0, 0).
//
// Backward walk (ket_sched_jac_kernel).  With U_s = D U' D^dag, dU_s/dphi_s = i [G, U_s],
// G = diag(0, 1[, 2]).  For a = e0^T U_N .. U_1 e0, b_s = U_s .. U_1 e0 and
// lambda_s^T = e0^T U_N .. U_{s+1} (no conjugate), g_s = lambda_s^T G b_s gives
// da/dphi_s = i (g_s - g_{s-1}).  The walk goes back from the final b and lambda = e0:
// b_{s-1} = U_s^{-1} b_s (the conjugate of the complex-symmetric U' in the frame),
// lambda_{s-1} = U_s^T lambda_s (U' itself, in the conjugate frame: nu = D lambda), and
// g = sum_k k nu_k w_k in any common frame.  The chunks and their segments are taken in
// reverse (SCHED_CHUNK_TO_LANE15, SCHED_CHUNK_ROR1); lane j keeps the four numbers of segment
// s0 + j, so a row stores 16 segments of a component as one 128-byte piece of
// jac[i ld_jac + c n_seg + s], c = Re da01, Im da01, Re da11, Im da11.
// A skipped segment and every segment of an invalid point get exact zeros.
//
// Control Jacobian (ket_sched_ctl_kernel, ryd_run_schedule_kets_ctl).  The same forward pass
// and one backward walk that writes the derivatives with respect to all four fields,
// jac[i ld_jac + (4 f + c) n_seg + s], f = RYD_SC_X .. RYD_SC_DELTA; its phase block, state,
// summary and status are ket_sched_jac_kernel's bit for bit.  The formulas stand with the code
// (ket_ctl_block, and the walk at the end of ket_sched_body).
//
// Registers (make resource-usage): 201 / 205 VGPRs forward (STATE false / true), 207 / 209 with
// the Jacobian, no scratch, no LDS: 2 waves per SIMD.  An amdgpu_waves_per_eu(3, 8) budget of
// 168 spills 116-132 bytes per lane around ket_blocks_build, so none is set.  The control
// kernel: 253 VGPRs, no scratch, 18,432 bytes of LDS (derivative rows, chunk results, and the
// walk's state parked across a build), 2 waves per SIMD under amdgpu_waves_per_eu(2, 8).

// Row r of the block-diagonal propagator in real form (r >= 10: zeros).
__device__ __forceinline__ void ket_sched_row(const KetBlocks& K, int r, double (&u)[10]) {
  const int e = r >> 1;
  const bool im = (r & 1) != 0;
  double ar[5], ai[5];
#pragma unroll
  for (int m = 0; m < 5; ++m) ar[m] = ai[m] = 0.0;
#pragma unroll
  for (int ee = 0; ee < 2; ++ee)
#pragma unroll
    for (int m = 0; m < 2; ++m)
      if (e == ee) {
        ar[m] = K.u2[ee + m][0];
        ai[m] = K.u2[ee + m][1];
      }
  const int U3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
  for (int ee = 0; ee < 3; ++ee)
#pragma unroll
    for (int m = 0; m < 3; ++m)
      if (e == 2 + ee) {
        ar[2 + m] = K.u3[U3[ee][m]][0];
        ai[2 + m] = K.u3[U3[ee][m]][1];
      }
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    u[2 * m] = im ? ai[m] : ar[m];
    u[2 * m + 1] = im ? ar[m] : -ai[m];
  }
}

// sum_m u[m] * (component m of the row's vector v): two chains of five FMAs and their sum
__device__ __forceinline__ double ket_sched_apply(const double (&u)[10], double v) {
  double lo = 0.0, hi = 0.0;
  dot5_bcast<0>(lo, v, u[0], u[1], u[2], u[3], u[4]);
  dot5_bcast<5, false>(hi, v, u[5], u[6], u[7], u[8], u[9]);
  return lo + hi;
}

// The frame step from (cp, sp) to (cs, ss): (cos, sin) of d = phi_new - phi_old and of 2 d
struct KetSchedStep {
  double cd, sd, c2, s2;
};
__device__ __forceinline__ KetSchedStep ket_sched_step(double cp, double sp, double cs, double ss) {
  KetSchedStep t;
  t.cd = fma(cp, cs, sp * ss);
  t.sd = fma(cp, ss, -sp * cs);
  t.c2 = fma(t.cd, t.cd, -t.sd * t.sd);
  t.s2 = 2.0 * t.cd * t.sd;
  return t;
}

// component of charge k: times e^{-i k d}; sg = +1 on a real lane, -1 on an imaginary one
__device__ __forceinline__ double ket_sched_rotate(double v, int k, double sg, const KetSchedStep& t) {
  const double ck = k == 0 ? 1.0 : (k == 1 ? t.cd : t.c2);
  const double sk = k == 0 ? 0.0 : (k == 1 ? t.sd : t.s2);
  return fma(quad_swap(v), sg * sk, v * ck);
}

// g = nu^T G w of both blocks (every lane of the row gets all four numbers)
__device__ __forceinline__ void ket_sched_g(double nu, double w, double (&g)[4]) {
  const double ps = nu * w, pc = nu * quad_swap(w);
  g[0] = row_bcast<2>(ps) - row_bcast<3>(ps);
  g[1] = row_bcast<2>(pc) + row_bcast<3>(pc);
  g[2] = (row_bcast<6>(ps) - row_bcast<7>(ps)) + 2.0 * (row_bcast<8>(ps) - row_bcast<9>(ps));
  g[3] = (row_bcast<6>(pc) + row_bcast<7>(pc)) + 2.0 * (row_bcast<8>(pc) + row_bcast<9>(pc));
}

// ---- the control Jacobian (ket_sched_ctl_kernel): duration, amplitude, phase, detuning
// With H_r = Q diag(lambda) Q^T the derivative of U' = exp(-i H_r dt) along H_theta is
//   dU'/dtheta = Q [ (Q^T H_theta Q) o Phi ] Q^T,
//   Phi_kl = -i dt e^{-i (lambda_k + lambda_l) dt / 2} sinc((lambda_k - lambda_l) dt / 2),
// finite for every gap (Phi_kk = -i dt e^{-i lambda_k dt}); H_a is the coupling pattern (cpl on
// the off-diagonals next to the diagonal), H_Delta = -diag(0, 1[, 2]).

// Row i of dU'/dtheta (the lane's own; any other i gives zeros) in the real form of
// ket_sched_row: out[2 j], out[2 j + 1] for column j.  F = 0: theta = a, cpl on the coupling
// pattern; F = 1: theta = Delta.
template <int N, int F>
__device__ __forceinline__ void ket_ctl_row(const KetEig& E, double cpl, int i, bool im, double (&out)[2 * N]) {
  double M[N][N];                            // Q^T H_theta Q
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int l = k; l < N; ++l) {
      double m = 0.0;
      if constexpr (F == 0) {
#pragma unroll
        for (int c = 0; c + 1 < N; ++c) m = fma(E.Q[c][k], E.Q[c + 1][l], fma(E.Q[c + 1][k], E.Q[c][l], m));
        m *= cpl;
      } else {
#pragma unroll
        for (int c = 1; c < N; ++c) m = fma(-(double)c * E.Q[c][k], E.Q[c][l], m);
      }
      M[k][l] = M[l][k] = m;
    }
  double q[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    q[k] = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) q[k] = (i == c) ? E.Q[c][k] : q[k];
  }
  // v_l = sum_k q_k (M o Phi)_kl, then dU'[i][j] = sum_l v_l Q[j][l]
  double vr[N], vi[N];
#pragma unroll
  for (int l = 0; l < N; ++l) {
    vr[l] = vi[l] = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int lo = k < l ? k : l, hi = k < l ? l : k;
      const int e = lo * N - lo * (lo - 1) / 2 + (hi - lo);
      const double qm = q[k] * M[k][l];
      vr[l] = fma(qm, E.P[e][0], vr[l]);
      vi[l] = fma(qm, E.P[e][1], vi[l]);
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double ar = 0.0, ai = 0.0;
#pragma unroll
    for (int l = 0; l < N; ++l) {
      ar = fma(vr[l], E.Q[j][l], ar);
      ai = fma(vi[l], E.Q[j][l], ai);
    }
    out[2 * j] = im ? ai : ar;
    out[2 * j + 1] = im ? ar : -ai;
  }
}

// lane r takes the value of lane (r - 2) mod 16 / (r + 2) mod 16 of its row: row_ror:2, row_ror:14
__device__ __forceinline__ double row_ror2(double v) { return dpp32x2<0x122>(v); }
__device__ __forceinline__ double row_rol2(double v) { return dpp32x2<0x12E>(v); }

// nu^T y of both blocks from the lanes' products ps = sg nu y and pc = nu y(partner): o = Re, Im
// of the 2 x 2 block's sum (lanes 0..3), Re, Im of the 3 x 3 block's (lanes 4..9); every lane of
// the row gets all four.  `one` is 1.0 in a register (the FMA's second factor).
__device__ __forceinline__ void ket_ctl_sums(double ps, double pc, double one, double (&o)[4]) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#define RYD_CTL_FMAC(acc, src, lane) \
  "v_fmac_f64_dpp " acc ", " src ", %6 row_newbcast:" #lane " row_mask:0xf bank_mask:0xf\n\t"
  asm volatile("s_nop 1\n\t"
               RYD_CTL_FMAC("%0", "%4", 0) RYD_CTL_FMAC("%1", "%5", 0) RYD_CTL_FMAC("%2", "%4", 4)
               RYD_CTL_FMAC("%3", "%5", 4) RYD_CTL_FMAC("%0", "%4", 1) RYD_CTL_FMAC("%1", "%5", 1)
               RYD_CTL_FMAC("%2", "%4", 5) RYD_CTL_FMAC("%3", "%5", 5) RYD_CTL_FMAC("%0", "%4", 2)
               RYD_CTL_FMAC("%1", "%5", 2) RYD_CTL_FMAC("%2", "%4", 6) RYD_CTL_FMAC("%3", "%5", 6)
               RYD_CTL_FMAC("%0", "%4", 3) RYD_CTL_FMAC("%1", "%5", 3) RYD_CTL_FMAC("%2", "%4", 7)
               RYD_CTL_FMAC("%3", "%5", 7) RYD_CTL_FMAC("%2", "%4", 8) RYD_CTL_FMAC("%3", "%5", 8)
               RYD_CTL_FMAC("%2", "%4", 9) "v_fmac_f64_dpp %3, %5, %6 row_newbcast:9 row_mask:0xf bank_mask:0xf"
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
               : "v"(ps), "v"(pc), "v"(one));
#undef RYD_CTL_FMAC
  o[0] = a0;
  o[1] = a1;
  o[2] = a2;
  o[3] = a3;
}

template <bool STATE, bool JAC, bool CTL = false>
__device__ __forceinline__ void ket_sched_body(const double* __restrict__ prm, int64_t n, int64_t ldp,
                                               const double* __restrict__ sched, int64_t ldsc, int n_seg,
                                               double* __restrict__ st, int64_t lds, double* __restrict__ sm,
                                               int64_t ldm, double* __restrict__ jac, int64_t ldj,
                                               uint32_t* __restrict__ status) {
  const int l = (int)threadIdx.x;
  const int p = l >> 4, r = l & 15;
  // the wave's first point and the lane's point, both clamped to the batch
  const int64_t b0 = xcd_block(blockIdx.x, gridDim.x) * S16_PPW;
  const int64_t i0 = b0 < n ? b0 : n - 1;    // a wave past the batch (padded grid) reads point n - 1
  const int64_t last = n - 1 - i0;           // >= 0
  const int pc = min(p, last < S16_PPW - 1 ? (int)last : S16_PPW - 1);
  const bool active = b0 + p < n;            // the row's point is its own: it stores
  const int64_t ip = i0 + (int64_t)pc;       // <= n - 1
  const double* __restrict__ row = sched + ip * ldsc;   // ldsc = 0: the shared row

  bool valid;
  double Om, V, d1;
  {
    const PointP q = load_point16<RYD_PROTO_LP_SQUARE>(prm, ldp, i0, 8u * (unsigned)pc);
    valid = sched16_point_valid(q);
    Om = q.Om;
    V = q.V;
    d1 = q.d1;
  }
  SCHED_TABLE_VALID(valid, row, n_seg, r, p)
  if (!valid) {                              // an invalid row builds identities of finite numbers
    Om = 1.0;
    V = d1 = 0.0;
  }

  // the chunk at s0: lane r's segment s0 + r (clamped), its key, its phase; a capped segment
  // has the duration -1, an invalid row durations 0
  auto load_chunk = [&](int s0, double& Ka, double& Kd, double& Kt, double& Pc, double& Ps) {
    SCHED_CHUNK_LOAD(row, n_seg, s0, r, Om)
    Seg g;
    g.om_re = Ka;
    g.om_im = 0.0;
    g.dl = Kd;
    g.dt = Kt;
    double emin, emax;
    h_bounds(g, V, d1, emin, emax);
    if (!(0.5 * (emax - emin) * Kt <= X_CAP)) Kt = -1.0;
    if (!valid) {
      SCHED_CHUNK_NEUTRAL()
    }
  };

  // lane constants: the component's charge and the sign of its partner in a rotation
  const int kq = (r < 2 || r == 4 || r == 5) ? 0 : (r < 8 ? 1 : 2);
  const double sg = (r & 1) ? -1.0 : 1.0;

  double w = (r == 0 || r == 4) ? 1.0 : 0.0; // c01 = 1, c11 = 1
  double cp = 1.0, sp = 0.0;                 // frame the state is in
  int nuse = 0, nsq = 0;
  bool over_cap = false;
  double u[10];
#pragma unroll
  for (int m = 0; m < 10; ++m) u[m] = (m == r) ? 1.0 : 0.0;
  double La = 0.0, Ld = 0.0, Lt = 0.0;       // the key of the row's last build

  // every row of the wave rebuilds, a row that does not need to with its last key
  auto build = [&](bool need, double a, double dl, double dt) {
    La = need ? a : La;
    Ld = need ? dl : Ld;
    Lt = need ? dt : Lt;
    KetBlocks K;
    ket_blocks_build(K, La, Ld, Lt, d1, V);
    ket_sched_row(K, r, u);
  };

  for (int s0 = 0; s0 < n_seg; s0 += 16) {
    double Ka, Kd, Kt, Pc, Ps;
    load_chunk(s0, Ka, Kd, Kt, Pc, Ps);
    const int cnt = min(16, n_seg - s0);
    // A chunk whose segments all run on every row's current propagator (a phase-only stretch):
    // each lane forms its own segment's frame step, sixteen at once, and the segments take
    // theirs from lane 0 as the general loop does: no key, no compare, no build.  The same arithmetic
    // on the same numbers as the general loop below, so a row's bits do not depend on which
    // loop its wave took.
    const bool plain = r >= cnt || (Kt > 0.0 && Ka == La && Kd == Ld && Kt == Lt);
    if (__builtin_amdgcn_ballot_w64(!plain) == 0) {
      double pcm = row_ror1(Pc), psm = row_ror1(Ps);   // the frame before: the lane below, or (cp, sp)
      pcm = r == 0 ? cp : pcm;
      psm = r == 0 ? sp : psm;
      KetSchedStep T = ket_sched_step(pcm, psm, Pc, Ps);
      for (int j = 0; j < cnt; ++j) {        // segment s0 + j: lane 0 after j rotations
        const KetSchedStep t = {row_bcast<0>(T.cd), row_bcast<0>(T.sd), row_bcast<0>(T.c2), row_bcast<0>(T.s2)};
        w = ket_sched_apply(u, ket_sched_rotate(w, kq, sg, t));
        T.cd = row_rol1(T.cd);
        T.sd = row_rol1(T.sd);
        T.c2 = row_rol1(T.c2);
        T.s2 = row_rol1(T.s2);
      }
      nuse += cnt;
      cp = row_bcast<15>(Pc);                // lanes past cnt hold the last segment too
      sp = row_bcast<15>(Ps);
      continue;
    }
    for (int j = 0; j < cnt; ++j) {
      // segment s0 + j: lane 0 of the row after j rotations
      const double a = row_bcast<0>(Ka), dl = row_bcast<0>(Kd), dt = row_bcast<0>(Kt);
      const bool skip = !(dt > 0.0);
      over_cap = over_cap || dt < 0.0;
      const bool need = !skip && !(a == La && dl == Ld && dt == Lt);
      if (__builtin_amdgcn_ballot_w64(need) != 0) {
        build(need, a, dl, dt);
        nsq += need ? 1 : 0;
      }
      // into the segment's frame, then U'; a skipping row computes along and keeps its values
      const double cs = skip ? cp : row_bcast<0>(Pc), ss = skip ? sp : row_bcast<0>(Ps);
      const double wn = ket_sched_apply(u, ket_sched_rotate(w, kq, sg, ket_sched_step(cp, sp, cs, ss)));
      w = skip ? w : wn;
      nuse += skip ? 0 : 1;
      cp = cs;
      sp = ss;
      SCHED_CHUNK_ROL1()
    }
  }

  // ---- epilogue: back to the lab frame, b = D w; outputs as ryd_ket_block_body.inc
  {
    const double wl = ket_sched_rotate(w, kq, sg, ket_sched_step(cp, sp, 1.0, 0.0));
    double b[10];
    static_for<10>([&](auto M) { b[decltype(M)::value] = row_bcast<decltype(M)::value>(wl); });
    const double h = 0.70710678118654752440;
    const double c1r = h * b[6], c1i = h * b[7];
    if constexpr (STATE) {
      if (active) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int R = r + 16 * pass;       // ket row 2 basis + part; 18 rows
          if (R < 18) {
            const int bi = R >> 1;
            const bool im = (R & 1) != 0;
            const double e01 = im ? b[1] : b[0], e0r = im ? b[3] : b[2];
            const double e11 = im ? b[5] : b[4], epl = im ? c1i : c1r, err = im ? b[9] : b[8];
            const double v0 = R == 0 ? 1.0 : 0.0;                                   // |00>
            const double v1 = bi == 1 ? e01 : (bi == 2 ? e0r : 0.0);              // |01> -> c01 |01> + c0r |0r>
            const double v2 = bi == 3 ? e01 : (bi == 6 ? e0r : 0.0);              // |10>: atom-swap mirror
            const double v3 = bi == 4 ? e11 : ((bi == 5 || bi == 7) ? epl : (bi == 8 ? err : 0.0));
            double* o = st + ((int64_t)R * lds + 4 * ip);
            o[0] = v0;
            o[1] = v1;
            o[2] = v2;
            o[3] = v3;
          }
        }
      }
    }
    if (active && r == 0) {
      uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
      if (over_cap) stat |= RYD_STATUS_STEP_CAP;
      bool fin = true;
#pragma unroll
      for (int m = 0; m < 10; ++m) fin = fin && isfinite(b[m]);
      if (!fin) stat |= RYD_STATUS_NONFINITE;
      const double orr[4] = {1.0, b[0], b[0], b[4]}, oii[4] = {0.0, b[1], b[1], b[5]};
      double pp[4], ph[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        pp[x] = orr[x] * orr[x] + oii[x] * oii[x];
        ph[x] = atan2(oii[x], orr[x]);
      }
      double cph = ph[3] - ph[1] - ph[2] + ph[0];
      cph = cph + M_PI;
      cph = cph - 2.0 * M_PI * floor(cph / (2.0 * M_PI));
      cph = cph - M_PI;
      const double err = fmin(fabs(cph - M_PI), fabs(cph + M_PI));
      const double cerr = cos(err / 2);
      const double pen = cerr * cerr;
      const double avgp = 0.25 * (pp[0] + pp[1] + pp[2] + pp[3]);
      const double avgf = 0.25 * (pp[0] + pp[1] + pp[2] + pp[3] * pen);
      double nrm11 = 0.0;
#pragma unroll
      for (int e = 0; e < 3; ++e) nrm11 += b[4 + 2 * e] * b[4 + 2 * e] + b[5 + 2 * e] * b[5 + 2 * e];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        sm[(int64_t)(RYD_S_POP0 + x) * ldm + ip] = pp[x];
        sm[(int64_t)(RYD_S_OV_RE0 + x) * ldm + ip] = orr[x];
        sm[(int64_t)(RYD_S_OV_IM0 + x) * ldm + ip] = oii[x];
      }
      sm[(int64_t)RYD_S_AVG_POP * ldm + ip] = avgp;
      sm[(int64_t)RYD_S_CTRL_PHASE * ldm + ip] = cph;
      sm[(int64_t)RYD_S_PENALTY * ldm + ip] = pen;
      sm[(int64_t)RYD_S_AVG_F * ldm + ip] = avgf;
      sm[(int64_t)RYD_S_NMV_USEFUL * ldm + ip] = (double)nuse;   // forward segments applied
      sm[(int64_t)RYD_S_NMV_EXEC * ldm + ip] = (double)nuse;
      sm[(int64_t)RYD_S_TRACE11 * ldm + ip] = nrm11;
      sm[(int64_t)RYD_S_NSQUARE * ldm + ip] = (double)nsq;       // forward propagator builds
      status[ip] = stat;
    }
  }

  // ---- the backward walk: w = D^dag b and nu = D lambda in the frame (cp, sp)
  if constexpr (JAC) {
    double nu = (r == 0 || r == 4) ? 1.0 : 0.0;   // lambda_N = e0 in both blocks
    double g[4] = {0.0, 0.0, 0.0, 0.0};      // g_N: e0 carries no charge
    for (int s0 = ((n_seg - 1) / 16) * 16; s0 >= 0; s0 -= 16) {
      double Ka, Kd, Kt, Pc, Ps;
      load_chunk(s0, Ka, Kd, Kt, Pc, Ps);
      const int cnt = min(16, n_seg - s0);
      SCHED_CHUNK_TO_LANE15(cnt)
      double J0 = 0.0, J1 = 0.0, J2 = 0.0, J3 = 0.0;
      for (int j = cnt - 1; j >= 0; --j) {
        // segment s0 + j: lane 15 of the row after cnt - 1 - j rotations
        const double a = row_bcast<15>(Ka), dl = row_bcast<15>(Kd), dt = row_bcast<15>(Kt);
        const bool skip = !(dt > 0.0);
        const bool need = !skip && !(a == La && dl == Ld && dt == Lt);
        if (__builtin_amdgcn_ballot_w64(need) != 0) build(need, a, dl, dt);
        const double cs = skip ? cp : row_bcast<15>(Pc), ss = skip ? sp : row_bcast<15>(Ps);
        const KetSchedStep fw = ket_sched_step(cp, sp, cs, ss);
        const KetSchedStep bw = {fw.cd, -fw.sd, fw.c2, -fw.s2};
        // conj(U') on w, U' on nu, both in the segment's frame
        double uc[10];
#pragma unroll
        for (int m = 0; m < 10; ++m) uc[m] = ((m ^ r) & 1) ? -u[m] : u[m];
        const double wn = ket_sched_apply(uc, ket_sched_rotate(w, kq, sg, fw));
        const double nn = ket_sched_apply(u, ket_sched_rotate(nu, kq, sg, bw));
        double gn[4];
        ket_sched_g(nn, wn, gn);
        // da/dphi_s = i (g_s - g_{s-1})
        const bool mine = r == j;
        J0 = mine ? (skip ? 0.0 : -(g[1] - gn[1])) : J0;
        J1 = mine ? (skip ? 0.0 : g[0] - gn[0]) : J1;
        J2 = mine ? (skip ? 0.0 : -(g[3] - gn[3])) : J2;
        J3 = mine ? (skip ? 0.0 : g[2] - gn[2]) : J3;
        w = skip ? w : wn;
        nu = skip ? nu : nn;
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = skip ? g[c] : gn[c];
        cp = cs;
        sp = ss;
        SCHED_CHUNK_ROR1()
      }
      if (active && r < cnt) {               // s0 + r <= n_seg - 1
        double* o = jac + (ip * ldj + (int64_t)s0 + r);
        o[0] = J0;
        o[(int64_t)n_seg] = J1;
        o[2 * (int64_t)n_seg] = J2;
        o[3 * (int64_t)n_seg] = J3;
      }
    }
  }

  // ---- the backward walk for all four fields (ket_sched_ctl_kernel).  The phase block is the
  // walk above, operation for operation.  In the segment's frame, with w_s, nu_s before the
  // step and w_{s-1} after it:
  //   da/dx_s     = -(i / Omega) nu_s^T H_r w_s      (U' commutes with H_r: no propagator
  //                 derivative; H_r = H0 + a Ha - Delta G from the key, tridiagonal)
  //   da/da_s     = Omega nu_s^T (dU'/da) w_{s-1},   da/ddelta_s = Omega nu_s^T (dU'/dDelta) w_{s-1}
  // with each lane's rows of dU'/da and dU'/dDelta kept in LDS ([coefficient][lane]: a lane reads
  // and writes its own column, conflict-free, no barrier) and memoised with the build.  The
  // forward pass leaves no derivative rows, so the walk's first applied segment builds.  A segment
  // of zero duration has the one-sided da/dx_s of the same form in its own phi_s, with nu and w
  // as they stand (the frame is not committed) and exact zeros elsewhere; a capped segment and an
  // invalid point get exact zeros in all four fields.
  if constexpr (CTL) {
    __shared__ double Drow[20][S16_BLOCK];
    __shared__ double Jrow[16][S16_BLOCK];   // the chunk's results: lane j's sixteen numbers of segment s0 + j
    const double hs = 0.70710678118654752440;
    // (not const: parked with the walk's state across a build)
    double kqd = (double)kq;
    double e0 = r < 2 ? d1 : (r < 4 ? 0.0 : (r < 6 ? 2.0 * d1 : (r < 8 ? d1 : (r < 10 ? V : 0.0))));
    double cl = (r == 2 || r == 3) ? 0.5 : ((r >= 6 && r < 10) ? hs : 0.0);   // to lane r - 2
    double cu = r < 2 ? 0.5 : ((r >= 4 && r < 8) ? hs : 0.0);                 // to lane r + 2
    double iOm = 1.0 / Om;
    const double one = 1.0;
    bool have = false;                       // the LDS rows belong to every row's last key
    double nu = (r == 0 || r == 4) ? 1.0 : 0.0;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s0 = ((n_seg - 1) / 16) * 16; s0 >= 0; s0 -= 16) {
      double Ka, Kd, Kt, Pc, Ps;
      load_chunk(s0, Ka, Kd, Kt, Pc, Ps);
      const int cnt = min(16, n_seg - s0);
      SCHED_CHUNK_TO_LANE15(cnt)
      for (int j = cnt - 1; j >= 0; --j) {
        const double a = row_bcast<15>(Ka), dl = row_bcast<15>(Kd), dt = row_bcast<15>(Kt);
        const bool skip = !(dt > 0.0);
        const bool dead = !valid || dt < 0.0;          // no derivative at all: invalid point, capped segment
        const bool need = !skip && !(have && a == La && dl == Ld && dt == Lt);
        if (__builtin_amdgcn_ballot_w64(need) != 0) {
          // Every row rebuilds, a row that does not need to with its last key.  The build is the
          // kernel's register peak, so the walk's state waits in the derivative rows, which the
          // build replaces (the fence keeps the reads after the build).
          double* const park[18] = {&w, &nu, &g[0], &g[1], &g[2], &g[3], &Ka, &Kd, &Kt, &Pc, &Ps, &cp, &sp,
                                    &kqd, &e0, &cl, &cu, &iOm};
#pragma unroll
          for (int m = 0; m < 18; ++m) Drow[m][l] = *park[m];
          wave_sync();
          La = need ? a : La;
          Ld = need ? dl : Ld;
          Lt = need ? dt : Lt;
          KetBlocks K;
          KetEig E2, E3;
          ket_blocks_build<true>(K, La, Ld, Lt, d1, V, &E2, &E3);
          ket_sched_row(K, r, u);
          wave_sync();
#pragma unroll
          for (int m = 0; m < 18; ++m) *park[m] = Drow[m][l];
          // the lane's row of each block's derivative (zeros off its block), laid out as u
          const int e = r >> 1;
          const bool im = (r & 1) != 0;
          double t2[4], t3[6];
          ket_ctl_row<2, 0>(E2, 0.5, e, im, t2);
          ket_ctl_row<3, 0>(E3, hs, e - 2, im, t3);
#pragma unroll
          for (int m = 0; m < 4; ++m) Drow[m][l] = t2[m];
#pragma unroll
          for (int m = 0; m < 6; ++m) Drow[4 + m][l] = t3[m];
          ket_ctl_row<2, 1>(E2, 0.5, e, im, t2);
          ket_ctl_row<3, 1>(E3, hs, e - 2, im, t3);
#pragma unroll
          for (int m = 0; m < 4; ++m) Drow[10 + m][l] = t2[m];
#pragma unroll
          for (int m = 0; m < 6; ++m) Drow[14 + m][l] = t3[m];
          have = true;
        }
        // the segment's own frame, committed only where the segment is applied
        const double oc = row_bcast<15>(Pc), os = row_bcast<15>(Ps);
        const double cs = skip ? cp : oc, ss = skip ? sp : os;
        const KetSchedStep fw = ket_sched_step(cp, sp, oc, os);
        const KetSchedStep bw = {fw.cd, -fw.sd, fw.c2, -fw.s2};
        const double wr = ket_sched_rotate(w, kq, sg, fw), nr = ket_sched_rotate(nu, kq, sg, bw);
        double uc[10];
#pragma unroll
        for (int m = 0; m < 10; ++m) uc[m] = ((m ^ r) & 1) ? -u[m] : u[m];
        const double wn = ket_sched_apply(uc, wr);
        const double nn = ket_sched_apply(u, nr);
        double gn[4];
        ket_sched_g(nn, wn, gn);
        const double snr = sg * nr;
        // duration: y = H_r w_s
        double X[4];
        {
          const double y = fma(fma(-dl, kqd, e0), wr, a * fma(cl, row_ror2(wr), cu * row_rol2(wr)));
          ket_ctl_sums(snr * y, nr * quad_swap(y), one, X);
        }
        // amplitude and detuning: y = (dU'/dtheta) w_{s-1}
        double A[4], D[4];
        {
          double t[10];
#pragma unroll
          for (int m = 0; m < 10; ++m) t[m] = Drow[m][l];
          const double ya = ket_sched_apply(t, wn);
          ket_ctl_sums(snr * ya, nr * quad_swap(ya), one, A);
#pragma unroll
          for (int m = 0; m < 10; ++m) t[m] = Drow[10 + m][l];
          const double yd = ket_sched_apply(t, wn);
          ket_ctl_sums(snr * yd, nr * quad_swap(yd), one, D);
        }
        if (r == j) {                          // the lane's own segment: table order, c within
          // -(i / Omega) (S_re + i S_im) = (S_im - i S_re) / Omega
          Jrow[4 * RYD_SC_X + 0][l] = dead ? 0.0 : X[1] * iOm;
          Jrow[4 * RYD_SC_X + 1][l] = dead ? 0.0 : -(X[0] * iOm);
          Jrow[4 * RYD_SC_X + 2][l] = dead ? 0.0 : X[3] * iOm;
          Jrow[4 * RYD_SC_X + 3][l] = dead ? 0.0 : -(X[2] * iOm);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            Jrow[4 * RYD_SC_AMP + c][l] = skip ? 0.0 : Om * A[c];
            Jrow[4 * RYD_SC_DELTA + c][l] = skip ? 0.0 : Om * D[c];
          }
          // da/dphi_s = i (g_s - g_{s-1})
          Jrow[4 * RYD_SC_PHASE + 0][l] = skip ? 0.0 : -(g[1] - gn[1]);
          Jrow[4 * RYD_SC_PHASE + 1][l] = skip ? 0.0 : g[0] - gn[0];
          Jrow[4 * RYD_SC_PHASE + 2][l] = skip ? 0.0 : -(g[3] - gn[3]);
          Jrow[4 * RYD_SC_PHASE + 3][l] = skip ? 0.0 : g[2] - gn[2];
        }
        w = skip ? w : wn;
        nu = skip ? nu : nn;
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = skip ? g[c] : gn[c];
        cp = cs;
        sp = ss;
        SCHED_CHUNK_ROR1()
      }
      if (active && r < cnt) {               // s0 + r <= n_seg - 1: within the point's 16 n_seg
        double* o = jac + (ip * ldj + (int64_t)s0 + r);
#pragma unroll
        for (int c = 0; c < 16; ++c) o[c * (int64_t)n_seg] = Jrow[c][l];
      }
    }
  }
}

template <bool STATE>
__global__ __launch_bounds__(S16_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 8))) void
ket_sched_ctl_kernel(const double* __restrict__ prm, int64_t n, int64_t ldp, const double* __restrict__ sched,
                     int64_t ldsc, int n_seg, double* __restrict__ st, int64_t lds, double* __restrict__ sm,
                     int64_t ldm, double* __restrict__ jac, int64_t ldj, uint32_t* __restrict__ status) {
  ket_sched_body<STATE, false, true>(prm, n, ldp, sched, ldsc, n_seg, st, lds, sm, ldm, jac, ldj, status);
}

template <bool STATE>
__global__ __launch_bounds__(S16_BLOCK) void ket_sched_kernel(const double* __restrict__ prm, int64_t n, int64_t ldp,
                                                              const double* __restrict__ sched, int64_t ldsc,
                                                              int n_seg, double* __restrict__ st, int64_t lds,
                                                              double* __restrict__ sm, int64_t ldm,
                                                              uint32_t* __restrict__ status) {
  ket_sched_body<STATE, false>(prm, n, ldp, sched, ldsc, n_seg, st, lds, sm, ldm, nullptr, 0, status);
}

template <bool STATE>
__global__ __launch_bounds__(S16_BLOCK) void ket_sched_jac_kernel(const double* __restrict__ prm, int64_t n,
                                                                  int64_t ldp, const double* __restrict__ sched,
                                                                  int64_t ldsc, int n_seg, double* __restrict__ st,
                                                                  int64_t lds, double* __restrict__ sm, int64_t ldm,
                                                                  double* __restrict__ jac, int64_t ldj,
                                                                  uint32_t* __restrict__ status) {
  ket_sched_body<STATE, true>(prm, n, ldp, sched, ldsc, n_seg, st, lds, sm, ldm, jac, ldj, status);
}
