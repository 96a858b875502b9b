// ryd_sched16.inc -- custom pulse schedules on the identical-atom row layout of ryd_sym16.inc
// (included by ryd_engine.hip after it, inside the anonymous namespace).
//
// ryd_run_schedule[_device]: every point brings its own table of n_seg piecewise-constant
// segments (include/ryd_engine.h, "custom pulse schedules"); segment s is
//   Seg{om = a_s Omega e^{i phi_s}, dl = delta_s Omega, dt = x_s / Omega}
// in the sense of segment<PROTO>().  The kernel is the bang-bang loop of ryd_sym16_body.inc
// with the segments read from the table: four points per wave, one 16-lane DPP row each,
// build16 for a propagator, rotate_state / seg_apply per segment, sym16_epilogue at the end.
//
// Table.  Read by the protocol of ryd_sched_table.inc (SCHED_TABLE_VALID, SCHED_CHUNK_*).
//
// Memo.  A propagator depends on (a Omega, delta Omega, x / Omega) and the point's scalars
// only (the phase is carried by the frame), so a segment whose key equals -- ==, the three
// products are formed the same way every time -- the key of the row's last build reuses it.
// The wave builds when any of its rows needs to (ballot); a row that does not need to is
// rebuilt with the key of ITS last build, the same propagator bit for bit, so a row's bits
// and its NSQUARE / NMV_USEFUL never depend on its neighbours (NMV_EXEC counts what the wave
// executed, as in every kernel of this family).  Before the first build the row holds the
// identity under the key (0, 0, 0), which no segment of positive duration equals.
//
// Validity.  The pass of ryd_sched_table.inc.  An invalid row keeps its basis states -- it takes
// part in no segment, and its builds are identities -- and is flagged BAD_INPUT.
// A segment of duration zero (x_s / Omega == 0) is skipped and keeps the frame.
//
// Registers: the states, the frame, the chunk's values and the memo key are parked in LDS
// across an in-loop build, as the bang-bang branch parks its states.

constexpr int SC16_WAVES = 3;                // amdgpu_waves_per_eu: the bang-bang instantiation's budget

template <bool STATE>
__global__ __launch_bounds__(S16_BLOCK) __attribute__((amdgpu_waves_per_eu(SC16_WAVES, 8))) void
lindblad_sched16_kernel(const double* __restrict__ prm, int64_t n, int64_t ldp, const double* __restrict__ sched,
                        int64_t ldsc, int n_seg, double* __restrict__ st, int64_t lds, double* __restrict__ sm,
                        int64_t ldm, uint32_t* __restrict__ status, int st32) {
  __shared__ __attribute__((aligned(16))) double Ut[S16_PPW][NS][16];   // transpose, then output staging
  __shared__ double Zl[16];                  // zero words (build16, lane 15's row)
  __shared__ double Sv[S16_PPW][16][7];      // parked across a build: t, z and the chunk's five values per lane
  __shared__ double Sp[S16_PPW][8];          // ... s00, cp, sp and the key the row is built with
  __shared__ int Sc[S16_PPW][2];             // ... nuse, nsq
#ifdef RYD_S16_PROF
  double s16_ts[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) s16_ts[k] = 0.0;
#endif
  const int l = (int)threadIdx.x;
  const int p = l >> 4, r = l & 15;
  if (l < 16) Zl[l] = 0.0;                   // same wave: ordered before the first build
  // the wave's first point and the lane's point, both clamped to the batch
  const int64_t b0 = xcd_block(blockIdx.x, gridDim.x) * S16_PPW;
  const int64_t i0 = b0 < n ? b0 : n - 1;    // a wave past the batch (padded grid) reads point n - 1
  const int64_t last = n - 1 - i0;           // >= 0
  const int pc = min(p, last < S16_PPW - 1 ? (int)last : S16_PPW - 1);
  const unsigned po8 = 8u * (unsigned)pc;
  // the lane's table row: point i0 + pc <= n - 1 (ldsc = 0: the shared row)
  const double* __restrict__ row = sched + (i0 + (int64_t)pc) * ldsc;

  bool valid;
  {
    const PointP q = load_point16<RYD_PROTO_LP_SQUARE>(prm, ldp, i0, po8);
    valid = sched16_point_valid(q);
  }
  SCHED_TABLE_VALID(valid, row, n_seg, r, p)

  // states: |11> triangle coordinate r; |01> atom-B coordinate r (r < 5); |00> scalar
  double t = (r == sym_index(1, 1)) ? 1.0 : 0.0;
  double z = (r == 1) ? 1.0 : 0.0;
  double s00 = 1.0;
  double cp = 1.0, sp = 0.0;                 // frame the states are in
  int nuse = 0, nexec = 0, nsq = 0;
  bool over_cap = false;
  // row r of the current propagator: the identity until the first build
  double u[NS];
#pragma unroll
  for (int m = 0; m < NS; ++m) u[m] = (m == r) ? 1.0 : 0.0;
  SegRow01 k1 = seg_row01(u, r);
  double La = 0.0, Ld = 0.0, Lt = 0.0;       // the key of the row's last build
  int rep = 0, nrep = 0;                     // (no level is left unsquared here: keep = 0)

  for (int s0 = 0; s0 < n_seg; s0 += 16) {
    // ---- the chunk: lane r's segment s0 + r (clamped), key and phase
    double Ka, Kd, Kt, Pc, Ps;
    {
      const double* pp = prm;
      asm volatile("" : "+s"(pp));           // re-read (an L1 hit), not kept live through the builds
      const double Om = pp[(int64_t)RYD_P_OMEGA * ldp + i0 + (int64_t)pc];
      SCHED_CHUNK_LOAD(row, n_seg, s0, r, Om)
      if (!valid) {
        SCHED_CHUNK_NEUTRAL()
      }
    }
    const int cnt = min(16, n_seg - s0);
    for (int j = 0; j < cnt; ++j) {
      // segment s0 + j: lane 0 of the row after j rotations
      const double a = row_bcast<0>(Ka), dl = row_bcast<0>(Kd), dt = row_bcast<0>(Kt);
      const bool skip = !valid || dt == 0.0;
      const bool need = !skip && !(a == La && dl == Ld && dt == Lt);
      if (__builtin_amdgcn_ballot_w64(need) != 0) {
        // Every row of the wave rebuilds, a row that does not need to with its last key
        Sv[p][r][0] = t;
        Sv[p][r][1] = z;
        Sv[p][r][2] = Ka;
        Sv[p][r][3] = Kd;
        Sv[p][r][4] = Kt;
        Sv[p][r][5] = Pc;
        Sv[p][r][6] = Ps;
        if (r == 0) {
          Sp[p][0] = s00;
          Sp[p][1] = cp;
          Sp[p][2] = sp;
          Sp[p][3] = need ? a : La;
          Sp[p][4] = need ? dl : Ld;
          Sp[p][5] = need ? dt : Lt;
          Sc[p][0] = nuse;
          Sc[p][1] = nsq;
        }
        wave_sync();
        int nu = 0, nq = 0;
        {
          const double ba = Sp[p][3], bd = Sp[p][4], bt = Sp[p][5];
          const double* pb = prm;
          asm volatile("" : "+s"(pb));
          const PointP qb = load_point16<RYD_PROTO_LP_SQUARE>(pb, ldp, i0, po8);
          build16(u, Ut, qb, valid, need, ba, bd, bt, p, r, 0, rep, nrep, nu, nexec, nq, over_cap,
                  (lds_zero_t*)Zl S16_PROF_PASS);
        }
        t = Sv[p][r][0];
        z = Sv[p][r][1];
        Ka = Sv[p][r][2];
        Kd = Sv[p][r][3];
        Kt = Sv[p][r][4];
        Pc = Sv[p][r][5];
        Ps = Sv[p][r][6];
        s00 = Sp[p][0];
        cp = Sp[p][1];
        sp = Sp[p][2];
        La = Sp[p][3];
        Ld = Sp[p][4];
        Lt = Sp[p][5];
        nuse = Sc[p][0] + nu;
        nsq = Sc[p][1] + nq;
        wave_sync();
        k1 = seg_row01(u, r);                // the |01> row is not kept live across a build
      }
      // into the segment's frame, then U'; a skipping row computes along and keeps its values
      {
        const double cs = skip ? cp : row_bcast<0>(Pc), ss = skip ? sp : row_bcast<0>(Ps);
        const double cr = cp * cs + sp * ss, sr = sp * cs - cp * ss;
        const SegRot rw = seg_rot(r);
        double tn = t, zn = z, sn00 = s00;
        rotate_state(tn, zn, cr, sr, rw);
        seg_apply(u, k1, tn, zn, sn00);
        t = skip ? t : tn;
        z = skip ? z : zn;
        s00 = skip ? s00 : sn00;
        cp = cs;
        sp = ss;
      }
      SCHED_CHUNK_ROL1()
    }
  }
  // ---- back to the lab frame Q(cp, sp); the lane and point indices are recomputed here
  {
    const int lid = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    int pl = lid >> 4;
    asm volatile("" : "+v"(pl));
    const int64_t b2 = xcd_block(blockIdx.x, gridDim.x);
    const SegRot rw_out = seg_rot(lid & 15);
    return sym16_epilogue<STATE>(t, z, s00, cp, sp, rw_out, valid, over_cap, nuse, nexec, nsq, lid, pl, b2, n, st, lds,
                                 sm, ldm, status, st32 != 0, 0, Ut S16_PROF_PASS);
  }
}
