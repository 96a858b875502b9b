// ryd_sym16.inc -- identical-atom Lindblad propagator kernel, one 16-lane DPP row
// per parameter point (included by ryd_engine.hip inside its anonymous namespace).
//
// The hot path of BASELINE configs C2/C4 (LP square) and C3 (smooth JP): every
// evolve_state -> qutip.mesolve call of evolve_two_pulse_lp (RG/simulation.py:693-776),
// evolve_smooth_sinusoidal_jp (:1502-1760) and evolve_bangbang_jp (:1795-1943) for
// the 4 computational-basis inputs of a point whose two atoms carry equal rates.
//
// Layout.  A wave holds 4 points; point p owns lanes 16p..16p+15 (one DPP row).
// Lane c < 15 of a row is the triangle coordinate c = sym_index(i, j), i <= j, of the
// exchange-symmetric sector R[i][j] = R[j][i] (include/ryd_engine.h basis); lane 15
// idles.  Everything a point needs from another lane of its row comes through DPP
// row_newbcast (lane m of the row broadcast to all 16 as the operand of one VALU op):
// no LDS exchange and no barrier in the squarings or the per-segment state updates
// (only broadcast reads of ten zero words that clear accumulators).
//
//  1. Propagator U = exp(L dt) of the phase-0 segment generator in TRIANGLE
//     coordinates (t_s = R[i][j]; a symmetric R stays symmetric under L and under
//     the propagator): lane c runs the Chebyshev series of column c on the 15-entry
//     triangle (apply_Lsym_re, x / 2^s <= X_BASE_SYM; the unit start vector's terms as
//     DPP bank-masked FMAs), then s squarings.  U is block upper-triangular,
//     [[B, C], [0, D]] over the 5 coordinates (0, m) (an atom in |0><0|: invariant, the
//     single-atom propagator) and the other 10, so lane c's new column k is
//     sum_m U[k][m] U[m][c] with U[k][m] = lane m's column entry k: m < 5 contributes
//     to k < 5 only, m >= 5 to all 15 -- 171 DPP FMAs per lane (the (0,0) column feeds
//     only itself).  LP square leaves the last RYD_LP_UNSQUARED levels to the states.
//  2. One LDS transpose per propagator: lane r then holds row r of U' = S U S^-1 in
//     SEGMENT ORDER (rotated coordinate pairs on quad-partner lanes, below).
//  3. Segments (phase frame): U(Omega e^{i phi}) = Q U(Omega) Q^T, so each segment
//     rotates the state into its frame (each lane mixes in its partner lane ^ 1) and
//     applies U': t_r <- sum_m U'[r][m] bcast_m(t) (15 DPP FMAs).  The |01> input lives
//     on the (0, m) coordinates of atom B (single-atom propagator read off U's (0, m)
//     block, the (0,0) row's coherences halved), |10> is its atom-swap mirror, |00> is
//     coordinate (0, 0) times U'[0][0].
//  4. Rotate back to the lab frame, stage the 4 x 25 rows in LDS, coalesced stores.
// A new propagator is built only when a segment's amplitude or duration changes
// (LP square with |xi| = 1 and smooth JP: once per point; bang-bang: per segment).

constexpr int S16_BLOCK = 64;                // one wave, 4 points
constexpr int S16_PPW = 4;

// RYD_S16_PROF (tools/phase_prof.py builds a variant with it; never the product build):
// per-wave phase timestamps (shader clock) written to the summary's unused Lindblad
// columns instead of their NaNs.
// RYD_S16_SETPRIO: in a launch whose waves are all resident at once (one round: C2's
// 2500 waves on 1024 SIMDs x 4 slots), waves lower their issue priority as they advance
// (3 after the parameter loads, 2 after the Chebyshev columns, 1 after the squarings, 0
// in the state updates), so the arbiter favours the waves that lag behind and the 2-3
// waves of a SIMD stay in step instead of the oldest finishing first and leaving the last
// one alone at single-wave latency (C2 31.4 -> 30.1 us, profiles/r02/ab11).  Launches with
// refill (C3, C4) keep the default oldest-first order, which frees slots sooner (+4 %
// there with priorities).  256 CUs: MI355X / MI350X (gfx950).
#ifndef RYD_S16_SETPRIO
#define RYD_S16_SETPRIO 1
#endif
__device__ __forceinline__ bool s16_one_round() {
  return RYD_S16_SETPRIO && gridDim.x <= 256u * 4u * (unsigned)RYD_S16_WAVES;
}
#define S16_PRIO(n) do { if (s16_one_round()) __builtin_amdgcn_s_setprio(n); } while (0)
#ifndef RYD_S16_PRIO_SPLIT
#define RYD_S16_PRIO_SPLIT 1                 // squarings split over priorities 2 and 1 (C2 -1 %, ab13)
#endif
#ifdef RYD_S16_PROF
#define S16_MARK(k) (s16_ts[k] = (double)__builtin_readcyclecounter())
#define S16_PROF_ARG , double* s16_ts
#define S16_PROF_PASS , s16_ts
#else
#define S16_MARK(k) ((void)0)
#define S16_PROF_ARG
#define S16_PROF_PASS
#endif

// XCD-aware block order: workgroups are dispatched round-robin over the 8 XCDs
// (b -> XCD b % 8), each with its own L2.  The 4 workgroups whose 32-byte column
// pieces (params in, summary out) share a 128-byte line are mapped to the same XCD,
// so each line is fetched and written back once, not once per XCD; successive
// 16-point chunks still rotate over the XCDs, so each XCD gets points from the whole
// sweep (per-point cost varies along it).  A bijection for any grid size (the tail
// beyond the last whole 32-block group keeps its order); affinity only.
#ifndef RYD_XCD_MAP
#define RYD_XCD_MAP 2
#endif
__host__ __device__ __forceinline__ int64_t xcd_block(int64_t b, int64_t nb) {
  if (RYD_XCD_MAP == 0) return b;
  if (RYD_XCD_MAP == 1) {                    // one contiguous range per XCD
    const int64_t q = nb / 8, rem = nb % 8, x = b % 8, k = b / 8;
    return x * q + (x < rem ? x : rem) + k;
  }
  const int64_t full = (nb / 32) * 32;
  if (b >= full) return b;
  const int64_t x = b % 8, k = b / 8;
  return ((k / 4) * 8 + x) * 4 + (k % 4);
}

// wave_max with the partner lane as the DPP operand of the max itself: every lane of these
// four permutations has a valid source, so the move's `old` value never shows and the
// builtin without one (bound_ctrl) lets the compiler fold each move into its v_max_i32_dpp
// (wave_max: a copy, a DPP move and the max per step).  Call with every lane active.
__device__ __forceinline__ int wave_max16(int v) {
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true));   // row_half_mirror
  v = max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true));   // row_mirror
  const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
  const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
  return max(max(a, b), max(c, d));
}

// lane K of each 16-lane row, broadcast to the whole row (DPP row_newbcast, gfx90a+)
template <int K>
__device__ __forceinline__ double row_bcast(double v) {
  const long long x = __builtin_bit_cast(long long, v);
  const long long y = __builtin_amdgcn_update_dpp(0LL, x, 0x150 + K, 0xF, 0xF, false);
  return __builtin_bit_cast(double, y);
}

template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// acc_k += bcast_M(c_k) * w for 5 accumulators: fused v_fmac_f64 with a DPP
// row_newbcast operand (one VALU op per FMA).  Inline asm because the compiler's
// DPP combiner does not fuse 64-bit broadcasts into the FMA (it emits a zeroed
// temporary, a v_mov_b64_dpp and a serialising s_nop per term); the leading s_nop
// covers the VALU-write -> DPP-read hazard (2 wait states) for a source the compiler
// may have copied just before the group.
template <int M, bool NOP>
__device__ __forceinline__ void fmac5_bcast(double& a0, double& a1, double& a2, double& a3, double& a4,
                                            double c0, double c1, double c2, double c3, double c4,
                                            double w) {
  if constexpr (NOP) asm volatile("s_nop 1" ::: "memory");
  asm volatile(
      "v_fmac_f64_dpp %0, %5, %10 row_newbcast:%11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %1, %6, %10 row_newbcast:%11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %2, %7, %10 row_newbcast:%11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %3, %8, %10 row_newbcast:%11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %4, %9, %10 row_newbcast:%11 row_mask:0xf bank_mask:0xf"
      : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4)
      : "v"(c0), "v"(c1), "v"(c2), "v"(c3), "v"(c4), "v"(w), "i"(M));
}

// acc += sum_{m in [M0, M0+5)} bcast_m(x) * o_m   (the state update: one source
// register broadcast from five different lanes)
template <int M0, bool NOP = true>      // NOP: x may have been written just before
__device__ __forceinline__ void dot5_bcast(double& acc, double x, double o0, double o1, double o2, double o3,
                                           double o4) {
#define RYD_DOT5_BODY                                                                          \
  "v_fmac_f64_dpp %0, %1, %2 row_newbcast:%7 row_mask:0xf bank_mask:0xf\n\t"                  \
  "v_fmac_f64_dpp %0, %1, %3 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t"                  \
  "v_fmac_f64_dpp %0, %1, %4 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"                  \
  "v_fmac_f64_dpp %0, %1, %5 row_newbcast:%10 row_mask:0xf bank_mask:0xf\n\t"                 \
  "v_fmac_f64_dpp %0, %1, %6 row_newbcast:%11 row_mask:0xf bank_mask:0xf"
  if constexpr (NOP) {
    asm volatile("s_nop 1\n\t" RYD_DOT5_BODY
                 : "+v"(acc)
                 : "v"(x), "v"(o0), "v"(o1), "v"(o2), "v"(o3), "v"(o4), "i"(M0), "i"(M0 + 1), "i"(M0 + 2),
                   "i"(M0 + 3), "i"(M0 + 4));
  } else {
    asm volatile(RYD_DOT5_BODY
                 : "+v"(acc)
                 : "v"(x), "v"(o0), "v"(o1), "v"(o2), "v"(o3), "v"(o4), "i"(M0), "i"(M0 + 1), "i"(M0 + 2),
                   "i"(M0 + 3), "i"(M0 + 4));
  }
#undef RYD_DOT5_BODY
}

// dst <- column c of src^2 (lane c holds column c of the block upper-triangular U).
// The sources are only read here, so after the leading s_nop (a source may have been
// written just before the call) no DPP read can follow its VALU write within 2 wait
// states.  The accumulators of rows k >= 5 (first used by the m = 5 group, 21 FMAs in)
// are cleared by LDS reads of a zero word instead of VALU moves: 10 VALU fewer per
// squaring, the reads land while the m < 5 groups run.
typedef const __attribute__((address_space(3))) double lds_zero_t;

// MASK (RYD_S16_MASK_IDLE, the balanced form's first build): the 150 FMAs of the m >= 5 groups
// with lanes 0-4 and 15 of every row switched off.  There own = U[m][c] is a structural zero
// (c < 5 <= m; lane 15's column is all zeros), so the unmasked form adds +-0 to accumulators
// that started from +0 and are never -0: the same bits for finite columns.  The broadcast
// sources are lanes 5-14, which stay on (a DPP read of a lane that exec switches off is
// invalid), and a row is on or off as a whole under the caller's `if (it < sq)`.  One asm
// statement, so that no compiler-made move can fall under the narrowed exec; exec is ANDed, not
// overwritten, and restored.  An SALU write of exec needs no wait states before a VALU op; the
// s_nop covers a source copied just before the statement (VALU write -> DPP read).
#ifndef RYD_S16_MASK_IDLE
#define RYD_S16_MASK_IDLE 1                  // C2 -0.19 to -0.21 us, in-kernel clock 1.98 -> 2.00 GHz: profiles/sym16_entry/
#endif
#define S16_SQ_F(k, kc, m, mc) \
  "v_fmac_f64_dpp %" #k ", %" #kc ", %" #mc " row_newbcast:" #m " row_mask:0xf bank_mask:0xf\n\t"
#define S16_SQ_G(m, mc)                                                                                    \
  S16_SQ_F(0, 16, m, mc) S16_SQ_F(1, 17, m, mc) S16_SQ_F(2, 18, m, mc) S16_SQ_F(3, 19, m, mc)              \
  S16_SQ_F(4, 20, m, mc) S16_SQ_F(5, 21, m, mc) S16_SQ_F(6, 22, m, mc) S16_SQ_F(7, 23, m, mc)              \
  S16_SQ_F(8, 24, m, mc) S16_SQ_F(9, 25, m, mc) S16_SQ_F(10, 26, m, mc) S16_SQ_F(11, 27, m, mc)            \
  S16_SQ_F(12, 28, m, mc) S16_SQ_F(13, 29, m, mc) S16_SQ_F(14, 30, m, mc)
__device__ __forceinline__ void square_upper_masked(const double (&c)[NS], double (&a)[NS]) {
  static_assert(NS == 15, "operands 0-14: accumulators, 15: the saved exec, 16-30: columns");
  uint64_t saved;
  asm volatile(
      "s_mov_b64 %15, exec\n\t"
      "s_and_b32 exec_lo, exec_lo, 0x7fe07fe0\n\t"
      "s_and_b32 exec_hi, exec_hi, 0x7fe07fe0\n\t"
      "s_nop 1\n\t"
      S16_SQ_G(5, 21) S16_SQ_G(6, 22) S16_SQ_G(7, 23) S16_SQ_G(8, 24) S16_SQ_G(9, 25)
      S16_SQ_G(10, 26) S16_SQ_G(11, 27) S16_SQ_G(12, 28) S16_SQ_G(13, 29) S16_SQ_G(14, 30)
      "s_mov_b64 exec, %15"
      : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]),
        "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "=&s"(saved)
      : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7]), "v"(c[8]), "v"(c[9]),
        "v"(c[10]), "v"(c[11]), "v"(c[12]), "v"(c[13]), "v"(c[14])
      : "scc");
}
#undef S16_SQ_G
#undef S16_SQ_F

template <bool MASK = false>
__device__ __forceinline__ void square_cols16(const double (&col)[NS], double (&acc)[NS], lds_zero_t* zl) {
  asm volatile("" ::: "memory");             // the zero words are re-read, not forwarded
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = 0.0;
#pragma unroll
  for (int k = 5; k < NS; ++k) {             // distinct words: no load CSE; the empty asm
    acc[k] = zl[k - 5];                      // keeps the loads single (a merged b128 pair
    asm volatile("" ::: "memory");           // would need adjacent registers: v_mov copies)
  }
  static_for<MASK ? 5 : NS>([&](auto M) {
    constexpr int m = decltype(M)::value;
    const double own = col[m];               // U[m][c]
    // U[k][m] = 0 for k >= 5 > m: the lower-left block is structurally zero
    if constexpr (m == 0) {
      // column (0, 0) of U is U[0][0] e_0 (nothing leaves |00><00|): only k = 0
      asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf"
                   : "+v"(acc[0])
                   : "v"(col[0]), "v"(own));
    } else {
      fmac5_bcast<m, m == 1>(acc[0], acc[1], acc[2], acc[3], acc[4], col[0], col[1], col[2], col[3], col[4],
                             own);
    }
    if constexpr (m >= 5) {
      fmac5_bcast<m, false>(acc[5], acc[6], acc[7], acc[8], acc[9], col[5], col[6], col[7], col[8], col[9], own);
      fmac5_bcast<m, false>(acc[10], acc[11], acc[12], acc[13], acc[14], col[10], col[11], col[12], col[13],
                            col[14], own);
    }
  });
  if constexpr (MASK) square_upper_masked(col, acc);
}

// ---- laser phases (smooth JP, bang-bang) -------------------------------------------
// sin and cos in ~40 VALU: k = rint(x 2/pi), the reduction r = x - k pi/2 by three FMAs
// against the 3-part split of pi/2 (P1 + P2 + P3 carries ~160 bits; each FMA forms its
// product exactly, so r is within an ulp for |x| < 1e15), then the fdlibm/musl minimax
// kernels on |r| <= pi/4 (< 1 ulp) and the quadrant swap.  |x| >= 1e15, inf and NaN give
// NaN (a laser phase that large has no meaning; the point is flagged NONFINITE).  No
// library call: its large-argument path would spill this kernel's registers.  Against
// the library the results differ by an ulp at most, ~1e-15 on a 300-segment state.
__device__ __forceinline__ void fast_sincos(double x, double& s, double& c) {
  const bool ok = fabs(x) < 1e15;
  const double k = rint(x * 0.63661977236758134308);            // 2 / pi
  double r = fma(-k, 1.5707963267948966, x);                       // pi/2 = P1 + P2 + P3
  r = fma(-k, 6.123233995736766e-17, r);
  r = fma(-k, -1.4973849048591698e-33, r);
  const double z = r * r;
  const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                           2.75573137070700676789e-06), -1.98412698298579493134e-04),
                               8.33333333332248946124e-03), -1.66666666666666324348e-01);
  const double sr = fma(z * r, ps, r);
  const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                           -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                               -1.38888888888741095749e-03), 4.16666666666666019037e-02);
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cr = w + (((1.0 - w) - hz) + z * z * pc);
  const int n = (int)fma(-4.0, floor(k * 0.25), k);                // k mod 4, exact for |k| < 2^53
  const double a = (n & 1) ? cr : sr, b = (n & 1) ? sr : cr;     // sin, cos of the quadrant
  const double nan = __builtin_nan("");
  s = ok ? ((n & 2) ? -a : a) : nan;
  c = ok ? (((n + 1) & 2) ? -b : b) : nan;
}

// Segment s in polar form for the phase frame: amplitude a >= 0, laser phase
// (c, sn), static detuning dl, duration dt; `hold` = keep the current frame (bang-bang
// padding beyond the point's own segment count).
template <int PROTO>
__device__ __forceinline__ void seg_polar(const PointP& q, int s, int n_steps, bool frame_ok, double& a,
                                          double& c, double& sn, double& dl, double& dt, bool& hold) {
  hold = false;
  dl = q.Dl;
  if (PROTO == RYD_PROTO_LP_SQUARE) {            // simulation.py:728-735
    dt = q.tau;
    if (s == 0) {
      a = q.Om;
      c = 1.0;
      sn = 0.0;
    } else {
      a = q.Om;                                  // |xi| = 1 (compute_phase_shift_xi)
      c = q.xr;
      sn = q.xi;
      // ABI callers may pass any xi: the normalisation (a sqrt and two divisions) sits
      // behind a wave-uniform branch, so a wave of unit xi never issues it
      if (__builtin_amdgcn_ballot_w64(!frame_ok) != 0 && !frame_ok) {
        const double m = sqrt(q.xr * q.xr + q.xi * q.xi);
        a = q.Om * m;
        c = m > 0.0 ? q.xr / m : 1.0;
        sn = m > 0.0 ? q.xi / m : 0.0;
      }
    }
  } else if (PROTO == RYD_PROTO_SMOOTH_JP) {     // simulation.py:1698-1731
    a = q.Om;
    dt = q.tau / (double)n_steps;
    segment_phase<PROTO>(q, s, n_steps, c, sn);
  } else {                                       // bang-bang, simulation.py:1853-1924, Delta = 0
    const Seg g = segment<PROTO>(q, s, n_steps, RYD_SHAPE_SQUARE);
    dl = 0.0;
    dt = g.dt;
    a = q.Om;
    if (s >= q.nseg) {
      hold = true;
      a = 0.0;
      c = 1.0;
      sn = 0.0;
      dt = 0.0;
    } else {
      fast_sincos(col(q.prm, RYD_P_PHI0 + s, q.ld, q.i), sn, c);
    }
  }
}

// b += a on lanes E, 16 + E, 32 + E, 48 + E only (lane E of each DPP row): the unit
// start vector's a_k e_r term of the Clenshaw recurrence as ONE masked VALU add per
// coordinate instead of a compare-and-select per coordinate and lane.  The mask is
// ANDed into the current exec and exec is restored inside the same statement.
// RYD_MASKED_ADD: 3 = DPP bank-masked FMAs, no exec writes (add_unit15_dpp, default;
// bit-identical, C2 -1 % against 2), 2 = five coordinates per exec save/restore (add_unit15;
// C2 -1 % against 1), 1 = one save/restore per coordinate, 0 = compare-and-select.
#ifndef RYD_MASKED_ADD
#define RYD_MASKED_ADD 3
#endif
template <int E>
__device__ __forceinline__ void add_on_row_lane(double& b, double a) {
  if constexpr (RYD_MASKED_ADD == 0) {      // compare-and-select form (A/B reference)
    int rl = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 15;
    if (rl == E) b += a;
    return;
  }
  uint64_t saved;
  asm volatile(
      "s_mov_b64 %1, exec\n\t"
      "s_and_b32 exec_lo, exec_lo, %3\n\t"
      "s_and_b32 exec_hi, exec_hi, %3\n\t"
      "v_add_f64 %0, %0, %2\n\t"
      "s_mov_b64 exec, %1"
      : "+v"(b), "=&s"(saved)
      : "v"(a), "i"(0x00010001u << E)
      : "scc");
}

// b[E0 + j] += a on lane E0 + j of each DPP row, j < 5: exec saved once, then per
// coordinate one s_and_b64 (exec = saved & lanes {E, 16+E, 32+E, 48+E}) and one add;
// the lane masks are loop-invariant SGPR pairs.
template <int E0>
__device__ __forceinline__ void add_on_row_lanes5(double& b0, double& b1, double& b2, double& b3, double& b4,
                                                  double a) {
  constexpr uint64_t M = 0x0001000100010001ull;
  uint64_t saved;
  asm volatile(
      "s_mov_b64 %5, exec\n\t"
      "s_and_b64 exec, %5, %7\n\t"
      "v_add_f64 %0, %0, %6\n\t"
      "s_and_b64 exec, %5, %8\n\t"
      "v_add_f64 %1, %1, %6\n\t"
      "s_and_b64 exec, %5, %9\n\t"
      "v_add_f64 %2, %2, %6\n\t"
      "s_and_b64 exec, %5, %10\n\t"
      "v_add_f64 %3, %3, %6\n\t"
      "s_and_b64 exec, %5, %11\n\t"
      "v_add_f64 %4, %4, %6\n\t"
      "s_mov_b64 exec, %5"
      : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "=&s"(saved)
      : "v"(a), "s"(M << E0), "s"(M << (E0 + 1)), "s"(M << (E0 + 2)), "s"(M << (E0 + 3)), "s"(M << (E0 + 4))
      : "scc");   // s_and writes SCC: the compiler may hold a loop compare in it
}

template <int E0>
__device__ __forceinline__ void add_unit15(double (&b)[NS], double a) {
  if constexpr (RYD_MASKED_ADD == 2) {
    add_on_row_lanes5<0>(b[0], b[1], b[2], b[3], b[4], a);
    add_on_row_lanes5<5>(b[5], b[6], b[7], b[8], b[9], a);
    add_on_row_lanes5<10>(b[10], b[11], b[12], b[13], b[14], a);
  } else {
    static_for<NS>([&](auto E) { add_on_row_lane<decltype(E)::value>(b[decltype(E)::value], a); });
  }
}

// RYD_MASKED_ADD == 3: the same unit adds with no exec writes.  b[E] += a on lane E of
// each row is v_fmac_f64_dpp b[E], a, sel row_newbcast:E bank_mask:(bank of E): the DPP
// bank mask writes only the 4-lane bank holding lane E, and sel (1.0 on the lanes whose
// index is E mod 4, 0.0 on the other three of the bank) zeroes their product, so b + 1*a
// lands on lane E alone (exactly b + a; every lane of a row carries the same a).  15 VALU,
// no SALU, no exec dependency chain; sel = 4 lane constants.
template <int E>
__device__ __forceinline__ void fmac_unit_dpp(double& b, double a, double sel, bool nop) {
  if (nop) {
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:%4"
                 : "+v"(b) : "v"(a), "v"(sel), "i"(E), "i"(1 << (E >> 2)));
  } else {
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:%4"
                 : "+v"(b) : "v"(a), "v"(sel), "i"(E), "i"(1 << (E >> 2)));
  }
}
__device__ __forceinline__ void add_unit15_dpp(double (&b)[NS], double a, const double (&sel)[4]) {
  static_for<NS>([&](auto E) {
    constexpr int e = decltype(E)::value;
    fmac_unit_dpp<e>(b[e], a, sel[e & 3], e == 0);   // a may have been written just before
  });
}

// apply_Lsym for a generator with a real Rabi frequency (hy = hy2 = 0: every propagator
// this kernel builds is the phase-0 one of the phase frame): the same fma chains with the
// terms that multiply hy or hy2 (exact zeros) left out -- 66 generator ops per column
// instead of 90, bit-identical up to the sign of a zero.
__device__ __forceinline__ double mrow_re(const Gen& a, int r, double u1, double u2, double u3, double u4,
                                          double o) {
  switch (r) {
    case 0: return fma(a.g0, u2, o);
    case 1: return fma(a.g1, u2, fma(-a.hx2, u4, o));
    case 2: return fma(a.mg01, u2, fma(a.hx2, u4, o));
    case 3: return fma(-a.G, u3, fma(a.hz2, u4, o));
    default: return fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o)));
  }
}

__device__ __forceinline__ void apply_Lsym_re(const Gen& a, double vs, const double (&t)[15], double (&o)[15]) {
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = i; j < 5; ++j) {
      const int s = sym_index(i, j);
      double acc = mrow_re(a, i, t[tri(1, j)], t[tri(2, j)], t[tri(3, j)], t[tri(4, j)], o[s]);
      o[s] = mrow_re(a, j, t[tri(i, 1)], t[tri(i, 2)], t[tri(i, 3)], t[tri(i, 4)], acc);
    }
  const double v2 = 2.0 * vs;
  const double r23 = t[tri(2, 3)], r24 = t[tri(2, 4)], r33 = t[tri(3, 3)], r34 = t[tri(3, 4)],
               r44 = t[tri(4, 4)];
  o[tri(2, 3)] = fma(-v2, r24, o[tri(2, 3)]);
  o[tri(2, 4)] = fma(v2, r23, o[tri(2, 4)]);
  o[tri(3, 3)] = fma(-v2, r34, o[tri(3, 3)]);
  o[tri(3, 4)] = fma(-vs, r44, fma(vs, r33, o[tri(3, 4)]));
  o[tri(4, 4)] = fma(v2, r34, o[tri(4, 4)]);
}

// Chebyshev degree for the sym16 kernel's scaled arguments (x <= X_BASE_SYM <= 1): the
// first k with (x/2)^k / k! < 1e-17 (k > x holds for every k >= 1, and the terms
// decrease).  1e-17 (cheb_terms: 1e-18) -- the s <= 14 squarings amplify the truncation
// to < 2e-13, below their own rounding (~4e-12 on the propagator entries, DESIGN.md
// section 4); one term fewer at x near X_BASE_SYM.  The terms decrease in j and increase
// in h = x/2, so kt = 1 + #{j <= 17 : h >= TH_j} with TH_j the smallest double whose
// j-th term reaches 1e-17 (exact rational check, tools/cheb_thresholds.py): 17 compares
// instead of the 34-multiply product chain (identical kt on 2e5 random arguments).
// BOUNDED: the caller guarantees x <= X_BASE_SYM (build16's scaled argument).
template <bool BOUNDED = false>
__device__ __forceinline__ int cheb_terms_small(double x) {
  static_assert(X_BASE_SYM <= 1.0, "cheb_terms_small covers x <= 1 (17 terms)");
  constexpr double TH[17] = {1e-17, 4.4721359549995795e-09, 3.914867641168864e-06, 0.00012446659545769568,
                             0.0010371372893366482, 0.004394290351366487, 0.0125993232817844,
                             0.02822864716464555, 0.05356271212458357, 0.09036001686117834,
                             0.1398168813097236, 0.20262580209060138, 0.2790704614462359,
                             0.36912378048400807, 0.47253426642798413, 0.5888961629494429,
                             0.7177037357024775};
  // build16 passes y <= X_BASE_SYM (up to the rounding of x / X_BASE_SYM; exact at 0.5), so
  // a threshold above X_BASE_SYM / 2 is never reached there and its compare is left out:
  // 12 compares of the 17 at X_BASE_SYM = 0.5, the same count
  constexpr double HMAX = BOUNDED ? 0.5 * X_BASE_SYM * (1.0 + 1e-12) : 1.0;
  const double h = 0.5 * x;
  int k = 1;
#pragma unroll
  for (int j = 0; j < 17; ++j)
    if (TH[j] <= HMAX) k += (h >= TH[j]) ? 1 : 0;
  return k;
}

// Miller's backward recurrence starts at the fixed even order S16_KS for every lane: above
// every series cut (kt <= 18 for x <= 1, so kcut <= 18), so the Clenshaw loop carries no
// per-term seed test, and a lane's Bessel coefficients depend on its own x only.  From
// order 20 the normalised J_k agree with scipy's jv to ~1e-16 relative for x <= 1; the
// seed 1e-200 grows by < 20! (2/x)^20 down to J_0, finite for x > X_SKIP = 1e-20.
constexpr int S16_KS = 20;

// cheb_segment for the unit start vector e_r (this lane's column of the propagator):
// the same recurrence, with the a_k v terms added to coordinate r only (fma(a, 1, b) =
// a + b, fma(a, 0, b) = b), so v needs no registers during the series.  The lane of a
// row IS its column index (r = lane & 15), so "coordinate r" is "lane e of the row".
// An inactive lane (lane 15, an invalid or empty point) runs the recurrence with zero
// coefficients and J_0 = S = 1, which leaves exactly e_r (nothing for lane 15) without
// a select per coordinate; the caller zeroes an inactive point's generator.
// (double)k of a wave-uniform order 1 <= k < 2^20 put together on the scalar unit (exponent
// from the leading bit, the mantissa shifted into the high word): the same double as the
// conversion, which would be a VALU op per order of the recurrence
__device__ __forceinline__ double order_f64(int k) {
  const int e = 31 - __builtin_clz((unsigned)k);
  const unsigned hi = ((unsigned)(1023 + e) << 20) | (((unsigned)k << (20 - e)) & 0xFFFFFu);
  return __builtin_bit_cast(double, (unsigned long long)hi << 32);
}

template <typename Apply>
__device__ __forceinline__ void cheb_unit16(double (&out)[NS], int r, double x, bool active, Apply apply2Y,
                                            int& nuse, int& nexec, lds_zero_t* zl) {
  const int kt = active ? cheb_terms_small<true>(x) : -1;
  const int kmax = wave_max16(kt);
  if (kmax < 0) {                            // no active lane in the wave: identity columns
    asm volatile("" : "+v"(r));
#pragma unroll
    for (int e = 0; e < NS; ++e) out[e] = (e == r) ? 1.0 : 0.0;
    return;
  }
  const int kcut = (kmax + 1) & ~1;
  // the 30 accumulators start from LDS zero words, as the squarings' do: the reads land
  // behind the Miller-only orders and the first division instead of 30 VALU moves
  double bA[NS], bB[NS];
  asm volatile("" ::: "memory");             // re-read, not forwarded or merged
#pragma unroll
  for (int e = 0; e < NS; ++e) {
    bA[e] = zl[e];
    asm volatile("" ::: "memory");
  }
#pragma unroll
  for (int e = 0; e < NS; ++e) {
    bB[e] = zl[e];
    asm volatile("" ::: "memory");
  }
  double sel[4];                             // RYD_MASKED_ADD == 3: 1.0 on lanes = q mod 4
  {
    const int q = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) sel[j] = (q == j) ? 1.0 : 0.0;
  }
  auto unit_add = [&](double (&b)[NS], double a) {
    if constexpr (RYD_MASKED_ADD == 3) add_unit15_dpp(b, a, sel);
    else add_unit15<0>(b, a);
  };
  const double i2x = active ? 2.0 / x : 0.0;
  // J_KS = seed, J_KS+1 = 0; then J_KS-1 and the Miller-only pairs above the cut
  double Jp2 = 0.0, Jp1 = active ? MILLER_SEED : 0.0;
  double S = 2.0 * Jp1;
  {
    const double J = fma(i2x * (double)S16_KS, Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = J;
  }
  for (int k = S16_KS - 2; k > kcut; k -= 2) {
    const double Jk = fma(i2x * order_f64(k + 1), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk;
    S = fma(2.0, Jk, S);
    const double Jk1 = fma(i2x * order_f64(k), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk1;
  }
  // The first pair (k = kcut >= 2) is peeled: bA is still zero there, so its first
  // application adds exact zeros to bB = c_k e_r and is left out (same bits).
  {
    const int k = kcut;
    const double Jk = fma(i2x * order_f64(k + 1), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk;
    S = fma(2.0, Jk, S);
    unit_add(bB, k <= kt ? 2.0 * Jk : 0.0);
    const double Jk1 = fma(i2x * order_f64(k), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk1;
    unit_add(bA, k - 1 <= kt ? 2.0 * Jk1 : 0.0);
    apply2Y(bB, bA);
  }
  for (int k = kcut - 2; k >= 2; k -= 2) {
    double Jk = fma(i2x * order_f64(k + 1), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk;
    S = fma(2.0, Jk, S);
    const double ck = k <= kt ? 2.0 * Jk : 0.0;
    unit_add(bB, ck);
    apply2Y(bA, bB);
    double Jk1 = fma(i2x * order_f64(k), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk1;
    const double ck1 = k - 1 <= kt ? 2.0 * Jk1 : 0.0;
    unit_add(bA, ck1);
    apply2Y(bB, bA);
  }
  double J0 = fma(i2x, Jp1, -Jp2);
  S += J0;
  if (!active) {
    J0 = 1.0;
    S = 1.0;
  }
  unit_add(bB, J0);
#pragma unroll
  for (int e = 0; e < NS; ++e) bA[e] *= 0.5;
  apply2Y(bA, bB);
  const double inv = 1.0 / S;
#pragma unroll
  for (int e = 0; e < NS; ++e) out[e] = bB[e] * inv;
  if (active) nuse += kt + 1;
  nexec += kcut + 1;
}

// segment_phase for the sym16 smooth-JP chunk: the reference's phase A cos(w_mod t_m -
// phi_off) at the segment midpoint (RG/simulation.py:1698-1731), with fast_sincos
__device__ __forceinline__ void segment_phase16(const PointP& q, int s, int n_steps, double& c, double& sn) {
  const double dt = q.tau / (double)n_steps;
  const double tm = (double)s * dt + dt / 2;
  double st, ct;
  fast_sincos(q.wmod * tm - q.phoff, st, ct);
  fast_sincos(q.A * ct, sn, c);
}

// ---- the segment phase in SEGMENT ORDER --------------------------------------------
// The laser phase of a segment is a rotation T(c, s) of each atom's (ex, ey) pair, i.e.
// of the triangle coordinates (i, 3), (i, 4) for i = 0, 1, 2 by the angle and of the
// (3,3), (3,4), (4,4) block, a symmetric 2 x 2 tensor, which in the basis
// m = t33 - t44, q = 2 t34, p = t33 + t44 is p invariant and (m, q) rotated by the
// double angle.  Segment order puts every rotated pair on lanes (2k, 2k + 1):
//   lane  0:(0,0) 1:(0,1) 2:(0,3) 3:(0,4) 4:(0,2) 5:(1,1) 6:(1,3) 7:(1,4)
//         8:(2,3) 9:(2,4) 10:m 11:q 12:(1,2) 13:(2,2) 14:p 15:-
// so a segment rotates the STATE (each lane mixes in its quad partner, lane ^ 1: 11 FP64
// ops + 4 b32 DPP moves for t and z) instead of every lane's propagator row (25 ops),
// then applies the phase-0 propagator U' = S U S^-1 (rows built above).  The B block
// (an atom in |0><0|) stays on lanes 0-4, so |01> (z) uses the same lanes and pair.
constexpr int SEG_M = 10, SEG_Q = 11, SEG_P = 14;
__host__ __device__ constexpr int seg_old(int n) {      // plain segment coordinate -> triangle index
  return n == 0 ? 0 : n == 1 ? 1 : n == 2 ? 3 : n == 3 ? 4 : n == 4 ? 2 : n == 5 ? 5 : n == 6 ? 7
       : n == 7 ? 8 : n == 8 ? 10 : n == 9 ? 11 : n == 12 ? 6 : n == 13 ? 9 : 0;
}

// ---- the CU-balanced launch form (LP square, small launches) -------------------------
// One workgroup per CU runs `gpc` four-point groups, strided over the batch: workgroup b of W
// takes the groups k W + xcd_block(b, W), k < gpc (s16_bal_job).  Consecutive groups cost
// alike (C2: a row of the grid shares its Rabi frequency, hence its squaring depth), so gpc
// consecutive ones would load whole CUs heavy or light; the stride gives every CU a sample of
// the sweep, and xcd_block keeps the four groups of a 128-byte parameter line on one XCD as
// in the one-wave kernel.  Wave w of a workgroup
// takes its role from its index alone: the first waves run one whole job each (the
// one-wave kernel's body); when 1 or 2 jobs are left over beyond a multiple of 4, each of
// them is split in time between a PRODUCER wave (parameter load to S16_BAL_HSQ squarings
// into build16, the 15 column registers per lane parked in LDS) and a CONSUMER wave (the
// rest of the job), so that with round-robin wave placement the four SIMDs of a CU carry
// gpc / 4 jobs each (C2: 10 groups per CU -> 8 whole waves, 2 producers, 2 consumers, 2.5
// jobs per SIMD instead of 3, 3, 2, 2).  The schedule is static -- no queue, no counter --
// and correctness does not depend on where the waves land.  s16_bal_role is the one role
// table: the kernel and the host plan (ryd_sym16_balance_plan) both evaluate it.
constexpr int S16_BAL_MAXW = 16;             // waves per workgroup at most (gpc <= 16)
constexpr int S16_BAL_WHOLE = 0, S16_BAL_PRODUCER = 1, S16_BAL_CONSUMER = 2;
#ifndef RYD_S16_BAL_HSQ
#define RYD_S16_BAL_HSQ 2                    // squarings before the handoff (even: the ping-pong pairs stay
                                             // whole); 0, 2, 4 measured: profiles/sym16_balance/tuning.txt
#endif
static_assert(RYD_S16_BAL_HSQ >= 0 && RYD_S16_BAL_HSQ % 2 == 0, "handoff after whole squaring pairs");
#ifndef RYD_S16_BAL_POLLS
#define RYD_S16_BAL_POLLS 4096               // a consumer's polls before it runs the producer's part itself
#endif
#ifdef RYD_S16_PROF
constexpr int S16_BAL_NCNT = 4;
#else
constexpr int S16_BAL_NCNT = 2;
#endif
struct S16Role {
  int role, off;                             // the workgroup's off-th job; a split job's slot = off - (gpc & ~3)
};
__host__ __device__ __forceinline__ int64_t s16_bal_job(int64_t wg, int64_t nwg, int off) {
  return (int64_t)off * nwg + xcd_block(wg, nwg);
}
__host__ __device__ constexpr bool s16_bal_split(int gpc) { return (gpc & 3) == 1 || (gpc & 3) == 2; }
__host__ __device__ constexpr int s16_bal_waves(int gpc) { return gpc + (s16_bal_split(gpc) ? (gpc & 3) : 0); }
__host__ __device__ constexpr S16Role s16_bal_role(int gpc, int w) {
  const int rem = gpc & 3, nwhole = s16_bal_split(gpc) ? gpc - rem : gpc;
  if (w < nwhole) return {S16_BAL_WHOLE, w};
  if (w < nwhole + rem) return {S16_BAL_PRODUCER, w};
  return {S16_BAL_CONSUMER, w - rem};
}

// build16's view of a split job (S16NoHandoff: the whole build, today's code)
struct S16NoHandoff {};
struct S16Handoff {
  int role, slot;
  bool poll;                                 // false: the consumer takes the fallback at once
  double (&cols)[2][NS][64];                 // [slot][column entry][lane]
  int (&cnt)[2][S16_BAL_NCNT][64];           // nuse, nexec (PROF build: and the producer's stamps)
  int (&flag)[2];
  int* polls;                                // PROF build: polls made, fallback taken
};

// The consumer's wait: the producer's flag (LDS, workgroup scope) polled a bounded number
// of times with the wave asleep in between.  false = still clear: the caller runs the
// producer's part itself and never reads the slot, so no wait outlasts the bound and the
// result does not depend on the outcome.
__device__ __forceinline__ bool s16_wait_flag(int* f, int* polls) {
  for (int i = 0; i < RYD_S16_BAL_POLLS; ++i) {
    const int v = __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__builtin_amdgcn_readfirstlane(v) != 0) {
      if (polls) *polls = i + 1;
      return true;
    }
    __builtin_amdgcn_s_sleep(4);
  }
  if (polls) *polls = -RYD_S16_BAL_POLLS;
  return false;
}

// Issue priorities of the balanced form.  A split job is the launch's longest dependency
// chain (two waves run it one after the other, the second starts late), so its producer and
// its consumer keep the highest priority from start to end, and the whole-job waves run the
// one-round schedule's phase-stepped levels lowered by RYD_S16_BAL_PRIO_DROP: they fill the
// issue slots the split job leaves.
#ifndef RYD_S16_BAL_PRIO_DROP
#define RYD_S16_BAL_PRIO_DROP 0
#endif
template <int LEVEL, typename HO>
__device__ __forceinline__ void s16_phase_prio(const HO& ho) {
  if constexpr (std::is_same<HO, S16NoHandoff>::value) {
    S16_PRIO(LEVEL);
  } else {
    if (ho.role == S16_BAL_WHOLE)
      __builtin_amdgcn_s_setprio(LEVEL > RYD_S16_BAL_PRIO_DROP ? LEVEL - RYD_S16_BAL_PRIO_DROP : 0);
  }
}

// Build this point's phase-0 propagator for (amplitude a, detuning dl, duration dt)
// and leave row r of it in u (identity when the point is invalid or the segment is
// empty).  Called by the whole wave in uniform control flow; `count` = this point
// asked for the build (flop counters).
// The last min(s, keep) squaring levels are left out: U_built = exp(L dt)^(1 / 2^rep),
// rep = min(s, keep), and the caller applies it 2^rep times per segment (for the few
// states of LP square, 2^rep - 1 extra row updates cost less than `keep` squarings).
// nsq counts the full depth s (RYD_S_NSQUARE).  nrep = the wave's largest rep.
// HO = S16Handoff (the balanced form's first build): a producer wave leaves after the series
// and min(RYD_S16_BAL_HSQ, the wave's squaring count) squarings, its columns and series
// counters parked in the job's LDS slot, and returns true (the wave is done); a consumer
// repeats the set-up arithmetic (the same instructions, the same bits), takes the columns
// from the slot and goes on from there -- or, its wait exhausted, runs everything itself.
template <typename HO = S16NoHandoff>
__device__ __forceinline__ bool build16(double (&u)[NS], double (&Ut)[S16_PPW][NS][16], const PointP& q,
                                        bool valid, bool count, double a, double dl, double dt, int p, int r,
                                        int keep, int& rep, int& nrep, int& nuse, int& nexec, int& nsq,
                                        bool& over_cap, lds_zero_t* zl S16_PROF_ARG, const HO& ho = HO{}) {
  constexpr bool SPLIT = !std::is_same<HO, S16NoHandoff>::value;
  const bool lane_ok = r < NS;
  Seg g;
  g.om_re = a;
  g.om_im = 0.0;                             // phase 0: apply_Lsym_re below relies on it
  g.dl = dl;
  g.dt = dt;
  double rsum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) rsum += fabs(q.gA[k]) + fabs(q.gB[k]);
  // h_bounds' half-width 0.5 sqrt(a a + 0 0): the correctly rounded root of the rounded
  // square is |a| itself as long as a a neither overflows nor leaves the normal range
  // (or a = 0), so a wave of such amplitudes takes 0.5 |a| -- the same double -- and the
  // root stays behind a wave-uniform branch for the rest (NaN included)
  const double fa = fabs(a);
  const bool plain = (fa >= 0x1p-500 && fa <= 0x1p500) || fa == 0.0;
  double hw = 0.5 * fa;
  if (__builtin_amdgcn_ballot_w64(!plain) != 0) {
    double ar = g.om_re;
    asm volatile("" : "+v"(ar));             // stays a branch: the root is not speculated into a select
    hw = 0.5 * sqrt(ar * ar + g.om_im * g.om_im);
  }
  double emin, emax;
  h_bounds_w(hw, g.dl, q.V, q.d1, emin, emax);
  const double omega = (emax - emin) + rsum;
  const double x = omega * dt;
  const bool capped = valid && !(x <= 1e12);
  const bool act = valid && !capped && x > X_SKIP;
  over_cap = over_cap || (count && capped);
  int sqf = 0;                               // scaling-and-squaring depth
  if (act && x > X_BASE_SYM) {               // ceil(log2(x / X_BASE_SYM)), exactly, from the exponent
    int e;
    const double m = frexp(x / X_BASE_SYM, &e);
    sqf = m == 0.5 ? e - 1 : e;
  }
  const double y = act ? ldexp(x, -sqf) : 0.0;
#ifndef RYD_S16_SQ_CAP
  const int sq = sqf > keep ? sqf - keep : 0;          // squarings performed here
#else
  // measurement-only build (never the product; DESIGN.md section 10, the slow/fast block
  // A/B): at most RYD_S16_SQ_CAP squarings, the time floor of a build whose stiff block
  // would need no more levels than the slow one -- the results are wrong by construction
  const int sq = min(sqf > keep ? sqf - keep : 0, RYD_S16_SQ_CAP);
  rep = sqf > keep ? keep : sqf;                       // the levels beyond the cap are skipped
#endif
#ifndef RYD_S16_SQ_CAP
  rep = sqf - sq;
#endif
  const double sc = act ? 2.0 / omega : 0.0;
  Gen A = make_gen(g, q.d1, q.gA, sc);
  double vs = sc * 0.5 * q.V;
  if (!act) {                                // exact zeros (an invalid point may carry NaNs):
    A = Gen{};                               // cheb_unit16 then leaves the identity
    vs = 0.0;
  }
  // ---- (1) Chebyshev column r of exp(y L) on the triangle
  double v[NS];
  const int nuse0 = nuse;
  bool have = false;                         // the columns come from the producer's slot
  bool producer = false;
  if constexpr (SPLIT) {
    producer = ho.role == S16_BAL_PRODUCER;
    if (ho.role == S16_BAL_CONSUMER && ho.poll) have = s16_wait_flag(&ho.flag[ho.slot], ho.polls);
  }
  if (!SPLIT || !have) {
    cheb_unit16(v, r, y, act && lane_ok,
                [&](const double (&b)[NS], double (&o)[NS]) { apply_Lsym_re(A, vs, b, o); }, nuse, nexec, zl);
    if (!count) nuse = nuse0;                // each distinct propagator counted once
  }
  S16_MARK(2);
  s16_phase_prio<2>(ho);
  // ---- (2) squarings, column-held, DPP broadcasts within the row
  // one reduction of the full depth serves both loops: sq and rep are monotone in sqf, so
  // their maxima over the wave are the same functions of the largest depth
  const int sfm = wave_max16(sqf);
  nrep = sfm > keep ? keep : sfm;
#ifndef RYD_S16_SQ_CAP
  const int smx = sfm > keep ? sfm - keep : 0;
#else
  const int smx = min(sfm > keep ? sfm - keep : 0, RYD_S16_SQ_CAP);
#endif
  int it0 = 0, it1 = smx;                    // the squarings this wave runs
  if constexpr (SPLIT) {
    const int hs = min((int)RYD_S16_BAL_HSQ, smx);     // a shallower wave hands over where it ends
    const int l = 16 * p + r;
    if (producer) it1 = hs;
    if (have) {
      it0 = hs;
#pragma unroll
      for (int k = 0; k < NS; ++k) v[k] = ho.cols[ho.slot][k][l];
      nuse = ho.cnt[ho.slot][0][l];          // what cheb_unit16 left in the producer (count = valid there too)
      nexec = ho.cnt[ho.slot][1][l];
    }
  }
  {
    for (int it = it0; it < it1; it += 2) {
      double w[NS];                          // ping-pong: v -> w -> v (nothing carried in w)
      if (RYD_S16_PRIO_SPLIT && it == ((smx >> 1) & ~1)) s16_phase_prio<1>(ho);   // second half of the squarings
      if (it < sq) square_cols16<SPLIT && RYD_S16_MASK_IDLE != 0>(v, w, zl);
      if (it + 1 < sq) {
        square_cols16<SPLIT && RYD_S16_MASK_IDLE != 0>(w, v, zl);
      } else if (it < sq) {
#pragma unroll
        for (int k = 0; k < NS; ++k) v[k] = w[k];
      }
    }
  }
  if constexpr (SPLIT) {
    if (producer) {
      // park the columns and the series counters, then publish: the release orders the
      // slot's LDS writes before the flag for the consumer's acquire.  Nothing is awaited.
      const int l = 16 * p + r;
#pragma unroll
      for (int k = 0; k < NS; ++k) ho.cols[ho.slot][k][l] = v[k];
      ho.cnt[ho.slot][0][l] = nuse;
      ho.cnt[ho.slot][1][l] = nexec;
#ifdef RYD_S16_PROF
      S16_MARK(3);
      ho.cnt[ho.slot][2][l] = (int)(s16_ts[3] - s16_ts[0]);
      ho.cnt[ho.slot][3][l] = (int)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
#endif
      __hip_atomic_store(&ho.flag[ho.slot], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      return true;
    }
  }
  if (count) nsq += sqf;
  S16_MARK(3);
  s16_phase_prio<1>(ho);
  // ---- (3) transpose through LDS: lane r takes row r of U' = S U S^-1 (segment order)
  wave_sync();
  if (lane_ok) {
    // the row side of S on the column-held values (m = t33 - t44, q = 2 t34, p = t33 + t44:
    // 3 ops per lane), written in segment order: Ut[p][n][c] = (S U)[n][c]
    static_for<NS>([&](auto N) {
      constexpr int nn = decltype(N)::value;
      double w;
      if constexpr (nn == SEG_M) w = v[sym_index(3, 3)] - v[sym_index(4, 4)];
      else if constexpr (nn == SEG_Q) w = 2.0 * v[sym_index(3, 4)];
      else if constexpr (nn == SEG_P) w = v[sym_index(3, 3)] + v[sym_index(4, 4)];
      else w = v[seg_old(nn)];
      Ut[p][nn][r] = w;
    });
  }
  wave_sync();
  // row r of S U: 15 plain reads; lane 15 reads zero words (its row of U' is zero).  An
  // inactive point's columns are the unit vectors, U = I, and so is U' (the 1/2 weights
  // below are exact)
  lds_zero_t* const src = lane_ok ? (lds_zero_t*)&Ut[p][r][0] : zl;
  double R[NS];
#pragma unroll
  for (int m = 0; m < NS; ++m) R[m] = src[m];
  // columns: (S U) S^-1 -- plain coordinates are renamed, (m, q, p) recombined
  static_for<NS>([&](auto N) {
    constexpr int nn = decltype(N)::value;
    if constexpr (nn == SEG_M) u[nn] = 0.5 * (R[sym_index(3, 3)] - R[sym_index(4, 4)]);
    else if constexpr (nn == SEG_Q) u[nn] = 0.5 * R[sym_index(3, 4)];
    else if constexpr (nn == SEG_P) u[nn] = 0.5 * (R[sym_index(3, 3)] + R[sym_index(4, 4)]);
    else u[nn] = R[seg_old(nn)];
  });
  S16_MARK(4);
  s16_phase_prio<0>(ho);
  return false;
}

// Lane weights of the state rotation T(c, s) in segment order: t' = al t + be t[lane ^ 1]
// with al = wT c + w2 C2 + wI, be = bT s + b2 S2 (C2, S2 = cos, sin of the double angle).
struct SegRot {
  double wI, wT, w2, bT, b2;
};

__device__ __forceinline__ SegRot seg_rot(int r) {
  const bool th = r == 2 || r == 3 || r == 6 || r == 7 || r == 8 || r == 9;   // (i,3), (i,4)
  const bool dbl = r == SEG_M || r == SEG_Q;
  const double sg = (r & 1) ? -1.0 : 1.0;             // first of a pair: +s, second: -s
  SegRot w;
  w.wI = (th || dbl) ? 0.0 : 1.0;
  w.wT = th ? 1.0 : 0.0;
  w.w2 = dbl ? 1.0 : 0.0;
  w.bT = th ? sg : 0.0;
  w.b2 = dbl ? sg : 0.0;
  return w;
}

// the quad partner's value (lane ^ 1): two 32-bit DPP quad_perm [1,0,3,2] moves (64-bit
// DPP on gfx950 supports only row_newbcast)
template <int CTRL>
__device__ __forceinline__ double dpp32x2(double v) {
  const long long x = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_mov_dpp((int)(x & 0xffffffffll), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(x >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double quad_swap(double v) { return dpp32x2<0xB1>(v); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ double row_shr1(double v) { return dpp32x2<0x111>(v); }   // row_shr:1 (lane 0: 0)

// acc += bcast_J(a) * wa + bcast_J(b) * wb (row_newbcast operands of two fused FMAs; the
// leading s_nop covers a source the compiler may have copied just before the group)
template <int J>
__device__ __forceinline__ void fmac2_bcast(double& acc, double a, double wa, double b, double wb) {
  asm volatile(
      "s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %1, %2 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %3, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf"
      : "+v"(acc)
      : "v"(a), "v"(wa), "v"(b), "v"(wb), "i"(J));
}

// (t, z) <- T(c, s) (t, z) in segment order (z: the |01> state on lanes 0-4, pair 2-3)
__device__ __forceinline__ void rotate_state(double& t, double& z, double c, double s, const SegRot& w) {
  const double C2 = fma(c, c, -s * s), S2 = 2.0 * (c * s);
  const double al = fma(w.wT, c, fma(w.w2, C2, w.wI));
  const double be = fma(w.bT, s, w.b2 * S2);
  const double tp = quad_swap(t), zp = quad_swap(z);
  t = fma(al, t, be * tp);
  z = fma(al, z, be * zp);
}

// The |01> row of lane r (< 5): the single-atom block of U' with the (0,0) row's
// coherences halved (a triangle coordinate (0, m) is R[0][m] + R[m][0])
struct SegRow01 {
  double o[5], u00;
};

__device__ __forceinline__ SegRow01 seg_row01(const double (&u)[NS], int r) {
  SegRow01 k;
  const double h = r == 0 ? 0.5 : (r < 5 ? 1.0 : 0.0);
  k.o[0] = r < 5 ? u[0] : 0.0;
#pragma unroll
  for (int m = 1; m < 5; ++m) k.o[m] = h * u[m];
  k.u00 = row_bcast<0>(u[0]);
  return k;
}

// (t, z, s00) <- U' (t, z, s00), the states in the segment frame (lane 15: zero row,
// z beyond lane 4: zero row -- no output selects)
#ifndef RYD_JP_WTAB
#define RYD_JP_WTAB 1                        // smooth JP: rotation weights from an LDS table
#endif
typedef double d2v __attribute__((ext_vector_type(2)));
#ifndef RYD_SEG_LDS_ZERO
#define RYD_SEG_LDS_ZERO 1                   // smooth JP: chains start from LDS zero words (C3 -2 %, profiles/r02/ab7)
#endif
template <bool S00 = true>                   // S00 = false: the caller powers U'_00 itself
__device__ __forceinline__ void seg_apply(const double (&u)[NS], const SegRow01& k, double& t, double& z,
                                          double& s00, lds_zero_t* zl = nullptr) {
  double acc = 0.0, acc1 = 0.0;               // one 15-term chain for t, one 5-term for z
  if constexpr (RYD_SEG_LDS_ZERO != 0 && !S00) {   // A/B: the chain starts from LDS zero words
    asm volatile("" ::: "memory");
    acc = zl[0];
    asm volatile("" ::: "memory");
    acc1 = zl[1];
  }
  dot5_bcast<0>(acc, t, u[0], u[1], u[2], u[3], u[4]);
  dot5_bcast<5, false>(acc, t, u[5], u[6], u[7], u[8], u[9]);
  dot5_bcast<10, false>(acc, t, u[10], u[11], u[12], u[13], u[14]);
  dot5_bcast<0>(acc1, z, k.o[0], k.o[1], k.o[2], k.o[3], k.o[4]);
  t = acc;
  if constexpr (S00) s00 = k.u00 * s00;
  z = acc1;
}

// STATE = false: the summary-only twin (lindblad_sym16_nostate_kernel) -- no state rows staged or stored
template <bool STATE = true>
__device__ __forceinline__ void sym16_epilogue(double t, double z, double s00, double cp, double sp,
                                               const SegRot& rw, bool valid, bool over_cap, int nuse, int nexec,
                                               int nsq, int l, int p, int64_t blk, int64_t n,
                                               double* __restrict__ st, int64_t lds, double* __restrict__ sm,
                                               int64_t ldm, uint32_t* __restrict__ status, bool st32, int wt,
                                               double (&Ut)[S16_PPW][NS][16] S16_PROF_ARG);

// load_point for a lane of this kernel: column f of the lane's point is read at the
// wave-uniform address prm + f ld + i0 (64-bit, SGPRs) plus the lane's 32-bit byte offset
// po8 (8 x its clamped point index within the wave): a global load with an SGPR base and
// a VGPR offset, no per-lane 64-bit add per column (LP square and bang-bang: every load;
// smooth JP: the first load_point, its chunk loop keeps the 64-bit adds).
typedef __attribute__((address_space(1))) char s16_gchar;
typedef __attribute__((address_space(1))) double s16_gdouble;
template <int PROTO>
__device__ __forceinline__ PointP load_point16(const double* __restrict__ prm, int64_t ldp, int64_t i0,
                                               unsigned po8) {
  unsigned off = po8;                        // widened where it is used: the offset operand is
  if constexpr (PROTO != RYD_PROTO_SMOOTH_JP)   // matched within the block of the loads (smooth
    asm("" : "+v"(off));                     // JP: its chunk loop's 3 loads; costs 5 VGPRs there)
  PointP q = load_point_with<PROTO>([&](int f) {
    const char* base = reinterpret_cast<const char*>(prm + ((int64_t)f * ldp + i0));
    asm("" : "+s"(base));                    // stays a scalar base: not re-associated with po8
    // the barrier loses the pointer's address space; as a global pointer again the load
    // takes the SGPR base and the lane offset directly (global_load ..., v_off, s[base])
    const s16_gchar* gbase = (const s16_gchar*)base;
    return *reinterpret_cast<const s16_gdouble*>(gbase + off);
  });
  q.prm = prm;
  q.ld = ldp;
  q.i = i0 + (int64_t)(po8 >> 3);
  return q;
}

// The balanced form's first load where launch() has checked that 8 (14 ldp + n) fits 31 bits
// (BAL = 2): ONE load instruction per wave.  Lane r of a row loads column r of the row's
// point (lane 15 repeats column 14) at the wave-uniform base prm + i0 plus its 32-bit byte
// offset 8 r ldp + po8, and the row's 15 values go to all its lanes by DPP row broadcasts
// (moves: the same doubles as 15 loads of 16 equal addresses each).  A one-round launch has
// every wave of a CU at this point at once, and the CU's one address unit takes a 64-lane load
// at a time: 15 per wave kept it busy for ~2900 cycles, the start-up of the last wave served
// (profiles/sym16_start/).  The 64-bit form (load_point16) stays for batches beyond the check
// and under RYD_S16_PARAM64=1, and for the rare reloads of the general path.
template <int PROTO>
__device__ __forceinline__ PointP load_point16_row(const double* __restrict__ prm, int64_t ldp, int64_t i0,
                                                   unsigned po8, int r) {
  static_assert(PROTO == RYD_PROTO_LP_SQUARE && RYD_P_XI_IM == NS - 1, "LP square: columns 0 .. 14, one per lane");
  const unsigned f = (unsigned)(r < NS ? r : NS - 1);
  const unsigned off = f * (8u * (unsigned)ldp) + po8;
  const char* base = reinterpret_cast<const char*>(prm + i0);
  asm("" : "+s"(base));                      // stays a scalar base (load_point16)
  const double x = *reinterpret_cast<const s16_gdouble*>((const s16_gchar*)base + off);
  double c[NS];
  static_for<NS>([&](auto K) { c[decltype(K)::value] = row_bcast<decltype(K)::value>(x); });
  PointP q = load_point_with<PROTO>([&](int k) { return c[k]; });
  q.prm = prm;
  q.ld = ldp;
  q.i = i0 + (int64_t)(po8 >> 3);
  return q;
}

// The balanced form's validity test of its first load: the loaded columns are taken in hand at
// one point (a single wait for the last of them instead of one per column as each is first
// compared), and point_valid's predicates are ANDed without its short-circuit order, which the
// compiler turns into nested exec-masked blocks.  Every predicate is a pure compare, so the
// result is point_valid's for every input, NaNs and negative values included.
__device__ __forceinline__ void s16_in_hand(PointP& q) {
  asm volatile("" : "+v"(q.Om), "+v"(q.Dl), "+v"(q.V), "+v"(q.d1), "+v"(q.gA[0]), "+v"(q.gA[1]), "+v"(q.gA[2]),
               "+v"(q.gA[3]), "+v"(q.gB[0]), "+v"(q.gB[1]), "+v"(q.gB[2]), "+v"(q.gB[3]), "+v"(q.tau), "+v"(q.xr),
               "+v"(q.xi));
}
template <int PROTO>
__device__ __forceinline__ bool point_valid_flat(const PointP& q) {
  static_assert(PROTO == RYD_PROTO_LP_SQUARE, "point_valid's LP-square predicates");
  const auto fin = [](double x) { return (int)isfinite(x); };
  int ok = (int)(q.Om > 0.0) & fin(q.Om) & fin(q.V) & fin(q.Dl) & fin(q.d1);
#pragma unroll
  for (int c = 0; c < 4; ++c)
    ok &= (int)(q.gA[c] >= 0.0) & (int)(q.gB[c] >= 0.0) & fin(q.gA[c]) & fin(q.gB[c]);
  return (ok & (int)(q.tau > 0.0) & fin(q.tau)) != 0;
}

template <int PROTO>
__global__ __launch_bounds__(S16_BLOCK) __attribute__((amdgpu_waves_per_eu(PROTO == RYD_PROTO_BANGBANG ? 3 : RYD_S16_WAVES, 8))) void
lindblad_sym16_kernel(const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st,
                      int64_t lds, double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status,
                      int n_steps, int shape, int st32) {
  (void)shape;
  constexpr int BAL = PROTO < 0 ? 1 : 0;     // 0, and dependent: the balanced form's statements are discarded
  constexpr int gpc = 0, nohandoff = 0, wt = 0, p32 = 0, nwg = 0;
  constexpr bool STATE = true;
#include "ryd_sym16_body.inc"
}

// The summary-only twin (launch() with a null state pointer): the same body, the epilogue
// without the state rows.  `st` is NULL and `lds` unread.
template <int PROTO>
__global__ __launch_bounds__(S16_BLOCK) __attribute__((amdgpu_waves_per_eu(PROTO == RYD_PROTO_BANGBANG ? 3 : RYD_S16_WAVES, 8))) void
lindblad_sym16_nostate_kernel(const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st,
                              int64_t lds, double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status,
                              int n_steps, int shape, int st32) {
  (void)shape;
  constexpr int BAL = PROTO < 0 ? 1 : 0;
  constexpr int gpc = 0, nohandoff = 0, wt = 0, p32 = 0, nwg = 0;
  constexpr bool STATE = false;
#include "ryd_sym16_body.inc"
}

// The balanced form: one workgroup of s16_bal_waves(gpc) waves per gpc groups.
// Its LDS (a copy of every array per wave and the two handoff slots) keeps one workgroup
// on a CU, so a launch of at most one workgroup per CU puts gpc groups on each.
// BAL = 2: the first load is one instruction with 32-bit lane offsets (load_point16_row; launch()
// picks it where the offsets fit).  A template argument, not a kernel argument: behind a
// run-time branch the compiler merges the two forms' loads and gives every column a per-lane
// 64-bit address.
// The argument list is the launch's entry: the first eight arguments, 14 dwords -- what a wave
// needs up to its parameter load, then what the summary stores need -- are the ones the
// balanced kernels' translation unit (ryd_sym16_bal.hip) has preloaded into SGPRs, so no wave
// waits for an argument fetch before its load.  `cfg` packs the small integers (s16_bal_cfg),
// `nwg` is the grid size (gridDim.x would be a fetch from the implicit arguments).
__host__ __device__ constexpr int s16_bal_cfg(int gpc, int st32, int nohandoff, int wt) {
  return gpc | (st32 ? 32 : 0) | (nohandoff ? 64 : 0) | (wt << 7);
}
#define RYD_S16_BAL_PARAMS                                                                                   \
  const double* __restrict__ prm, int64_t n, int64_t ldp, int cfg, int nwg, double* __restrict__ sm,         \
      uint32_t* __restrict__ status, int64_t ldm, double* __restrict__ st, int64_t lds, int n_steps
#define RYD_S16_BAL_UNPACK                                                                                   \
  static_assert(PROTO == RYD_PROTO_LP_SQUARE && (BAL == 1 || BAL == 2), "the balanced form is built for LP square"); \
  static_assert(S16_BAL_MAXW < 32, "gpc takes cfg's low five bits");                                         \
  constexpr int p32 = BAL == 2;                                                                              \
  const int gpc = cfg & 31, st32 = cfg & 32, nohandoff = cfg & 64, wt = cfg >> 7
template <int PROTO, int BAL>
__global__ __launch_bounds__(S16_BLOCK * S16_BAL_MAXW) __attribute__((amdgpu_waves_per_eu(RYD_S16_WAVES, 8))) void
lindblad_sym16_kernel(RYD_S16_BAL_PARAMS) {
  RYD_S16_BAL_UNPACK;
  constexpr bool STATE = true;
#include "ryd_sym16_body.inc"
}

// the balanced form's summary-only twin (`wt & S16_WT_SUMMARY` still selects write-through)
template <int PROTO, int BAL>
__global__ __launch_bounds__(S16_BLOCK * S16_BAL_MAXW) __attribute__((amdgpu_waves_per_eu(RYD_S16_WAVES, 8))) void
lindblad_sym16_nostate_kernel(RYD_S16_BAL_PARAMS) {
  RYD_S16_BAL_UNPACK;
  constexpr bool STATE = false;
#include "ryd_sym16_body.inc"
}

// Output stores of the balanced form (`wt`, a kernel argument: RYD_S16_WT in launch()).  A
// one-round launch ends everywhere at once: with plain stores the 956 bytes per point sit
// dirty in the XCDs' L2s until the end-of-kernel release writes them back while nothing else
// runs.  A write-through store (relaxed, agent scope: global_store ... sc1) sends its line on
// to memory as it is issued, while other waves still compute, and the release finds the L2s
// clean.  The same values at the same addresses either way.  C2, kernel time: plain 25.96 us,
// the state rows write-through 25.09, the 32-byte summary and status pieces too 24.77 (four
// partial writes per line instead of one merged in L2 still cost less than leaving the line
// for the release): profiles/sym16_edges/.
constexpr int S16_WT_STATE = 1, S16_WT_SUMMARY = 2;
constexpr int S16_WT_AUTO = S16_WT_STATE | S16_WT_SUMMARY;   // launch() without RYD_S16_WT
template <bool WT, typename P, typename T>
__device__ __forceinline__ void s16_store(P* ptr, T v) {
  if constexpr (WT) __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *ptr = v;
}

// the 25 state rows of a wave's four points: lane l stores column cc of rows l / 16 + 4 j
template <bool WT>
__device__ __forceinline__ void s16_store_state(const double (&v)[7], double* __restrict__ st, int64_t lds,
                                                int64_t i0, int l, int cc, bool in, bool st32) {
  if (st32) {
    // the wave-uniform address st + 4 i0 + 4 j lds (SGPRs) plus the lane's 32-bit byte
    // offset 8 (cc + (l / 16) lds); launch() has checked that the offset fits
    const unsigned lo = 8u * ((unsigned)cc + (unsigned)(l >> 4) * (unsigned)lds);
    if (in) {
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        if (j < 6 || l < 16) {
          char* bj = reinterpret_cast<char*>(st + (4 * i0 + 4 * j * lds));
          asm("" : "+s"(bj));
          s16_store<WT>(reinterpret_cast<s16_gdouble*>((s16_gchar*)bj + lo), v[j]);
        }
      }
    }
  } else {
    double* dst = st + 4 * i0 + cc;
    if (in) {
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int row = (l >> 4) + 4 * j;
        if (j < 6 || l < 16) s16_store<WT>(dst + (int64_t)row * lds, v[j]);
      }
    }
  }
}

// lane r's summary column of point i = i0 + p, the counters (lanes 0-3) and the status word
template <bool WT>
__device__ __forceinline__ void s16_store_summary(double v, double c, uint32_t stat, double* __restrict__ sm,
                                                  int64_t ldm, uint32_t* __restrict__ status, int64_t i0, int64_t i,
                                                  int r, int p, bool st32) {
  if (st32) {
    // the point is i0 + p.  Wave-uniform bases sm + i0, sm + 16 ldm + i0 and status + i0 plus
    // the lane's 32-bit byte offsets (checked by launch())
    char* b0 = reinterpret_cast<char*>(sm + i0);
    char* b1 = reinterpret_cast<char*>(sm + (RYD_S_NMV_USEFUL * ldm + i0));
    char* b2 = reinterpret_cast<char*>(status + i0);
    asm("" : "+s"(b0));
    asm("" : "+s"(b1));
    asm("" : "+s"(b2));
    const unsigned lo = 8u * ((unsigned)r * (unsigned)ldm + (unsigned)p);
    s16_store<WT>(reinterpret_cast<s16_gdouble*>((s16_gchar*)b0 + lo), v);
    if (r < 4) s16_store<WT>(reinterpret_cast<s16_gdouble*>((s16_gchar*)b1 + lo), c);
    if (r == 0)
      s16_store<WT>(reinterpret_cast<__attribute__((address_space(1))) uint32_t*>((s16_gchar*)b2 + 4u * (unsigned)p),
                    stat);
  } else {
    s16_store<WT>(sm + ((int64_t)r * ldm + i), v);
    if (r < 4) s16_store<WT>(sm + ((int64_t)(RYD_S_NMV_USEFUL + r) * ldm + i), c);
    if (r == 0) s16_store<WT>(status + i, stat);
  }
}

template <bool STATE>
__device__ __forceinline__ void sym16_epilogue(double t, double z, double s00, double cp, double sp,
                                               const SegRot& rw, bool valid, bool over_cap, int nuse, int nexec,
                                               int nsq, int l, int p, int64_t blk, int64_t n,
                                               double* __restrict__ st, int64_t lds, double* __restrict__ sm,
                                               int64_t ldm, uint32_t* __restrict__ status, bool st32, int wt,
                                               double (&Ut)[S16_PPW][NS][16] S16_PROF_ARG) {
  const int r = l & 15;
  const bool lane_ok = r < NS;
  const int64_t ip = blk * S16_PPW + p;
  const int64_t i = ip < n ? ip : n - 1;
  rotate_state(t, z, cp, sp, rw);
  // segment order -> triangle coordinates: (3,3) = (p + m)/2, (3,4) = q/2, (4,4) = (p - m)/2
  {
    const double mv = row_bcast<SEG_M>(t), pv = row_bcast<SEG_P>(t);
    if (r == SEG_M) t = 0.5 * (pv + mv);
    if (r == SEG_Q) t = 0.5 * t;
    if (r == SEG_P) t = 0.5 * (pv - mv);
  }
  // ---- stage the 4 x 25 sector rows of each point (in Ut) and store them coalesced
  // (STATE = false, the summary-only twin: nothing is staged or stored; the summary below is
  // formed from registers either way)
  const int64_t i0 = blk * S16_PPW;
  if constexpr (STATE) {
    double (*Ro)[4][NC] = reinterpret_cast<double (*)[4][NC]>(&Ut[0][0][0]);
    wave_sync();                               // the last transpose is read
#pragma unroll
    for (int e = r; e < 4 * NC; e += 16) (&Ro[p][0][0])[e] = 0.0;
    wave_sync();
    if (lane_ok) {
      // lane -> (ia, ja) in segment order (after the conversion above lanes 10, 11, 14 hold
      // (3,3), (3,4), (4,4)): nibble tables
      const int ia = (int)((0x0421332211100000ull >> (4 * r)) & 15);
      const int ja = (int)((0x0422434343124310ull >> (4 * r)) & 15);
      Ro[p][3][5 * ia + ja] = t;
      Ro[p][3][5 * ja + ia] = t;
    }
    if (r < 5) {
      const int mz = (int)((0x24310u >> (4 * r)) & 15);  // z lanes 0-4 hold (0,0) (0,1) (0,3) (0,4) (0,2)
      Ro[p][1][mz] = z;
      Ro[p][2][5 * mz] = z;
    }
    if (r == 0) Ro[p][0][0] = s00;
    wave_sync();
    // lane l stores column cc = l % 16 (point cc / 4, input cc % 4) of rows l / 16 + 4 j
    {
      const int cc = l & 15, pp = cc >> 2, k = cc & 3;
      const bool in = i0 + pp < n;
      double v[7];
#pragma unroll
      for (int j = 0; j < 7; ++j)              // rows 25 .. 27 (j = 6, lanes >= 16): read inside Ut, never stored
        v[j] = (&Ro[pp][k][0])[(l >> 4) + 4 * j];
      static_assert(NC == 25, "rows l/16 + 4 j: j < 6 always inside, j = 6 on the first 16 lanes only");
      if (wt & S16_WT_STATE) s16_store_state<true>(v, st, lds, i0, l, cc, in, st32);
      else s16_store_state<false>(v, st, lds, i0, l, cc, in, st32);
    }
  }
#ifdef RYD_S16_PROF
  S16_MARK(7);
#endif
  static_assert(RYD_S_POP0 == 0 && RYD_S_AVG_POP == 12 && RYD_S_AVG_F == 15 && RYD_S_NMV_USEFUL == 16 &&
                    RYD_S_NMV_EXEC == 17 && RYD_S_TRACE11 == 18 && RYD_S_NSQUARE == 19,
                "summary columns are written by lane index");
  // ---- per-point summary from the row's lanes (DPP broadcasts and one ballot; no LDS
  // round trips): the staged values are t (lab frame) on lanes < 15, z on lanes < 5 and
  // s00, all other staged entries are zeros
  const bool ok = (!lane_ok || isfinite(t)) && (r >= 5 || isfinite(z)) && isfinite(s00);
  const uint64_t bad = __builtin_amdgcn_ballot_w64(!ok);
  const bool fin = ((bad >> (16 * p)) & 0xFFFFull) == 0;
  const double z1 = row_bcast<1>(z), t11 = row_bcast<5>(t);        // (0,1) and (1,1)
  // Tr rho_11 = sum over the 3 x 3 qubit block of R11, in row-major order of the 5 x 5 rows
  const double t00 = row_bcast<0>(t), t01 = row_bcast<1>(t);       // segment-order lanes
  const double t02 = row_bcast<4>(t), t12 = row_bcast<12>(t);
  const double t22 = row_bcast<13>(t);
  const double tr11 = ((((((((0.0 + t00) + t01) + t02) + t01) + t11) + t12) + t02) + t12) + t22;
  if (ip < n) {
    const double nan = __builtin_nan("");
    const double avg = 0.25 * (s00 + z1 + z1 + t11);    // pops |00>, |01>, |10>, |11>
    // lane r writes summary column r (POP0..AVG_F); lanes 0-3 also the counters
    double v = nan;
    if (r < 4) v = r == 0 ? s00 : (r == 3 ? t11 : z1);
    else if (r == RYD_S_AVG_POP || r == RYD_S_AVG_F) v = avg;
#ifdef RYD_S16_PROF
    S16_MARK(6);
    s16_ts[9] = (double)__builtin_amdgcn_s_memrealtime();
    if (r >= 4 && r < 10) v = s16_ts[r - 3] - s16_ts[0];
    if (r == 10 || r == 11) v = s16_ts[r - 2];
    if (r == 13) v = (double)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
    if (r == 14) v = s16_ts[7] - s16_ts[0];
    if (s16_ts[10] != 0.0 && (r == 12 || r == 15)) v = s16_ts[r == 12 ? 10 : 11];
#endif
    // the counters: one integer select, then one conversion (the same doubles)
    const int ci = r == 0 ? NS * nuse : r == 1 ? 16 * nexec : nsq;
    double c = r == 2 ? tr11 : (double)ci;
#ifdef RYD_S16_PROF
    // the start-up stamps in place of three counters: barrier passed, column loads issued,
    // values in hand (cycles from entry; 'load' ends at column 4)
    if (r >= 1 && r < 4) c = s16_ts[11 + r] - s16_ts[0];
#endif
    uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
    if (over_cap) stat |= RYD_STATUS_STEP_CAP;
    if (!fin) stat |= RYD_STATUS_NONFINITE;
    if (wt & S16_WT_SUMMARY) s16_store_summary<true>(v, c, stat, sm, ldm, status, i0, i, r, p, st32);
    else s16_store_summary<false>(v, c, stat, sm, ldm, status, i0, i, r, p, st32);
  }
}
