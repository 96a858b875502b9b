// ryd_coh_prop.inc -- the process-map coherences (SURVEY.md §8 a12 / f2) by propagator.
// Included by ryd_engine.hip after coherence_cheb_kernel (whose sector generators
// apply_coh, make_gen, make_cgen it uses) and after ryd_sym16.inc (DPP helpers).
//
// coherence_cheb_kernel evolves each coherence input with a per-lane Chebyshev series over
// the whole pulse: the series length grows with omega tau ~ V tau ~ 10^3 (4.9 MFLOP per C2
// point, 120x the Lindblad state evolution itself).  Here, as lindblad_sym16_kernel does
// for the 25-dim sector, each sector's propagator exp(L dt) at laser phase 0 is built ONCE
// per point -- Chebyshev columns at dt / 2^s (x <= CP_XS) and s squarings -- and applied to
// the sector's inputs, segment by segment in the laser-phase frame:
// L(phi) = R L(0) R^-1 with R rho = e^{i phi N_r} rho e^{-i phi N_r}, which in a sector's
// coordinates rotates each (ex, ey) pair of a q = 0 factor by phi and multiplies each
// |0><r| (|r><0|) coordinate of a q = -1 (+1) factor by e^{-i phi} (e^{+i phi}).  One
// propagator per sector serves LP square's two pulses and smooth JP's 300 segments; a
// schedule whose |Omega|, Delta or dt changes (bang-bang) rebuilds it.  LP shaped keeps
// coherence_cheb_kernel (a new amplitude every segment).
//
// Mapping (round 5): one wave = 4 points, one 16-lane DPP row per point.
//  * (0,-1) sector (and (-1,0) for unequal atoms): n = 10 complex coordinates, lane c < 10
//    builds column c.  Squarings in registers: new column c = sum_m U[:, m] U[m][c] with
//    U[k][m] = lane m's entry k fetched by DPP row_newbcast:m as the operand of the FMA
//    itself (4 v_fmac_f64_dpp per complex product, the -Im part through the DPP source's
//    neg modifier).  The coordinates with atom A (B) in |0><0| are invariant (nothing
//    leaves |0>), so U is block upper-triangular and those 2 columns feed only themselves:
//    84 complex products per squaring instead of 100.  (Round 4 read U[k][m] from an LDS
//    copy of the row: 100 16-byte LDS reads, two waits and a store per squaring, at 2
//    waves per SIMD.)
//  * (-1,-1) and (-1,+1) sectors together: n = 4, quad 0 of the row builds (-1,-1), quad
//    1 builds (-1,+1) (the same generator code with per-lane V weight and conjugation),
//    squarings by DPP row_newbcast from each sector's own lanes, written per 4-lane bank.
// The built propagator goes to the row's LDS slice once; the segment updates read rows
// of it (2 pulses for LP square; smooth JP's 300 segments are 10 complex products each).
// With identical atoms (every reference configuration) the (-1,0) sector is the
// atom-swap mirror of (0,-1) and its outputs are copied; otherwise it is built too.

#ifndef RYD_CP_OCC
#define RYD_CP_OCC 2                           // waves per SIMD the register budget allows
#endif
constexpr int CP_BLOCK = 64;                   // one wave, 4 points
constexpr int CP_NR = CP_BLOCK / 16;           // rows (points) per block
// the Chebyshev argument the squarings start from (cheb_terms_small / S16_KS cover x <= 1):
// a term pair costs ~2 generator applications, a squaring ~1.3; 0.5 balances them as in
// the sym16 kernel (the propagator entries stay within ~2^s eps of exact, s <= 14)
#ifndef RYD_CP_XS
#define RYD_CP_XS 0.5
#endif
constexpr double CP_XS = RYD_CP_XS;
// cp_cheb (and the dim-4 kernel, which shares CP_XS) take cheb_terms_small's count and the
// fixed Miller start S16_KS: both cover x <= 1 only, so a larger start would cut the series
static_assert(CP_XS > 0.0 && CP_XS <= 1.0, "cheb_terms_small / S16_KS cover x <= 1");
constexpr int CP_NMAX = 10;

__device__ __forceinline__ void cp_wsync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ int cp_lane() {
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// Chebyshev series of exp(x Y) e_u (the unit start vector of this lane's column u) on NV
// doubles (NV/2 complex coordinates, interleaved re/im), as cheb_unit16: Miller's
// recurrence from the fixed order S16_KS, the a_k e_u terms added to Re(coordinate u) only.
// ROW layout: u = lane & 15 (lanes u >= NV/2 carry no column and end at zero); the unit adds
// are DPP bank-masked FMAs (fmac_unit_dpp).  QUAD layout: u = lane & 3, the unit adds are
// fma(a, sel_u, b) with sel_u = 1 on lanes u mod 4.  An inactive lane runs with zero
// coefficients and J_0 = S = 1: it ends with e_u, the identity column.
// General unit position (ryd_dim4_prop.inc): the unit goes to b[STRIDE u + OFF] on lanes u < NU.
template <int NV, bool QUAD, int STRIDE = 2, int OFF = 0, int NU = NV / 2, typename Apply>
__device__ __forceinline__ void cp_cheb(double (&out)[NV], double x, bool active, Apply apply2Y) {
  const int kt = active ? cheb_terms_small(x) : -1;
  const int kmax = wave_max(kt);
  const int lane = cp_lane();
  const int u = QUAD ? (lane & 3) : (lane & 15);
  if (kmax < 0) {
#pragma unroll
    for (int e = 0; e < NV; ++e) out[e] = (e == STRIDE * u + OFF && u < NU) ? 1.0 : 0.0;
    return;
  }
  const int kcut = (kmax + 1) & ~1;
  const double i2x = active ? 2.0 / x : 0.0;
  double bA[NV], bB[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) bA[e] = bB[e] = 0.0;
  double sel[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sel[j] = ((lane & 3) == j) ? 1.0 : 0.0;
  auto unit_add = [&](double (&b)[NV], double a) {
    if constexpr (QUAD) {
#pragma unroll
      for (int e = 0; e < NU; ++e) b[STRIDE * e + OFF] = fma(a, sel[e], b[STRIDE * e + OFF]);
    } else {
      static_for<NU>([&](auto E) {
        constexpr int e = decltype(E)::value;
        fmac_unit_dpp<e>(b[STRIDE * e + OFF], a, sel[e & 3], e == 0);
      });
    }
  };
  double Jp2 = 0.0, Jp1 = active ? MILLER_SEED : 0.0;
  double S = 2.0 * Jp1;
  {
    const double J = fma(i2x * (double)S16_KS, Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = J;
  }
  for (int k = S16_KS - 2; k > kcut; k -= 2) {
    const double Jk = fma(i2x * (double)(k + 1), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk;
    S = fma(2.0, Jk, S);
    const double Jk1 = fma(i2x * (double)k, Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk1;
  }
  for (int k = kcut; k >= 2; k -= 2) {
    double Jk = fma(i2x * (double)(k + 1), Jp1, -Jp2);
    Jp2 = Jp1;
    Jp1 = Jk;
    S = fma(2.0, Jk, S);
    const double ck = k <= kt ? 2.0 * Jk : 0.0;
    unit_add(bB, ck);
    apply2Y(bA, bB);
    double Jk1 = fma(i2x * (double)k, Jp1, -Jp2);
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
  for (int e = 0; e < NV; ++e) bA[e] *= 0.5;
  apply2Y(bA, bB);
  const double inv = 1.0 / S;
#pragma unroll
  for (int e = 0; e < NV; ++e) out[e] = bB[e] * inv;
}

// The phase-0 generator of a build has a real Rabi frequency (om_im = 0): hy = hy2 = 0 in the
// q = 0 block and m01r = m10r = 0, m01i = m10i in the q = -1 (+1) block.  apply_coh with
// those exact zeros left out (122 instead of 158 FMAs per (0,-1) column term, 50 instead
// of 66 for n = 4; fma(0, x, y) = y, so the same numbers), and 13 + 10 registers of
// coefficients instead of 18 + 16.
struct CpGen0 {                // q = 0 single-atom block, scaled, real Rabi frequency
  double g0, g1, mg01, hx, hx2, hz2, G;
};
struct CpCGen0 {               // q = -1 (conj: +1) block: [[m00, i mo], [i mo, m11]]
  double m00r, m00i, mo, m11r, m11i;
};
__device__ __forceinline__ CpGen0 cp_gen0(const Gen& a) {
  return CpGen0{a.g0, a.g1, a.mg01, a.hx, a.hx2, a.hz2, a.G};
}
__device__ __forceinline__ CpCGen0 cp_cgen0(const CGen& c) { return CpCGen0{c.m00r, c.m00i, c.m01i, c.m11r, c.m11i}; }

template <int ST>
__device__ __forceinline__ void cp_m0_apply(const CpGen0& a, const double* b, double* o) {
  const double u1 = b[1 * ST], u2 = b[2 * ST], u3 = b[3 * ST], u4 = b[4 * ST];
  o[0] = fma(a.g0, u2, o[0]);
  o[1 * ST] = fma(a.g1, u2, fma(-a.hx2, u4, o[1 * ST]));
  o[2 * ST] = fma(a.mg01, u2, fma(a.hx2, u4, o[2 * ST]));
  o[3 * ST] = fma(-a.G, u3, fma(a.hz2, u4, o[3 * ST]));
  o[4 * ST] = fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o[4 * ST])));
}

// (o0, o1) += [[m00, i mo], [i mo, m11]] (z0, z1), complex
__device__ __forceinline__ void cp_cblock(const CpCGen0& m, double z0r, double z0i, double z1r, double z1i,
                                          double& o0r, double& o0i, double& o1r, double& o1i) {
  o0r = fma(m.m00r, z0r, fma(-m.m00i, z0i, fma(-m.mo, z1i, o0r)));
  o0i = fma(m.m00r, z0i, fma(m.m00i, z0r, fma(m.mo, z1r, o0i)));
  o1r = fma(m.m11r, z1r, fma(-m.m11i, z1i, fma(-m.mo, z0i, o1r)));
  o1i = fma(m.m11r, z1i, fma(m.m11i, z1r, fma(m.mo, z0r, o1i)));
}

// o += 2Y b on a coherence sector at phase 0 (apply_coh with the zeros above left out)
template <int KIND>
__device__ __forceinline__ void cp_apply0(const CpGen0& A0, const CpGen0& B0, const CpCGen0& Am, const CpCGen0& Bm,
                                          double vs, const double* b, double* o) {
  if (KIND == 0) {                 // C[5][2]: index 2*alpha + beta
#pragma unroll
    for (int be = 0; be < 2; ++be)
#pragma unroll
      for (int c = 0; c < 2; ++c) cp_m0_apply<4>(A0, b + 2 * be + c, o + 2 * be + c);
#pragma unroll
    for (int al = 0; al < 5; ++al)
      cp_cblock(Bm, b[4 * al], b[4 * al + 1], b[4 * al + 2], b[4 * al + 3], o[4 * al], o[4 * al + 1],
                o[4 * al + 2], o[4 * al + 3]);
#pragma unroll
    for (int al = 2; al < 5; ++al) {
      const double sa = (al == 2) ? 2.0 * vs : vs;
      o[4 * al + 2] = fma(-sa, b[4 * al + 3], o[4 * al + 2]);
      o[4 * al + 3] = fma(sa, b[4 * al + 2], o[4 * al + 3]);
    }
    o[4 * 4 + 2] = fma(vs, b[4 * 3 + 2], o[4 * 4 + 2]);
    o[4 * 4 + 3] = fma(vs, b[4 * 3 + 3], o[4 * 4 + 3]);
    o[4 * 3 + 2] = fma(-vs, b[4 * 4 + 2], o[4 * 3 + 2]);
    o[4 * 3 + 3] = fma(-vs, b[4 * 4 + 3], o[4 * 3 + 3]);
  } else if (KIND == 1) {          // C[2][5]: index 5*alpha + beta
#pragma unroll
    for (int al = 0; al < 2; ++al)
#pragma unroll
      for (int c = 0; c < 2; ++c) cp_m0_apply<2>(B0, b + 10 * al + c, o + 10 * al + c);
#pragma unroll
    for (int be = 0; be < 5; ++be)
      cp_cblock(Am, b[2 * be], b[2 * be + 1], b[10 + 2 * be], b[10 + 2 * be + 1], o[2 * be], o[2 * be + 1],
                o[10 + 2 * be], o[10 + 2 * be + 1]);
    o[10 + 2 * 4] = fma(vs, b[10 + 2 * 3], o[10 + 2 * 4]);
    o[10 + 2 * 4 + 1] = fma(vs, b[10 + 2 * 3 + 1], o[10 + 2 * 4 + 1]);
    o[10 + 2 * 3] = fma(-vs, b[10 + 2 * 4], o[10 + 2 * 3]);
    o[10 + 2 * 3 + 1] = fma(-vs, b[10 + 2 * 4 + 1], o[10 + 2 * 3 + 1]);
#pragma unroll
    for (int be = 2; be < 5; ++be) {
      const double sb = (be == 2) ? 2.0 * vs : vs;
      o[10 + 2 * be] = fma(-sb, b[10 + 2 * be + 1], o[10 + 2 * be]);
      o[10 + 2 * be + 1] = fma(sb, b[10 + 2 * be], o[10 + 2 * be + 1]);
    }
  } else {                         // C[2][2]: index 2*alpha + beta; A q=-1, B q=-1 (+1: Bm conjugated, vs = 0)
#pragma unroll
    for (int be = 0; be < 2; ++be)
      cp_cblock(Am, b[2 * be], b[2 * be + 1], b[4 + 2 * be], b[4 + 2 * be + 1], o[2 * be], o[2 * be + 1],
                o[4 + 2 * be], o[4 + 2 * be + 1]);
#pragma unroll
    for (int al = 0; al < 2; ++al)
      cp_cblock(Bm, b[4 * al], b[4 * al + 1], b[4 * al + 2], b[4 * al + 3], o[4 * al], o[4 * al + 1],
                o[4 * al + 2], o[4 * al + 3]);
    o[6] = fma(-2.0 * vs, b[7], o[6]);
    o[7] = fma(2.0 * vs, b[6], o[7]);
  }
}

// coordinates of the invariant block (the atom in q = 0 sits in |0><0|: nothing leaves it):
// (0,-1) k = 2 al + be -> al = 0; (-1,0) k = 5 al + be -> be = 0
template <int K>
__host__ __device__ constexpr bool cp_inv(int k) { return K == 0 ? k < 2 : (k % 5 == 0); }

// acc(k0), acc(k1) += U[k][m] * own for two rows k0, k1 of one column m: U[k][m] = lane m's
// v[k] by row_newbcast:m; own = (br, bi) = U[m][c] of this lane.  re += a_re br - a_im bi,
// im += a_re bi + a_im br (the -a_im through the DPP neg modifier on the broadcast source).
#define RYD_CMAC2_BODY(CTRL)                                                     \
  "v_fmac_f64_dpp %0, %4, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"            \
  "v_fmac_f64_dpp %2, %6, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"            \
  "v_fmac_f64_dpp %1, %4, %9 " CTRL " row_mask:0xf bank_mask:0xf\n\t"            \
  "v_fmac_f64_dpp %3, %6, %9 " CTRL " row_mask:0xf bank_mask:0xf\n\t"            \
  "v_fmac_f64_dpp %0, -%5, %9 " CTRL " row_mask:0xf bank_mask:0xf\n\t"           \
  "v_fmac_f64_dpp %2, -%7, %9 " CTRL " row_mask:0xf bank_mask:0xf\n\t"           \
  "v_fmac_f64_dpp %1, %5, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"            \
  "v_fmac_f64_dpp %3, %7, %8 " CTRL " row_mask:0xf bank_mask:0xf"

// NOP: the first group of a squaring (a source may have been written just before: the
// VALU-write -> DPP-read hazard needs 2 wait states)
template <int M, bool NOP>
__device__ __forceinline__ void cmac2_row(double& a0r, double& a0i, double& a1r, double& a1i, double v0r,
                                          double v0i, double v1r, double v1i, double br, double bi) {
  if constexpr (NOP)
    asm volatile("s_nop 1\n\t" RYD_CMAC2_BODY("row_newbcast:%10")
                 : "+v"(a0r), "+v"(a0i), "+v"(a1r), "+v"(a1i)
                 : "v"(v0r), "v"(v0i), "v"(v1r), "v"(v1i), "v"(br), "v"(bi), "i"(M));
  else
    asm volatile(RYD_CMAC2_BODY("row_newbcast:%10")
                 : "+v"(a0r), "+v"(a0i), "+v"(a1r), "+v"(a1i)
                 : "v"(v0r), "v"(v0i), "v"(v1r), "v"(v1i), "v"(br), "v"(bi), "i"(M));
}
// the quad pair: lanes 0-3 of a row hold the (-1,-1) sector, lanes 4-7 (-1,+1).  64-bit DPP
// on gfx950 has row_newbcast only (no quad_perm), so each sector's products broadcast from
// its own lanes (row_newbcast:4 BANK + m) and write only its bank (bank_mask 1 << BANK).
template <int M, int BANK, bool NOP>
__device__ __forceinline__ void cmac2_bank(double& a0r, double& a0i, double& a1r, double& a1i, double v0r,
                                           double v0i, double v1r, double v1i, double br, double bi) {
#define RYD_CMAC2_BODY_B                                                                   \
  "v_fmac_f64_dpp %0, %4, %8 row_newbcast:%10 row_mask:0xf bank_mask:%11\n\t"             \
  "v_fmac_f64_dpp %2, %6, %8 row_newbcast:%10 row_mask:0xf bank_mask:%11\n\t"             \
  "v_fmac_f64_dpp %1, %4, %9 row_newbcast:%10 row_mask:0xf bank_mask:%11\n\t"             \
  "v_fmac_f64_dpp %3, %6, %9 row_newbcast:%10 row_mask:0xf bank_mask:%11\n\t"             \
  "v_fmac_f64_dpp %0, -%5, %9 row_newbcast:%10 row_mask:0xf bank_mask:%11\n\t"            \
  "v_fmac_f64_dpp %2, -%7, %9 row_newbcast:%10 row_mask:0xf bank_mask:%11\n\t"            \
  "v_fmac_f64_dpp %1, %5, %8 row_newbcast:%10 row_mask:0xf bank_mask:%11\n\t"             \
  "v_fmac_f64_dpp %3, %7, %8 row_newbcast:%10 row_mask:0xf bank_mask:%11"
  if constexpr (NOP)
    asm volatile("s_nop 1\n\t" RYD_CMAC2_BODY_B
                 : "+v"(a0r), "+v"(a0i), "+v"(a1r), "+v"(a1i)
                 : "v"(v0r), "v"(v0i), "v"(v1r), "v"(v1i), "v"(br), "v"(bi), "i"(4 * BANK + M), "i"(1 << BANK));
  else
    asm volatile(RYD_CMAC2_BODY_B
                 : "+v"(a0r), "+v"(a0i), "+v"(a1r), "+v"(a1i)
                 : "v"(v0r), "v"(v0i), "v"(v1r), "v"(v1i), "v"(br), "v"(bi), "i"(4 * BANK + M), "i"(1 << BANK));
#undef RYD_CMAC2_BODY_B
}

// acc += column (lane) of v v for the (0,-1) / (-1,0) sector (10 complex coordinates).
// v is only read (DPP sources), after one s_nop for a write just before the call.
template <int K>
__device__ __forceinline__ void cp_square_row(const double (&v)[20], double (&acc)[20]) {
  static_for<10>([&](auto MM) {
    constexpr int m = decltype(MM)::value;
    const double br = v[2 * m], bi = v[2 * m + 1];
    if constexpr (cp_inv<K>(m)) {            // feeds the invariant rows only
      constexpr int k0 = K == 0 ? 0 : 0, k1 = K == 0 ? 1 : 5;
      cmac2_row<m, m == 0>(acc[2 * k0], acc[2 * k0 + 1], acc[2 * k1], acc[2 * k1 + 1], v[2 * k0], v[2 * k0 + 1],
                           v[2 * k1], v[2 * k1 + 1], br, bi);
    } else {
      static_for<5>([&](auto KK) {
        constexpr int k0 = 2 * decltype(KK)::value, k1 = k0 + 1;
        cmac2_row<m, m == 0 && k0 == 0>(acc[2 * k0], acc[2 * k0 + 1], acc[2 * k1], acc[2 * k1 + 1], v[2 * k0],
                                        v[2 * k0 + 1], v[2 * k1], v[2 * k1 + 1], br, bi);
      });
    }
  });
}

// the (-1,-1) / (-1,+1) quads: acc(bank BANK) += column of v v (4 complex coordinates,
// dense); lanes of the other banks are not written
template <int BANK>
__device__ __forceinline__ void cp_square_bank(const double (&v)[8], double (&acc)[8]) {
  static_for<4>([&](auto MM) {
    constexpr int m = decltype(MM)::value;
    const double br = v[2 * m], bi = v[2 * m + 1];
    cmac2_bank<m, BANK, m == 0>(acc[0], acc[1], acc[2], acc[3], v[0], v[1], v[2], v[3], br, bi);
    cmac2_bank<m, BANK, false>(acc[4], acc[5], acc[6], acc[7], v[4], v[5], v[6], v[7], br, bi);
  });
}

// frame action on sector coordinate k: phase power p (coordinate x e^{-i p th}) and the
// (ex, ey) rotation role of a q = 0 factor: 0 none, 1 ex (partner k + d), 2 ey (partner k - d).
// K = 2 / 3 is chosen per lane in the quad layout (k3).
template <int K>
__device__ __forceinline__ void cp_frame_role(int k, bool k3, int& p, int& role, int& d) {
  if (K == 0) {                                  // k = 2 al + be: A q = 0, B q = -1
    const int al = k >> 1, be = k & 1;
    p = be;
    role = al == 3 ? 1 : (al == 4 ? 2 : 0);
    d = 2;
  } else if (K == 1) {                           // k = 5 al + be: A q = -1, B q = 0
    const int al = k / 5, be = k % 5;
    p = al;
    role = be == 3 ? 1 : (be == 4 ? 2 : 0);
    d = 1;
  } else {                                       // k = 2 al + be: A q = -1, B q = -1 (K2) / +1 (K3)
    const int al = k >> 1, be = k & 1;
    p = k3 ? al - be : al + be;
    role = 0;
    d = 0;
  }
}

// coordinate k of R_th u, from the stage u (complex, n entries); (c1, s1) = (cos th, sin th),
// (c2, s2) = (cos 2 th, sin 2 th)
template <int K>
__device__ __forceinline__ double2 cp_frame_at(const double2* u, int k, bool k3, double c1, double s1, double c2,
                                               double s2) {
  int p, role, d;
  cp_frame_role<K>(k, k3, p, role, d);
  double2 z = u[k];
  if (role == 1) {                               // x' = c x + s y
    const double2 y = u[k + d];
    z = make_double2(fma(c1, z.x, s1 * y.x), fma(c1, z.y, s1 * y.y));
  } else if (role == 2) {                        // y' = -s x + c y
    const double2 x = u[k - d];
    z = make_double2(fma(c1, z.x, -s1 * x.x), fma(c1, z.y, -s1 * x.y));
  }
  // x e^{-i p th}
  double pc = 1.0, ps = 0.0;
  if (p == 1) { pc = c1; ps = -s1; }
  else if (p == -1) { pc = c1; ps = s1; }
  else if (p == 2) { pc = c2; ps = -s2; }
  return make_double2(fma(pc, z.x, -ps * z.y), fma(pc, z.y, ps * z.x));
}

// One sector group of one row: build U(phase 0) when (|Omega|, Delta, dt) changes, apply it
// to the inputs through every segment in the laser-phase frame, write the qubit images.
// K = 0 / 1: the row sectors; K = 2: the quad pair ((-1,-1) on quad 0, (-1,+1) on quad 1).
template <int PROTO, int K>
__device__ __forceinline__ void cp_sector(const double* prm, int64_t ldp, bool valid, int n_steps, int shape, int l,
                                          double2* Ul, double2* stg, lds_zero_t* zl, double* __restrict__ out,
                                          int64_t ldo, int64_t i, bool live, bool mirror, uint32_t& stat) {
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
  // inputs: K0 C[0][0], C[1][0] (coordinates 0, 2); K1 C[0][0], C[0][1] (0, 1); K2/K3 C[0][0]
  double2 u[NIN];
#pragma unroll
  for (int s = 0; s < NIN; ++s) {
    const int k0 = s == 0 ? 0 : (K == 0 ? 2 : 1);
    u[s] = make_double2(col && e == k0 ? 1.0 : 0.0, 0.0);
  }
  double kw = -1.0, kdl = 0.0, kdt = -1.0;       // the propagator's key
  double fc = 1.0, fs = 0.0;                     // the frame e^{i phi} the inputs are carried in
  const int nseg = n_segments<PROTO>(n_steps);
  for (int sgi = 0; sgi < nseg; ++sgi) {
    // the point's parameters reloaded per segment (L2 hits) rather than held across the
    // build, where they spilled; only the frame and the build key stay live across it
    const double* pq = prm;
    asm volatile("" : "+s"(pq));
    const PointP q = load_point<PROTO>(pq, ldp, i);
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
      double rsum = 0.0;
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
        // both quads run cp_apply0<2>: quad 1's (-1,+1) generator is the conjugated B block and
        // no V term (V drops out of that sector)
        const CpCGen0 Am = cp_cgen0(make_cgen(g0, q.d1, q.gA, sc, false));
        const CpCGen0 Bm = cp_cgen0(make_cgen(g0, q.d1, q.gB, sc, k3));
        const double vs = k3 ? 0.0 : sc * 0.5 * q.V;
        const CpGen0 Z = {};
        cp_cheb<NV, true>(v, xs, cact,
                          [&](const double (&b)[NV], double (&o)[NV]) { cp_apply0<2>(Z, Z, Am, Bm, vs, b, o); });
      } else {
        // K0 reads A0 and Bm, K1 B0 and Am
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
      // ping-pong v -> w -> v (no copies); the accumulators are cleared by LDS reads of zero
      // words (the LDS pipe, not the VALU, as square_cols16)
      auto square = [&](const double (&a)[NV], double (&o)[NV], int lvl) {
        asm volatile("" ::: "memory");         // re-read the zero words every level
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          o[j] = zl[j];
          asm volatile("" ::: "memory");
        }
        if constexpr (QUAD) {
          if (lvl < smax0) cp_square_bank<0>(a, o);
          if (lvl < smax1) cp_square_bank<1>(a, o);
        } else {
          cp_square_row<K>(a, o);
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
            for (int j = 0; j < NV; ++j) v[j] = w[j];
          }
        }
      }
      cp_wsync();
      if (rebuild && col) {
#pragma unroll
        for (int k = 0; k < n; ++k) U[e * n + k] = make_double2(v[2 * k], v[2 * k + 1]);
      }
      cp_wsync();
    }
    if (!act) continue;
    // ---- the segment: u <- U R_{-(phi - phi_prev)} u (inputs carried in the current frame) ----
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
        const double2 a = U[c * n + e];          // U[e][c]
#pragma unroll
        for (int s = 0; s < NIN; ++s) {
          const double2 z = cp_frame_at<K>(sg + s * CP_NMAX, c, k3, c1, s1, c2, s2);
          acc[s].x = fma(a.x, z.x, fma(-a.y, z.y, acc[s].x));
          acc[s].y = fma(a.x, z.y, fma(a.y, z.x, acc[s].y));
        }
      }
#pragma unroll
      for (int s = 0; s < NIN; ++s) u[s] = acc[s];
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
  } else if (col && e == 0) {
    const int base = k3 ? RYD_C_K3 : RYD_C_K2;
    out[(int64_t)(base + 0) * ldo + i] = z[0].x;
    out[(int64_t)(base + 1) * ldo + i] = z[0].y;
  }
}

template <int PROTO>
__global__ __launch_bounds__(CP_BLOCK) __attribute__((amdgpu_waves_per_eu(RYD_CP_OCC, 8))) void coherence_prop_kernel(const double* __restrict__ prm, int64_t n,
                                                               int64_t ldp, double* __restrict__ out, int64_t ldo,
                                                               uint32_t* __restrict__ status, int n_steps,
                                                               int shape) {
  __shared__ double2 s_U[CP_NR][CP_NMAX * CP_NMAX];
  __shared__ double2 s_stg[CP_NR][2 * CP_NMAX];
  __shared__ double s_zero[2 * CP_NMAX];        // zero words: squaring accumulator clears
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  if (threadIdx.x < 2 * CP_NMAX) s_zero[threadIdx.x] = 0.0;   // one wave: ordered before the first read
  lds_zero_t* zl = (lds_zero_t*)s_zero;
  // XCD-aware block order (xcd_block, ryd_sym16.inc): the 4 blocks whose 32-byte parameter and
  // output pieces share a 128-byte line run on one XCD (one L2 fill per line)
  const int64_t gi = xcd_block(blockIdx.x, gridDim.x) * CP_NR + row;
  const bool live = gi < n;
  const int64_t i = live ? gi : n - 1;
  bool valid, sym = true;
  {
    const PointP q = load_point<PROTO>(prm, ldp, i);
    valid = live && point_valid<PROTO>(q, n_steps);
#pragma unroll
    for (int c = 0; c < 4; ++c) sym = sym && q.gA[c] == q.gB[c];
  }
  uint32_t stat = 0u;
  double2* Ul = s_U[row];
  double2* stg = s_stg[row];
  // (-1,0) is the atom-swap mirror of (0,-1) when the atoms are identical (the images are
  // the same numbers); otherwise it is built
  cp_sector<PROTO, 0>(prm, ldp, valid, n_steps, shape, l, Ul, stg, zl, out, ldo, i, live, sym, stat);
  cp_sector<PROTO, 2>(prm, ldp, valid, n_steps, shape, l, Ul, stg, zl, out, ldo, i, live, false, stat);
  if (__ballot(!sym && live)) cp_sector<PROTO, 1>(prm, ldp, valid, n_steps, shape, l, Ul, stg, zl, out, ldo, i, live && !sym, false, stat);
  // the row's flags (every lane of the wave reaches this)
  uint32_t st = stat;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) st |= (uint32_t)__shfl_xor((int)st, o, 16);
  if (live && !valid) st |= RYD_STATUS_BAD_INPUT;
  if (live && l == 0) status[i] = st;
}
