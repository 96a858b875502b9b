// ryd_traj_sym.inc -- the C5 quantum-jump kernel in the exchange-symmetry-adapted basis
// (included by ryd_engine.hip after ryd_traj.inc, whose Philox stream, jump operators,
// reduction pairs and TrajArgs it shares).  Same model, unravelling, random streams,
// ladder depth and outputs as traj3_kernel (DESIGN.md section 9); what changes is the
// representation of H_eff's blocks.
//
// The three atoms are identical, so every block of H_eff (the atoms in {1, r}) commutes
// with permutations of its atoms and splits by symmetry type.  With w = |Omega|/2 and
// E_k(n) = n (-Delta - i hgr) + (k - n)(delta1 - i hgs) + V n(n - 1)/2 (n atoms in |r>):
//   1 atom  : 2 x 2           {|1>, |r>}                      [[E1(0), w], [w, E1(1)]]
//   2 atoms : 3 x 3 symmetric {|11>, (|1r> + |r1>)/sqrt2, |rr>}  tridiagonal, off sqrt2 w
//             1 x 1 antisym   (|1r> - |r1>)/sqrt2               E2(1)
//   3 atoms : 4 x 4 symmetric {|111>, W1, W2, |rrr>}            tridiagonal, off sqrt3 w, 2w, sqrt3 w
//             2 x 2 standard  (n_r = 1 and 2 components) twice  [[E3(1), w], [w, E3(2)]]
// (W1, W2: the symmetric superpositions with one / two atoms in |r>; the standard pairs
// A = ((|11r> - |1r1>)/sqrt2, (|r1r> - |rr1>)/sqrt2) and B = ((|11r> + |1r1> - 2|r11>)/sqrt6,
// (2|1rr> - |r1r> - |rr1>)/sqrt6) are mapped onto each other by the raising part of H
// with coefficient 1.)  Every block is complex symmetric (H_eff^T = H_eff in the phase-0
// frame), so one ladder level is 23 complex numbers (packed upper triangles) instead of
// 84, and a walk step costs 66 complex MACs instead of 124.  Each adapted component
// has a definite number of atoms in |r>, so the laser-phase frame stays diagonal.  The
// ket lives in the adapted basis; jumps (monomials in the atom basis) and the outputs
// go through the fixed orthogonal change of basis.  With ~12 KB of LDS per point and
// <= 256 registers, two waves share each SIMD.

constexpr int TS_NU = 23;                      // packed complex entries per ladder level
constexpr int TS_LD = 24;                      // ladder/scratch stride: entry 23 is a zero word
constexpr int TS_NBLK = 5;                     // block types: 1-atom, 2-sym, 2-anti, 3-sym, 3-std
#ifndef RYD_T_SYM_WAVES
#define RYD_T_SYM_WAVES 2                      // 2 waves/SIMD (~530 B/lane of spill) beats 1 (0.69 vs 0.88 ms)
#endif
#ifndef RYD_T_JB
#define RYD_T_JB 8                             // parked jumps that trigger a wave's jump pass
#endif

__host__ __device__ constexpr int ts_dim(int B) { return B == 0 ? 2 : B == 1 ? 3 : B == 2 ? 1 : B == 3 ? 4 : 2; }
__host__ __device__ constexpr int ts_off(int B) { return B == 0 ? 0 : B == 1 ? 3 : B == 2 ? 9 : B == 3 ? 10 : 20; }
// packed index of (r, c) in a symmetric block (either order)
__host__ __device__ constexpr int ts_pk(int B, int r, int c) {
  return r <= c ? ts_off(B) + r * ts_dim(B) - r * (r - 1) / 2 + (c - r)
                : ts_off(B) + c * ts_dim(B) - c * (c - 1) / 2 + (r - c);
}
// entry e -> (block, r, c), r <= c
__device__ __forceinline__ void ts_entry(int e, int& B, int& r, int& c) {
  B = e < 3 ? 0 : e < 9 ? 1 : e < 10 ? 2 : e < 20 ? 3 : 4;
  const int D = ts_dim(B);
  int k = e - ts_off(B);
  r = 0;
  while (k >= D - r) {
    k -= D - r;
    ++r;
  }
  c = r + k;
}

// atoms in |r> of adapted component j (0..26): the frame phase e^{i ang n_r}
__host__ __device__ constexpr int ts_nr(int j) {
  return j == 0 ? 0
       : j < 7 ? ((j - 1) & 1)                                            // 1-atom (|1>, |r>) x 3
       : j < 19 ? ((j - 7) % 4 == 3 ? 1 : (j - 7) % 4)                    // (s0, s1, s2, anti) x 3
       : j < 23 ? j - 19                                                  // W0..W3
       : ((j - 23) & 1) + 1;                                              // A1 A2 B1 B2
}

// basis index 9 a0 + 3 a1 + a2 from the three digits (0: '0', 1: '1', 2: 'r')
__host__ __device__ constexpr int ts_idx(int a0, int a1, int a2) { return 9 * a0 + 3 * a1 + a2; }
// digit of atom `at` when atom `on` of a pair/single is the one set to level `lv`
__host__ __device__ constexpr int ts_pair_idx(int q, int d1, int d2) {   // pair without atom q, first atom d1
  return q == 0 ? ts_idx(0, d1, d2) : q == 1 ? ts_idx(d1, 0, d2) : ts_idx(d1, d2, 0);
}

// atom basis (re, im interleaved) -> adapted basis
__device__ __forceinline__ void ts_to_adapted(const double (&x)[T_NV], double (&a)[T_NV]) {
  constexpr double R2 = 0.70710678118654752440, R3 = 0.57735026918962576451, R6 = 0.40824829046386301637;
#pragma unroll
  for (int p = 0; p < 2; ++p) {                 // re, im
    a[p] = x[2 * ts_idx(0, 0, 0) + p];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i1 = j == 0 ? ts_idx(1, 0, 0) : j == 1 ? ts_idx(0, 1, 0) : ts_idx(0, 0, 1);
      const int ir = j == 0 ? ts_idx(2, 0, 0) : j == 1 ? ts_idx(0, 2, 0) : ts_idx(0, 0, 2);
      a[2 * (1 + 2 * j) + p] = x[2 * i1 + p];
      a[2 * (2 + 2 * j) + p] = x[2 * ir + p];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double v11 = x[2 * ts_pair_idx(q, 1, 1) + p], v1r = x[2 * ts_pair_idx(q, 1, 2) + p],
                   vr1 = x[2 * ts_pair_idx(q, 2, 1) + p], vrr = x[2 * ts_pair_idx(q, 2, 2) + p];
      a[2 * (7 + 4 * q) + p] = v11;
      a[2 * (8 + 4 * q) + p] = R2 * (v1r + vr1);
      a[2 * (9 + 4 * q) + p] = vrr;
      a[2 * (10 + 4 * q) + p] = R2 * (v1r - vr1);
    }
    const double R0 = x[2 * ts_idx(2, 1, 1) + p], Rr1 = x[2 * ts_idx(1, 2, 1) + p], Rr2 = x[2 * ts_idx(1, 1, 2) + p];
    const double Q0 = x[2 * ts_idx(1, 2, 2) + p], Q1 = x[2 * ts_idx(2, 1, 2) + p], Q2 = x[2 * ts_idx(2, 2, 1) + p];
    a[2 * 19 + p] = x[2 * ts_idx(1, 1, 1) + p];
    a[2 * 20 + p] = R3 * (R0 + Rr1 + Rr2);
    a[2 * 21 + p] = R3 * (Q0 + Q1 + Q2);
    a[2 * 22 + p] = x[2 * ts_idx(2, 2, 2) + p];
    a[2 * 23 + p] = R2 * (Rr2 - Rr1);                        // A1
    a[2 * 24 + p] = R2 * (Q1 - Q2);                          // A2
    a[2 * 25 + p] = R6 * (Rr2 + Rr1 - 2.0 * R0);             // B1
    a[2 * 26 + p] = R6 * (2.0 * Q0 - Q1 - Q2);               // B2
  }
}

// adapted basis -> atom basis (the transpose of ts_to_adapted)
__device__ __forceinline__ void ts_to_atom(const double (&a)[T_NV], double (&x)[T_NV]) {
  constexpr double R2 = 0.70710678118654752440, R3 = 0.57735026918962576451, R6 = 0.40824829046386301637;
#pragma unroll
  for (int e = 0; e < T_NV; ++e) x[e] = 0.0;              // atom-0-in-|0> states not set below stay 0
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    x[2 * ts_idx(0, 0, 0) + p] = a[p];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i1 = j == 0 ? ts_idx(1, 0, 0) : j == 1 ? ts_idx(0, 1, 0) : ts_idx(0, 0, 1);
      const int ir = j == 0 ? ts_idx(2, 0, 0) : j == 1 ? ts_idx(0, 2, 0) : ts_idx(0, 0, 2);
      x[2 * i1 + p] = a[2 * (1 + 2 * j) + p];
      x[2 * ir + p] = a[2 * (2 + 2 * j) + p];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double s1 = a[2 * (8 + 4 * q) + p], an = a[2 * (10 + 4 * q) + p];
      x[2 * ts_pair_idx(q, 1, 1) + p] = a[2 * (7 + 4 * q) + p];
      x[2 * ts_pair_idx(q, 1, 2) + p] = R2 * (s1 + an);
      x[2 * ts_pair_idx(q, 2, 1) + p] = R2 * (s1 - an);
      x[2 * ts_pair_idx(q, 2, 2) + p] = a[2 * (9 + 4 * q) + p];
    }
    const double W1 = a[2 * 20 + p], W2 = a[2 * 21 + p];
    const double A1 = a[2 * 23 + p], A2 = a[2 * 24 + p], B1 = a[2 * 25 + p], B2 = a[2 * 26 + p];
    x[2 * ts_idx(1, 1, 1) + p] = a[2 * 19 + p];
    x[2 * ts_idx(2, 2, 2) + p] = a[2 * 22 + p];
    x[2 * ts_idx(2, 1, 1) + p] = fma(R3, W1, -2.0 * R6 * B1);                 // R0 (atom 0 in |r>)
    x[2 * ts_idx(1, 2, 1) + p] = fma(R3, W1, fma(-R2, A1, R6 * B1));          // R1
    x[2 * ts_idx(1, 1, 2) + p] = fma(R3, W1, fma(R2, A1, R6 * B1));           // R2
    x[2 * ts_idx(1, 2, 2) + p] = fma(R3, W2, 2.0 * R6 * B2);                  // Q0 (atom 0 in |1>)
    x[2 * ts_idx(2, 1, 2) + p] = fma(R3, W2, fma(R2, A2, -R6 * B2));          // Q1
    x[2 * ts_idx(2, 2, 1) + p] = fma(R3, W2, fma(-R2, A2, -R6 * B2));         // Q2
  }
}

// H_eff entry (block B, r <= c) as (re, im), frame phase 0
__host__ __device__ __forceinline__ double2 ts_heff(int B, int r, int c, double w, double dl, double d1, double V,
                                                    const TRates& R) {
  const int k = B == 0 ? 1 : (B < 3 ? 2 : 3);
  double re = 0.0, im = 0.0;
  if (r == c) {
    // atoms in |r> of diagonal state r: 1-atom and symmetric blocks: r; antisym: 1; standard: r + 1
    const int n = B == 2 ? 1 : (B == 4 ? r + 1 : r);
    re = -dl * n + d1 * (k - n) + V * (double)(n * (n - 1) / 2);
    im = -(R.hgr * n + R.hgs * (k - n));
  } else if (c == r + 1) {                       // tridiagonal couplings
    const double s2 = 1.41421356237309504880, s3 = 1.73205080756887729353;
    re = B == 0 || B == 4 ? w : (B == 1 ? s2 * w : (r == 1 ? 2.0 * w : s3 * w));
  }
  return make_double2(re, im);
}
// A = -i H_eff h, packed entry (block B, r <= c), frame phase 0
__device__ __forceinline__ double2 ts_gen(int B, int r, int c, double w, double dl, double d1, double V,
                                          const TRates& R, double h) {
  const double2 z = ts_heff(B, r, c, w, dl, d1, V, R);
  return make_double2(z.y * h, -z.x * h);
}

// the packed operands of (M N)[r][c] for the lane owning entry e: M[ia[j]] N[ib[j]],
// j < 4; terms beyond the block's dimension (and every term of lanes e >= 23) read the
// zero word at index 23, so the product is four branch-free complex MACs
__device__ __forceinline__ void ts_mm_index(int e, int (&ia)[4], int (&ib)[4]) {
  int B = 0, r = 0, c = 0;
  if (e < TS_NU) ts_entry(e, B, r, c);
  const int D = ts_dim(B);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool t = e < TS_NU && j < D;
    ia[j] = t ? ts_pk(B, r, j) : TS_NU;
    ib[j] = t ? ts_pk(B, j, c) : TS_NU;
  }
}
__device__ __forceinline__ double2 ts_mm(const double2* M, const double2* Nm, const int (&ia)[4],
                                         const int (&ib)[4]) {
  double re = 0.0, im = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double2 a = M[ia[j]], b = Nm[ib[j]];
    re = fma(a.x, b.x, fma(-a.y, b.y, re));
    im = fma(a.x, b.y, fma(a.y, b.x, im));
  }
  return make_double2(re, im);
}

// lad[l] = exp(-i H_eff dt / 2^l) - I, l = 0..L, packed (the same levels and bottom-level
// Taylor order as t_build_ladder); S0..S2: 3 x 23 scratch; every thread of the block calls
__device__ __forceinline__ int ts_build_ladder(double2* lad, double2* S0, double2* S1, double2* S2, int L, double w,
                                               double dl, double d1, double V, const TRates& R, double dt,
                                               double* tpp = nullptr) {
  const double tb0 = T_CLK();
  const int tid = threadIdx.x;
  const bool own = tid < TS_LD;                  // lane 23 keeps every array's zero word
  int ia[4], ib[4];
  ts_mm_index(tid, ia, ib);
  int B = 0, r = 0, c = 0;
  if (tid < TS_NU) ts_entry(tid, B, r, c);
  const double bnd = 3.0 * (fabs(dl) + fabs(d1) + R.hgr + R.hgs + fabs(V) + w);
  const double x = ldexp(bnd * dt, -L);
  int s0 = 0;
  if (x > 0x1.0p-10) s0 = (int)ceil(log2(x)) + 10;
  const double h = ldexp(dt, -(L + s0));
  double2* Xb = lad + (size_t)L * TS_LD;
  if (own) {
    const double2 a = tid < TS_NU ? ts_gen(B, r, c, w, dl, d1, V, R, h) : make_double2(0.0, 0.0);
    S0[tid] = a;
    S1[tid] = a;
    S2[tid] = make_double2(0.0, 0.0);
    Xb[tid] = a;
  }
  __syncthreads();
  double2* Tc = S1;
  double2* Tn = S2;
  double2 xb = own ? Xb[tid] : make_double2(0.0, 0.0);
  for (int nn = 2; nn <= T_TAYLOR; ++nn) {
    const double inv = 1.0 / (double)nn;
    double2 t = ts_mm(Tc, S0, ia, ib);
    t.x *= inv;
    t.y *= inv;
    xb.x += t.x;
    xb.y += t.y;
    if (own) Tn[tid] = t;
    __syncthreads();
    double2* tmp = Tc;
    Tc = Tn;
    Tn = tmp;
  }
  if (own) Xb[tid] = xb;
  __syncthreads();
  const double tb1 = T_CLK();
  for (int qq = 0; qq < s0; ++qq) {
    const double2 p = ts_mm(Xb, Xb, ia, ib);
    xb = make_double2(2.0 * xb.x + p.x, 2.0 * xb.y + p.y);
    __syncthreads();
    if (own) Xb[tid] = xb;
    __syncthreads();
  }
  const double tb2 = T_CLK();
  for (int l = L - 1; l >= 0; --l) {
    const double2* Xs = lad + (size_t)(l + 1) * TS_LD;
    double2* Xd = lad + (size_t)l * TS_LD;
    const double2 p = ts_mm(Xs, Xs, ia, ib);
    xb = make_double2(2.0 * xb.x + p.x, 2.0 * xb.y + p.y);
    if (own) Xd[tid] = xb;
    __syncthreads();
  }
  if (tpp) {
    tpp[0] += tb1 - tb0;
    tpp[1] += tb2 - tb1;
    tpp[2] += T_CLK() - tb2;
    tpp[3] += (double)s0;
  }
  return s0 + L;
}

// one-atom blocks at adapted components 1, 3, 5; per pair (s0, s1, s2) at 7 + 4q, anti at 10 + 4q;
// the 3-atom symmetric block at 19, the standard pairs at 23 and 25 (instances 9, 10, 11)
__host__ __device__ constexpr int ts_inst_block(int ii) {
  return ii < 3 ? 0 : ii < 9 ? ((ii - 3) % 2 == 0 ? 1 : 2) : (ii == 9 ? 3 : 4);
}
__host__ __device__ constexpr int ts_inst_start(int ii) {
  return ii < 3 ? 1 + 2 * ii : ii < 9 ? 7 + 4 * ((ii - 3) / 2) + ((ii - 3) % 2 == 0 ? 0 : 3) : 19 + 4 * (ii - 9) - (ii == 11 ? 2 : 0);
}
constexpr int TS_NINST = 12;

// y = (I + X) a block by block (a block's outputs depend only on its own inputs);
// returns ||y||^2 -- the trial of a walk step; a taken step keeps y
__device__ __forceinline__ double ts_trial(const double2* __restrict__ X, const double (&a)[T_NV], double (&y)[T_NV]) {
  y[0] = a[0];
  y[1] = a[1];
  double s = fma(a[0], a[0], a[1] * a[1]);
  static_for<TS_NINST>([&](auto II) {
    constexpr int ii = decltype(II)::value;
    constexpr int B = ts_inst_block(ii), s0 = ts_inst_start(ii), D = ts_dim(B);
    static_for<D>([&](auto RR) {
      constexpr int r = decltype(RR)::value;
      double vr = a[2 * (s0 + r)], vi = a[2 * (s0 + r) + 1];
      static_for<D>([&](auto CC) {
        constexpr int c = decltype(CC)::value;
        const double2 m = X[ts_pk(B, r, c)];
        const double xr = a[2 * (s0 + c)], xi = a[2 * (s0 + c) + 1];
        vr = fma(m.x, xr, fma(-m.y, xi, vr));
        vi = fma(m.x, xi, fma(m.y, xr, vi));
      });
      y[2 * (s0 + r)] = vr;
      y[2 * (s0 + r) + 1] = vi;
      s = fma(vr, vr, fma(vi, vi, s));
    });
  });
  return s;
}

// a_j *= e^{i ang n_r(j)}
__device__ __forceinline__ void ts_rotate(double (&a)[T_NV], double ang) {
  double s1, c1;
  sincos(ang, &s1, &c1);
  const double c2 = c1 * c1 - s1 * s1, s2 = 2.0 * s1 * c1;
  const double c3 = c2 * c1 - s2 * s1, s3 = s2 * c1 + c2 * s1;
  const double cs[4] = {1.0, c1, c2, c3}, sn[4] = {0.0, s1, s2, s3};
#pragma unroll
  for (int j = 0; j < T_NB; ++j) {
    const int n = ts_nr(j);
    if (n == 0) continue;
    const double re = a[2 * j], im = a[2 * j + 1];
    a[2 * j] = re * cs[n] - im * sn[n];
    a[2 * j + 1] = re * sn[n] + im * cs[n];
  }
}

// LDS per point: the packed ladder + 3 x 23 scratch + the 8-ket reduction tile
__host__ __device__ constexpr size_t ts_lds_bytes(int L) {
  return sizeof(double2) * ((size_t)(L + 1) * TS_LD + 3 * TS_LD + T_TILE * T_NB);
}

// one round's finished kets z (atom basis, normalised; lanes with act) into the shifted sums
// accg[3 e + (0, 1, 2)] = sum (X - X_phi), its im part, sum |X - X_phi|^2 (X = z_a conj(z_b)),
// through 8-ket LDS tiles, in lane order; the kets are those of lanes l0 .. l0 + nk - 1
__device__ __forceinline__ void ts_reduce_round(double2* stg, double* accg, const double* s_phi,
                                                const double (&z)[T_NV], bool act, int lane, int l0, int nk) {
  for (int tb = l0; tb < l0 + nk; tb += T_TILE) {
    __syncthreads();
    if (act && lane >= tb && lane < tb + T_TILE)
#pragma unroll
      for (int idx = 0; idx < T_NB; ++idx)
        stg[(lane - tb) * T_NB + idx] = make_double2(z[2 * idx], z[2 * idx + 1]);
    __syncthreads();
    const int tn = min(T_TILE, l0 + nk - tb);
#pragma unroll
    for (int k = 0; k < T_EPL; ++k) {
      const int e = lane + k * T_WAVE;
      if (e < T_NPAIR) {
        int pa, pb;
        t_pair(e, pa, pb);
        const double ar = s_phi[2 * pa], ai = s_phi[2 * pa + 1], br = s_phi[2 * pb], bi = s_phi[2 * pb + 1];
        const double rr = fma(ar, br, ai * bi), ri = fma(ai, br, -ar * bi);   // the shift X_phi
        double a0 = accg[3 * e], a1 = accg[3 * e + 1], a2 = accg[3 * e + 2];
        for (int t = 0; t < tn; ++t) {
          const double2 u1 = stg[t * T_NB + pa], u2 = stg[t * T_NB + pb];
          const double xr = fma(u1.x, u2.x, u1.y * u2.y) - rr;
          const double xi = fma(u1.y, u2.x, -u1.x * u2.y) - ri;
          a0 += xr;
          a1 += xi;
          a2 = fma(xr, xr, fma(xi, xi, a2));
        }
        accg[3 * e] = a0;
        accg[3 * e + 1] = a1;
        accg[3 * e + 2] = a2;
      }
    }
  }
}

// mean rho (both triangles), its standard errors, and this lane's share of the trace and of
// the qubit population, from the shifted sums (which live in orho itself: read first)
__device__ __forceinline__ void ts_write_moments(double* orho, double* ose, const double* accg, const double* s_phi,
                                                 int lane, double ntr, double& trl, double& qpl) {
  double omr[T_EPL], omi[T_EPL], osev[T_EPL];
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {            // read every sum before any output overwrites them
    omr[k] = omi[k] = osev[k] = 0.0;
    const int e = lane + k * T_WAVE;
    if (e < T_NPAIR) {
      int pa, pb;
      t_pair(e, pa, pb);
      const double ar = s_phi[2 * pa], ai = s_phi[2 * pa + 1], br = s_phi[2 * pb], bi = s_phi[2 * pb + 1];
      const double dr = accg[3 * e] / ntr, di = accg[3 * e + 1] / ntr;
      omr[k] = fma(ar, br, ai * bi) + dr;
      omi[k] = fma(ai, br, -ar * bi) + di;
      const double var = accg[3 * e + 2] / ntr - (dr * dr + di * di);
      osev[k] = ntr > 1.0 ? sqrt(fmax(var, 0.0) / (ntr - 1.0)) : 0.0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {
    const int e = lane + k * T_WAVE;
    if (e < T_NPAIR) {
      int pa, pb;
      t_pair(e, pa, pb);
      const double mr = omr[k], mi = omi[k], sev = osev[k];
      orho[2 * (pa + T_NB * pb)] = mr;
      orho[2 * (pa + T_NB * pb) + 1] = mi;
      orho[2 * (pb + T_NB * pa)] = mr;
      orho[2 * (pb + T_NB * pa) + 1] = -mi;
      ose[pa + T_NB * pb] = sev;
      ose[pb + T_NB * pa] = sev;
      if (pa == pb) {
        trl += mr;
        if (t_qubit(pa)) qpl += mr;
      }
    }
  }
}

// The traj3_kernel algorithm (one wave per point: no-jump branch once, classify, walk
// the jumpers 64 per round, shifted 8-ket tile reduction) on adapted-basis kets.
template <int PROTO>
__global__ __launch_bounds__(T_WAVE) __attribute__((amdgpu_waves_per_eu(RYD_T_SYM_WAVES, 8))) void
traj3s_kernel(TrajArgs a) {
  double tp_start = T_CLK(), tp_pass1 = 0.0, tp_cls = 0.0, tp_walk = 0.0, tp_red = 0.0, tp_mark = 0.0;
#ifdef RYD_T_PROF
  double tpb_[4] = {0.0, 0.0, 0.0, 0.0};
  double* tpb = tpb_;
#else
  double* tpb = nullptr;
#endif
  (void)tp_start; (void)tp_pass1; (void)tp_cls; (void)tp_walk; (void)tp_red; (void)tp_mark;
  extern __shared__ double2 t_lds[];
  __shared__ uint32_t s_list[T_CHUNK];
  __shared__ double s_psi0[T_NV];                    // adapted basis
  __shared__ double s_phi[T_NV];                     // atom basis (the reduction's shift)
  const int L = a.L;
  double2* lad = t_lds;                              // [(L + 1)][23]
  double2* S0 = lad + (size_t)(L + 1) * TS_LD;
  double2* S1 = S0 + TS_LD;
  double2* S2 = S1 + TS_LD;
  double2* stg = S2 + TS_LD;                         // [8][27] atom-basis ket tile
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  if (i >= a.n) return;
  // the fallback pass after traj3e_kernel: only the points it declined
  if (a.fix && !(a.status[i] & RYD_STATUS_EXACT_FALLBACK)) return;
  const uint32_t st0 = a.fix ? RYD_STATUS_EXACT_FALLBACK : 0u;
  const uint64_t gpoint = (uint64_t)(a.point_offset + a.point_stride * i);
  const PointP q0 = load_point<PROTO>(a.prm, a.ld, i);
  const bool valid = point_valid<PROTO>(q0, a.n_steps);
  double* orho = a.rho + (size_t)i * a.ld_rho;
  double* ose = a.se + (size_t)i * a.ld_se;
  double* sm = a.summ;
  const int64_t ldm = a.ld_summ;
  if (!valid) {
    for (int e = lane; e < RYD_T_RHO_WIDTH; e += T_WAVE) orho[e] = 0.0;
    for (int e = lane; e < RYD_T_SE_WIDTH; e += T_WAVE) ose[e] = 0.0;
    if (lane < RYD_T_NSUMMARY) sm[lane * ldm + i] = 0.0;
    if (lane == 0) a.status[i] = st0 | RYD_STATUS_BAD_INPUT;
    return;
  }
  if (lane == 0) {
    double x[T_NV], y[T_NV];
#pragma unroll
    for (int e = 0; e < T_NV; ++e) x[e] = a.psi0[e];
    ts_to_adapted(x, y);
#pragma unroll
    for (int e = 0; e < T_NV; ++e) s_psi0[e] = y[e];
  }
  __syncthreads();
  TRates R;
#pragma unroll
  for (int c = 0; c < 4; ++c) R.g[c] = q0.gA[c];
  R.hgr = 0.5 * (R.g[0] + R.g[1] + R.g[2]);
  R.hgs = 0.5 * R.g[3];
  const int nseg = n_segments<PROTO>(a.n_steps);
  const uint64_t NQ = 1ull << L;
  double kw = -1.0, kdl = 0.0, kdt = -1.0;
  double nlad = 0.0, nsq = 0.0;
  bool cap = false, nonfin = false;

  // ---- pass 1: the no-jump branch ----
  double surv = 1.0, phf = 0.0;
  int nseg_eff = 0;
  {
    double x[T_NV], y[T_NV];
#pragma unroll
    for (int e = 0; e < T_NV; ++e) x[e] = s_psi0[e];
    surv = 1.0;
    for (int sg = 0; sg < nseg; ++sg) {
      const double* pp = a.prm;
      asm volatile("" : "+s"(pp));
      const PointP q = load_point<PROTO>(pp, a.ld, i);
      const Seg g = segment<PROTO>(q, sg, a.n_steps, a.shape);
      if (!(g.dt > 0.0)) continue;
      const double w = 0.5 * sqrt(g.om_re * g.om_re + g.om_im * g.om_im);
      const double ph = (g.om_re == 0.0 && g.om_im == 0.0) ? phf : atan2(g.om_im, g.om_re);
      if (w != kw || g.dl != kdl || g.dt != kdt) {
        __syncthreads();
        const double tl0 = T_CLK();
        nsq += (double)ts_build_ladder(lad, S0, S1, S2, L, w, g.dl, q.d1, q.V, R, g.dt, tpb);
        tp_cls += T_CLK() - tl0;                     // (prof build: ladder cycles in the classify column)
        nlad += 1.0;
        kw = w;
        kdl = g.dl;
        kdt = g.dt;
      }
      if (ph != phf) {
        ts_rotate(x, phf - ph);
        phf = ph;
      }
      surv = ts_trial(lad, x, y);                    // level 0: the whole segment
#pragma unroll
      for (int e = 0; e < T_NV; ++e) x[e] = y[e];
      ++nseg_eff;
    }
    ts_rotate(x, phf);
    const double inv = surv > 0.0 ? 1.0 / sqrt(surv) : 0.0;
    if (lane == 0) {
      ts_to_atom(x, y);
#pragma unroll
      for (int e = 0; e < T_NV; ++e) s_phi[e] = y[e] * inv;
    }
  }
  __syncthreads();
  tp_pass1 = T_CLK() - tp_start;
  // the shifted sums (3 per rho element) accumulate in this point's own rho output row
  // (1134 <= 1458 doubles, L2-resident), not in registers: the walk keeps the ket and
  // its trial ket in registers and stays within two waves per SIMD
  double* accg = orho;
  for (int e = lane; e < 3 * T_NPAIR; e += T_WAVE) accg[e] = 0.0;
  double sum_j = 0.0, sum_hit = 0.0, max_j = 0.0;
  double it_use = lane == 0 ? (double)nseg_eff : 0.0, it_exec = lane == 0 ? 64.0 * nseg_eff : 0.0;
  double napply = lane == 0 ? (double)nseg_eff : 0.0;   // block applications (flop accounting)

  for (int c0 = 0; c0 < a.n_traj; c0 += T_CHUNK) {
    const int cn = min(T_CHUNK, a.n_traj - c0);
    tp_mark = T_CLK();
    int J = 0;
    for (int t0 = 0; t0 < cn; t0 += T_WAVE) {
      const uint32_t traj = (uint32_t)(c0 + t0 + lane);
      double r, s;
      t_draw(traj, 0u, gpoint, a.seed, r, s);
      const bool jumps = !(surv > r);
      const uint64_t m = __ballot(jumps);
      const int pos = __popcll(m & ((1ull << lane) - 1ull));
      if (jumps) s_list[J + pos] = traj;
      J += __popcll(m);
      if (!jumps && a.rec) {
        double* rec = a.rec + ((size_t)i * a.n_traj + traj) * RYD_T_REC_WIDTH;
        for (int e = 0; e < T_NV; ++e) rec[e] = s_phi[e];
        rec[RYD_T_REC_NJUMPS] = 0.0;
        for (int k = 0; k < 2 * RYD_T_REC_JUMPS; ++k) rec[RYD_T_REC_JUMP0 + k] = -1.0;
        rec[RYD_T_REC_ITERS] = (double)nseg_eff;
      }
    }
    __syncthreads();
    for (int j0 = 0; j0 < J; j0 += T_WAVE) {
      tp_mark = T_CLK();
      const bool act = j0 + lane < J;
      const uint32_t traj = act ? s_list[j0 + lane] : 0u;
      double* rec = (a.rec && act) ? a.rec + ((size_t)i * a.n_traj + traj) * RYD_T_REC_WIDTH : nullptr;
      if (rec)
        for (int k = 0; k < 2 * RYD_T_REC_JUMPS; ++k) rec[RYD_T_REC_JUMP0 + k] = -1.0;
      double x[T_NV];
#pragma unroll
      for (int e = 0; e < T_NV; ++e) x[e] = s_psi0[e];
      double r, s;
      uint32_t cycle = 0;
      t_draw(traj, cycle, gpoint, a.seed, r, s);
      int nj = 0;
      double iters = 0.0, phl = 0.0, t0 = 0.0, wsteps = 0.0;
      for (int sg = 0; sg < nseg; ++sg) {
        const double* pp = a.prm;
        asm volatile("" : "+s"(pp));
        const PointP q = load_point<PROTO>(pp, a.ld, i);
        const Seg g = segment<PROTO>(q, sg, a.n_steps, a.shape);
        if (!(g.dt > 0.0)) continue;
        const double w = 0.5 * sqrt(g.om_re * g.om_re + g.om_im * g.om_im);
        const double ph = (g.om_re == 0.0 && g.om_im == 0.0) ? phl : atan2(g.om_im, g.om_re);
        if (w != kw || g.dl != kdl || g.dt != kdt) {   // wave-uniform
          __syncthreads();
          nsq += (double)ts_build_ladder(lad, S0, S1, S2, L, w, g.dl, q.d1, q.V, R, g.dt);
          nlad += 1.0;
          kw = w;
          kdl = g.dl;
          kdt = g.dt;
        }
        if (ph != phl) {
          ts_rotate(x, phl - ph);
          phl = ph;
        }
        uint64_t u = act ? 0 : NQ, uend = 0;
        int l = 0;
        // A lane whose quantum ends in a jump parks (pend) and the wave applies the
        // jumps of all parked lanes together, once RYD_T_JB of them wait or no lane can
        // step: the jump code (basis change, jump operators, renormalisation, Philox)
        // then runs once per batch instead of on nearly every step.  Each lane's own
        // sequence of trials and jumps is unchanged, so the results are too.
        bool pend = false;
        for (;;) {
          const bool stp = !pend && u < NQ && iters < T_ITER_CAP;
          if (__ballot(stp)) wsteps += 1.0;
          if (stp) {
            if (u) l = max(l, L - (int)__builtin_ctzll(u));
            double y[T_NV];
            const double n2 = ts_trial(lad + (size_t)l * TS_LD, x, y);
            iters += 1.0;
            const bool take = n2 > r;
            if (take || l == L) {                    // a taken step, or the quantum that ends in a jump
#pragma unroll
              for (int e = 0; e < T_NV; ++e) x[e] = y[e];
              napply += 1.0;
            }
            if (take) {
              u += 1ull << (L - l);
              l = u < uend ? min(l + 1, L) : 0;
            } else if (l < L) {
              uend = u + (1ull << (L - l));
              ++l;
            } else {
              u += 1;                                // the jump ends this quantum
              uend = 0;
              pend = true;
            }
          }
          const uint64_t pm = __ballot(pend);
          const uint64_t sm = __ballot(!pend && u < NQ && iters < T_ITER_CAP);
          if (!pm && !sm) break;
          if (pm && (!sm || __popcll(pm) >= RYD_T_JB) && pend) {
            pend = false;
            double z[T_NV];
            ts_to_atom(x, z);
            const int ch = t_jump(z, s, R);
            const double nn = t_norm2(z);
            const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
#pragma unroll
            for (int e = 0; e < T_NV; ++e) z[e] *= inv;
            ts_to_adapted(z, x);
            if (ch >= 0) {
              if (rec && nj < RYD_T_REC_JUMPS) {
                rec[RYD_T_REC_JUMP0 + 2 * nj] = t0 + g.dt * ((double)u / (double)NQ);
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
          }
        }
        if (u < NQ) cap = true;
        t0 += g.dt;
      }
      ts_rotate(x, phl);
      double z[T_NV];
      ts_to_atom(x, z);
      const double nn = t_norm2(z);
      const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
      bool fin = nn > 0.0;
#pragma unroll
      for (int e = 0; e < T_NV; ++e) {
        z[e] *= inv;
        fin = fin && isfinite(z[e]);
      }
      if (act && !fin) nonfin = true;
      if (rec) {
        for (int e = 0; e < T_NV; ++e) rec[e] = z[e];
        rec[RYD_T_REC_NJUMPS] = (double)nj;
        rec[RYD_T_REC_ITERS] = iters;
      }
      if (act) {
        sum_j += (double)nj;
        sum_hit += nj > 0 ? 1.0 : 0.0;
        max_j = fmax(max_j, (double)nj);
        it_use += iters;
      }
      if (lane == 0) it_exec += 64.0 * wsteps;      // lane-steps the wave issued (parked lanes included)
      tp_walk += T_CLK() - tp_mark;
      tp_mark = T_CLK();
      ts_reduce_round(stg, accg, s_phi, z, act, lane, 0, min(T_WAVE, J - j0));
      __syncthreads();
      tp_red += T_CLK() - tp_mark;
    }
  }
  tp_mark = T_CLK();
  const double ntr = (double)a.n_traj;
  double trl = 0.0, qpl = 0.0;
  ts_write_moments(orho, ose, accg, s_phi, lane, ntr, trl, qpl);
  sum_j = t_wave_sum(sum_j);
  sum_hit = t_wave_sum(sum_hit);
  max_j = t_wave_max(max_j);
  it_use = t_wave_sum(it_use);
  it_exec = t_wave_sum(it_exec);
  napply = t_wave_sum(napply);
  trl = t_wave_sum(trl);
  qpl = t_wave_sum(qpl);
  const bool any_cap = __ballot(cap) != 0ull, any_nonfin = __ballot(nonfin) != 0ull;
  if (lane == 0) {
    sm[RYD_TS_MEAN_JUMPS * ldm + i] = sum_j / ntr;
    sm[RYD_TS_FRAC_JUMPED * ldm + i] = sum_hit / ntr;
    sm[RYD_TS_MAX_JUMPS * ldm + i] = max_j;
    sm[RYD_TS_TRACE * ldm + i] = trl;
    sm[RYD_TS_QUBIT_POP * ldm + i] = qpl;
    sm[RYD_TS_ITER_USEFUL * ldm + i] = it_use;
    sm[RYD_TS_ITER_EXEC * ldm + i] = it_exec;
    sm[RYD_TS_NLADDER * ldm + i] = nlad;
    sm[RYD_TS_NSQUARE * ldm + i] = nsq;
    sm[RYD_TS_RESERVED * ldm + i] = napply;             // (I + X) applications (flop accounting)
    a.status[i] = st0 | (any_cap ? RYD_STATUS_STEP_CAP : 0u) | (any_nonfin ? RYD_STATUS_NONFINITE : 0u);
#ifdef RYD_T_PROF
    sm[RYD_TS_MEAN_JUMPS * ldm + i] = tp_pass1;
    sm[RYD_TS_FRAC_JUMPED * ldm + i] = tp_cls;
    sm[RYD_TS_MAX_JUMPS * ldm + i] = tp_walk;
    sm[RYD_TS_TRACE * ldm + i] = tp_red;
    sm[RYD_TS_QUBIT_POP * ldm + i] = T_CLK() - tp_mark;
    sm[RYD_TS_RESERVED * ldm + i] = T_CLK() - tp_start;
    sm[RYD_TS_ITER_USEFUL * ldm + i] = tpb[0];
    sm[RYD_TS_ITER_EXEC * ldm + i] = tpb[1];
    sm[RYD_TS_NLADDER * ldm + i] = tpb[2];
    sm[RYD_TS_NSQUARE * ldm + i] = tpb[3];
#endif
  }
}

// RYD_T_SYM=0 selects traj3_kernel (the atom-basis kernel: A/B and cross-check runs)
bool t_sym_enabled() {
  const char* e = getenv("RYD_T_SYM");
  return !(e && e[0] == '0');
}

template <int PROTO>
int ts_launch_proto(const TrajArgs& ta, hipStream_t stream) {
  const size_t lds = ts_lds_bytes(ta.L);
  if (lds > 32768)
    HIPCHK(hipFuncSetAttribute((const void*)traj3s_kernel<PROTO>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  TrajArgs arg = ta;
  void* args[] = {(void*)&arg};
  HIPCHK(hipLaunchKernel((const void*)traj3s_kernel<PROTO>, dim3((unsigned)ta.n), dim3(T_WAVE), args, lds,
                         stream));
  return RYD_OK;
}
