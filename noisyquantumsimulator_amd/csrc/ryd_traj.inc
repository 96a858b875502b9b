// ryd_traj.inc -- three-atom Rydberg blockade with quantum-jump (Monte-Carlo
// wave-function) trajectories on MI355X.  Included by ryd_engine.hip inside its
// anonymous namespace (shares the protocol schedules, PointP and error plumbing).
//
// BASELINE configs[4] / SURVEY.md §8d C5 / §8f row 4.  The reference has no
// 3-atom model (RG/hamiltonians.py builds two atoms only), so this build defines
// it as the natural extension of the two-atom path:
//   * three identical atoms on an equilateral triangle: V P_r (x) P_r on each of
//     the 3 pairs, the single-atom H of RG/hamiltonians.py:584-1274
//     (sum_j (Omega e^{i phi}/2 |r><1|_j + h.c.) - Delta P_r,j + delta1 P_1,j),
//   * the per-atom channels of the two-atom kernel (RG/noise_models.py:1449-1620
//     collapsed onto 4 channels): sqrt(g1)|1><r|, sqrt(g0)|0><r|, sqrt(gphi) P_r,
//     sqrt(gsc) P_1 on every atom (12 jump operators; atom-A rate columns),
//   * any of the four protocol schedules of the two-atom engine (segment<PROTO>),
//   * one initial ket per batch (27 amplitudes, basis 9 a0 + 3 a1 + a2).
//
// Unravelling: the waiting-time MCWF method.  Each trajectory draws r ~ U(0,1],
// evolves its unnormalised ket under H_eff = H - (i/2) sum_k L_k^dag L_k until
// ||psi||^2 = r, then applies jump k with probability ||L_k psi||^2 / sum, renormalises
// and draws again.  H_eff is block diagonal in the "which atoms are in {1, r}" pattern
// (atoms in |0> are frozen): blocks of dimension 1, 2 (x3), 4 (x3) and 8; identical
// atoms make blocks of equal size identical, so one segment's non-unitary propagator
// is 84 complex numbers (2x2 + 4x4 + 8x8).
//
// Jump times without a stepper: per constant-H segment of length dt the block
// builds a LADDER X_l = exp(-i H_eff dt / 2^l) - I, l = 0..L, in LDS (expm1 form:
// Taylor at the bottom level, then X_{l-1} = 2 X_l + X_l^2, which keeps full
// relative accuracy).  A trajectory walks the segment in binary: it tries the
// largest aligned step, keeps it if the norm stays above r, otherwise halves; a
// failed check at the finest level places the jump at the end of that quantum
// dt / 2^L (default L = 24).  While a crossing is bracketed the walk descends one
// level per step, so a jump costs ~1.5L ladder steps.
//
// Segments that differ only in laser phase share one ladder: U(phi) = Q U(0) Q^dag
// with Q = e^{i phi N_r}, so the ket is carried in the frame of the current phase (a
// diagonal rotation when the phase changes).  The jump operators are monomials, so a
// jump in the frame equals the lab-frame jump up to a global phase.
//
// Random numbers: Philox4x32-10, counter = (trajectory, jump cycle, point lo,
// point hi), key = seed: a trajectory's stream depends only on (seed, global point
// index, trajectory index), not on the launch shape or the device partition.
//
// Work mapping: one wave per parameter point.  The no-jump branch is deterministic:
// it is computed once, and a trajectory jumps at all iff its first threshold r0 is
// >= the no-jump survival probability, so only the jumping trajectories are walked,
// compacted 64 per round (full waves instead of one jumping lane per wave).  The
// mean rho (27x27) and the standard error of each element are reduced on chip
// (shifted sums around the no-jump state, 8-ket LDS tiles) and written point-major
// (one contiguous 11.7 KB row per point).

constexpr int T_NB = 27;             // 3^3 amplitudes
constexpr int T_NV = 2 * T_NB;       // interleaved (re, im)
constexpr int T_XN = 84;             // ladder entries per level: 2x2 + 4x4 + 8x8 (complex)
constexpr int T_NPAIR = 378;         // upper triangle (with diagonal) of the 27x27 rho
constexpr int T_WAVE = 64;            // one wave = one point
constexpr int T_CHUNK = 256;          // trajectories classified per pass (jumper list in LDS)
constexpr int T_TILE = 8;             // kets per reduction tile
constexpr int T_EPL = 6;              // rho elements per lane (6 x 64 >= 378)
#ifndef RYD_T_KEEP8
#define RYD_T_KEEP8 1                 // walk: keep the 8 x 8 block's trial rows for the commit (C5 -3 %)
#endif
#ifndef RYD_T_WAVES
#define RYD_T_WAVES 1
#endif
constexpr int T_WAVES_PER_SIMD = RYD_T_WAVES; // register budget: 512 / this per lane
constexpr int T_MAX_JUMPS = 4096;    // per trajectory (status STEP_CAP beyond)
constexpr double T_ITER_CAP = 1.0e6; // ladder iterations per trajectory (STEP_CAP beyond)
constexpr int T_TAYLOR = 7;          // Taylor order of the bottom ladder level (||A|| <= 2^-10)

__host__ __device__ constexpr int t_digit(int idx, int j) {
  return j == 0 ? idx / 9 : (j == 1 ? (idx / 3) % 3 : idx % 3);
}
__host__ __device__ constexpr int t_pow3(int j) { return j == 0 ? 9 : (j == 1 ? 3 : 1); }
__host__ __device__ constexpr int t_popc3(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1); }
__host__ __device__ constexpr int t_nr(int idx) {
  return (t_digit(idx, 0) == 2) + (t_digit(idx, 1) == 2) + (t_digit(idx, 2) == 2);
}
__host__ __device__ constexpr bool t_qubit(int idx) {
  return t_digit(idx, 0) < 2 && t_digit(idx, 1) < 2 && t_digit(idx, 2) < 2;
}
__host__ __device__ constexpr int t_xoff(int k) { return k == 1 ? 0 : (k == 2 ? 4 : 20); }
// basis index of block-local state b (bit set = atom in |r>, first active atom most
// significant) of the block whose {1, r}-manifold atoms are the bits of m (bit j = atom j)
__host__ __device__ constexpr int t_blk_idx(int m, int b) {
  int k = t_popc3(m), t = 0, idx = 0;
  for (int j = 0; j < 3; ++j) {
    int lev = 0;
    if ((m >> j) & 1) {
      lev = ((b >> (k - 1 - t)) & 1) ? 2 : 1;
      ++t;
    }
    idx = idx * 3 + lev;
  }
  return idx;
}

// ---- Philox4x32-10 (Salmon et al., SC'11; Random123 round constants) ----
struct TU4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ TU4 t_philox(TU4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = TU4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// (r, s) of jump cycle `cycle`: r in (0, 1] (waiting threshold), s in [0, 1) (channel)
__device__ __forceinline__ void t_draw(uint32_t traj, uint32_t cycle, uint64_t point, uint64_t seed,
                                       double& r, double& s) {
  const TU4 o = t_philox(TU4{traj, cycle, (uint32_t)point, (uint32_t)(point >> 32)}, (uint32_t)seed,
                         (uint32_t)(seed >> 32));
  const uint64_t a = ((uint64_t)o.y << 32) | o.x, b = ((uint64_t)o.w << 32) | o.z;
  r = (double)((a >> 11) + 1) * 0x1.0p-53;
  s = (double)(b >> 11) * 0x1.0p-53;
}

// ---- the ladder (block-cooperative) ----
struct TRates {
  double hgr, hgs;        // (g1 + g0 + gphi)/2 on |r>, gsc/2 on |1>
  double g[4];            // g1, g0, gphi, gsc
};

// entry e in [0, 84) -> block k (1..3), row, col
__device__ __forceinline__ void t_entry(int e, int& k, int& r, int& c) {
  int rc;
  if (e < 4) {
    k = 1;
    rc = e;
  } else if (e < 20) {
    k = 2;
    rc = e - 4;
  } else {
    k = 3;
    rc = e - 20;
  }
  const int D = 1 << k;
  r = rc / D;
  c = rc % D;
}

// A = -i H_eff h on the k-atom block, frame phase 0 (real coupling w = |Omega|/2)
__device__ __forceinline__ double2 t_gen(int k, int r, int c, double w, double dl, double d1, double V,
                                         const TRates& R, double h) {
  double re = 0.0, im = 0.0;
  if (r == c) {
    const int nr = __popc(r);
    re = -dl * nr + d1 * (k - nr) + V * (double)(nr * (nr - 1) / 2);
    im = -(R.hgr * nr + R.hgs * (k - nr));
  } else if (__popc(r ^ c) == 1) {
    re = w;
  }
  return make_double2(im * h, -re * h);
}

// sum_j M[r, j] N[j, c] within block k
__device__ __forceinline__ double2 t_mm(const double2* M, const double2* Nm, int k, int r, int c) {
  const int D = 1 << k, o = t_xoff(k);
  double re = 0.0, im = 0.0;
  for (int j = 0; j < D; ++j) {
    const double2 a = M[o + r * D + j], b = Nm[o + j * D + c];
    re = fma(a.x, b.x, fma(-a.y, b.y, re));
    im = fma(a.x, b.y, fma(a.y, b.x, im));
  }
  return make_double2(re, im);
}

// lad[l] = exp(-i H_eff dt / 2^l) - I for l = 0..L; S0..S2: 3 x 84 scratch.  Called by
// every thread of the block (it synchronises).  Returns the squarings performed.
__device__ int t_build_ladder(double2* lad, double2* S0, double2* S1, double2* S2, int L, double w,
                              double dl, double d1, double V, const TRates& R, double dt) {
  const int tid = threadIdx.x, nt = blockDim.x;
  // Gershgorin bound of the 8x8 block (the largest)
  const double bnd = 3.0 * (fabs(dl) + fabs(d1) + R.hgr + R.hgs + fabs(V) + w);
  const double x = ldexp(bnd * dt, -L);
  int s0 = 0;
  if (x > 0x1.0p-10) s0 = (int)ceil(log2(x)) + 10;
  const double h = ldexp(dt, -(L + s0));
  double2* Xb = lad + (size_t)L * T_XN;
  for (int e = tid; e < T_XN; e += nt) {
    int k, r, c;
    t_entry(e, k, r, c);
    const double2 a = t_gen(k, r, c, w, dl, d1, V, R, h);
    S0[e] = a;
    S1[e] = a;
    Xb[e] = a;
  }
  __syncthreads();
  // Taylor: T_n = T_{n-1} A / n, X += T_n
  double2* Tc = S1;
  double2* Tn = S2;
  for (int nn = 2; nn <= T_TAYLOR; ++nn) {
    const double inv = 1.0 / (double)nn;
    for (int e = tid; e < T_XN; e += nt) {
      int k, r, c;
      t_entry(e, k, r, c);
      double2 t = t_mm(Tc, S0, k, r, c);
      t.x *= inv;
      t.y *= inv;
      Tn[e] = t;
      Xb[e].x += t.x;
      Xb[e].y += t.y;
    }
    __syncthreads();
    double2* tmp = Tc;
    Tc = Tn;
    Tn = tmp;
  }
  // s0 unstored squarings up to the bottom level: X <- 2X + X^2
  for (int qq = 0; qq < s0; ++qq) {
    for (int e = tid; e < T_XN; e += nt) {
      int k, r, c;
      t_entry(e, k, r, c);
      const double2 p = t_mm(Xb, Xb, k, r, c);
      S1[e] = make_double2(2.0 * Xb[e].x + p.x, 2.0 * Xb[e].y + p.y);
    }
    __syncthreads();
    for (int e = tid; e < T_XN; e += nt) Xb[e] = S1[e];
    __syncthreads();
  }
  // the stored levels
  for (int l = L - 1; l >= 0; --l) {
    const double2* Xs = lad + (size_t)(l + 1) * T_XN;
    double2* Xd = lad + (size_t)l * T_XN;
    for (int e = tid; e < T_XN; e += nt) {
      int k, r, c;
      t_entry(e, k, r, c);
      const double2 p = t_mm(Xs, Xs, k, r, c);
      Xd[e] = make_double2(2.0 * Xs[e].x + p.x, 2.0 * Xs[e].y + p.y);
    }
    __syncthreads();
  }
  return s0 + L;
}

// The 3 masks with k atoms in {1, r}: k = 1 -> {1, 2, 4}, k = 2 -> {3, 5, 6}, k = 3 -> {7}.
__host__ __device__ constexpr int t_mask(int k, int q) {
  return k == 1 ? (1 << q) : (k == 2 ? (7 ^ (1 << q)) : 7);
}
__host__ __device__ constexpr int t_nmask(int k) { return k == 3 ? 1 : 3; }

// ||(I + X) x||^2 without forming the trial ket: block rows accumulated in a few
// registers (one LDS read of each X entry serves every mask of its size)
// y8 (optional) keeps the trial rows of the 8 x 8 block (half the MACs), so a step that
// is taken recomputes only the small blocks (t_commit)
template <bool KEEP8 = false>
__device__ __forceinline__ double t_trial_norm2(const double2* __restrict__ X, const double (&x)[T_NV],
                                                double* __restrict__ y8 = nullptr) {
  double s = fma(x[0], x[0], x[1] * x[1]);           // |000>: frozen
#pragma unroll
  for (int k = 1; k <= 3; ++k) {
    const int D = 1 << k;
#pragma unroll
    for (int r = 0; r < D; ++r) {
      double ar[3], ai[3];
#pragma unroll
      for (int q = 0; q < t_nmask(k); ++q) {
        const int o = t_blk_idx(t_mask(k, q), r);
        ar[q] = x[2 * o];
        ai[q] = x[2 * o + 1];
      }
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const double2 a = X[t_xoff(k) + r * D + c];
#pragma unroll
        for (int q = 0; q < t_nmask(k); ++q) {
          const int i = t_blk_idx(t_mask(k, q), c);
          ar[q] = fma(a.x, x[2 * i], fma(-a.y, x[2 * i + 1], ar[q]));
          ai[q] = fma(a.x, x[2 * i + 1], fma(a.y, x[2 * i], ai[q]));
        }
      }
#pragma unroll
      for (int q = 0; q < t_nmask(k); ++q) s = fma(ar[q], ar[q], fma(ai[q], ai[q], s));
      if (KEEP8 && k == 3) {
        y8[2 * r] = ar[0];
        y8[2 * r + 1] = ai[0];
      }
    }
  }
  return s;
}

// x <- (I + X) x in place, block by block (a block's outputs depend only on its inputs)
template <int KMAX = 3>
__device__ __forceinline__ void t_apply_inplace(const double2* __restrict__ X, double (&x)[T_NV]) {
#pragma unroll
  for (int k = 1; k <= KMAX; ++k) {
    const int D = 1 << k;
    double tr[3][8], ti[3][8];
#pragma unroll
    for (int r = 0; r < D; ++r) {
#pragma unroll
      for (int q = 0; q < t_nmask(k); ++q) {
        const int o = t_blk_idx(t_mask(k, q), r);
        tr[q][r] = x[2 * o];
        ti[q][r] = x[2 * o + 1];
      }
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const double2 a = X[t_xoff(k) + r * D + c];
#pragma unroll
        for (int q = 0; q < t_nmask(k); ++q) {
          const int i = t_blk_idx(t_mask(k, q), c);
          tr[q][r] = fma(a.x, x[2 * i], fma(-a.y, x[2 * i + 1], tr[q][r]));
          ti[q][r] = fma(a.x, x[2 * i + 1], fma(a.y, x[2 * i], ti[q][r]));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
      for (int q = 0; q < t_nmask(k); ++q) {
        const int o = t_blk_idx(t_mask(k, q), r);
        x[2 * o] = tr[q][r];
        x[2 * o + 1] = ti[q][r];
      }
  }
}

// x <- (I + X) x after t_trial_norm2<true>: the small blocks again, the 8 x 8 block from y8
// (the same arithmetic as t_apply_inplace)
__device__ __forceinline__ void t_commit(const double2* __restrict__ X, double (&x)[T_NV], const double (&y8)[16]) {
  t_apply_inplace<2>(X, x);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int o = t_blk_idx(t_mask(3, 0), r);
    x[2 * o] = y8[2 * r];
    x[2 * o + 1] = y8[2 * r + 1];
  }
}

__device__ __forceinline__ double t_norm2(const double (&x)[T_NV]) {
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < T_NV; ++e) s = fma(x[e], x[e], s);
  return s;
}

// x <- L_{J,C} x in place (unnormalised); C: 0 |1><r|, 1 |0><r|, 2 P_r, 3 P_1 on atom J
template <int J, int C>
__device__ __forceinline__ void t_jump_op(double (&x)[T_NV]) {
  constexpr int dst = C == 0 ? 1 : (C == 1 ? 0 : (C == 2 ? 2 : 1));
  constexpr int src = C == 3 ? 1 : 2;
#pragma unroll
  for (int idx = 0; idx < T_NB; ++idx)               // move first (dst and src digits differ)
    if (t_digit(idx, J) == dst && src != dst) {
      const int s = idx + (src - dst) * t_pow3(J);
      x[2 * idx] = x[2 * s];
      x[2 * idx + 1] = x[2 * s + 1];
    }
#pragma unroll
  for (int idx = 0; idx < T_NB; ++idx)
    if (t_digit(idx, J) != dst) {
      x[2 * idx] = 0.0;
      x[2 * idx + 1] = 0.0;
    }
}

// choose and apply a jump to x (the state at the jump time) in place; returns the
// channel 4 j + c, or -1 if no channel has weight (x unchanged)
__device__ __forceinline__ int t_jump(double (&x)[T_NV], double sel, const TRates& R) {
  double pr[3] = {0.0, 0.0, 0.0}, p1[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int idx = 0; idx < T_NB; ++idx) {
    const double p = fma(x[2 * idx], x[2 * idx], x[2 * idx + 1] * x[2 * idx + 1]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (t_digit(idx, j) == 2) pr[j] += p;
      if (t_digit(idx, j) == 1) p1[j] += p;
    }
  }
  double wt[12], tot = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      wt[4 * j + c] = R.g[c] * (c < 3 ? pr[j] : p1[j]);
      tot += wt[4 * j + c];
    }
  int ch = -1, last = -1;
  if (tot > 0.0) {
    const double thr = sel * tot;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      acc += wt[k];
      if (wt[k] > 0.0) last = k;
      if (ch < 0 && thr < acc && wt[k] > 0.0) ch = k;
    }
    if (ch < 0) ch = last;
  }
  switch (ch) {
    case 0: t_jump_op<0, 0>(x); break;
    case 1: t_jump_op<0, 1>(x); break;
    case 2: t_jump_op<0, 2>(x); break;
    case 3: t_jump_op<0, 3>(x); break;
    case 4: t_jump_op<1, 0>(x); break;
    case 5: t_jump_op<1, 1>(x); break;
    case 6: t_jump_op<1, 2>(x); break;
    case 7: t_jump_op<1, 3>(x); break;
    case 8: t_jump_op<2, 0>(x); break;
    case 9: t_jump_op<2, 1>(x); break;
    case 10: t_jump_op<2, 2>(x); break;
    case 11: t_jump_op<2, 3>(x); break;
    default: break;
  }
  return ch;
}

// x_idx *= e^{i ang n_r(idx)}
__device__ __forceinline__ void t_rotate(double (&x)[T_NV], double ang) {
  double s1, c1;
  sincos(ang, &s1, &c1);
  const double c2 = c1 * c1 - s1 * s1, s2 = 2.0 * s1 * c1;
  const double c3 = c2 * c1 - s2 * s1, s3 = s2 * c1 + c2 * s1;
  const double cs[4] = {1.0, c1, c2, c3}, sn[4] = {0.0, s1, s2, s3};
#pragma unroll
  for (int idx = 0; idx < T_NB; ++idx) {
    const int n = t_nr(idx);
    if (n == 0) continue;
    const double re = x[2 * idx], im = x[2 * idx + 1];
    x[2 * idx] = re * cs[n] - im * sn[n];
    x[2 * idx + 1] = re * sn[n] + im * cs[n];
  }
}

// (a, b), a <= b, of upper-triangle element e (row-major over a)
__device__ __forceinline__ void t_pair(int e, int& a, int& b) {
  // row r starts at off(r) = r NB - r (r - 1) / 2: the largest r with off(r) <= e from the
  // quadratic's root in single precision, then one step either way (exact for every e < 378;
  // the row-by-row walk it replaces cost up to 27 trips per pair)
  constexpr int B2 = 2 * T_NB + 1;
  int row = (int)(0.5f * ((float)B2 - __builtin_sqrtf((float)(B2 * B2 - 8 * e))));
  int off = row * T_NB - row * (row - 1) / 2;
  if (off > e) {
    --row;
    off -= T_NB - row;
  } else if (e >= off + (T_NB - row)) {
    off += T_NB - row;
    ++row;
  }
  a = row;
  b = row + (e - off);
}

struct TrajArgs {
  const double* prm;
  int64_t n, ld, point_offset, point_stride;      // global point index: point_offset + point_stride * i
  double* rho;                 // [n][ld_rho >= RYD_T_RHO_WIDTH]
  int64_t ld_rho;
  double* se;                  // [n][ld_se >= RYD_T_SE_WIDTH]
  int64_t ld_se;
  double* summ;                // [RYD_T_NSUMMARY][ld_summ]
  int64_t ld_summ;
  double* rec;                 // nullable: [n][n_traj][RYD_T_REC_WIDTH]
  uint32_t* status;
  int n_steps, shape, L, n_traj;
  int fix;                     // traj3s_kernel: run only points marked RYD_STATUS_EXACT_FALLBACK
  // traj3e_kernel's grid: npair waves x split trajectory ranges; split > 1 merges through
  // kets [n][n_traj][T_NV] (jumpers only), stats [n][split][8] and arrive [n] (zeroed)
  int split;
  int64_t npair;
  double* kets;
  double* stats;
  uint32_t* arrive;
  uint64_t seed;
  double psi0[T_NV];
};

__device__ __forceinline__ double t_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double t_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// LDS per point: the ladder + 3 x 84 scratch for building it; the scratch doubles as
// the 8-ket reduction tile (8 x 27 <= 3 x 84), so L = 24 needs 37.6 KB -> 4 points per CU.
__host__ __device__ constexpr size_t t_lds_bytes(int L) {
  return sizeof(double2) * ((size_t)(L + 1) * T_XN + 3 * T_XN);
}

// One wave = one parameter point.
//  pass 1: the no-jump branch, once (every lane computes it identically): its final
//          norm^2 is the survival probability S, its normalised state phi;
//  classify: trajectory t jumps at all iff its first threshold r0(t) >= S (the norm
//          decreases monotonically), so quiet trajectories end in phi without being
//          simulated (bit-identical to walking them: the same arithmetic);
//  pass 2: the jumping trajectories, compacted 64 per round, walk the ladder;
//  reduce: shifted sums with the shift X_phi, so quiet trajectories contribute 0.
// RYD_T_PROF (tools/traj_prof.py builds a variant with it; never the product build): per-wave
// shader-clock phase totals written over the summary's MEAN_JUMPS..QUBIT_POP and RESERVED
// columns: ladder + no-jump branch, classify, walk, reduction, outputs, whole wave.
#ifdef RYD_T_PROF
#define T_CLK() ((double)__builtin_readcyclecounter())
#define T_RTC() ((double)__builtin_amdgcn_s_memrealtime())   // 100 MHz, common to the XCDs
#else
#define T_CLK() 0.0
#define T_RTC() 0.0
#endif
template <int PROTO>
__global__ __launch_bounds__(T_WAVE, T_WAVES_PER_SIMD) void traj3_kernel(TrajArgs a) {
  double tp_start = T_CLK(), tp_pass1 = 0.0, tp_cls = 0.0, tp_walk = 0.0, tp_red = 0.0, tp_mark = 0.0;
  (void)tp_start; (void)tp_pass1; (void)tp_cls; (void)tp_walk; (void)tp_red; (void)tp_mark;
  extern __shared__ double2 t_lds[];
  __shared__ uint32_t s_list[T_CHUNK];
  __shared__ double s_psi0[T_NV];
  __shared__ double s_phi[T_NV];
  const int L = a.L;
  double2* lad = t_lds;                              // [(L + 1)][84]
  double2* S0 = lad + (size_t)(L + 1) * T_XN;
  double2* S1 = S0 + T_XN;
  double2* S2 = S1 + T_XN;
  double2* stg = S0;                                 // [8][27] ket tile (aliases the scratch)
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  if (i >= a.n) return;                              // uniform per block
  const uint64_t gpoint = (uint64_t)(a.point_offset + a.point_stride * i);
  const PointP q0 = load_point<PROTO>(a.prm, a.ld, i);
  const bool valid = point_valid<PROTO>(q0, a.n_steps);
  double* orho = a.rho + (size_t)i * a.ld_rho;
  double* ose = a.se + (size_t)i * a.ld_se;
  double* sm = a.summ;
  const int64_t ldm = a.ld_summ;
  if (!valid) {                                      // uniform
    for (int e = lane; e < RYD_T_RHO_WIDTH; e += T_WAVE) orho[e] = 0.0;
    for (int e = lane; e < RYD_T_SE_WIDTH; e += T_WAVE) ose[e] = 0.0;
    if (lane < RYD_T_NSUMMARY) sm[lane * ldm + i] = 0.0;
    if (lane == 0) a.status[i] = RYD_STATUS_BAD_INPUT;
    return;
  }
  if (lane < T_NV) s_psi0[lane] = a.psi0[lane];
  __syncthreads();
  TRates R;
#pragma unroll
  for (int c = 0; c < 4; ++c) R.g[c] = q0.gA[c];
  R.hgr = 0.5 * (R.g[0] + R.g[1] + R.g[2]);
  R.hgs = 0.5 * R.g[3];
  const int nseg = n_segments<PROTO>(a.n_steps);
  const uint64_t NQ = 1ull << L;
  double kw = -1.0, kdl = 0.0, kdt = -1.0;           // ladder cache key (wave-uniform)
  double nlad = 0.0, nsq = 0.0;
  bool cap = false, nonfin = false;

  // ---- pass 1: the no-jump branch ----
  double surv = 1.0, phf = 0.0;
  int nseg_eff = 0;
  {
    double x[T_NV];
#pragma unroll
    for (int e = 0; e < T_NV; ++e) x[e] = s_psi0[e];
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
        nsq += (double)t_build_ladder(lad, S0, S1, S2, L, w, g.dl, q.d1, q.V, R, g.dt);
        nlad += 1.0;
        kw = w;
        kdl = g.dl;
        kdt = g.dt;
      }
      if (ph != phf) {
        t_rotate(x, phf - ph);
        phf = ph;
      }
      surv = t_trial_norm2(lad, x);                  // the walk's top-level check, same arithmetic
      t_apply_inplace(lad, x);                       // level 0: the whole segment
      ++nseg_eff;
    }
    t_rotate(x, phf);
    const double inv = surv > 0.0 ? 1.0 / sqrt(surv) : 0.0;
    if (lane == 0)
#pragma unroll
      for (int e = 0; e < T_NV; ++e) s_phi[e] = x[e] * inv;
  }
  __syncthreads();
  tp_pass1 = T_CLK() - tp_start;
  double ref[T_EPL][2], acc[T_EPL][3];              // per lane: rho elements lane + 64 k
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    ref[k][0] = ref[k][1] = 0.0;
    const int e = lane + k * T_WAVE;
    if (e < T_NPAIR) {
      int pa, pb;
      t_pair(e, pa, pb);
      const double ar = s_phi[2 * pa], ai = s_phi[2 * pa + 1], br = s_phi[2 * pb], bi = s_phi[2 * pb + 1];
      ref[k][0] = fma(ar, br, ai * bi);
      ref[k][1] = fma(ai, br, -ar * bi);
    }
  }
  double sum_j = 0.0, sum_hit = 0.0, max_j = 0.0;
  double it_use = lane == 0 ? (double)nseg_eff : 0.0, it_exec = lane == 0 ? 64.0 * nseg_eff : 0.0;

  for (int c0 = 0; c0 < a.n_traj; c0 += T_CHUNK) {
    const int cn = min(T_CHUNK, a.n_traj - c0);      // a multiple of 64
    // ---- classify: who jumps at all ----
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
    tp_cls += T_CLK() - tp_mark;
    // ---- pass 2: the jumping trajectories, 64 per round ----
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
      double iters = 0.0, phl = 0.0, t0 = 0.0;
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
          nsq += (double)t_build_ladder(lad, S0, S1, S2, L, w, g.dl, q.d1, q.V, R, g.dt);
          nlad += 1.0;
          kw = w;
          kdl = g.dl;
          kdt = g.dt;
        }
        if (ph != phl) {
          t_rotate(x, phl - ph);
          phl = ph;
        }
        // u: position in quanta; while a crossing is bracketed in [u, uend) the walk
        // descends one level per step, otherwise it takes the largest aligned step
        uint64_t u = act ? 0 : NQ, uend = 0;
        int l = 0;
        while (u < NQ && iters < T_ITER_CAP) {
          if (u) l = max(l, L - (int)__builtin_ctzll(u));
          const double2* X = lad + (size_t)l * T_XN;
#if RYD_T_KEEP8
          double y8[16];
          const double n2 = t_trial_norm2<true>(X, x, y8);
#else
          const double n2 = t_trial_norm2(X, x);
#endif
          iters += 1.0;
          if (n2 > r) {
#if RYD_T_KEEP8
            t_commit(X, x, y8);
#else
            t_apply_inplace(X, x);
#endif
            u += 1ull << (L - l);
            l = u < uend ? min(l + 1, L) : 0;
          } else if (l < L) {
            uend = u + (1ull << (L - l));
            ++l;
          } else {
            u += 1;                                  // the jump ends this quantum
            uend = 0;
#if RYD_T_KEEP8
            t_commit(X, x, y8);
#else
            t_apply_inplace(X, x);
#endif
            const int ch = t_jump(x, s, R);
            const double nn = t_norm2(x);
            const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
#pragma unroll
            for (int e = 0; e < T_NV; ++e) x[e] *= inv;
            if (ch >= 0) {
              if (rec && nj < RYD_T_REC_JUMPS) {
                rec[RYD_T_REC_JUMP0 + 2 * nj] = t0 + g.dt * ((double)u / (double)NQ);
                rec[RYD_T_REC_JUMP0 + 2 * nj + 1] = (double)ch;
              }
              ++nj;
            }
            ++cycle;
            if (nj >= T_MAX_JUMPS) {
              r = 0.0;                               // no further jumps (flagged)
              cap = true;
            } else {
              t_draw(traj, cycle, gpoint, a.seed, r, s);
            }
          }
        }
        if (u < NQ) cap = true;
        t0 += g.dt;
      }
      // back to the lab frame; the normalised conditional state
      t_rotate(x, phl);
      const double nn = t_norm2(x);
      const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
      bool fin = nn > 0.0;
#pragma unroll
      for (int e = 0; e < T_NV; ++e) {
        x[e] *= inv;
        fin = fin && isfinite(x[e]);
      }
      if (act && !fin) nonfin = true;
      if (rec) {
        for (int e = 0; e < T_NV; ++e) rec[e] = x[e];
        rec[RYD_T_REC_NJUMPS] = (double)nj;
        rec[RYD_T_REC_ITERS] = iters;
      }
      if (act) {
        sum_j += (double)nj;
        sum_hit += nj > 0 ? 1.0 : 0.0;
        max_j = fmax(max_j, (double)nj);
        it_use += iters;
      }
      const double wmax = t_wave_max(act ? iters : 0.0);
      if (lane == 0) it_exec += 64.0 * wmax;        // the wave runs as long as its slowest lane
      tp_walk += T_CLK() - tp_mark;
      tp_mark = T_CLK();
      // reduce this round's kets through 8-ket tiles
      const int nk = min(T_WAVE, J - j0);
      for (int tb = 0; tb < nk; tb += T_TILE) {
        __syncthreads();
        if (act && lane >= tb && lane < tb + T_TILE)
#pragma unroll
          for (int idx = 0; idx < T_NB; ++idx)
            stg[(lane - tb) * T_NB + idx] = make_double2(x[2 * idx], x[2 * idx + 1]);
        __syncthreads();
        const int tn = min(T_TILE, nk - tb);
#pragma unroll
        for (int k = 0; k < T_EPL; ++k) {
          const int e = lane + k * T_WAVE;
          if (e < T_NPAIR) {
            int pa, pb;
            t_pair(e, pa, pb);
            for (int t = 0; t < tn; ++t) {
              const double2 u1 = stg[t * T_NB + pa], u2 = stg[t * T_NB + pb];
              const double xr = fma(u1.x, u2.x, u1.y * u2.y) - ref[k][0];
              const double xi = fma(u1.y, u2.x, -u1.x * u2.y) - ref[k][1];
              acc[k][0] += xr;
              acc[k][1] += xi;
              acc[k][2] = fma(xr, xr, fma(xi, xi, acc[k][2]));
            }
          }
        }
      }
      __syncthreads();
      tp_red += T_CLK() - tp_mark;
    }
  }
  tp_mark = T_CLK();
  // ---- per-point outputs (quiet trajectories contribute X_phi - ref = 0) ----
  const double ntr = (double)a.n_traj;
  double trl = 0.0, qpl = 0.0;
#pragma unroll
  for (int k = 0; k < T_EPL; ++k) {
    const int e = lane + k * T_WAVE;
    if (e < T_NPAIR) {
      int pa, pb;
      t_pair(e, pa, pb);
      const double dr = acc[k][0] / ntr, di = acc[k][1] / ntr;
      const double mr = ref[k][0] + dr, mi = ref[k][1] + di;
      const double var = acc[k][2] / ntr - (dr * dr + di * di);
      const double sev = ntr > 1.0 ? sqrt(fmax(var, 0.0) / (ntr - 1.0)) : 0.0;
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
  sum_j = t_wave_sum(sum_j);
  sum_hit = t_wave_sum(sum_hit);
  max_j = t_wave_max(max_j);
  it_use = t_wave_sum(it_use);
  it_exec = t_wave_sum(it_exec);
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
    sm[RYD_TS_RESERVED * ldm + i] = 0.0;
    a.status[i] = (any_cap ? RYD_STATUS_STEP_CAP : 0u) | (any_nonfin ? RYD_STATUS_NONFINITE : 0u);
#ifdef RYD_T_PROF
    sm[RYD_TS_MEAN_JUMPS * ldm + i] = tp_pass1;
    sm[RYD_TS_FRAC_JUMPED * ldm + i] = tp_cls;
    sm[RYD_TS_MAX_JUMPS * ldm + i] = tp_walk;
    sm[RYD_TS_TRACE * ldm + i] = tp_red;
    sm[RYD_TS_QUBIT_POP * ldm + i] = T_CLK() - tp_mark;
    sm[RYD_TS_RESERVED * ldm + i] = T_CLK() - tp_start;
#endif
  }
}

#include "ryd_traj_sym.inc"
#include "ryd_traj_eig.inc"

template <int PROTO>
int t_launch_proto(const TrajArgs& ta, hipStream_t stream) {
  if (ta.L == RYD_T_EXACT) return te_launch_proto<PROTO>(ta, stream);
  if (t_sym_enabled()) return ts_launch_proto<PROTO>(ta, stream);
  const size_t lds = t_lds_bytes(ta.L);
  if (lds > 32768)
    HIPCHK(hipFuncSetAttribute((const void*)traj3_kernel<PROTO>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  TrajArgs arg = ta;
  void* args[] = {(void*)&arg};
  HIPCHK(hipLaunchKernel((const void*)traj3_kernel<PROTO>, dim3((unsigned)ta.n), dim3(T_WAVE), args, lds,
                         stream));
  return RYD_OK;
}

int validate_traj(const ryd_traj_desc* d, int64_t n, int64_t ldp) {
  if (!d) return fail(RYD_ERR_INVALID, "desc is NULL");
  if (d->abi_version != RYD_ABI_VERSION) return fail(RYD_ERR_INVALID, "abi_version mismatch");
  if (int rc = validate_protocol(d->protocol, d->n_steps, d->shape)) return rc;
  if (d->n_traj < T_WAVE || d->n_traj % T_WAVE != 0 || d->n_traj > (1 << 20))
    return fail(RYD_ERR_INVALID, "n_traj must be a positive multiple of 64 (<= 2^20)");
  if ((d->flags & ~RYD_T_FLAG_LANES) != 0u)
    return fail(RYD_ERR_INVALID, "flags: RYD_T_FLAG_ROWS (1) was retired; use 0 or RYD_T_FLAG_LANES");
  if (d->ladder_levels < RYD_T_EXACT || d->ladder_levels > RYD_T_LADDER_MAX)
    return fail(RYD_ERR_INVALID, "ladder_levels must be RYD_T_EXACT (0) or in [1, RYD_T_LADDER_MAX]");
  if (d->ladder_levels == RYD_T_EXACT && d->protocol == RYD_PROTO_LP_SHAPED && d->shape != RYD_SHAPE_SQUARE)
    return fail(RYD_ERR_INVALID, "exact jump times need a constant |Omega| and Delta: use ladder_levels >= 1 "
                                 "for a shaped LP envelope");
  double nn = 0.0;
  for (int e = 0; e < T_NV; ++e) {
    if (!isfinite(d->psi0[e])) return fail(RYD_ERR_INVALID, "psi0 is not finite");
    nn += d->psi0[e] * d->psi0[e];
  }
  if (fabs(nn - 1.0) > 1e-12) return fail(RYD_ERR_INVALID, "psi0 must be normalised (|1 - <psi|psi>| <= 1e-12)");
  if (n < 0) return fail(RYD_ERR_INVALID, "n < 0");
  if (n > 0x7fffffffLL) return fail(RYD_ERR_INVALID, "batch too large for one launch");
  if (ldp < n) return fail(RYD_ERR_INVALID, "leading dimension too small");
  return RYD_OK;
}

int launch_traj(const ryd_traj_desc* d, const double* dp, int64_t n, int64_t ldp, int64_t off, double* drho,
                int64_t ldr, double* dse, int64_t ldse, double* dsum, int64_t ldsum, double* drec,
                uint32_t* dstat, hipStream_t stream) {
  if (n == 0) return RYD_OK;
  TrajArgs ta;
  ta.prm = dp;
  ta.n = n;
  ta.ld = ldp;
  ta.point_offset = off;
  ta.point_stride = d->point_stride > 1u ? (int64_t)d->point_stride : 1;
  ta.rho = drho;
  ta.ld_rho = ldr;
  ta.se = dse;
  ta.ld_se = ldse;
  ta.summ = dsum;
  ta.ld_summ = ldsum;
  ta.rec = drec;
  ta.status = dstat;
  ta.n_steps = d->n_steps;
  ta.shape = d->shape;
  ta.L = d->ladder_levels;
  ta.n_traj = d->n_traj;
  ta.fix = 0;
  ta.split = 1;
  ta.npair = 0;
  ta.kets = nullptr;
  ta.stats = nullptr;
  ta.arrive = nullptr;
  ta.seed = d->seed;
  for (int e = 0; e < T_NV; ++e) ta.psi0[e] = d->psi0[e];
  return with_protocol(d->protocol,
                       [&](auto proto) { return t_launch_proto<decltype(proto)::value>(ta, stream); });
}
