// ryd_engine.hip -- MI355X (gfx950) batched Lindblad / Schrodinger engine for the
// two-atom Rydberg CZ gate, behind the C-ABI of include/ryd_engine.h.
//
// Replaces qutip.mesolve as called by the reference evolvers
// (src/qpu_simulator/micro_physics/neutral_atoms/rydberg_gates/simulation.py:647-2231).
//
// Design:
//  * one lane per (parameter point, basis input): lane = 4*point + 2*a1 + a2, so
//    a 64-lane wavefront integrates 16 points x 4 density matrices;
//  * the 4 basis inputs live in the exact 25-dim real invariant sector of the
//    Lindbladian (each atom's {1,r}-excitation number is conserved by H and by
//    every c_op of RG/noise_models.py:1449-1620); the generator is
//        dR = M_A R + R M_B^T + V-term,     M_X: 5x5 real single-atom generator,
//    applied in ~162 FMAs with R, the Chebyshev vectors and M in VGPRs -- no
//    LDS and no cross-lane traffic in the inner loop;
//  * per constant-H segment, exp(L dt) is applied with a Chebyshev expansion of
//    degree K = x + 12 x^(1/3) + 10 (x = omega*dt, omega a Gershgorin bound of
//    the spectrum) evaluated by Clenshaw's recurrence; the Bessel coefficients
//    J_k(x) are produced by Miller's downward recurrence IN the same loop (both
//    run k = K..0), normalised at the end by J_0 + 2 sum J_2k = 1.
//    Truncation < 1e-17; measured error vs exact expm ~1e-14 (tests/);
//  * segment schedules are generated on-device from per-point scalars exactly
//    as the reference evolvers build their tlists (linspace midpoints etc.);
//  * FP64 VALU bound (no MFMA: per-point operators are 5x5); HBM traffic is
//    ~300 B in + 800 B out per point.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <complex>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/ryd_engine.h"

// Persistent per-slot workspace of the host-buffer entry points: one device buffer and
// one pinned host staging buffer with the same layout [params | outputs... | status],
// grown on demand and reused across calls, plus the slot's timing events.
struct ryd_slot_work {
  void* dbuf = nullptr;
  size_t dcap = 0;
  void* hbuf = nullptr;     // hipHostMalloc (pinned, portable)
  size_t hcap = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ev_ok = false;
  hipEvent_t mark[2] = {nullptr, nullptr};   // ryd_mark / ryd_mark_elapsed
};

// one stream per device slot; defined at global scope (the header's opaque type)
struct ryd_handle {
  std::vector<int> dev;
  std::vector<hipStream_t> stream;
  std::vector<ryd_slot_work> work;
  std::vector<double> timeline;   // ryd_last_timeline
  std::mutex mu;                  // one host-buffer call at a time per handle
};

// The launch of the CU-balanced sym16 LP-square kernels (ryd_sym16.inc).  They are compiled in
// a translation unit of their own, ryd_sym16_bal.hip, whose compiler option preloads their
// first arguments into SGPRs (an option of the whole unit: every other kernel keeps its code).
// form: 2 the one-instruction parameter load, 1 the 64-bit column loads; state: false takes the
// summary-only twin.  cfg = s16_bal_cfg(gpc, st32, nohandoff, wt).
__attribute__((visibility("hidden"))) hipError_t ryd_s16_bal_launch(
    int form, bool state, unsigned workgroups, unsigned block, hipStream_t stream, const double* prm, int64_t n,
    int64_t ldp, int cfg, double* sm, uint32_t* status, int64_t ldm, double* st, int64_t lds, int n_steps);

namespace {

constexpr int BLOCK = 256;
constexpr double MILLER_SEED = 1e-200;
constexpr int MILLER_MARGIN = 10;
constexpr double X_SKIP = 1e-20;   // segments with omega*dt below this are identity
constexpr double X_CAP = 2.0e6;    // > 2e6 rad in one segment: refuse (status STEP_CAP), the
                                   // analogue of mesolve's nsteps cap (RG/simulation.py:687)

// ---------------------------------------------------------------------------
// per-point inputs
// ---------------------------------------------------------------------------
struct PointP {
  double Om, Dl, V, d1;
  double gA[4], gB[4];      // g1, g0, gphi, gsc
  double tau, xr, xi, corr, A, wmod, phoff, otau;
  int nseg;
  int64_t i, ld;
  const double* prm;
};

__device__ __forceinline__ double col(const double* p, int f, int64_t ld, int64_t i) {
  return p[(int64_t)f * ld + i];
}

// The point's columns through an accessor get(f) = column f of this point (load_point: the
// plain per-lane index; ryd_sym16.inc: a wave-uniform base plus a 32-bit lane offset).
template <int PROTO, typename Get>
__device__ __forceinline__ PointP load_point_with(Get get) {
  PointP q;
  q.prm = nullptr; q.ld = 0; q.i = 0;
  q.Om = get(RYD_P_OMEGA);
  q.Dl = get(RYD_P_DELTA);
  q.V = get(RYD_P_V);
  q.d1 = get(RYD_P_DELTA1);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    q.gA[c] = get(RYD_P_G1_A + c);
    q.gB[c] = get(RYD_P_G1_B + c);
  }
  q.tau = get(RYD_P_TAU);
  q.xr = q.xi = q.corr = q.A = q.wmod = q.phoff = q.otau = 0.0;
  q.nseg = 0;
  if (PROTO == RYD_PROTO_LP_SQUARE || PROTO == RYD_PROTO_LP_SHAPED) {
    q.xr = get(RYD_P_XI_RE);
    q.xi = get(RYD_P_XI_IM);
    q.corr = (PROTO == RYD_PROTO_LP_SHAPED) ? get(RYD_P_AREA_CORR) : 1.0;
  } else if (PROTO == RYD_PROTO_SMOOTH_JP) {
    q.A = get(RYD_P_A);
    q.wmod = get(RYD_P_OMEGA_MOD);
    q.phoff = get(RYD_P_PHI_OFF);
  } else {
    q.otau = get(RYD_P_OMEGA_TAU);
    q.nseg = (int)get(RYD_P_NSEG);
  }
  return q;
}

template <int PROTO>
__device__ __forceinline__ PointP load_point(const double* __restrict__ p, int64_t ld, int64_t i) {
  PointP q = load_point_with<PROTO>([&](int f) { return col(p, f, ld, i); });
  q.prm = p; q.ld = ld; q.i = i;
  return q;
}

struct Seg {
  double om_re, om_im, dl, dt;
};

// Segment s of the protocol schedule, exactly as the reference evolvers build it.
template <int PROTO>
__device__ __forceinline__ Seg segment(const PointP& q, int s, int n_steps, int shape) {
  Seg g;
  if (PROTO == RYD_PROTO_LP_SQUARE) {            // simulation.py:728-735 (H1, then H2=H(Omega*xi))
    g.om_re = s == 0 ? q.Om : q.Om * q.xr;
    g.om_im = s == 0 ? 0.0 : q.Om * q.xi;
    g.dl = q.Dl;
    g.dt = q.tau;
  } else if (PROTO == RYD_PROTO_LP_SHAPED) {     // simulation.py:2179-2220
    const int m = n_steps - 1;                   // 499 segments per pulse
    const int pulse = s >= m ? 1 : 0;
    const int j = s - pulse * m;
    const double step = q.tau / (double)(n_steps - 1);     // linspace(0, tau, n)
    const double t0 = (double)j * step;
    const double t1 = (j + 1 == n_steps - 1) ? q.tau : (double)(j + 1) * step;
    const double tm = (t0 + t1) / 2;
    double env = 1.0;                            // gaussian/blackman: scalar t -> 1
    if (shape == RYD_SHAPE_COSINE) {
      const double sn = sin(M_PI * tm / q.tau);
      env = sn * sn;
    }
    const double a = q.Om * q.corr * env;
    g.om_re = pulse ? a * q.xr : a;
    g.om_im = pulse ? a * q.xi : 0.0;
    g.dl = q.Dl;
    g.dt = q.tau / (double)n_steps;              // dt = tau / n_time_steps (0.998 tau total)
  } else if (PROTO == RYD_PROTO_SMOOTH_JP) {     // simulation.py:1698-1731
    const double dt = q.tau / (double)n_steps;
    const double tm = (double)s * dt + dt / 2;   // linspace(0,tau,n+1)[s] + dt/2
    const double ph = q.A * cos(q.wmod * tm - q.phoff);
    double sn, cs;
    sincos(ph, &sn, &cs);
    g.om_re = q.Om * cs;
    g.om_im = q.Om * sn;
    g.dl = q.Dl;
    g.dt = dt;
  } else {                                       // simulation.py:1853-1924, Delta = 0
    if (s >= q.nseg) {
      g.om_re = g.om_im = g.dl = g.dt = 0.0;
      return g;
    }
    const double b0 = s == 0 ? 0.0 : col(q.prm, RYD_P_SWT0 + s - 1, q.ld, q.i) / q.Om;
    const double b1 = (s + 1 == q.nseg) ? q.otau / q.Om : col(q.prm, RYD_P_SWT0 + s, q.ld, q.i) / q.Om;
    const double ph = col(q.prm, RYD_P_PHI0 + s, q.ld, q.i);
    double sn, cs;
    sincos(ph, &sn, &cs);
    g.om_re = q.Om * cs;
    g.om_im = q.Om * sn;
    g.dl = 0.0;
    double dt = b1 - b0;
    g.dt = dt < 1e-18 ? 0.0 : dt;                // zero-length segments skipped
  }
  return g;
}

// Gershgorin bound on the spectrum of the two-atom H for one segment:
// diag E(a1,a2) = e(a1)+e(a2)+V[rr], e = {0, delta1, -Delta}; |Omega|/2 per excitable atom.
// h_bounds_w: the same with the half-width w = |Omega| / 2 supplied by the caller.
__device__ __forceinline__ void h_bounds_w(double w, double dl, double V, double d1, double& emin,
                                           double& emax) {
  const double e[3] = {0.0, d1, -dl};
  emin = 1e300;
  emax = -1e300;
#pragma unroll
  for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
    for (int a2 = a1; a2 < 3; ++a2) {        // (a1, a2) and (a2, a1) give the same bounds
      const double E = e[a1] + e[a2] + ((a1 == 2 && a2 == 2) ? V : 0.0);
      const double r = w * ((a1 ? 1.0 : 0.0) + (a2 ? 1.0 : 0.0));
      emin = fmin(emin, E - r);
      emax = fmax(emax, E + r);
    }
}

__device__ __forceinline__ void h_bounds(const Seg& g, double V, double d1, double& emin, double& emax) {
  h_bounds_w(0.5 * sqrt(g.om_re * g.om_re + g.om_im * g.om_im), g.dl, V, d1, emin, emax);
}

// Chebyshev degree for tail J_K(x) < 1e-17 (Airy asymptotics; exact series test for small x).
__device__ __forceinline__ int cheb_terms(double x) {
  if (x < 24.0) {
    double t = 1.0;
    int k = 0;
    do {
      ++k;
      t *= 0.5 * x / (double)k;
    } while (!(t < 1e-18 && (double)k > x));
    return k;
  }
  return (int)ceil(x + 12.0 * cbrt(x) + 10.0);
}

// Max over the wave: DPP within each 16-lane row (quad swaps, half-row and row
// mirrors), then the four row results through readlane -- ALU only (the
// __shfl_xor form goes through ds_bpermute, an LDS round trip per step).  Call with
// every lane active.
__device__ __forceinline__ int wave_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));  // row_mirror
  const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
  const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
  return max(max(a, b), max(c, d));
}

// ---------------------------------------------------------------------------
// Lindblad generator on the 25-dim real sector
// ---------------------------------------------------------------------------
// Single-atom generator M (rows = output coordinate, basis e00,e11,err,ex,ey),
// with H = (Omega/2)|r><1| + h.c. - Delta P_r + delta1 P_1 (RG/hamiltonians.py:584-1274),
// hx = Re(Omega)/2, hy = -Im(Omega)/2, hz = (delta1+Delta)/2, G = (g1+g0+gphi+gsc)/2:
//   e00: [0, 0,   g0,      0,    0  ]
//   e11: [0, 0,   g1,      2hy, -2hx]
//   err: [0, 0, -(g0+g1), -2hy,  2hx]
//   ex : [0, -hy, hy,     -G,    2hz]
//   ey : [0,  hx, -hx,    -2hz, -G  ]
// All entries pre-scaled by s = 2/omega (Clenshaw uses 2Y, Y = L/omega).
struct Gen {
  double g0, g1, mg01, hx, hy, hx2, hy2, hz2, G;
};

__device__ __forceinline__ Gen make_gen(const Seg& g, double d1, const double* r, double s) {
  Gen a;
  const double hx = 0.5 * g.om_re, hy = -0.5 * g.om_im, hz = 0.5 * (d1 + g.dl);
  a.g0 = s * r[1];
  a.g1 = s * r[0];
  a.mg01 = -s * (r[0] + r[1]);
  a.hx = s * hx;
  a.hy = s * hy;
  a.hx2 = 2.0 * a.hx;
  a.hy2 = 2.0 * a.hy;
  a.hz2 = s * 2.0 * hz;
  a.G = s * 0.5 * (r[0] + r[1] + r[2] + r[3]);
  return a;
}

// o += (M (x) I) b   (acts on the atom-A index i of R[i][j] = b[5i+j])
__device__ __forceinline__ void apply_A(const Gen& a, const double (&b)[25], double (&o)[25]) {
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const double u1 = b[5 + j], u2 = b[10 + j], u3 = b[15 + j], u4 = b[20 + j];
    o[j] = fma(a.g0, u2, o[j]);
    o[5 + j] = fma(a.g1, u2, fma(a.hy2, u3, fma(-a.hx2, u4, o[5 + j])));
    o[10 + j] = fma(a.mg01, u2, fma(-a.hy2, u3, fma(a.hx2, u4, o[10 + j])));
    o[15 + j] = fma(a.hy, u2 - u1, fma(-a.G, u3, fma(a.hz2, u4, o[15 + j])));
    o[20 + j] = fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o[20 + j])));
  }
}

// o += (I (x) M) b   (acts on the atom-B index j)
__device__ __forceinline__ void apply_B(const Gen& a, const double (&b)[25], double (&o)[25]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const double u1 = b[5 * i + 1], u2 = b[5 * i + 2], u3 = b[5 * i + 3], u4 = b[5 * i + 4];
    o[5 * i] = fma(a.g0, u2, o[5 * i]);
    o[5 * i + 1] = fma(a.g1, u2, fma(a.hy2, u3, fma(-a.hx2, u4, o[5 * i + 1])));
    o[5 * i + 2] = fma(a.mg01, u2, fma(-a.hy2, u3, fma(a.hx2, u4, o[5 * i + 2])));
    o[5 * i + 3] = fma(a.hy, u2 - u1, fma(-a.G, u3, fma(a.hz2, u4, o[5 * i + 3])));
    o[5 * i + 4] = fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o[5 * i + 4])));
  }
}

// Interaction V P_rr: -iV[P_r (x) P_r, .] = (V/2)(S (x) D + D (x) S) with
// S = {P_r,.}: err->2err, ex->ex, ey->ey;  D = -i[P_r,.]: ex->ey, ey->-ex.
// vs = (2/omega) * V/2 = V/omega.
__device__ __forceinline__ void apply_V(double vs, const double (&b)[25], double (&o)[25]) {
  const double v2 = 2.0 * vs;
  // S (x) D on rows i = rr (s=2), x, y (s=1)
  o[2 * 5 + 4] = fma(v2, b[2 * 5 + 3], o[2 * 5 + 4]);
  o[2 * 5 + 3] = fma(-v2, b[2 * 5 + 4], o[2 * 5 + 3]);
  o[3 * 5 + 4] = fma(vs, b[3 * 5 + 3], o[3 * 5 + 4]);
  o[3 * 5 + 3] = fma(-vs, b[3 * 5 + 4], o[3 * 5 + 3]);
  o[4 * 5 + 4] = fma(vs, b[4 * 5 + 3], o[4 * 5 + 4]);
  o[4 * 5 + 3] = fma(-vs, b[4 * 5 + 4], o[4 * 5 + 3]);
  // D (x) S on columns j = rr (s=2), x, y (s=1)
  o[4 * 5 + 2] = fma(v2, b[3 * 5 + 2], o[4 * 5 + 2]);
  o[3 * 5 + 2] = fma(-v2, b[4 * 5 + 2], o[3 * 5 + 2]);
  o[4 * 5 + 3] = fma(vs, b[3 * 5 + 3], o[4 * 5 + 3]);
  o[3 * 5 + 3] = fma(-vs, b[4 * 5 + 3], o[3 * 5 + 3]);
  o[4 * 5 + 4] = fma(vs, b[3 * 5 + 4], o[4 * 5 + 4]);
  o[3 * 5 + 4] = fma(-vs, b[4 * 5 + 4], o[3 * 5 + 4]);
}

__host__ __device__ constexpr int sym_index(int i, int j) {      // i <= j
  return i * 5 - i * (i - 1) / 2 + (j - i);
}

// Identical atoms, exchange-symmetric R (R[i][j] = R[j][i]) stored as its upper
// triangle t[sym_index(i, j)], i <= j.  o(i,j) += (M R)(i,j) + (R M^T)(i,j) + V(R)(i,j):
// the A part (row i of M on column j of R) then the B part (row j of M on row i), as
// apply_A/apply_B accumulate them, on 15 outputs instead of 25 (95 FMAs, not 162).
__host__ __device__ constexpr int tri(int i, int j) { return i <= j ? sym_index(i, j) : sym_index(j, i); }

// o += sum_c M[r][c] u[c] with apply_A's fma order for row r (u = a column of R)
__device__ __forceinline__ double mrow(const Gen& a, int r, double u1, double u2, double u3, double u4,
                                       double o) {
  switch (r) {
    case 0: return fma(a.g0, u2, o);
    case 1: return fma(a.g1, u2, fma(a.hy2, u3, fma(-a.hx2, u4, o)));
    case 2: return fma(a.mg01, u2, fma(-a.hy2, u3, fma(a.hx2, u4, o)));
    case 3: return fma(a.hy, u2 - u1, fma(-a.G, u3, fma(a.hz2, u4, o)));
    default: return fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o)));
  }
}

__device__ __forceinline__ void apply_Lsym(const Gen& a, double vs, const double (&t)[15], double (&o)[15]) {
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = i; j < 5; ++j) {
      const int s = sym_index(i, j);
      double acc = mrow(a, i, t[tri(1, j)], t[tri(2, j)], t[tri(3, j)], t[tri(4, j)], o[s]);
      o[s] = mrow(a, j, t[tri(i, 1)], t[tri(i, 2)], t[tri(i, 3)], t[tri(i, 4)], acc);
    }
  // V P_rr on the symmetric triangle (apply_V's S (x) D + D (x) S, both halves summed)
  const double v2 = 2.0 * vs;
  const double r23 = t[tri(2, 3)], r24 = t[tri(2, 4)], r33 = t[tri(3, 3)], r34 = t[tri(3, 4)],
               r44 = t[tri(4, 4)];
  o[tri(2, 3)] = fma(-v2, r24, o[tri(2, 3)]);
  o[tri(2, 4)] = fma(v2, r23, o[tri(2, 4)]);
  o[tri(3, 3)] = fma(-v2, r34, o[tri(3, 3)]);
  o[tri(3, 4)] = fma(-vs, r44, fma(vs, r33, o[tri(3, 4)]));
  o[tri(4, 4)] = fma(v2, r34, o[tri(4, 4)]);
}

template <bool SYM>
__device__ __forceinline__ void apply_L(const Gen& a, const Gen& b2, double vs, const double (&b)[25],
                                        double (&o)[25]) {
  apply_A(a, b, o);
  apply_B(SYM ? a : b2, b, o);
  apply_V(vs, b, o);
}

// ---------------------------------------------------------------------------
// Schrodinger generator (kets, 9 complex amplitudes, basis 3*a1+a2)
// 2Z b = (2/a)(-i)(H - c) b ; all entries prescaled by 2/a.
// ---------------------------------------------------------------------------
struct KGen {
  double E[9];     // scaled diagonal (E - c) * 2/a
  double wr, wi;   // scaled Omega/2
};

__device__ __forceinline__ KGen make_kgen(const Seg& g, double V, double d1, double c, double s) {
  KGen k;
  const double e[3] = {0.0, d1, -g.dl};
#pragma unroll
  for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
    for (int a2 = 0; a2 < 3; ++a2)
      k.E[3 * a1 + a2] = s * (e[a1] + e[a2] + ((a1 == 2 && a2 == 2) ? V : 0.0) - c);
  k.wr = s * 0.5 * g.om_re;
  k.wi = s * 0.5 * g.om_im;
  return k;
}

// o += 2Z b  with b, o interleaved complex [re0, im0, re1, ...]
__device__ __forceinline__ void apply_K(const KGen& k, const double (&b)[18], double (&o)[18]) {
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int a1 = s / 3, a2 = s % 3;
    double hr = k.E[s] * b[2 * s], hi = k.E[s] * b[2 * s + 1];
    // atom 1: |r><1| carries Omega/2, |1><r| carries conj(Omega)/2
    if (a1 == 2) {
      const int t = 3 + a2;
      hr = fma(k.wr, b[2 * t], fma(-k.wi, b[2 * t + 1], hr));
      hi = fma(k.wr, b[2 * t + 1], fma(k.wi, b[2 * t], hi));
    } else if (a1 == 1) {
      const int t = 6 + a2;
      hr = fma(k.wr, b[2 * t], fma(k.wi, b[2 * t + 1], hr));
      hi = fma(k.wr, b[2 * t + 1], fma(-k.wi, b[2 * t], hi));
    }
    if (a2 == 2) {
      const int t = 3 * a1 + 1;
      hr = fma(k.wr, b[2 * t], fma(-k.wi, b[2 * t + 1], hr));
      hi = fma(k.wr, b[2 * t + 1], fma(k.wi, b[2 * t], hi));
    } else if (a2 == 1) {
      const int t = 3 * a1 + 2;
      hr = fma(k.wr, b[2 * t], fma(k.wi, b[2 * t + 1], hr));
      hi = fma(k.wr, b[2 * t + 1], fma(-k.wi, b[2 * t], hi));
    }
    o[2 * s] += hi;        // -i (hr + i hi) = hi - i hr
    o[2 * s + 1] -= hr;
  }
}

// ---------------------------------------------------------------------------
// Chebyshev propagation of one segment:  v <- exp(x Y) v,  Y = generator/omega
//   exp(xY) = sum_k (2 - d_k0) J_k(x) T^_k(Y),  T^_{k+1} = 2Y T^_k + T^_{k-1}
//   Clenshaw: b_k = a_k v + 2Y b_{k+1} + b_{k+2};  result = J_0 v + Y b_1 + b_2
// ---------------------------------------------------------------------------
template <int NV, typename Apply>
__device__ __forceinline__ void cheb_segment(double (&v)[NV], double x, bool active, Apply apply2Y,
                                             double& nuse, double& nexec) {
  const int kt = active ? cheb_terms(x) : -1;   // series terms that matter (tail < 1e-17)
  int ks = active ? kt + MILLER_MARGIN : -1;    // Miller's recurrence starts higher
  int kmax = wave_max(ks);
  kmax = __builtin_amdgcn_readfirstlane(kmax);
  if (kmax < 0) return;                      // whole wave skips this segment
  const int kstart = (kmax + 1) & ~1;        // even
  int kc = wave_max(kt);
  kc = __builtin_amdgcn_readfirstlane(kc);
  const int kcut = (kc + 1) & ~1;            // even; Clenshaw vectors from here down
  const double i2x = active ? 2.0 / x : 0.0;
  double bA[NV], bB[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) bA[e] = bB[e] = 0.0;
  double Jp1 = 0.0, Jp2 = 0.0, S = 0.0;
  // the margin: Bessel recurrence only (the coefficients there are below 1e-17 of
  // the sum, so their Clenshaw vector updates are skipped)
  for (int k = kstart; k > kcut; k -= 2) {
    const double Jk = fma(i2x * (double)(k + 1), Jp1, -Jp2) + (k == ks ? MILLER_SEED : 0.0);
    Jp2 = Jp1;
    Jp1 = Jk;
    S = fma(2.0, Jk, S);
    const double Jk1 = fma(i2x * (double)k, Jp1, -Jp2) + (k - 1 == ks ? MILLER_SEED : 0.0);
    Jp2 = Jp1;
    Jp1 = Jk1;
  }
  for (int k = kcut; k >= 2; k -= 2) {
    // step k (even): bB <- a_k v + 2Y bA + bB
    double Jk = fma(i2x * (double)(k + 1), Jp1, -Jp2) + (k == ks ? MILLER_SEED : 0.0);
    Jp2 = Jp1;
    Jp1 = Jk;
    S = fma(2.0, Jk, S);
    // terms above this lane's own cut stay out, so a point's result does not depend
    // on its wave neighbours (bit for bit)
    const double ck = k <= kt ? 2.0 * Jk : 0.0;
#pragma unroll
    for (int e = 0; e < NV; ++e) bB[e] = fma(ck, v[e], bB[e]);
    apply2Y(bA, bB);
    // step k-1 (odd): bA <- a_{k-1} v + 2Y bB + bA
    double Jk1 = fma(i2x * (double)k, Jp1, -Jp2) + (k - 1 == ks ? MILLER_SEED : 0.0);
    Jp2 = Jp1;
    Jp1 = Jk1;
    const double ck1 = k - 1 <= kt ? 2.0 * Jk1 : 0.0;
#pragma unroll
    for (int e = 0; e < NV; ++e) bA[e] = fma(ck1, v[e], bA[e]);
    apply2Y(bB, bA);
  }
  // bA = b_1, bB = b_2 ; k = 0
  const double J0 = fma(i2x, Jp1, -Jp2);
  S += J0;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    bB[e] = fma(J0, v[e], bB[e]);
    bA[e] *= 0.5;
  }
  apply2Y(bA, bB);
  if (active) {
    const double inv = 1.0 / S;
#pragma unroll
    for (int e = 0; e < NV; ++e) v[e] = bB[e] * inv;
    nuse += (double)(kt + 1);
  }
  nexec += (double)(kcut + 1);
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool finite_all(const double* v, int n) {
  bool ok = true;
  for (int e = 0; e < n; ++e) ok = ok && isfinite(v[e]);
  return ok;
}

template <int PROTO>
__device__ __forceinline__ int n_segments(int n_steps) {
  if (PROTO == RYD_PROTO_LP_SQUARE) return 2;
  if (PROTO == RYD_PROTO_LP_SHAPED) return 2 * (n_steps - 1);
  return n_steps;       // smooth JP: n_steps; bang-bang: max segments in batch
}

template <int PROTO>
__device__ __forceinline__ bool point_valid(const PointP& q, int n_steps) {
  bool ok = q.Om > 0.0 && isfinite(q.Om) && isfinite(q.V) && isfinite(q.Dl) && isfinite(q.d1);
#pragma unroll
  for (int c = 0; c < 4; ++c) ok = ok && q.gA[c] >= 0.0 && q.gB[c] >= 0.0 && isfinite(q.gA[c]) && isfinite(q.gB[c]);
  if (PROTO == RYD_PROTO_BANGBANG) ok = ok && q.nseg >= 1 && q.nseg <= 8 && q.nseg <= n_steps;
  else ok = ok && q.tau > 0.0 && isfinite(q.tau);
  return ok;
}

__device__ __forceinline__ bool gmj_valid(double gmA, double gmB) {
  return gmA >= 0.0 && gmB >= 0.0 && isfinite(gmA) && isfinite(gmB);
}
// ok && gmj_valid(gmA, gmB) as one chain of tests.  The compiler turns the two spellings into
// different compare sequences, so each kernel keeps the one it was measured with: the state
// kernels the chain, the coherence kernels the nested form.
__device__ __forceinline__ bool gmj_valid(bool ok, double gmA, double gmB) {
  return ok && gmA >= 0.0 && gmB >= 0.0 && isfinite(gmA) && isfinite(gmB);
}

// The Chebyshev scaling of one segment in the per-lane kernels: the generator's spectrum lies
// within omega = (Gershgorin width of H) + rsum (the rate sum), x = omega dt is the series
// argument, sc the generator's scale (0 on a lane that sits the segment out).
struct SegScale {
  double x;
  bool active, capped;
  double sc;
};
__device__ __forceinline__ SegScale seg_scale(const Seg& g, double V, double d1, double rsum, bool valid) {
  double emin, emax;
  h_bounds(g, V, d1, emin, emax);
  const double omega = (emax - emin) + rsum;
  const double x = omega * g.dt;
  const bool capped = valid && !(x <= X_CAP);
  const bool active = valid && !capped && x > X_SKIP;
  return {x, active, capped, active ? 2.0 / omega : 0.0};
}

// What differs between hilbert_space_dim = 3 and 4 in the per-lane Chebyshev kernels (states
// and coherences): sizes, the extra parameter columns, generators, the trace mask.  Sector3 is
// defined below (before coherence_sector), Sector4 in ryd_coh4_prop.inc, each after the helpers
// it names; the kernels that name them are templates, instantiated after both.  The bodies
// templated on them reach everything dimension-specific through their members.
struct Sector3;
struct Sector4;

// Epilogue shared by both evolutions: gather the 4 lanes of a point.
__device__ __forceinline__ double lane_get(double v, int src) { return __shfl(v, src, 64); }

// One lane per (point, basis input): the S::NS-vector of the real (0,0) sector through every
// segment by cheb_segment, then the populations, the trace of the |11> input and the summary.
template <int PROTO, bool SYM, typename S>
__device__ __forceinline__ void lindblad_cheb_body(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  constexpr int NB = S::NB, NS = S::NS;
  const int64_t gid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = gid < 4 * n;
  const int64_t i = live ? (gid >> 2) : (n - 1);
  const int inp = (int)(gid & 3);
  const int a1 = inp >> 1, a2 = inp & 1;
  const PointP q = load_point<PROTO>(prm, ldp, i);
  const typename S::Mj mj = S::load_mj(prm, ldp, i);
  const bool valid = S::mj_valid(point_valid<PROTO>(q, n_steps), mj);

  const int e0 = NB * a1 + a2;     // |a1 a2><a1 a2| = e_{a1} (x) e_{a2}
  double v[NS];
#pragma unroll
  for (int e = 0; e < NS; ++e) v[e] = (e == e0) ? 1.0 : 0.0;   // static indices: stays in VGPRs
  double nuse = 0.0, nexec = 0.0;
  bool over_cap = false;
  const int nseg = n_segments<PROTO>(n_steps);
  double rsum = S::rate_extra(mj);
#pragma unroll
  for (int c = 0; c < 4; ++c) rsum += fabs(q.gA[c]) + fabs(q.gB[c]);
  for (int s = 0; s < nseg; ++s) {
    const Seg g = segment<PROTO>(q, s, n_steps, shape);
    const SegScale k = seg_scale(g, q.V, q.d1, rsum, valid);
    over_cap = over_cap || k.capped;
    const auto G = S::template state_gen<SYM>(g, q, mj, k.sc);
    const double vs = k.sc * 0.5 * q.V;
    cheb_segment<NS>(v, k.x, k.active,
                     [&](const double (&b)[NS], double (&o)[NS]) { S::template state_apply<SYM>(G, vs, b, o); },
                     nuse, nexec);
  }

  // epilogue
  double pop = 0.0;
#pragma unroll
  for (int e = 0; e < NS; ++e) pop = (e == e0) ? v[e] : pop;
  double tr = 0.0;                 // trace: the population coordinates of both atoms
#pragma unroll
  for (int ii = 0; ii < NB; ++ii)
#pragma unroll
    for (int jj = 0; jj < NB; ++jj)
      if (S::population(ii) && S::population(jj)) tr += v[NB * ii + jj];
  uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
  if (over_cap) stat |= RYD_STATUS_STEP_CAP;
  if (!finite_all(v, NS)) stat |= RYD_STATUS_NONFINITE;
  if (live) {
#pragma unroll
    for (int e = 0; e < NS; ++e) st[(int64_t)e * lds + gid] = v[e];
  }
  const int lane = threadIdx.x & 63, base = lane & ~3;
  double p[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) p[x] = lane_get(pop, base + x);
  const double tr11 = lane_get(tr, base + 3);
  uint32_t st_all = stat;
#pragma unroll
  for (int x = 1; x < 4; ++x) st_all |= (uint32_t)__shfl((int)stat, base + x, 64);
  if (live && inp == 0) {
    const double avg = 0.25 * (p[0] + p[1] + p[2] + p[3]);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      sm[(int64_t)(RYD_S_POP0 + x) * ldm + i] = p[x];
      sm[(int64_t)(RYD_S_OV_RE0 + x) * ldm + i] = nan;
      sm[(int64_t)(RYD_S_OV_IM0 + x) * ldm + i] = nan;
    }
    sm[(int64_t)RYD_S_AVG_POP * ldm + i] = avg;
    sm[(int64_t)RYD_S_CTRL_PHASE * ldm + i] = nan;
    sm[(int64_t)RYD_S_PENALTY * ldm + i] = nan;
    sm[(int64_t)RYD_S_AVG_F * ldm + i] = avg;
    sm[(int64_t)RYD_S_NMV_USEFUL * ldm + i] = 4.0 * nuse;   // 4 basis-input lanes per point
    sm[(int64_t)RYD_S_NMV_EXEC * ldm + i] = 4.0 * nexec;
    sm[(int64_t)RYD_S_TRACE11 * ldm + i] = tr11;
    sm[(int64_t)RYD_S_NSQUARE * ldm + i] = 0.0;
    status[i] = st_all;
  }
}

template <int PROTO, bool SYM>
__global__ __launch_bounds__(BLOCK) void lindblad_cheb_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  lindblad_cheb_body<PROTO, SYM, Sector3>(prm, n, ldp, st, lds, sm, ldm, status, n_steps, shape);
}

template <int PROTO, int KD>
__global__ __launch_bounds__(BLOCK) void ket_cheb_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  const int64_t gid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = gid < 4 * n;
  const int64_t i = live ? (gid >> 2) : (n - 1);
  const int inp = (int)(gid & 3);
  const int a1 = inp >> 1, a2 = inp & 1;
  const PointP q = load_point<PROTO>(prm, ldp, i);
  const bool valid = point_valid<PROTO>(q, n_steps);
  const int s0 = 3 * a1 + a2;

  double v[18];
#pragma unroll
  for (int e = 0; e < 18; ++e) v[e] = (e == 2 * s0) ? 1.0 : 0.0;
  double nuse = 0.0, nexec = 0.0;
  bool over_cap = false;
  const int nseg = n_segments<PROTO>(n_steps);
  for (int s = 0; s < nseg; ++s) {
    const Seg g = segment<PROTO>(q, s, n_steps, shape);
    double emin, emax;
    h_bounds(g, q.V, q.d1, emin, emax);
    const double c = 0.5 * (emax + emin);
    const double a = fmax(0.5 * (emax - emin), 1e-300);
    const double x = a * g.dt;
    const bool capped = valid && !(x <= X_CAP);
    const bool active = valid && !capped && x > X_SKIP;
    over_cap = over_cap || capped;
    const KGen K = make_kgen(g, q.V, q.d1, c, active ? 2.0 / a : 0.0);
    cheb_segment<18>(v, x, active,
                     [&](const double (&b)[18], double (&o)[18]) { apply_K(K, b, o); }, nuse, nexec);
    if (active) {   // global phase exp(-i c dt)
      double sn, cs;
      sincos(c * g.dt, &sn, &cs);
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        const double re = v[2 * e], im = v[2 * e + 1];
        v[2 * e] = fma(re, cs, im * sn);
        v[2 * e + 1] = fma(im, cs, -re * sn);
      }
    }
  }

  double ovr = 0.0, ovi = 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    ovr = (e == s0) ? v[2 * e] : ovr;
    ovi = (e == s0) ? v[2 * e + 1] : ovi;
  }
  uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
  if (over_cap) stat |= RYD_STATUS_STEP_CAP;
  if (!finite_all(v, 18)) stat |= RYD_STATUS_NONFINITE;
  if (live) {
    if (KD == 3) {
#pragma unroll
      for (int e = 0; e < 18; ++e) st[(int64_t)e * lds + gid] = v[e];
    } else {   // dim 4: the sigma+ drive never populates |r->, whose amplitudes stay 0
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        const int b1 = s4 >> 2, b2 = s4 & 3;
        const bool in3 = b1 < 3 && b2 < 3;
        const int s3 = in3 ? 3 * b1 + b2 : 0;
        st[(int64_t)(2 * s4) * lds + gid] = in3 ? v[2 * s3] : 0.0;
        st[(int64_t)(2 * s4 + 1) * lds + gid] = in3 ? v[2 * s3 + 1] : 0.0;
      }
    }
  }
  const int lane = threadIdx.x & 63, base = lane & ~3;
  double orr[4], oii[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    orr[x] = lane_get(ovr, base + x);
    oii[x] = lane_get(ovi, base + x);
  }
  double nrm11 = 0.0;
#pragma unroll
  for (int e = 0; e < 18; ++e) nrm11 += v[e] * v[e];
  nrm11 = lane_get(nrm11, base + 3);
  uint32_t st_all = stat;
#pragma unroll
  for (int x = 1; x < 4; ++x) st_all |= (uint32_t)__shfl((int)stat, base + x, 64);
  if (live && inp == 0) {
    // compute_CZ_fidelity pure branch (RG/simulation.py:483-631)
    double p[4], ph[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      p[x] = orr[x] * orr[x] + oii[x] * oii[x];
      ph[x] = atan2(oii[x], orr[x]);
    }
    double cp = ph[3] - ph[1] - ph[2] + ph[0];
    cp = cp + M_PI;                         // (cp + pi) % 2pi - pi   (python modulo)
    cp = cp - 2.0 * M_PI * floor(cp / (2.0 * M_PI));
    cp = cp - M_PI;
    const double err = fmin(fabs(cp - M_PI), fabs(cp + M_PI));
    const double cerr = cos(err / 2);
    const double pen = cerr * cerr;
    const double avgp = 0.25 * (p[0] + p[1] + p[2] + p[3]);
    const double avgf = 0.25 * (p[0] + p[1] + p[2] + p[3] * pen);
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      sm[(int64_t)(RYD_S_POP0 + x) * ldm + i] = p[x];
      sm[(int64_t)(RYD_S_OV_RE0 + x) * ldm + i] = orr[x];
      sm[(int64_t)(RYD_S_OV_IM0 + x) * ldm + i] = oii[x];
    }
    sm[(int64_t)RYD_S_AVG_POP * ldm + i] = avgp;
    sm[(int64_t)RYD_S_CTRL_PHASE * ldm + i] = cp;
    sm[(int64_t)RYD_S_PENALTY * ldm + i] = pen;
    sm[(int64_t)RYD_S_AVG_F * ldm + i] = avgf;
    sm[(int64_t)RYD_S_NMV_USEFUL * ldm + i] = 4.0 * nuse;
    sm[(int64_t)RYD_S_NMV_EXEC * ldm + i] = 4.0 * nexec;
    sm[(int64_t)RYD_S_TRACE11 * ldm + i] = nrm11;
    sm[(int64_t)RYD_S_NSQUARE * ldm + i] = 0.0;
    status[i] = st_all;
  }
}

// ---------------------------------------------------------------------------
// Noise-free kets by exact block propagators (the default ket method)
// ---------------------------------------------------------------------------
// H conserves which atoms sit in |0>, so each computational input stays in a block:
// |00> (energy 0: amplitude 1), {|01>, |0r>} (2 x 2; |10> is its atom-swap mirror)
// and {|11>, |1r>, |r1>, |rr>}, where |11> only reaches the exchange-symmetric
// {|11>, |+> = (|1r> + |r1>)/sqrt2, |rr>} (3 x 3).  With Omega = a e^{i phi}:
//   H2 = D2 Hr2 D2^dag, Hr2 = [[d1, a/2], [a/2, -Delta]],                 D2 = diag(1, e^{i phi})
//   H3 = D3 Hr3 D3^dag, Hr3 = [[2 d1, a/sqrt2, 0], [a/sqrt2, d1 - Delta, a/sqrt2],
//                              [0, a/sqrt2, V - 2 Delta]],                 D3 = diag(1, e^{i phi}, e^{2 i phi})
// (energies e = {0, d1, -Delta} per atom + V on |rr>, couplings Omega/2 as apply_K).
// exp(-i Hr2 dt) in closed form; exp(-i Hr3 dt) = Q diag(e^{-i lambda dt}) Q^T from a
// cyclic Jacobi eigendecomposition of the real symmetric Hr3 (backward stable: the
// result is exp(-i (H + E) dt) with |E| ~ eps |H|, the same class of error as the
// Chebyshev series).  Segments that differ only in laser phase share the real factors
// (the phase frame), so LP square and smooth JP build once per point, bang-bang once
// per segment; a segment then costs 13 complex MACs + the frame phases.  One lane per
// point (ket_cheb_kernel, the cross-check method, spends ~x Chebyshev terms of an
// 84-FMA generator on each of 4 lanes per segment, x = |H| dt up to ~5e3 on LP).
struct KetBlocks {
  double a, dl, dt;                          // the real factors below are for these
  double u2[3][2];                           // exp(-i Hr2 dt): m00, m01 (= m10), m11 (re, im)
  double u3[6][2];                           // exp(-i Hr3 dt): 00 01 02 11 12 22 (complex symmetric)
};

__device__ __forceinline__ void jacobi_rot(double (&A)[3][3], double (&Q)[3][3], int p, int q) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));   // inf theta -> 0
  const double c = 1.0 / sqrt(fma(t, t, 1.0)), sn = t * c;
  A[p][p] = fma(-t, apq, A[p][p]);
  A[q][q] = fma(t, apq, A[q][q]);
  A[p][q] = A[q][p] = 0.0;
  const int r = 3 - p - q;
  const double arp = A[r][p], arq = A[r][q];
  A[r][p] = A[p][r] = fma(c, arp, -sn * arq);
  A[r][q] = A[q][r] = fma(sn, arp, c * arq);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double qkp = Q[k][p], qkq = Q[k][q];
    Q[k][p] = fma(c, qkp, -sn * qkq);
    Q[k][q] = fma(sn, qkp, c * qkq);
  }
}

// sin h / h; below the switch its series, whose next term is h^6 / 5040 < 2e-22
constexpr double KET_SINC_SWITCH = 1e-3;
__device__ __forceinline__ double ket_sinc(double h) {
  const double h2 = h * h;
  const double ser = fma(h2, fma(h2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
  return fabs(h) < KET_SINC_SWITCH ? ser : sin(h) / h;
}

// The eigen data of one N x N block (the upper left of Q): H_r = Q diag(lambda) Q^T, and Phi's
// upper triangle in KetBlocks' order (00 01 [02] 11 [12 22])
struct KetEig {
  double Q[3][3];
  double P[6][2];
};

// Phi from the eigenvalues; (er, ei)_k = e^{-i lambda_k dt}
template <int N>
__device__ __forceinline__ void ket_ctl_phi(KetEig& E, const double (&lam)[3], const double (&er)[3],
                                            const double (&ei)[3], double dt) {
  int e = 0;
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int l = k; l < N; ++l, ++e) {
      if (k == l) {
        E.P[e][0] = dt * ei[k];
        E.P[e][1] = -dt * er[k];
      } else {
        double sn, cs;
        sincos(0.5 * (lam[k] + lam[l]) * dt, &sn, &cs);
        const double sc = dt * ket_sinc(0.5 * (lam[k] - lam[l]) * dt);
        E.P[e][0] = -sc * sn;
        E.P[e][1] = -sc * cs;
      }
    }
}

// EIG: beside the propagator the eigen data of both blocks (the control Jacobian of
// ryd_ket_sched.inc); B has the same bits either way.  The 2 x 2 block's eigenvectors come from
// one Jacobi rotation, exact for a 2 x 2 matrix.
template <bool EIG = false>
__device__ __forceinline__ void ket_blocks_build(KetBlocks& B, double a, double dl, double dt, double d1, double V,
                                                 KetEig* E2 = nullptr, KetEig* E3 = nullptr) {
  B.a = a;
  B.dl = dl;
  B.dt = dt;
  // 2 x 2: exp(-i (c I + M) dt) = e^{-i c dt} (cos(r dt) I - i sin(r dt)/r M), M = [[h, w], [w, -h]]
  {
    const double c = 0.5 * (d1 - dl), h = 0.5 * (d1 + dl), w = 0.5 * a;
    const double r = sqrt(fma(h, h, w * w));
    double sr, cr, sc, cc;
    sincos(r * dt, &sr, &cr);
    sincos(c * dt, &sc, &cc);
    const double snc = r > 0.0 ? sr / r : dt;
    // e^{-i c dt} = cc - i sc times (cr - i snc h, -i snc w, cr + i snc h)
    const double m[3][2] = {{cr, -snc * h}, {0.0, -snc * w}, {cr, snc * h}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      B.u2[k][0] = fma(cc, m[k][0], sc * m[k][1]);
      B.u2[k][1] = fma(cc, m[k][1], -sc * m[k][0]);
    }
    if constexpr (EIG) {
      double A[3][3] = {{d1, w, 0.0}, {w, -dl, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) E2->Q[i][j] = i == j ? 1.0 : 0.0;
      jacobi_rot(A, E2->Q, 0, 1);
      const double lam[3] = {A[0][0], A[1][1], 0.0};
      double er[3] = {1.0, 1.0, 1.0}, ei[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        double sn, cs;
        sincos(lam[k] * dt, &sn, &cs);
        er[k] = cs;
        ei[k] = -sn;
      }
      ket_ctl_phi<2>(*E2, lam, er, ei, dt);
    }
  }
  // 3 x 3 symmetric block: Jacobi (fixed 6 sweeps: quadratic convergence, exact zeros stop)
  {
    const double g = a * 0.70710678118654752440;     // a / sqrt2
    double A[3][3] = {{2.0 * d1, g, 0.0}, {g, d1 - dl, g}, {0.0, g, V - 2.0 * dl}};
    double Ql[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double (&Q)[3][3] = EIG ? E3->Q : Ql;
    if constexpr (EIG) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Q[i][j] = i == j ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < 6; ++sweep) {
      jacobi_rot(A, Q, 0, 1);
      jacobi_rot(A, Q, 0, 2);
      jacobi_rot(A, Q, 1, 2);
    }
    double er[3], ei[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double sn, cs;
      sincos(A[k][k] * dt, &sn, &cs);
      er[k] = cs;
      ei[k] = -sn;
    }
    const int I[6] = {0, 0, 0, 1, 1, 2}, J[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      double re = 0.0, im = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double w = Q[I[e]][k] * Q[J[e]][k];
        re = fma(w, er[k], re);
        im = fma(w, ei[k], im);
      }
      B.u3[e][0] = re;
      B.u3[e][1] = im;
    }
    if constexpr (EIG) {
      const double lam[3] = {A[0][0], A[1][1], A[2][2]};
      ket_ctl_phi<3>(*E3, lam, er, ei, dt);
    }
  }
}

// the segment in polar form: amplitude a >= 0, laser phase (c, sn), detuning, duration
template <int PROTO>
__device__ __forceinline__ void ket_seg_polar(const PointP& q, int s, int n_steps, int shape, double& a, double& c,
                                              double& sn, double& dl, double& dt) {
  const Seg g = segment<PROTO>(q, s, n_steps, shape);
  dl = g.dl;
  dt = g.dt;
  if (PROTO == RYD_PROTO_SMOOTH_JP || PROTO == RYD_PROTO_BANGBANG) {
    a = q.Om;                                  // |Omega e^{i phi}| = Omega (the reference's H)
    c = q.Om > 0.0 ? g.om_re / q.Om : 1.0;
    sn = q.Om > 0.0 ? g.om_im / q.Om : 0.0;
    if (PROTO == RYD_PROTO_BANGBANG && s >= q.nseg) a = 0.0;
  } else if (PROTO == RYD_PROTO_LP_SQUARE && s == 1) {
    // H2 = H(Omega xi): |xi| = 1 (compute_phase_shift_xi) to rounding -> the same real
    // factors as segment 0 (one build, as the Lindblad kernel's frame_ok); other xi as given
    const double m = sqrt(fma(q.xr, q.xr, q.xi * q.xi));
    const bool unit = fabs(m - 1.0) <= 1e-14;
    a = unit ? q.Om : q.Om * m;
    c = unit ? q.xr : (m > 0.0 ? q.xr / m : 1.0);
    sn = unit ? q.xi : (m > 0.0 ? q.xi / m : 0.0);
  } else {
    a = sqrt(fma(g.om_re, g.om_re, g.om_im * g.om_im));
    if (g.om_im == 0.0 && g.om_re >= 0.0) a = g.om_re;   // phase-0 segments: exact amplitude
    c = a > 0.0 ? g.om_re / a : 1.0;
    sn = a > 0.0 ? g.om_im / a : 0.0;
  }
}

#define CMUL_RE(ar, ai, br, bi) fma(ar, br, -(ai) * (bi))
#define CMUL_IM(ar, ai, br, bi) fma(ar, bi, (ai) * (br))

template <int PROTO, int KD>
__global__ __launch_bounds__(BLOCK) void ket_block_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  constexpr bool STATE = true;
#include "ryd_ket_block_body.inc"
}

// the summary-only twin (launch() with a null state pointer)
template <int PROTO, int KD>
__global__ __launch_bounds__(BLOCK) void ket_block_nostate_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  constexpr bool STATE = false;
#include "ryd_ket_block_body.inc"
}
#undef CMUL_RE
#undef CMUL_IM

// ---------------------------------------------------------------------------
// dim 4 (mJ sublevels |r+>, |r->) Lindblad kernel on the 36-dim real sector
// ---------------------------------------------------------------------------
// RG/hamiltonians.py:655-663 (sigma+ drives |1> <-> |r+> only), :741-753 (-Delta on
// both r+-, zeeman_splitting 0), :835-853 (V on every r(+-) r(+-) pair);
// RG/noise_models.py:1253-1295 (decay and losses from both r+-, mJ mixing
// |r-><r+| and |r+><r-| at the same rate gm, dephasing on P_r+ and P_r-), :1415
// (scattering on P_1).  No |r-> coherence is ever created, so the basis inputs
// live in span{e00, e11, e++, ex, ey, e--} per atom.  Single-atom generator rows
// (output) over columns (input):
//   e00: [0, 0,   g0,        0,    0,   g0       ]
//   e11: [0, 0,   g1,        2hy, -2hx, g1       ]
//   e++: [0, 0, -(g0+g1+gm), -2hy, 2hx, gm       ]
//   ex : [0, -hy, hy,       -G,   2hz,  0        ]
//   ey : [0,  hx, -hx,      -2hz, -G,   0        ]
//   e--: [0, 0,   gm,        0,    0, -(g0+g1+gm)]
// G = (g1+g0+gphi+gsc+gm)/2; V P_R (x) P_R with P_R = P_r+ + P_r- gives (V/2)(S (x) D +
// D (x) S), S: e++, e-- -> 2x, ex, ey -> 1x; D: ex -> ey, ey -> -ex.
struct Gen4 {
  double g0, g1, gm, mg, hx, hy, hx2, hy2, hz2, G;
};

__device__ __forceinline__ Gen4 make_gen4(const Seg& g, double d1, const double* r, double gm, double s) {
  Gen4 a;
  const double hx = 0.5 * g.om_re, hy = -0.5 * g.om_im, hz = 0.5 * (d1 + g.dl);
  a.g0 = s * r[1];
  a.g1 = s * r[0];
  a.gm = s * gm;
  a.mg = -s * (r[0] + r[1] + gm);
  a.hx = s * hx;
  a.hy = s * hy;
  a.hx2 = 2.0 * a.hx;
  a.hy2 = 2.0 * a.hy;
  a.hz2 = s * 2.0 * hz;
  a.G = s * 0.5 * (r[0] + r[1] + r[2] + r[3] + gm);
  return a;
}

// o += (M (x) I) b on R[i][j] = b[6i+j] (ST = 6, index i) or (I (x) M) b (ST = 1, index j)
template <int ST>
__device__ __forceinline__ void apply4_one(const Gen4& a, const double (&b)[36], double (&o)[36]) {
  constexpr int OS = ST == 6 ? 1 : 6;      // stride of the other index
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int c = OS * k;
    const double u1 = b[c + ST], u2 = b[c + 2 * ST], u3 = b[c + 3 * ST], u4 = b[c + 4 * ST],
                 u5 = b[c + 5 * ST];
    const double u25 = u2 + u5;
    o[c] = fma(a.g0, u25, o[c]);
    o[c + ST] = fma(a.g1, u25, fma(a.hy2, u3, fma(-a.hx2, u4, o[c + ST])));
    o[c + 2 * ST] = fma(a.mg, u2, fma(-a.hy2, u3, fma(a.hx2, u4, fma(a.gm, u5, o[c + 2 * ST]))));
    o[c + 3 * ST] = fma(a.hy, u2 - u1, fma(-a.G, u3, fma(a.hz2, u4, o[c + 3 * ST])));
    o[c + 4 * ST] = fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o[c + 4 * ST])));
    o[c + 5 * ST] = fma(a.gm, u2, fma(a.mg, u5, o[c + 5 * ST]));
  }
}

__device__ __forceinline__ void apply4_V(double vs, const double (&b)[36], double (&o)[36]) {
#pragma unroll
  for (int i = 2; i < 6; ++i) {            // S (x) D: rows i = ++ / x / y / --
    const double w = (i == 2 || i == 5) ? 2.0 * vs : vs;
    o[6 * i + 4] = fma(w, b[6 * i + 3], o[6 * i + 4]);
    o[6 * i + 3] = fma(-w, b[6 * i + 4], o[6 * i + 3]);
  }
#pragma unroll
  for (int j = 2; j < 6; ++j) {            // D (x) S: columns j
    const double w = (j == 2 || j == 5) ? 2.0 * vs : vs;
    o[6 * 4 + j] = fma(w, b[6 * 3 + j], o[6 * 4 + j]);
    o[6 * 3 + j] = fma(-w, b[6 * 4 + j], o[6 * 3 + j]);
  }
}

template <int PROTO, bool SYM>
__global__ __launch_bounds__(BLOCK) void lindblad4_cheb_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  lindblad_cheb_body<PROTO, SYM, Sector4>(prm, n, ldp, st, lds, sm, ldm, status, n_steps, shape);
}

// ---------------------------------------------------------------------------
// Propagator-squaring kernel (LP square, bang-bang, smooth JP)
// ---------------------------------------------------------------------------
// Per point, U = exp(L dt) on the 25-dim sector is built as
//   (1) U0 = exp(L dt / 2^s): one basis column per lane (25 lanes per point),
//       the same Chebyshev/Miller Clenshaw loop as above on x/2^s <= X_BASE;
//   (2) s squarings U <- U U in LDS; each lane owns a 5x5 output tile
//       (point p, row block rb, col block cb), 625 FMAs and ~200 LDS reads per
//       squaring;
// and the 4 basis-input states (kept in LDS) are advanced by R_k <- U R_k.
// Work per propagator is O(log x) instead of O(x) and about the same for every
// point, which removes the launch's critical-path imbalance.
//
// Phase frame.  Segments that differ only in the laser phase share one
// propagator: with D = exp(i phi (P_r (x) 1 + 1 (x) P_r)), H(Omega e^{i phi}) =
// D H(Omega) D^dag, and every collapse operator of the model maps to a phase
// multiple of itself, so L(Omega e^{i phi}) = Q L(Omega) Q^T where Q = Q1 (x) Q1
// and Q1 rotates the (ex, ey) coordinates by phi (Q1 = [[c, s], [-s, c]]).
// Hence exp(L(Omega e^{i phi}) dt) = Q exp(L(Omega) dt) Q^T exactly:
//   LP square  (RG/simulation.py:728-735): U_gate = Q(xi) U0 Q(xi)^T U0
//   smooth JP  (RG/simulation.py:1698-1731): U_gate = prod_s Q_s U0 Q_s^T,
// one propagator per point instead of 2 (LP) or n_steps (smooth JP).  The
// state update between two matvecs is the rotation Q_{s+1}^T Q_s =
// Q(phi_s - phi_{s+1}).  LP uses the frame only when |xi| = 1 to 1e-14 for the
// whole block (xi from compute_phase_shift_xi always is; an ABI caller may pass
// any xi), otherwise it builds both propagators.
#ifndef RYD_PROP_OCC_SYM
#define RYD_PROP_OCC_SYM 3                  // waves per SIMD for the identical-atom LP-square propagator kernel (168 VGPRs, a few spills; measured C2/C4); other protocols keep 2
#endif
constexpr int PPB = 10;                     // points per 256-lane block (250 lanes used)
constexpr int NC = 25;
// Chebyshev argument after scaling.  Lower means fewer Chebyshev terms and more
// squarings: with the block-triangular symmetric squaring (1875 FMAs, 75 per lane)
// 0.5 is best (C2 0.093 ms vs 0.098 at 2; C3 flat), with the full 25^3 one 3-6 are
// equal (profiles/r01/tune_*).  RYD_X_BASE overrides both.
#ifdef RYD_X_BASE
constexpr double X_BASE_SYM = RYD_X_BASE, X_BASE_FULL = RYD_X_BASE;
#else
constexpr double X_BASE_SYM = 0.5, X_BASE_FULL = 6.0;
#endif

template <int PROTO>
constexpr bool phase_frame_protocol() {
  return PROTO == RYD_PROTO_LP_SQUARE || PROTO == RYD_PROTO_SMOOTH_JP;
}

// (cos, sin) of the laser phase of segment s (the same arithmetic as segment<>)
template <int PROTO>
__device__ __forceinline__ void segment_phase(const PointP& q, int s, int n_steps, double& c, double& sn) {
  if (PROTO == RYD_PROTO_LP_SQUARE) {
    c = s == 0 ? 1.0 : q.xr;
    sn = s == 0 ? 0.0 : q.xi;
  } else {
    const double dt = q.tau / (double)n_steps;
    const double tm = (double)s * dt + dt / 2;
    sincos(q.A * cos(q.wmod * tm - q.phoff), &sn, &c);
  }
}

// Exchange symmetry (identical atoms, SYM): L commutes with the atom swap R -> R^T,
// so in the orthonormal basis {sym_s = (E_ij + E_ji)/sqrt2 (i<j), E_ii ; asym_a =
// (E_ij - E_ji)/sqrt2 (i<j)} the propagator is block-diagonal, U = Us (15x15) (+)
// Ua (10x10).  A squaring then costs 15^3 + 10^3 = 4375 FMAs instead of 25^3.
__host__ __device__ constexpr int asym_index(int i, int j) {     // i < j
  return i * 4 - i * (i - 1) / 2 + (j - i - 1);
}
constexpr double RSQRT2 = 0.70710678118654752440;
constexpr int NS = 15;                       // symmetric coordinates (the 10 antisymmetric are not built)

// Build U = exp(L(g) g.dt) for every point of the block (block-uniform control
// flow; lane (pl, j) computes one Chebyshev column, then one output tile per
// squaring) and return this lane's row j of U (full 25-coordinate form) in u.
// Without SYM, U[p] holds the 25x25 matrix; with SYM its first 325 doubles hold
// Us (15x15, row-major) then Ua (10x10).
// LDS doubles per point for the propagator: the 15x15 symmetric block, or the 25x25 U
template <bool SYM>
constexpr int u_size() { return SYM ? NS * NS : NC * NC; }

template <bool SYM>
__device__ __forceinline__ void build_propagator(double (&U)[PPB][u_size<SYM>()], int& s_max, const PointP& q,
                                                 const Seg& g, bool valid, bool lane_ok, int t, int pl,
                                                 int j, double& nuse, double& nexec, double& nsq,
                                                 bool& over_cap, double (&u)[NC]) {
  double rsum = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) rsum += fabs(q.gA[c]) + fabs(q.gB[c]);
  double emin, emax;
  h_bounds(g, q.V, q.d1, emin, emax);
  const double omega = (emax - emin) + rsum;
  const double x = omega * g.dt;
  const bool capped = valid && !(x <= 1e12);
  const bool active = valid && !capped && x > X_SKIP && lane_ok;
  over_cap = over_cap || capped;
  constexpr double X_BASE = SYM ? X_BASE_SYM : X_BASE_FULL;
  int sq = 0;
  if (active && x > X_BASE) sq = (int)ceil(log2(x / X_BASE));
  const double y = active ? ldexp(x, -sq) : 0.0;
  const double sc = active ? 2.0 / omega : 0.0;
  const Gen A = make_gen(g, q.d1, q.gA, sc);
  const Gen B = make_gen(g, q.d1, q.gB, sc);
  const double vs = sc * 0.5 * q.V;
  // SYM: lane j < 15 starts from sym_j, lane 15 + a from asym_a; else from e_j
  int bi = 0, bj = 0;                       // basis pair (bi <= bj)
  if (SYM) {
    if (j < NS) {
      while (sym_index(bi, 4) < j) ++bi;
      bj = bi + (j - sym_index(bi, bi));
    } else {
      while (bi < 3 && asym_index(bi, 4) < j - NS) ++bi;
      bj = bi + 1 + (j - NS - asym_index(bi, bi + 1));
    }
  }
  const bool is_sym = j < NS;
  const double w0 = SYM ? ((bi == bj) ? 1.0 : RSQRT2) : 1.0;
  const int e1 = SYM ? 5 * bi + bj : j, e2 = SYM ? 5 * bj + bi : j;
  const double w2 = SYM ? (is_sym ? w0 : -w0) : 0.0;
  // (1) column of exp(y Y).  SYM: only the 15 symmetric columns are needed (see the
  // squaring below), and a symmetric column stays symmetric: it runs on the 15-entry
  // upper triangle (apply_Lsym)
  constexpr int NV = SYM ? NS : 25;
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = SYM ? ((e == j) ? w0 : 0.0) : ((e == e1) ? w0 : ((e == e2) ? w2 : 0.0));
  if constexpr (SYM) {
    (void)B;
    cheb_segment<NS>(v, y, active && is_sym,
                     [&](const double (&b)[NS], double (&o)[NS]) { apply_Lsym(A, vs, b, o); }, nuse, nexec);
  } else {
    cheb_segment<25>(v, y, active,
                     [&](const double (&b)[25], double (&o)[25]) { apply_L<SYM>(A, B, vs, b, o); }, nuse,
                     nexec);
  }
  if (t == 0) s_max = 0;
  __syncthreads();
  double* Ub = &U[pl][0];
  if (lane_ok) {
    if constexpr (!SYM) {
#pragma unroll
      for (int r = 0; r < 25; ++r) Ub[r * NC + j] = v[r];
    } else if (is_sym) {                    // Us[s'][j] = <sym_s', v> = sqrt2 R[i2][j2] off the diagonal
#pragma unroll
      for (int i2 = 0; i2 < 5; ++i2)
#pragma unroll
        for (int j2 = i2; j2 < 5; ++j2) {
          const double r = v[sym_index(i2, j2)];
          Ub[sym_index(i2, j2) * NS + j] = (i2 == j2) ? r : RSQRT2 * (r + r);
        }
    }
    // (SYM: the antisymmetric block is not built -- see the squaring below)
    atomicMax(&s_max, sq);
  }
  __syncthreads();
  const int smx = s_max;
  nsq += (double)sq;
  // (2) squarings.  Full: lane owns the 5x5 tile (j/5, j%5) of U U.
  // SYM: the symmetric block is block-triangular, Us = [[B, C], [0, D]] over the
  // coordinates (0, m) (atom A or B in |0><0|: an invariant subspace, the single-atom
  // propagator) and the other 10, so Us^2 = [[B^2, BC + CD], [0, D^2]]: 1875 FMAs,
  // 75 per lane (one B^2 entry, a 1x2 tile of BC + CD, a 2x2 tile of D^2).  The
  // antisymmetric block is never needed: the 4 basis inputs have antisymmetric
  // parts only on the (0, m) coordinates, where the propagator is B again.
  if (SYM) {
    const int rb = j / 5, cb = j % 5;
    const int cc = 5 + 2 * cb, rd = 5 + 2 * rb;
    for (int it = 0; it < smx; ++it) {
      double b2 = 0.0, c2a = 0.0, c2b = 0.0, d00 = 0.0, d01 = 0.0, d10 = 0.0, d11 = 0.0;
      const bool go = lane_ok && it < sq;
      if (go) {
#pragma unroll
        for (int k = 0; k < 5; ++k) b2 = fma(Ub[rb * NS + k], Ub[k * NS + cb], b2);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const double a = Ub[rb * NS + k];
          c2a = fma(a, Ub[k * NS + cc], c2a);
          c2b = fma(a, Ub[k * NS + cc + 1], c2b);
        }
#pragma unroll
        for (int k = 5; k < NS; ++k) {
          const double a0 = Ub[rd * NS + k], a1 = Ub[(rd + 1) * NS + k];
          const double e0 = Ub[k * NS + cc], e1 = Ub[k * NS + cc + 1];
          d00 = fma(a0, e0, d00);
          d01 = fma(a0, e1, d01);
          d10 = fma(a1, e0, d10);
          d11 = fma(a1, e1, d11);
        }
      }
      __syncthreads();
      if (go) {
        Ub[rb * NS + cb] = b2;
        Ub[rb * NS + cc] = c2a;
        Ub[rb * NS + cc + 1] = c2b;
        Ub[rd * NS + cc] = d00;
        Ub[rd * NS + cc + 1] = d01;
        Ub[(rd + 1) * NS + cc] = d10;
        Ub[(rd + 1) * NS + cc + 1] = d11;
      }
      __syncthreads();
    }
  }
  const int ld = NC;
  const int nk = ld;
  const int r0 = 5 * (j / 5);
  const int c0 = 5 * (j % 5);
  const int ncol = 5;
  constexpr int TC = 5;                     // tile columns held per lane
  const double* Mb = Ub;
  for (int it = 0; it < (SYM ? 0 : smx); ++it) {
    double acc[5][TC];
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
      for (int b = 0; b < TC; ++b) acc[a][b] = 0.0;
    if (lane_ok && it < sq) {
#ifdef RYD_SQ_UNROLL
#pragma unroll RYD_SQ_UNROLL
#endif
      for (int k = 0; k < nk; ++k) {
        double ar[5], bc[TC];
#pragma unroll
        for (int a = 0; a < 5; ++a) ar[a] = Mb[(r0 + a) * ld + k];
#pragma unroll
        for (int b = 0; b < TC; ++b) bc[b] = Mb[k * ld + c0 + (b < ncol ? b : ncol - 1)];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
          for (int b = 0; b < TC; ++b) acc[a][b] = fma(ar[a], bc[b], acc[a][b]);
      }
    }
    __syncthreads();
    if (lane_ok && it < sq) {
      double* Mw = Ub;
#pragma unroll
      for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < TC; ++b)
          if (b < ncol) Mw[(r0 + a) * ld + c0 + b] = acc[a][b];
    }
    __syncthreads();
  }
  // (3) this lane's row of U in full coordinates
  if (!SYM) {
#pragma unroll
    for (int m = 0; m < NC; ++m) u[m] = Ub[j * NC + m];
  } else {
    const int ra = j / 5, rb = j % 5;
    const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
    const int sr = sym_index(lo, hi);
    const double* Us = Ub;
#pragma unroll
    for (int m = 0; m < NC; ++m) {
      const int ca = m / 5, cb = m % 5;
      const int clo = ca < cb ? ca : cb, chi = ca < cb ? cb : ca;
      // basis-change weights with (1/sqrt2)^2 taken as exactly 1/2 (RSQRT2 * RSQRT2 is
      // 0.5000000000000001): the symmetric and antisymmetric parts of an entry between
      // the two different invariant subspaces (atom A vs atom B in |0><0|) then cancel
      // to an exact zero instead of a rounding residue
      const double wsym = (ra == rb) ? ((ca == cb) ? 1.0 : RSQRT2) : ((ca == cb) ? RSQRT2 : 0.5);
      const double wanti = (ra == rb || ca == cb) ? 0.0 : (((ra < rb) == (ca < cb)) ? 0.5 : -0.5);
      double val = wsym * Us[sr * NS + sym_index(clo, chi)];
      // antisymmetric part: on the (0, m) coordinates it is the single-atom block B
      // (Ua[(0,hi)][(0,chi)] = Us[(0,hi)][(0,chi)] = Us[hi][chi]); elsewhere the basis
      // inputs never have support, so it is left out
      if (ca != cb && lo == 0 && clo == 0) val = fma(wanti, Us[hi * NS + chi], val);
      u[m] = val;
    }
  }
}

// Row j of U applied to the 4 basis-input states, each summed over its support only:
// |00>: coordinate 0 (e00 (x) e00); |01>: atom A in |0><0| (coordinates 0..4); |10>:
// atom B in |0><0| (0, 5, .., 20); |11>: all 25.  A subspace with an atom in |0><0| is
// invariant (that atom's column of M is zero and V needs both atoms in r), so the
// skipped terms are exact zeros and the sums are bit-identical to the full ones.
__device__ __forceinline__ void update_rows(const double (&u)[NC], const double (&R)[4][NC], double (&nr)[4]) {
  nr[0] = fma(u[0], R[0][0], 0.0);
  nr[1] = nr[2] = nr[3] = 0.0;
#pragma unroll
  for (int m = 0; m < 5; ++m) nr[1] = fma(u[m], R[1][m], nr[1]);
#pragma unroll
  for (int a = 0; a < 5; ++a) nr[2] = fma(u[5 * a], R[2][5 * a], nr[2]);
#pragma unroll
  for (int m = 0; m < NC; ++m) nr[3] = fma(u[m], R[3][m], nr[3]);
}

// update_rows with the row rotated first: o = (Q1 (x) Q1)^T u for a propagator row u,
// so that o . R = u . (Q R) -- the frame rotation of rotate_coord moved onto the lane's
// own row (registers only).  Q1 mixes the (ex, ey) coordinates 3, 4: rows [c s; -s c]
// (t: the atom-A index pass, then the atom-B pass).  The rotated row is produced one
// atom-A index a at a time and consumed at once (ascending coordinate order), so the 25
// rotated coefficients are never live together.
__device__ __forceinline__ void update_rows_rot(const double (&u)[NC], double c, double s,
                                                const double (&R)[4][NC], double (&nr)[4]) {
  nr[0] = nr[1] = nr[2] = nr[3] = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    double t[5], o[5];
#pragma unroll
    for (int b = 0; b < 5; ++b)
      t[b] = a < 3 ? u[5 * a + b]
                   : (a == 3 ? fma(c, u[15 + b], -s * u[20 + b]) : fma(s, u[15 + b], c * u[20 + b]));
    o[0] = t[0];
    o[1] = t[1];
    o[2] = t[2];
    o[3] = fma(c, t[3], -s * t[4]);
    o[4] = fma(s, t[3], c * t[4]);
    if (a == 0) {
      nr[0] = fma(o[0], R[0][0], 0.0);
#pragma unroll
      for (int b = 0; b < 5; ++b) nr[1] = fma(o[b], R[1][b], nr[1]);
    }
    nr[2] = fma(o[0], R[2][5 * a], nr[2]);
#pragma unroll
    for (int b = 0; b < 5; ++b) nr[3] = fma(o[b], R[3][5 * a + b], nr[3]);
  }
}

// One basis input only: sum_m o[m] R[m] with o the rotated row (the nr[3] chain of
// update_rows_rot; with u zero outside an input's support the extra terms are exact zeros).
__device__ __forceinline__ double update_row_rot(const double (&u)[NC], double c, double s,
                                                 const double* __restrict__ R) {
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    double t[5];
#pragma unroll
    for (int b = 0; b < 5; ++b)
      t[b] = a < 3 ? u[5 * a + b]
                   : (a == 3 ? fma(c, u[15 + b], -s * u[20 + b]) : fma(s, u[15 + b], c * u[20 + b]));
    acc = fma(t[0], R[5 * a], acc);
    acc = fma(t[1], R[5 * a + 1], acc);
    acc = fma(t[2], R[5 * a + 2], acc);
    acc = fma(fma(c, t[3], -s * t[4]), R[5 * a + 3], acc);
    acc = fma(fma(s, t[3], c * t[4]), R[5 * a + 4], acc);
  }
  return acc;
}

// dst_k[j] = (Q(c,s) R_k)[j] for this lane's coordinate j = 5a + b, Q = Q1 (x) Q1:
// coordinate 3 -> c r3 + s r4, coordinate 4 -> -s r3 + c r4 on each atom index.
__device__ __forceinline__ void rotate_coord(const double (&src)[4][NC], double (&dst)[4][NC], int j,
                                            double c, double s) {
  const int a = j / 5, b = j % 5;
  const int a0 = a < 3 ? a : 3, b0 = b < 3 ? b : 3;
  // weights of (a0, a0+1) and (b0, b0+1); non-rotating indices use (1, 0)
  const double wa0 = a < 3 ? 1.0 : (a == 3 ? c : -s), wa1 = a < 3 ? 0.0 : (a == 3 ? s : c);
  const double wb0 = b < 3 ? 1.0 : (b == 3 ? c : -s), wb1 = b < 3 ? 0.0 : (b == 3 ? s : c);
  const int a1 = a < 3 ? a0 : a0 + 1, b1 = b < 3 ? b0 : b0 + 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double r00 = src[k][5 * a0 + b0], r01 = src[k][5 * a0 + b1];
    const double r10 = src[k][5 * a1 + b0], r11 = src[k][5 * a1 + b1];
    dst[k][j] = wa0 * (wb0 * r00 + wb1 * r01) + wa1 * (wb0 * r10 + wb1 * r11);
  }
}

template <int PROTO, bool SYM>
__global__ __launch_bounds__(BLOCK, (SYM && PROTO == RYD_PROTO_LP_SQUARE) ? RYD_PROP_OCC_SYM : 2) void lindblad_prop_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  __shared__ __attribute__((aligned(16))) double U[PPB][u_size<SYM>()];   // per point: Us (SYM) or row-major U
  __shared__ __attribute__((aligned(16))) double Rs[PPB][4][NC];    // basis-input states
  __shared__ __attribute__((aligned(16))) double Rt[PPB][4][NC];    // rotated states (frame path)
  __shared__ int s_max;

  const int t = threadIdx.x;
  const bool lane_ok = t < PPB * NC;
  const int pl = lane_ok ? t / NC : 0;     // point within block
  const int j = t % NC;                    // column (phase 1) / tile id (phase 2) / coordinate
  const int64_t ip = (int64_t)blockIdx.x * PPB + pl;
  const bool live = lane_ok && ip < n;
  const int64_t i = ip < n ? ip : n - 1;
  bool valid, frame_ok;
  {
    const PointP q0 = load_point<PROTO>(prm, ldp, i);
    valid = point_valid<PROTO>(q0, n_steps);
    frame_ok = !(PROTO == RYD_PROTO_LP_SQUARE) || !valid ||
               fabs(q0.xr * q0.xr + q0.xi * q0.xi - 1.0) <= 1e-14;
  }

  for (int e = t; e < PPB * 4 * NC; e += BLOCK) {
    const int p = e / (4 * NC), k = (e / NC) % 4, r = e % NC;
    const int e0 = 5 * (k >> 1) + (k & 1);
    Rs[p][k][r] = (r == e0) ? 1.0 : 0.0;
  }
  double nuse = 0.0, nexec = 0.0, nsq = 0.0;
  bool over_cap = false;
  const int nseg = n_segments<PROTO>(n_steps);
  const bool use_frame = phase_frame_protocol<PROTO>() && __syncthreads_and(frame_ok || !lane_ok);

  // one propagator per segment, or a single phase-0 propagator in the frame path;
  // u = this lane's row of the latest propagator
  double u[NC];
  const int nprop = use_frame ? 1 : nseg;
  for (int s = 0; s < nprop; ++s) {
    // re-read this point's scalars every segment (L1/L2 hits) instead of keeping
    // them live across the loop: the Chebyshev phase needs the VGPRs
    const double* pp = prm;
    asm volatile("" : "+s"(pp));
    const PointP q = load_point<PROTO>(pp, ldp, i);
    Seg g = segment<PROTO>(q, s, n_steps, shape);
    if (use_frame) {                         // reference frame: phase 0
      g.om_re = q.Om;
      g.om_im = 0.0;
    }
    build_propagator<SYM>(U, s_max, q, g, valid, lane_ok, t, pl, j, nuse, nexec, nsq, over_cap, u);
    if (!use_frame) {
      // R_k <- U R_k ; lane (pl, r = j) computes row r for the 4 inputs
      double nr[4] = {0.0, 0.0, 0.0, 0.0};
      if (lane_ok) update_rows(u, Rs[pl], nr);
      __syncthreads();
      if (lane_ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) Rs[pl][k][j] = nr[k];
      }
      __syncthreads();
    }
  }

  if (use_frame) {
    // U0 row j stays in registers for every segment
    double cp = 1.0, sp = 0.0;               // phase of the frame R is currently in
    // Smooth JP: the (cos, sin) of every segment's phase (a cos and a sincos in fp64)
    // is computed once per (point, segment) by the whole block into a table that
    // reuses U's LDS (free now: each lane holds its row) instead of redundantly by
    // the point's 25 lanes every segment; same arithmetic, so the same bits.
    constexpr bool TAB = PROTO == RYD_PROTO_SMOOTH_JP;
    constexpr int CH = u_size<SYM>() / 2;    // segments per table chunk (112 SYM, 312)
    static_assert(2 * CH <= u_size<SYM>(), "phase table must fit in U");
    double* ph = &U[0][0];                   // ph[(p * CH + s % CH) * 2 + {0: cos, 1: sin}]
    for (int s = 0; s < nseg; ++s) {
      double c, sn;
      if (TAB) {
        if (s % CH == 0) {
          const int len = nseg - s < CH ? nseg - s : CH;
          __syncthreads();                   // U rows / the previous chunk fully read
          for (int e = t; e < PPB * len; e += BLOCK) {
            const int p = e / len, sl = e % len;
            const int64_t ie = (int64_t)blockIdx.x * PPB + p;
            const PointP qe = load_point<PROTO>(prm, ldp, ie < n ? ie : n - 1);
            double ce, se;
            segment_phase<PROTO>(qe, s + sl, n_steps, ce, se);
            ph[(p * CH + sl) * 2] = ce;
            ph[(p * CH + sl) * 2 + 1] = se;
          }
          __syncthreads();
        }
        c = ph[(pl * CH + s % CH) * 2];
        sn = ph[(pl * CH + s % CH) * 2 + 1];
      } else {
        const double* pp = prm;
        asm volatile("" : "+s"(pp));
        const PointP q = load_point<PROTO>(pp, ldp, i);
        segment_phase<PROTO>(q, s, n_steps, c, sn);
      }
      // into this segment's frame, Q_s^T Q_{s-1} = Q(phi_{s-1} - phi_s), folded into
      // the lane's row; the states ping-pong between Rs and Rt (one barrier a segment)
      const double cr = cp * c + sp * sn, sr = sp * c - cp * sn;
      if (lane_ok) {
        double nr[4];
        if ((s & 1) == 0) {
          update_rows_rot(u, cr, sr, Rs[pl], nr);
#pragma unroll
          for (int k = 0; k < 4; ++k) Rt[pl][k][j] = nr[k];
        } else {
          update_rows_rot(u, cr, sr, Rt[pl], nr);
#pragma unroll
          for (int k = 0; k < 4; ++k) Rs[pl][k][j] = nr[k];
        }
      }
      __syncthreads();
      cp = c;
      sp = sn;
    }
    // back to the lab frame: Q_{N-1}; the result ends in Rs
    const bool in_t = (nseg & 1) != 0;       // the latest state is in Rt
    if (lane_ok) {
      if (in_t) rotate_coord(Rt[pl], Rs[pl], j, cp, sp);
      else rotate_coord(Rs[pl], Rt[pl], j, cp, sp);
    }
    __syncthreads();
    if (!in_t && lane_ok) {
#pragma unroll
      for (int k = 0; k < 4; ++k) Rs[pl][k][j] = Rt[pl][k][j];
    }
    __syncthreads();
  }

  // outputs: state rows st[e][4*i + k] (staged through LDS, coalesced over 40 lanes/row)
  const int64_t i0 = (int64_t)blockIdx.x * PPB;
  for (int e = t; e < NC * PPB * 4; e += BLOCK) {
    const int r = e / (PPB * 4), c = e % (PPB * 4);
    const int p = c / 4, k = c % 4;
    if (i0 + p < n) st[(int64_t)r * lds + 4 * i0 + c] = Rs[p][k][r];
  }
  uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
  if (over_cap) stat |= RYD_STATUS_STEP_CAP;
  if (live && j == 0) {
    double pops[4], tr11 = 0.0;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e0 = 5 * (k >> 1) + (k & 1);
      pops[k] = Rs[pl][k][e0];
    }
    for (int r = 0; r < NC; ++r)
      for (int k = 0; k < 4; ++k) fin = fin && isfinite(Rs[pl][k][r]);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) tr11 += Rs[pl][3][5 * a + b];
    if (!fin) stat |= RYD_STATUS_NONFINITE;
    const double nan = __builtin_nan("");
    const double avg = 0.25 * (pops[0] + pops[1] + pops[2] + pops[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sm[(int64_t)(RYD_S_POP0 + k) * ldm + i] = pops[k];
      sm[(int64_t)(RYD_S_OV_RE0 + k) * ldm + i] = nan;
      sm[(int64_t)(RYD_S_OV_IM0 + k) * ldm + i] = nan;
    }
    sm[(int64_t)RYD_S_AVG_POP * ldm + i] = avg;
    sm[(int64_t)RYD_S_CTRL_PHASE * ldm + i] = nan;
    sm[(int64_t)RYD_S_PENALTY * ldm + i] = nan;
    sm[(int64_t)RYD_S_AVG_F * ldm + i] = avg;
    sm[(int64_t)RYD_S_NMV_USEFUL * ldm + i] = (SYM ? NS : NC) * nuse;   // basis columns per point
    sm[(int64_t)RYD_S_NMV_EXEC * ldm + i] = NC * nexec;
    sm[(int64_t)RYD_S_TRACE11 * ldm + i] = tr11;
    sm[(int64_t)RYD_S_NSQUARE * ldm + i] = nsq;
    status[i] = stat;
  }
}

// ---------------------------------------------------------------------------
// Smooth JP in two launches (many segments, one propagator)
// ---------------------------------------------------------------------------
// The fused kernel above runs smooth JP's 300 frame-rotated state updates at the
// occupancy its propagator build needs (255 VGPRs, 66 KB LDS: 2 waves per SIMD) and
// with a block barrier per segment, because its 25-lane points straddle waves.
// Split: jp_rows_kernel builds the phase-0 propagator (build_propagator, as above)
// and writes each lane's row to a workspace; jp_frame_kernel walks the segments with
// two points per wave (32 lanes each, 25 used), so every exchange is wave-local (no
// s_barrier), 21 KB LDS per block.  Same operands and operation order as the fused
// path (identical atoms: its terms that are exact zeros skipped), same bits.
constexpr int FPW = 2;                       // points per wave (frame kernel)
constexpr int FPB = FPW * (BLOCK / 64);      // 8 points per block
constexpr int FCH = 64;                      // segments per wave-local phase-table chunk

// LDS exchange among the lanes of one wave: a wave's LDS operations complete in
// order, so ordering the compiler is all that is needed (no s_barrier).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// W[m][25 i + j] = row j, column m of point i's phase-0 segment propagator
template <bool SYM>
__global__ __launch_bounds__(BLOCK, 2) void jp_rows_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ W,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape) {
  constexpr int PROTO = RYD_PROTO_SMOOTH_JP;
  __shared__ __attribute__((aligned(16))) double U[PPB][u_size<SYM>()];
  __shared__ int s_max;
  const int t = threadIdx.x;
  const bool lane_ok = t < PPB * NC;
  const int pl = lane_ok ? t / NC : 0;
  const int j = t % NC;
  const int64_t ip = (int64_t)blockIdx.x * PPB + pl;
  const bool live = lane_ok && ip < n;
  const int64_t i = ip < n ? ip : n - 1;
  const PointP q = load_point<PROTO>(prm, ldp, i);
  const bool valid = point_valid<PROTO>(q, n_steps);
  double nuse = 0.0, nexec = 0.0, nsq = 0.0;
  bool over_cap = false;
  Seg g = segment<PROTO>(q, 0, n_steps, shape);
  g.om_re = q.Om;                            // reference frame: phase 0
  g.om_im = 0.0;
  double u[NC];
  build_propagator<SYM>(U, s_max, q, g, valid, lane_ok, t, pl, j, nuse, nexec, nsq, over_cap, u);
  if (live) {
    const int64_t ld = (int64_t)NC * n;
#pragma unroll
    for (int m = 0; m < NC; ++m) W[m * ld + NC * i + j] = u[m];
  }
  if (live && j == 0) {
    uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
    if (over_cap) stat |= RYD_STATUS_STEP_CAP;
    status[i] = stat;
    sm[(int64_t)RYD_S_NMV_USEFUL * ldm + i] = (SYM ? NS : NC) * nuse;
    sm[(int64_t)RYD_S_NMV_EXEC * ldm + i] = NC * nexec;
    sm[(int64_t)RYD_S_NSQUARE * ldm + i] = nsq;
  }
}

// Identical atoms (SYM): each 32-lane half is one point with one output per lane --
// lanes 0..24 |11><11| row j (reads R_11), 25..29 |01><01| row j-25 (reads R_01, row
// zeroed outside (0, m)), 30 |00><00| (row 0, column 0) -- 25 products a lane instead
// of 36.  |10><10| is the atom-swap mirror of |01><01| (U[5a][5b] and U[a][b] come
// from the same symmetric-block expression, the row rotation acts on the same index
// pair), so lane 25 + r writes it too.  Entries of U between the two invariant
// subspaces are exact zeros (build_propagator step 3), so this equals the fused
// kernel's full sums bit for bit (tests/test_gpu_c3.py).
template <int OCC, bool SYM>                 // OCC: waves per SIMD the register budget targets
__global__ __launch_bounds__(BLOCK, OCC) void jp_frame_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, const double* __restrict__ W,
    double* __restrict__ st, int64_t lds, double* __restrict__ sm, int64_t ldm,
    uint32_t* __restrict__ status, int n_steps) {
  constexpr int PROTO = RYD_PROTO_SMOOTH_JP;
  __shared__ __attribute__((aligned(16))) double Rs[FPB][4][NC];
  __shared__ __attribute__((aligned(16))) double Rt[FPB][4][NC];
  __shared__ __attribute__((aligned(16))) double ph[FPB][FCH][2];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int j = l & 31;
  const int pl = FPW * w + (l >> 5);
  const bool lane_ok = j < NC;
  const bool role_ok = SYM ? j < 31 : lane_ok;   // lanes that own an update output
  const int row = j < NC ? j : (j < 30 ? j - NC : 0);
  const int ksrc = j < NC ? 3 : (j < 30 ? 1 : 0);
  const int64_t ip = (int64_t)blockIdx.x * FPB + pl;
  const bool live = lane_ok && ip < n;
  const int64_t i = ip < n ? ip : n - 1;
  double u[NC];
  {
    const int64_t ld = (int64_t)NC * n;
    const int mmax = (!SYM || j < NC) ? NC : (j < 30 ? 5 : (j == 30 ? 1 : 0));
#pragma unroll
    for (int m = 0; m < NC; ++m) u[m] = m < mmax ? W[m * ld + NC * i + row] : 0.0;
  }
  for (int e = l; e < FPW * 4 * NC; e += 64) {
    const int p = FPW * w + e / (4 * NC), k = (e / NC) % 4, r = e % NC;
    const int e0 = 5 * (k >> 1) + (k & 1);
    Rs[p][k][r] = (r == e0) ? 1.0 : 0.0;
    Rt[p][k][r] = 0.0;                       // coordinates outside a support stay zero
  }
  wave_sync();
  const int nseg = n_segments<PROTO>(n_steps);
  double cp = 1.0, sp = 0.0;                 // phase of the frame R is currently in
  for (int s = 0; s < nseg; ++s) {
    if (s % FCH == 0) {                      // this wave's two points, next FCH segments
      const int len = nseg - s < FCH ? nseg - s : FCH;
      for (int e = l; e < FPW * len; e += 64) {
        const int p = e / len, sl = e % len;
        const int64_t ie = (int64_t)blockIdx.x * FPB + FPW * w + p;
        const PointP qe = load_point<PROTO>(prm, ldp, ie < n ? ie : n - 1);
        double ce, se;
        segment_phase<PROTO>(qe, s + sl, n_steps, ce, se);
        ph[FPW * w + p][sl][0] = ce;
        ph[FPW * w + p][sl][1] = se;
      }
      wave_sync();
    }
    const double c = ph[pl][s % FCH][0], sn = ph[pl][s % FCH][1];
    const double cr = cp * c + sp * sn, sr = sp * c - cp * sn;
    if (role_ok) {
      double (&Rsrc)[4][NC] = (s & 1) == 0 ? Rs[pl] : Rt[pl];
      double (&Rdst)[4][NC] = (s & 1) == 0 ? Rt[pl] : Rs[pl];
      if (SYM) {
        const double v = update_row_rot(u, cr, sr, Rsrc[ksrc]);
        if (j < NC) {
          Rdst[3][j] = v;
        } else if (j < 30) {
          Rdst[1][row] = v;
          Rdst[2][5 * row] = v;
        } else {
          Rdst[0][0] = v;
        }
      } else {
        double nr[4];
        update_rows_rot(u, cr, sr, Rsrc, nr);
#pragma unroll
        for (int k = 0; k < 4; ++k) Rdst[k][j] = nr[k];
      }
    }
    wave_sync();
    cp = c;
    sp = sn;
  }
  // back to the lab frame: Q_{N-1}; the result ends in Rs
  const bool in_t = (nseg & 1) != 0;
  if (lane_ok) {
    if (in_t) rotate_coord(Rt[pl], Rs[pl], j, cp, sp);
    else rotate_coord(Rs[pl], Rt[pl], j, cp, sp);
  }
  wave_sync();
  if (!in_t && lane_ok) {
#pragma unroll
    for (int k = 0; k < 4; ++k) Rs[pl][k][j] = Rt[pl][k][j];
  }
  wave_sync();
  if (live) {
#pragma unroll
    for (int k = 0; k < 4; ++k) st[(int64_t)j * lds + 4 * i + k] = Rs[pl][k][j];
  }
  if (live && j == 0) {
    uint32_t stat = status[i];               // BAD_INPUT / STEP_CAP from jp_rows_kernel
    double pops[4], tr11 = 0.0;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) pops[k] = Rs[pl][k][5 * (k >> 1) + (k & 1)];
    for (int r = 0; r < NC; ++r)
      for (int k = 0; k < 4; ++k) fin = fin && isfinite(Rs[pl][k][r]);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) tr11 += Rs[pl][3][5 * a + b];
    if (!fin) stat |= RYD_STATUS_NONFINITE;
    const double nan = __builtin_nan("");
    const double avg = 0.25 * (pops[0] + pops[1] + pops[2] + pops[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sm[(int64_t)(RYD_S_POP0 + k) * ldm + i] = pops[k];
      sm[(int64_t)(RYD_S_OV_RE0 + k) * ldm + i] = nan;
      sm[(int64_t)(RYD_S_OV_IM0 + k) * ldm + i] = nan;
    }
    sm[(int64_t)RYD_S_AVG_POP * ldm + i] = avg;
    sm[(int64_t)RYD_S_CTRL_PHASE * ldm + i] = nan;
    sm[(int64_t)RYD_S_PENALTY * ldm + i] = nan;
    sm[(int64_t)RYD_S_AVG_F * ldm + i] = avg;
    sm[(int64_t)RYD_S_TRACE11 * ldm + i] = tr11;
    status[i] = stat;
  }
}

#ifndef RYD_S16_WAVES
#define RYD_S16_WAVES 4                      // waves per SIMD the sym16 register budget targets (LP: 128 VGPRs, no scratch)
#endif
#ifndef RYD_LP_UNSQUARED
#define RYD_LP_UNSQUARED 2                   // LP square, identical atoms: squaring levels left to the states
#endif
#include "ryd_sym16.inc"
#ifdef RYD_S16_BAL_TU
// ryd_sym16_bal.hip, the balanced sym16 kernels' own translation unit, takes this file up to
// here: the device code those kernels are made of, and nothing that would emit another kernel
}  // namespace
#else
// custom pulse schedules on the same row layout: the table reader, then ryd_run_schedule
#include "ryd_sched_table.inc"
#include "ryd_sched16.inc"
// the same tables as kets, with the overlaps' phase gradients (ryd_run_schedule_kets)
#include "ryd_ket_sched.inc"

// ---------------------------------------------------------------------------
// Adaptive Dormand-Prince 5(4) kernel (RYD_METHOD_DOPRI5)
// ---------------------------------------------------------------------------
// The error-controlled stepper the north star names, fused in-kernel: one lane
// per (point, basis input).  The state y, the stage input, the RHS output and the
// error accumulator live in VGPRs; the stage derivatives k1..k6 are staged in LDS
// (one private column per lane, [stage][coord][lane] so a wave's accesses are
// conflict-free, no barriers needed).  FSAL, weighted-RMS error control as
// ZVODE/QuTiP (atol + rtol*max|y|), exact stops at the reference's segment
// boundaries, a step cap per segment (mesolve's nsteps, RG/simulation.py:687)
// -> status bit.  It needs ~15x the generator applications of the Chebyshev
// propagator at 1e-10 accuracy (V*dt ~ 1e3 rad per pulse); it is kept as an
// independent cross-check and as the reference-style comparison point.
constexpr int DP_BLOCK = 64;

__device__ __forceinline__ void lindblad_rhs(const Gen& A, const Gen& B, double vs,
                                             const double (&y)[25], double (&f)[25]) {
#pragma unroll
  for (int e = 0; e < 25; ++e) f[e] = 0.0;
  apply_A(A, y, f);
  apply_B(B, y, f);
  apply_V(vs, y, f);
}

// Dormand & Prince (1980) tableau
struct DP {
  static constexpr double a[6][5] = {
      {0, 0, 0, 0, 0},
      {1.0 / 5, 0, 0, 0, 0},
      {3.0 / 40, 9.0 / 40, 0, 0, 0},
      {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
      {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
      {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
  static constexpr double b[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
  static constexpr double e[6] = {71.0 / 57600, 0, -71.0 / 16695, 71.0 / 1920, -17253.0 / 339200,
                                  22.0 / 525};
  static constexpr double e7 = -1.0 / 40;
};

using KStore = double[6][25][DP_BLOCK];

// tmp = y + hh * sum_{l<J} a[J][l] k_l   (k_l from this lane's LDS column)
template <int J>
__device__ __forceinline__ void dp_stage_input(const double (&y)[25], double hh, const KStore& ks, int lt,
                                               double (&tmp)[25]) {
#pragma unroll
  for (int e = 0; e < 25; ++e) {
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) acc = fma(DP::a[J][l], ks[l][e][lt], acc);
    tmp[e] = fma(hh, acc, y[e]);
  }
}

template <int PROTO>
__global__ __launch_bounds__(DP_BLOCK) void lindblad_dopri5_kernel(
    const double* __restrict__ prm, int64_t n, int64_t ldp, double* __restrict__ st, int64_t lds,
    double* __restrict__ sm, int64_t ldm, uint32_t* __restrict__ status, int n_steps, int shape,
    double rtol, double atol, int64_t max_steps) {
  __shared__ KStore ks;                       // 6*25*64*8 = 75 KB
  const int lt = threadIdx.x;
  const int64_t gid = (int64_t)blockIdx.x * DP_BLOCK + lt;
  const bool live = gid < 4 * n;
  const int64_t i = live ? (gid >> 2) : (n - 1);
  const int inp = (int)(gid & 3);
  const int a1 = inp >> 1, a2 = inp & 1;
  const PointP q = load_point<PROTO>(prm, ldp, i);
  const bool valid = point_valid<PROTO>(q, n_steps);
  const int e0 = 5 * a1 + a2;
  double y[25];
#pragma unroll
  for (int e = 0; e < 25; ++e) y[e] = (e == e0) ? 1.0 : 0.0;
  double nrhs = 0.0;
  bool capped = false;
  const int nseg = n_segments<PROTO>(n_steps);
  double rsum = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) rsum += fabs(q.gA[c]) + fabs(q.gB[c]);
  double h = 0.0;
#pragma unroll 1
  for (int s = 0; s < nseg; ++s) {
    const Seg g = segment<PROTO>(q, s, n_steps, shape);
    double emin, emax;
    h_bounds(g, q.V, q.d1, emin, emax);
    const double omega = (emax - emin) + rsum;
    const bool active = valid && g.dt > 0.0 && omega * g.dt > X_SKIP;
    const Gen A = make_gen(g, q.d1, q.gA, 1.0);
    const Gen B = make_gen(g, q.d1, q.gB, 1.0);
    const double vs = 0.5 * q.V;
    double f[25], tmp[25];
    lindblad_rhs(A, B, vs, y, f);             // fresh k1 at every segment start (new H)
#pragma unroll
    for (int e = 0; e < 25; ++e) ks[0][e][lt] = f[e];
    nrhs += 1.0;
    double t = 0.0;
    if (h <= 0.0) h = 0.5 / omega;            // |h lambda| ~ 0.5 start
    int64_t nst = 0;
    bool done = !active;
    while (__any(!done)) {
      if (!done) {
        const double hh = fmin(h, g.dt - t);
        dp_stage_input<1>(y, hh, ks, lt, tmp);
        lindblad_rhs(A, B, vs, tmp, f);
#pragma unroll
        for (int e = 0; e < 25; ++e) ks[1][e][lt] = f[e];
        dp_stage_input<2>(y, hh, ks, lt, tmp);
        lindblad_rhs(A, B, vs, tmp, f);
#pragma unroll
        for (int e = 0; e < 25; ++e) ks[2][e][lt] = f[e];
        dp_stage_input<3>(y, hh, ks, lt, tmp);
        lindblad_rhs(A, B, vs, tmp, f);
#pragma unroll
        for (int e = 0; e < 25; ++e) ks[3][e][lt] = f[e];
        dp_stage_input<4>(y, hh, ks, lt, tmp);
        lindblad_rhs(A, B, vs, tmp, f);
#pragma unroll
        for (int e = 0; e < 25; ++e) ks[4][e][lt] = f[e];
        dp_stage_input<5>(y, hh, ks, lt, tmp);
        lindblad_rhs(A, B, vs, tmp, f);      // f = k6
#pragma unroll
        for (int e = 0; e < 25; ++e) {
          ks[5][e][lt] = f[e];
          tmp[e] = y[e] + hh * (DP::b[0] * ks[0][e][lt] + DP::b[2] * ks[2][e][lt] + DP::b[3] * ks[3][e][lt] +
                                DP::b[4] * ks[4][e][lt] + DP::b[5] * f[e]);
        }
        lindblad_rhs(A, B, vs, tmp, f);      // f = k7 = f(y_new)
        nrhs += 6.0;
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < 25; ++e) {
          const double ee = hh * (DP::e[0] * ks[0][e][lt] + DP::e[2] * ks[2][e][lt] + DP::e[3] * ks[3][e][lt] +
                                  DP::e[4] * ks[4][e][lt] + DP::e[5] * ks[5][e][lt] + DP::e7 * f[e]);
          const double sc = atol + rtol * fmax(fabs(y[e]), fabs(tmp[e]));
          const double r = ee / sc;
          acc = fma(r, r, acc);
        }
        const double err = sqrt(acc / 25.0);
        const bool ok = err <= 1.0 && isfinite(err);
        if (ok) {
#pragma unroll
          for (int e = 0; e < 25; ++e) {
            y[e] = tmp[e];
            ks[0][e][lt] = f[e];               // FSAL
          }
          const double rem = g.dt - t;
          t += hh;
          if (hh >= rem) done = true;          // that was the step to the segment end
        }
        double fac = isfinite(err) ? 0.9 * pow(fmax(err, 1e-10), -0.2) : 0.2;
        fac = fmin(5.0, fmax(0.2, fac));
        if (!ok) fac = fmin(fac, 1.0);
        h = hh * fac;
        if (t >= g.dt) done = true;
        if (++nst > max_steps) {
          capped = true;
          done = true;
        }
      }
    }
  }
  double pop = 0.0;
#pragma unroll
  for (int e = 0; e < 25; ++e) pop = (e == e0) ? y[e] : pop;
  double tr = 0.0;
#pragma unroll
  for (int ii = 0; ii < 3; ++ii)
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) tr += y[5 * ii + jj];
  uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
  if (capped) stat |= RYD_STATUS_STEP_CAP;
  if (!finite_all(y, 25)) stat |= RYD_STATUS_NONFINITE;
  if (live) {
#pragma unroll
    for (int e = 0; e < 25; ++e) st[(int64_t)e * lds + gid] = y[e];
  }
  const int lane = threadIdx.x & 63, base = lane & ~3;
  double p[4], nr[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    p[x] = lane_get(pop, base + x);
    nr[x] = lane_get(nrhs, base + x);
  }
  const double tr11 = lane_get(tr, base + 3);
  uint32_t st_all = stat;
#pragma unroll
  for (int x = 1; x < 4; ++x) st_all |= (uint32_t)__shfl((int)stat, base + x, 64);
  if (live && inp == 0) {
    const double avg = 0.25 * (p[0] + p[1] + p[2] + p[3]);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      sm[(int64_t)(RYD_S_POP0 + x) * ldm + i] = p[x];
      sm[(int64_t)(RYD_S_OV_RE0 + x) * ldm + i] = nan;
      sm[(int64_t)(RYD_S_OV_IM0 + x) * ldm + i] = nan;
    }
    sm[(int64_t)RYD_S_AVG_POP * ldm + i] = avg;
    sm[(int64_t)RYD_S_CTRL_PHASE * ldm + i] = nan;
    sm[(int64_t)RYD_S_PENALTY * ldm + i] = nan;
    sm[(int64_t)RYD_S_AVG_F * ldm + i] = avg;
    sm[(int64_t)RYD_S_NMV_USEFUL * ldm + i] = nr[0] + nr[1] + nr[2] + nr[3];   // RHS evaluations
    sm[(int64_t)RYD_S_NMV_EXEC * ldm + i] = nr[0] + nr[1] + nr[2] + nr[3];
    sm[(int64_t)RYD_S_TRACE11 * ldm + i] = tr11;
    sm[(int64_t)RYD_S_NSQUARE * ldm + i] = 0.0;
    status[i] = st_all;
  }
}

// ---------------------------------------------------------------------------
// Coherence sectors of the qubit process map
// ---------------------------------------------------------------------------
// Single-atom operators |i><j| carry q = n(i) - n(j), n(0) = 0, n(1) = n(r) = 1.
// H and every collapse channel conserve q, so the 16 qubit matrix units evolve in
// small invariant sectors of the two-atom operator space (C[alpha][beta] below,
// alpha over atom A's sector basis, beta over atom B's):
//   (0,0)   |x><x|               real 25-dim sector: the kernels above
//   KIND 0 (0,-1)  |00><01|, |10><11|   A: q=0 {e00,e11,err,ex,ey}, B: q=-1 {|0><1|, |0><r|}
//   KIND 1 (-1,0)  |00><10|, |01><11|   mirror
//   KIND 2 (-1,-1) |00><11|             A, B: q=-1
//   KIND 3 (-1,+1) |01><10|             A: q=-1, B: q=+1 {|1><0|, |r><0|}; V drops out
// q=0 block: the real single-atom M above, acting on complex coefficients.
// q=-1 block: d/dt (c01, c0r) = [[i d1 - gs/2, i Om/2], [i Om*/2, -i Delta - (g0+g1+gphi)/2]]
// q=+1 block: its complex conjugate.  V term (V/2)(S (x) D + D (x) S) with S = diag(0,1)
// and D = +-i diag(0,1) on q = -+1 (S, D on q=0 as in apply_V).  The other 6 matrix
// units are adjoints of these.  Verified against the column-stacked 81x81 Liouvillian
// (tests/test_gpu_process_map.py).
struct CGen {                  // scaled complex 2x2 block
  double m00r, m00i, m01r, m01i, m10r, m10i, m11r, m11i;
};

__device__ __forceinline__ CGen make_cgen(const Seg& g, double d1, const double* r, double s, bool conj) {
  CGen c;
  const double sg = conj ? -1.0 : 1.0;
  c.m00r = -0.5 * s * r[3];
  c.m00i = sg * s * d1;
  c.m01r = -0.5 * s * g.om_im;                   // i Om/2 (conj: imaginary parts flip)
  c.m01i = sg * (0.5 * s * g.om_re);
  c.m10r = 0.5 * s * g.om_im;                    // i Om*/2
  c.m10i = sg * (0.5 * s * g.om_re);
  c.m11r = -0.5 * s * (r[0] + r[1] + r[2]);
  c.m11i = -sg * s * g.dl;
  return c;
}

// complex o += m z
#define CMAC(or_, oi, mr, mi, zr, zi) \
  do {                                 \
    or_ = fma(mr, zr, or_);            \
    or_ = fma(-(mi), zi, or_);         \
    oi = fma(mr, zi, oi);              \
    oi = fma(mi, zr, oi);              \
  } while (0)

// o[0..4] += M0 u[0..4] for one (re or im) component, stride-addressed
template <int ST>
__device__ __forceinline__ void m0_apply(const Gen& a, const double* b, double* o) {
  const double u1 = b[1 * ST], u2 = b[2 * ST], u3 = b[3 * ST], u4 = b[4 * ST];
  o[0] = fma(a.g0, u2, o[0]);
  o[1 * ST] = fma(a.g1, u2, fma(a.hy2, u3, fma(-a.hx2, u4, o[1 * ST])));
  o[2 * ST] = fma(a.mg01, u2, fma(-a.hy2, u3, fma(a.hx2, u4, o[2 * ST])));
  o[3 * ST] = fma(a.hy, u2 - u1, fma(-a.G, u3, fma(a.hz2, u4, o[3 * ST])));
  o[4 * ST] = fma(a.hx, u1 - u2, fma(-a.hz2, u3, fma(-a.G, u4, o[4 * ST])));
}

// o += 2Y b on a coherence sector; complex C[alpha][beta] interleaved (re, im)
template <int KIND>
__device__ __forceinline__ void apply_coh(const Gen& A0, const Gen& B0, const CGen& Am, const CGen& Bm,
                                          double vs, const double* b, double* o) {
  if (KIND == 0) {                 // C[5][2]: index 2*alpha + beta
    // A (q=0) on alpha, each beta and re/im: stride 4 doubles
#pragma unroll
    for (int be = 0; be < 2; ++be)
#pragma unroll
      for (int c = 0; c < 2; ++c) m0_apply<4>(A0, b + 2 * be + c, o + 2 * be + c);
    // B (q=-1) on beta
#pragma unroll
    for (int al = 0; al < 5; ++al) {
      const double z0r = b[4 * al], z0i = b[4 * al + 1], z1r = b[4 * al + 2], z1i = b[4 * al + 3];
      CMAC(o[4 * al], o[4 * al + 1], Bm.m00r, Bm.m00i, z0r, z0i);
      CMAC(o[4 * al], o[4 * al + 1], Bm.m01r, Bm.m01i, z1r, z1i);
      CMAC(o[4 * al + 2], o[4 * al + 3], Bm.m10r, Bm.m10i, z0r, z0i);
      CMAC(o[4 * al + 2], o[4 * al + 3], Bm.m11r, Bm.m11i, z1r, z1i);
    }
    // V: S_A (x) (i on beta=1): alpha = err (x2), ex, ey ; D_A (x) S_B: ex -> ey, ey -> -ex on beta=1
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
      for (int c = 0; c < 2; ++c) m0_apply<2>(B0, b + 10 * al + c, o + 10 * al + c);
#pragma unroll
    for (int be = 0; be < 5; ++be) {
      const double z0r = b[2 * be], z0i = b[2 * be + 1], z1r = b[10 + 2 * be], z1i = b[10 + 2 * be + 1];
      CMAC(o[2 * be], o[2 * be + 1], Am.m00r, Am.m00i, z0r, z0i);
      CMAC(o[2 * be], o[2 * be + 1], Am.m01r, Am.m01i, z1r, z1i);
      CMAC(o[10 + 2 * be], o[10 + 2 * be + 1], Am.m10r, Am.m10i, z0r, z0i);
      CMAC(o[10 + 2 * be], o[10 + 2 * be + 1], Am.m11r, Am.m11i, z1r, z1i);
    }
    // V: S_A(alpha=1) (x) D_B: ex -> ey, ey -> -ex ; D_A (i on alpha=1) (x) S_B
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
  } else {                         // C[2][2]: index 2*alpha + beta; A q=-1, B q=-1 or q=+1
#pragma unroll
    for (int be = 0; be < 2; ++be) {
      const double z0r = b[2 * be], z0i = b[2 * be + 1], z1r = b[4 + 2 * be], z1i = b[4 + 2 * be + 1];
      CMAC(o[2 * be], o[2 * be + 1], Am.m00r, Am.m00i, z0r, z0i);
      CMAC(o[2 * be], o[2 * be + 1], Am.m01r, Am.m01i, z1r, z1i);
      CMAC(o[4 + 2 * be], o[4 + 2 * be + 1], Am.m10r, Am.m10i, z0r, z0i);
      CMAC(o[4 + 2 * be], o[4 + 2 * be + 1], Am.m11r, Am.m11i, z1r, z1i);
    }
#pragma unroll
    for (int al = 0; al < 2; ++al) {
      const double z0r = b[4 * al], z0i = b[4 * al + 1], z1r = b[4 * al + 2], z1i = b[4 * al + 3];
      CMAC(o[4 * al], o[4 * al + 1], Bm.m00r, Bm.m00i, z0r, z0i);
      CMAC(o[4 * al], o[4 * al + 1], Bm.m01r, Bm.m01i, z1r, z1i);
      CMAC(o[4 * al + 2], o[4 * al + 3], Bm.m10r, Bm.m10i, z0r, z0i);
      CMAC(o[4 * al + 2], o[4 * al + 3], Bm.m11r, Bm.m11i, z1r, z1i);
    }
    if (KIND == 2) {               // (S (x) D + D (x) S) on C[1][1]: i + i
      o[6] = fma(-2.0 * vs, b[7], o[6]);
      o[7] = fma(2.0 * vs, b[6], o[7]);
    }
  }
}

// hilbert_space_dim = 3: per-atom q = 0 block {e00, e11, err, ex, ey}, q = -1 block
// {|0><1|, |0><r|}, no extra parameter columns.
struct Sector3 {
  static constexpr int NB = 5;                 // q = 0 block of one atom
  static constexpr int NS = NB * NB;           // the real (0,0) sector (state vector)
  static constexpr int NROW = 2 * NB;          // complex coordinates of a row sector
  struct Mj {};                                // the extra parameter columns: none
  __device__ static __forceinline__ Mj load_mj(const double*, int64_t, int64_t) { return {}; }
  __device__ static __forceinline__ bool mj_valid(const Mj&) { return true; }
  __device__ static __forceinline__ bool mj_valid(bool ok, const Mj&) { return ok; }   // ok && mj_valid: gmj_valid
  __device__ static __forceinline__ double rate_extra(const Mj&) { return 0.0; }   // their term of the rate sum
  __host__ __device__ static constexpr bool population(int a) { return a < 3; }   // e00, e11, err

  struct StateGen {
    Gen A, B;
  };
  // SYM (identical atoms) is apply_L's to use: it reads A alone
  template <bool SYM>
  __device__ static __forceinline__ StateGen state_gen(const Seg& g, const PointP& q, const Mj&, double sc) {
    return {make_gen(g, q.d1, q.gA, sc), make_gen(g, q.d1, q.gB, sc)};
  }
  template <bool SYM>
  __device__ static __forceinline__ void state_apply(const StateGen& G, double vs, const double (&b)[NS],
                                                     double (&o)[NS]) {
    apply_L<SYM>(G.A, G.B, vs, b, o);
  }

  // sector KIND's generator blocks (KIND 0 reads A0 and Bm, KIND 1 B0 and Am, the quads Am and
  // Bm; B's block conjugated for KIND 3, the (-1,+1) sector)
  struct CohGen {
    Gen A0, B0;
    CGen Am, Bm;
  };
  template <int KIND>
  __device__ static __forceinline__ CohGen coh_gen(const Seg& g, const PointP& q, const Mj&, double sc) {
    return {make_gen(g, q.d1, q.gA, sc), make_gen(g, q.d1, q.gB, sc), make_cgen(g, q.d1, q.gA, sc, false),
            make_cgen(g, q.d1, q.gB, sc, KIND == 3)};
  }
  template <int KIND>
  __device__ static __forceinline__ void coh_apply(const CohGen& G, double vs, const double* b, double* o) {
    apply_coh<KIND>(G.A0, G.B0, G.Am, G.Bm, vs, b, o);
  }
};

// One lane per (point, input) of one sector, a Chebyshev series per segment.  The row sectors
// (KIND 0 / 1) hold S::NROW complex coordinates, the quads 4.
template <int PROTO, int KIND, typename S>
__device__ __forceinline__ void coherence_sector(const double* __restrict__ prm, int64_t n, int64_t ldp,
                                                 double* __restrict__ out, int64_t ldo,
                                                 uint32_t* __restrict__ status, int n_steps, int shape,
                                                 int64_t blk) {
  constexpr int NIN = KIND < 2 ? 2 : 1;     // inputs of this sector per point
  constexpr int NV = KIND < 2 ? 2 * S::NROW : 8;
  const int64_t gid = blk * BLOCK + threadIdx.x;
  const bool live = gid < NIN * n;
  const int64_t i = live ? gid / NIN : (n - 1);
  const int sub = (int)(gid % NIN);
  const PointP q = load_point<PROTO>(prm, ldp, i);
  const typename S::Mj mj = S::load_mj(prm, ldp, i);
  const bool valid = point_valid<PROTO>(q, n_steps) && S::mj_valid(mj);
  // start: KIND 0 C[sub][0] (|00><01|: e00 (x) |0><1| ; |10><11|: e11 (x) |0><1|),
  //        KIND 1 C[0][sub], KIND 2/3 C[0][0]
  const int e0 = KIND == 0 ? 4 * sub : (KIND == 1 ? 2 * sub : 0);
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = (e == e0) ? 1.0 : 0.0;
  double nuse = 0.0, nexec = 0.0;
  bool over_cap = false;
  const int nseg = n_segments<PROTO>(n_steps);
  double rsum = S::rate_extra(mj);
#pragma unroll
  for (int c = 0; c < 4; ++c) rsum += fabs(q.gA[c]) + fabs(q.gB[c]);
  // LP square's two segments of a quad sector (8 doubles) are unrolled -- said here because the
  // compiler's own size estimate of that loop sits at its threshold; the other loops stay rolled
  // (a count of 1 forbids unrolling them: what the compiler chose by itself for all of them,
  // to be looked at again, with make kernel-diff, when the compiler changes)
  constexpr int SEG_UNROLL = (KIND >= 2 && PROTO == RYD_PROTO_LP_SQUARE) ? 2 : 1;
#pragma unroll SEG_UNROLL
  for (int s = 0; s < nseg; ++s) {
    const Seg g = segment<PROTO>(q, s, n_steps, shape);
    const SegScale k = seg_scale(g, q.V, q.d1, rsum, valid);
    over_cap = over_cap || k.capped;
    const auto G = S::template coh_gen<KIND>(g, q, mj, k.sc);
    const double vs = k.sc * 0.5 * q.V;
    cheb_segment<NV>(v, k.x, k.active,
                     [&](const double (&b)[NV], double (&o)[NV]) { S::template coh_apply<KIND>(G, vs, b, o); },
                     nuse, nexec);
  }
  uint32_t stat = valid ? 0u : RYD_STATUS_BAD_INPUT;
  if (over_cap) stat |= RYD_STATUS_STEP_CAP;
  if (!finite_all(v, NV)) stat |= RYD_STATUS_NONFINITE;
  if (!live) return;
  // qubit-block images: KIND 0 o0 = C[0][0] (|00><01|), o1 = C[1][0] (|10><11|);
  // KIND 1 o0 = C[0][0] (|00><10|), o1 = C[0][1] (|01><11|); KIND 2/3 C[0][0]
  if (KIND < 2) {
    const int base = (KIND == 0 ? RYD_C_K0 : RYD_C_K1) + 4 * sub;
    const int i1 = KIND == 0 ? 4 : 2;
    out[(int64_t)(base + 0) * ldo + i] = v[0];
    out[(int64_t)(base + 1) * ldo + i] = v[1];
    out[(int64_t)(base + 2) * ldo + i] = v[i1];
    out[(int64_t)(base + 3) * ldo + i] = v[i1 + 1];
  } else {
    const int base = KIND == 2 ? RYD_C_K2 : RYD_C_K3;
    out[(int64_t)(base + 0) * ldo + i] = v[0];
    out[(int64_t)(base + 1) * ldo + i] = v[1];
  }
  if (stat) atomicOr(&status[i], stat);
  (void)nuse;
  (void)nexec;
}

// All four coherence sectors in ONE launch: blocks [0, b0) sector 0, [b0, b1) sector 1,
// [b1, b2) sector 2, then sector 3 (block-uniform branch).  The sectors used to be four
// back-to-back launches of 2n, 2n, n and n lanes -- each far below one wave per SIMD at
// C2 sizes, so the device idled through four serial latency-bound tails; together they
// fill the chip once (the two row sectors, whose lanes run longest, first).
template <int PROTO, typename S>
__device__ __forceinline__ void coherence_cheb_body(const double* __restrict__ prm, int64_t n, int64_t ldp,
                                                    double* __restrict__ out, int64_t ldo,
                                                    uint32_t* __restrict__ status, int n_steps, int shape,
                                                    int64_t b0, int64_t b1, int64_t b2) {
  const int64_t b = blockIdx.x;
  if (b < b0) coherence_sector<PROTO, 0, S>(prm, n, ldp, out, ldo, status, n_steps, shape, b);
  else if (b < b1) coherence_sector<PROTO, 1, S>(prm, n, ldp, out, ldo, status, n_steps, shape, b - b0);
  else if (b < b2) coherence_sector<PROTO, 2, S>(prm, n, ldp, out, ldo, status, n_steps, shape, b - b1);
  else coherence_sector<PROTO, 3, S>(prm, n, ldp, out, ldo, status, n_steps, shape, b - b2);
}

template <int PROTO>
__global__ __launch_bounds__(BLOCK) void coherence_cheb_kernel(const double* __restrict__ prm, int64_t n,
                                                               int64_t ldp, double* __restrict__ out, int64_t ldo,
                                                               uint32_t* __restrict__ status, int n_steps,
                                                               int shape, int64_t b0, int64_t b1, int64_t b2) {
  coherence_cheb_body<PROTO, Sector3>(prm, n, ldp, out, ldo, status, n_steps, shape, b0, b1, b2);
}

#include "ryd_coh_prop.inc"
#include "ryd_dim4_prop.inc"
#include "ryd_coh4_prop.inc"
#include "ryd_shaped16.inc"
// process-map coherences of a custom pulse schedule (ryd_run_schedule_coherences)
#include "ryd_coh_sched.inc"

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return fail(RYD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)

using KernelFn = void (*)(const double*, int64_t, int64_t, double*, int64_t, double*, int64_t,
                          uint32_t*, int, int);

// an off switch of the environment: the variable is set and starts with '0'.  Every switch
// is read at the launch it governs, never cached: tests alternate them within one process.
bool is_off(const char* e) { return e && e[0] == '0'; }

// d->protocol (validated) as a compile-time constant: f(std::integral_constant<int, PROTO>)
template <typename F>
int with_protocol(int protocol, F&& f) {
  switch (protocol) {
    case RYD_PROTO_LP_SQUARE: return f(std::integral_constant<int, RYD_PROTO_LP_SQUARE>{});
    case RYD_PROTO_LP_SHAPED: return f(std::integral_constant<int, RYD_PROTO_LP_SHAPED>{});
    case RYD_PROTO_BANGBANG: return f(std::integral_constant<int, RYD_PROTO_BANGBANG>{});
    default: return f(std::integral_constant<int, RYD_PROTO_SMOOTH_JP>{});
  }
}

// One kernel launch, checked against the kernel's own signature: each argument is converted to
// the parameter it fills (no narrowing, and no change of width: an int is not quietly widened
// into an int64_t slot), so a wrong count, order or type does not compile.
template <typename... P, typename... A>
int launch_typed(void (*kernel)(P...), int64_t blocks, unsigned block, size_t lds_bytes, hipStream_t stream,
                 A... a) {
  static_assert(((sizeof(A) == sizeof(P)) && ...), "an argument's width differs from the kernel parameter's");
  if (blocks > 0x7fffffffLL) return fail(RYD_ERR_INVALID, "batch too large for one launch");
  return [&](P... p) {
    void* args[] = {(void*)&p...};
    HIPCHK(hipLaunchKernel((const void*)kernel, dim3((unsigned)blocks), dim3(block), args, lds_bytes, stream));
    return RYD_OK;
  }(P{a}...);
}

// The kernel family a batch descriptor runs (RYD_PATH_*; ryd_batch_path reports it).
enum BatchPath {
  PATH_DOPRI5 = RYD_PATH_DOPRI5, PATH_DIM4_PROP = RYD_PATH_DIM4_PROP, PATH_SHAPED16 = RYD_PATH_SHAPED16,
  PATH_SYM16 = RYD_PATH_SYM16, PATH_JP_SPLIT = RYD_PATH_JP_SPLIT, PATH_LINDBLAD_PROP = RYD_PATH_LINDBLAD_PROP,
  PATH_LINDBLAD_CHEB = RYD_PATH_LINDBLAD_CHEB, PATH_KET_BLOCK = RYD_PATH_KET_BLOCK, PATH_KET_CHEB = RYD_PATH_KET_CHEB
};

// The one place that selects a kernel family for a validated descriptor; the first match wins
// ("Selection order").  Each =0 switch keeps the family's cross-check kernel (A/B
// measurements, tests).
BatchPath batch_path(const ryd_batch_desc* d) {
  const bool lind = d->evolution == RYD_EVOL_LINDBLAD, autom = d->method == RYD_METHOD_CHEBYSHEV;
  // the protocols whose gate is a product of few propagators: LP square and bang-bang (few long
  // segments), smooth JP (one propagator in the phase frame); LP shaped changes its amplitude
  // every segment
  const bool few = d->protocol != RYD_PROTO_LP_SHAPED;
  // identical atoms under the auto method: the 16-lane DPP-row kernels
  const bool rows16 = lind && autom && (d->flags & RYD_FLAG_SYMMETRIC_ATOMS) != 0;
  if (d->method == RYD_METHOD_DOPRI5) return PATH_DOPRI5;
  // dim 4, constant-|Omega| schedules: the triangle propagator kernel (ryd_dim4_prop.inc)
  if (rows16 && d->dim == 4 && few && !is_off(getenv("RYD_DIM4_PROP"))) return PATH_DIM4_PROP;
  // LP shaped: the state-vector kernel of ryd_shaped16.inc
  if (rows16 && d->dim == 3 && !few && !is_off(getenv("RYD_SHAPED16"))) return PATH_SHAPED16;
  // ryd_sym16.inc; the explicit RYD_METHOD_CHEB_SQUARING always runs the kernels below
  if (rows16 && d->dim == 3 && few && !is_off(getenv("RYD_SYM16"))) return PATH_SYM16;
  // the propagator kernel when asked for explicitly, or under the auto method for the
  // few-propagator protocols; RYD_JP_SPLIT=0 keeps smooth JP in the fused kernel (the
  // split-vs-fused bit-identity test)
  const bool prop = lind && d->dim == 3 && (d->method == RYD_METHOD_CHEB_SQUARING || (autom && few));
  if (prop && d->protocol == RYD_PROTO_SMOOTH_JP && !is_off(getenv("RYD_JP_SPLIT"))) return PATH_JP_SPLIT;
  if (prop) return PATH_LINDBLAD_PROP;
  if (lind) return PATH_LINDBLAD_CHEB;   // the per-lane state-vector Chebyshev kernel, dim 3 or 4
  // kets under the auto method: the exact block-propagator kernel, one lane per point;
  // RYD_METHOD_CHEB_VECTOR keeps the 4-lane Chebyshev state-vector kernel
  if (autom && !is_off(getenv("RYD_KET_BLOCK"))) return PATH_KET_BLOCK;
  return PATH_KET_CHEB;
}

// The paths with a store-free twin for summary-only launches: sym16 and the ket block kernel.
// Every other one runs into a scratch buffer.  shaped16 and lindblad4_prop_kernel had twins
// whose median did not lie below the storing kernel's range in every round (4.8 ms and 0.12 ms
// of arithmetic per C2 launch against the 8 and 11.5 MB of stores; profiles/summary_only/), so
// they were not kept.
bool has_twin(BatchPath p) { return p == PATH_SYM16 || p == PATH_KET_BLOCK; }

// RYD_S16_STORE64=1 makes the sym16 kernel form its output addresses per lane in 64 bits
// for every launch (the form it takes anyway when a leading dimension is too large for a
// 32-bit lane offset): tests run both
bool sym16_store32_enabled() {
  const char* e = getenv("RYD_S16_STORE64");
  return !(e && e[0] == '1');
}

// RYD_S16_PARAM64=1 makes the balanced sym16 kernel load its parameter columns one by one
// at 64-bit column addresses for every launch (the form it takes anyway when 8 (14 ld_params
// + n) does not fit 31 bits): tests run both
bool sym16_param32_enabled() {
  const char* e = getenv("RYD_S16_PARAM64");
  return !(e && e[0] == '1');
}

// The balanced launch form of the sym16 LP-square kernel (ryd_sym16.inc): the static plan
// for n points on `cus` compute units.  gpc_override > 0 sets the groups per workgroup.
// auto_on: the launches the form is measured to win -- every wave resident at once, more
// than one job per SIMD, and 1 or 2 jobs per CU left over beyond a multiple of 4 (C2's
// 10,000 points: 10 groups per CU; profiles/sym16_balance/ab_sizes.txt).
struct S16Plan {
  int64_t groups, workgroups;
  int gpc, waves;
  bool auto_on;
};
bool sym16_plan(int64_t n, int cus, int gpc_override, S16Plan* pl) {
  if (n <= 0 || cus <= 0 || gpc_override < 0 || gpc_override > S16_BAL_MAXW) return false;
  const int64_t G = (n + S16_PPW - 1) / S16_PPW;
  const int64_t natural = (G + cus - 1) / cus;
  const int gnat = (int)(natural < S16_BAL_MAXW ? natural : S16_BAL_MAXW);
  pl->groups = G;
  pl->gpc = gpc_override > 0 ? gpc_override : gnat;
  pl->workgroups = (G + pl->gpc - 1) / pl->gpc;
  pl->waves = s16_bal_waves(pl->gpc);
  pl->auto_on = natural <= S16_BAL_MAXW && gnat > 4 && s16_bal_split(gnat);
  return true;
}

// RYD_S16_BALANCE: 0 never, 2 always (LP square on the sym16 path, any n), otherwise auto;
// RYD_S16_BALANCE_GPC=<k> overrides the groups per workgroup; RYD_S16_BALANCE_NOHANDOFF=1
// makes every consumer run the producer's part itself (tests).  Read per launch.
int sym16_balance_mode() {
  const char* e = getenv("RYD_S16_BALANCE");
  return e && e[0] == '0' ? 0 : e && e[0] == '2' ? 2 : 1;
}
// RYD_S16_WT: the output stores of the balanced form (S16_WT_* in ryd_sym16.inc) -- 0 plain,
// 1 the state rows write-through, 3 the summary and status pieces too; unset: automatic (3).
// Read per launch, so both flavours can alternate in one process.  -1 unset, -2 not a value.
int sym16_wt_mode() {
  const char* e = getenv("RYD_S16_WT");
  if (!e) return -1;
  if ((e[0] == '0' || e[0] == '1' || e[0] == '3') && e[1] == '\0') return e[0] - '0';
  return -2;
}
int sym16_device_cus() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  int c = cached[dev].load(std::memory_order_relaxed);
  if (c == 0) {
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cached[dev].store(c, std::memory_order_relaxed);
  }
  return c;
}

// the protocol and its n_steps / shape, for batch and trajectory descriptors alike
int validate_protocol(int protocol, int n_steps, int shape) {
  if (protocol < 0 || protocol > 3) return fail(RYD_ERR_INVALID, "bad protocol");
  if (protocol == RYD_PROTO_LP_SHAPED && (n_steps < 2 || shape < 0 || shape > 3))
    return fail(RYD_ERR_INVALID, "LP_SHAPED needs n_steps >= 2 and a valid shape");
  if (protocol == RYD_PROTO_SMOOTH_JP && n_steps < 1) return fail(RYD_ERR_INVALID, "SMOOTH_JP needs n_steps >= 1");
  if (protocol == RYD_PROTO_BANGBANG && (n_steps < 1 || n_steps > 8))
    return fail(RYD_ERR_INVALID, "BANGBANG needs 1 <= n_steps (max segments) <= 8");
  return RYD_OK;
}

// has_state = false: a summary-only call (null state pointer), whose ld_state is ignored
int validate(const ryd_batch_desc* d, int64_t n, int64_t ldp, int64_t lds, int64_t ldm, bool has_state = true) {
  if (!d) return fail(RYD_ERR_INVALID, "desc is NULL");
  if (d->abi_version != RYD_ABI_VERSION) return fail(RYD_ERR_INVALID, "abi_version mismatch");
  if (d->dim != 3 && d->dim != 4) return fail(RYD_ERR_UNSUPPORTED, "hilbert_space_dim must be 3 or 4");
  if (d->dim == 4 && d->method != RYD_METHOD_CHEBYSHEV && d->method != RYD_METHOD_CHEB_VECTOR)
    return fail(RYD_ERR_UNSUPPORTED, "dim 4 runs the Chebyshev state-vector method only");
  if (d->method != RYD_METHOD_CHEBYSHEV && d->method != RYD_METHOD_CHEB_VECTOR &&
      d->method != RYD_METHOD_CHEB_SQUARING && d->method != RYD_METHOD_DOPRI5)
    return fail(RYD_ERR_UNSUPPORTED, "method not implemented");
  if (d->method == RYD_METHOD_DOPRI5) {
    if (d->evolution != RYD_EVOL_LINDBLAD) return fail(RYD_ERR_UNSUPPORTED, "DOPRI5 is Lindblad-only");
    if (!(d->rtol > 0.0) || !(d->atol > 0.0) || d->max_steps < 1)
      return fail(RYD_ERR_INVALID, "DOPRI5 needs rtol > 0, atol > 0, max_steps >= 1");
  }
  if (d->method == RYD_METHOD_CHEB_SQUARING && d->evolution != RYD_EVOL_LINDBLAD)
    return fail(RYD_ERR_UNSUPPORTED, "squaring method is Lindblad-only");
  if (d->evolution != RYD_EVOL_LINDBLAD && d->evolution != RYD_EVOL_KET)
    return fail(RYD_ERR_INVALID, "bad evolution");
  if (int rc = validate_protocol(d->protocol, d->n_steps, d->shape)) return rc;
  if (n < 0) return fail(RYD_ERR_INVALID, "n < 0");
  if (ldp < n || (has_state && lds < 4 * n) || ldm < n) return fail(RYD_ERR_INVALID, "leading dimension too small");
  return RYD_OK;
}

// The jp workspace pool: a private stream-ordered pool per device, kept warm
// (release threshold = max) without touching the process's default pool.
hipMemPool_t jp_pool(int dev) {
  static std::mutex mu;
  static std::vector<hipMemPool_t> pools;
  std::lock_guard<std::mutex> lk(mu);
  if ((int)pools.size() <= dev) pools.resize(dev + 1, nullptr);
  if (!pools[dev]) {
    hipMemPoolProps pp;
    memset(&pp, 0, sizeof(pp));
    pp.allocType = hipMemAllocationTypePinned;
    pp.location.type = hipMemLocationTypeDevice;
    pp.location.id = dev;
    hipMemPool_t p = nullptr;
    if (hipMemPoolCreate(&p, &pp) != hipSuccess) return nullptr;
    uint64_t keep = UINT64_MAX;
    (void)hipMemPoolSetAttribute(p, hipMemPoolAttrReleaseThreshold, &keep);
    pools[dev] = p;
  }
  return pools[dev];
}

// Smooth JP, propagator method: jp_rows_kernel -> workspace (25 x 25 doubles per
// point, from the private pool) -> jp_frame_kernel.
int launch_jp_split(const ryd_batch_desc* d, const double* dp, int64_t n, int64_t ldp, double* ds,
                    int64_t lds, double* dm, int64_t ldm, uint32_t* dstat, hipStream_t stream) {
  const bool sym = (d->flags & RYD_FLAG_SYMMETRIC_ATOMS) != 0;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  hipMemPool_t pool = jp_pool(dev);
  if (!pool) return fail(RYD_ERR_ALLOC, "jp workspace pool creation failed");
  double* W = nullptr;
  HIPCHK(hipMallocFromPoolAsync((void**)&W, sizeof(double) * NC * NC * (size_t)n, pool, stream));
  const int ns = d->n_steps, sh = d->shape;
  int rc = launch_typed(sym ? jp_rows_kernel<true> : jp_rows_kernel<false>, (n + PPB - 1) / PPB, BLOCK, 0, stream,
                        dp, n, ldp, W, dm, ldm, dstat, ns, sh);
  // SYM holds 157 VGPRs (3 waves per SIMD; a 128 budget spills), the 4-output form 127
  if (!rc)
    rc = launch_typed(sym ? jp_frame_kernel<3, true> : jp_frame_kernel<4, false>, (n + FPB - 1) / FPB, BLOCK, 0,
                      stream, dp, n, ldp, W, ds, lds, dm, ldm, dstat, ns);
  hipError_t ef = hipFreeAsync(W, stream);          // on the error path too
  if (rc) return rc;
  if (ef != hipSuccess) return fail(RYD_ERR_HIP, std::string("jp workspace free: ") + hipGetErrorString(ef));
  return RYD_OK;
}

// The sym16 path (ryd_sym16.inc): the one-wave kernel, or for LP square the CU-balanced form.
// ds = NULL takes either one's summary-only twin, with the same grid and arguments.
template <int PROTO>
int launch_sym16(const double* dp, int64_t n, int64_t ldp, double* ds, int64_t lds, double* dm, int64_t ldm,
                 uint32_t* dstat, int ns, int sh, hipStream_t stream) {
  // the output stores take a wave-uniform base plus a 32-bit lane byte offset where the
  // largest one fits: 8 (15 + 3 lds) on the state rows, 8 (15 ldm + 3) on the summary
  const int st32 = sym16_store32_enabled() && lds >= 0 && ldm >= 0 && lds <= (0x1fffffffLL - 15) / 3 &&
                   ldm <= (0x1fffffffLL - 3) / 15;
  const int bal = PROTO == RYD_PROTO_LP_SQUARE ? sym16_balance_mode() : 0;
  const int wtm = sym16_wt_mode();
  if (wtm == -2) return fail(RYD_ERR_INVALID, "RYD_S16_WT must be 0, 1 or 3");
  if (bal != 0) {
    // the form is chosen first (forced, or the automatic rule on this device's CU count);
    // the other switches are read, and checked, only by a launch that takes it
    const int cus = sym16_device_cus();
    S16Plan pl;
    const bool planned = sym16_plan(n, cus, 0, &pl);
    if (bal == 2 && !planned)
      return fail(RYD_ERR_HIP, "RYD_S16_BALANCE=2: the device's compute-unit count is not available");
    if (planned && (bal == 2 || pl.auto_on)) {
      if (const char* eg = getenv("RYD_S16_BALANCE_GPC")) {
        char* end = nullptr;
        const long over = strtol(eg, &end, 10);
        if (end == eg || *end != '\0' || over < 1 || over > S16_BAL_MAXW)
          return fail(RYD_ERR_INVALID, "RYD_S16_BALANCE_GPC must be an integer from 1 to 16");
        sym16_plan(n, cus, (int)over, &pl);
      }
      const char* eh = getenv("RYD_S16_BALANCE_NOHANDOFF");
      // the first parameter load is one instruction per wave (load_point16_row) where its
      // largest 32-bit lane offset, 8 (14 ldp + n), fits 31 bits: LP square reads columns
      // 0 .. RYD_P_XI_IM = 14
      static_assert(RYD_P_XI_IM == 14, "the largest LP-square parameter column");
      const bool p32 = sym16_param32_enabled() && ldp <= (0x7fffffffLL / 8 - n) / 14;
      const int noh = eh && eh[0] == '1', wt = wtm >= 0 ? wtm : S16_WT_AUTO;
      if (pl.workgroups > 0x7fffffffLL) return fail(RYD_ERR_INVALID, "batch too large for one launch");
      HIPCHK(ryd_s16_bal_launch(p32 ? 2 : 1, ds != nullptr, (unsigned)pl.workgroups, S16_BLOCK * pl.waves, stream, dp,
                                n, ldp, s16_bal_cfg(pl.gpc, st32, noh, wt), dm, dstat, ldm, ds, lds, ns));
      return RYD_OK;
    }
  }
  // the one-wave kernels have plain stores only: a forced write-through cannot be honoured
  if (wtm > 0) return fail(RYD_ERR_UNSUPPORTED, "RYD_S16_WT: write-through stores need the balanced launch form");
  return launch_typed(ds ? lindblad_sym16_kernel<PROTO> : lindblad_sym16_nostate_kernel<PROTO>,
                      (n + S16_PPW - 1) / S16_PPW, S16_BLOCK, 0, stream, dp, n, ldp, ds, lds, dm, ldm, dstat, ns, sh,
                      st32);
}

// The kernel launch of one batch on the path batch_path() selected.  ds = NULL (launch() alone
// passes it, and only on a path that has_twin()) takes the summary-only twin of the kernel
// the descriptor selects, with the same grid and arguments.  Families built for three
// protocols (or for LP shaped alone) are instantiated for those only.
int launch_kernels(BatchPath path, const ryd_batch_desc* d, const double* dp, int64_t n, int64_t ldp, double* ds,
                   int64_t lds, double* dm, int64_t ldm, uint32_t* dstat, hipStream_t stream) {
  const bool sym = (d->flags & RYD_FLAG_SYMMETRIC_ATOMS) != 0, dim4 = d->dim == 4;
  const int ns = d->n_steps, sh = d->shape;
  // the ten arguments every kernel here starts with
  auto go = [&](auto kernel, int64_t blocks, unsigned block, auto... more) {
    return launch_typed(kernel, blocks, block, 0, stream, dp, n, ldp, ds, lds, dm, ldm, dstat, ns, sh,
                        more...);
  };
  if (!ds && !has_twin(path)) return fail(RYD_ERR_UNSUPPORTED, "no kernel for this descriptor");
  return with_protocol(d->protocol, [&](auto proto) -> int {
    constexpr int P = decltype(proto)::value;
    constexpr bool FEW = P != RYD_PROTO_LP_SHAPED;
    KernelFn k = nullptr;
    switch (path) {
      case PATH_DOPRI5:
        return go(lindblad_dopri5_kernel<P>, (4 * n + DP_BLOCK - 1) / DP_BLOCK, DP_BLOCK, d->rtol, d->atol,
                  d->max_steps);
      case PATH_DIM4_PROP:
        if constexpr (FEW) return go(lindblad4_prop_kernel<P>, (n + D4_PPB - 1) / D4_PPB, D4_BLOCK);
        break;
      case PATH_SHAPED16:
        if constexpr (!FEW) return go(lindblad_shaped16_kernel<P>, (n + SH_PPW - 1) / SH_PPW, SH_BLOCK);
        break;
      case PATH_SYM16:
        if constexpr (FEW) return launch_sym16<P>(dp, n, ldp, ds, lds, dm, ldm, dstat, ns, sh, stream);
        break;
      case PATH_JP_SPLIT: return launch_jp_split(d, dp, n, ldp, ds, lds, dm, ldm, dstat, stream);
      case PATH_LINDBLAD_PROP:
        k = sym ? lindblad_prop_kernel<P, true> : lindblad_prop_kernel<P, false>;
        return go(k, (n + PPB - 1) / PPB, BLOCK);
      case PATH_LINDBLAD_CHEB:
        k = dim4 ? (sym ? lindblad4_cheb_kernel<P, true> : lindblad4_cheb_kernel<P, false>)
                 : (sym ? lindblad_cheb_kernel<P, true> : lindblad_cheb_kernel<P, false>);
        return go(k, (4 * n + BLOCK - 1) / BLOCK, BLOCK);
      case PATH_KET_BLOCK:
        k = ds ? (dim4 ? ket_block_kernel<P, 4> : ket_block_kernel<P, 3>)
               : (dim4 ? ket_block_nostate_kernel<P, 4> : ket_block_nostate_kernel<P, 3>);
        return go(k, (n + BLOCK - 1) / BLOCK, BLOCK);
      case PATH_KET_CHEB:
        return go(dim4 ? ket_cheb_kernel<P, 4> : ket_cheb_kernel<P, 3>, (4 * n + BLOCK - 1) / BLOCK, BLOCK);
    }
    return fail(RYD_ERR_UNSUPPORTED, "no kernel for this descriptor");
  });
}

// Whether a summary-only launch on this path runs the store-free twin.  RYD_NOSTATE=0 sends
// every one down the scratch-buffer path, the storing kernels (A/B measurements and the
// cross-check of the twins); read per launch.
bool takes_twin(BatchPath p) { return has_twin(p) && !is_off(getenv("RYD_NOSTATE")); }

// One batch on `stream`.  ds = NULL is a summary-only call, and this is the one place that
// knows: the descriptor's store-free twin where it has one, otherwise the ordinary kernel into
// a scratch state buffer from the private stream-ordered pool, freed on the stream (nothing
// copies it; as launch_jp_split's workspace).  No kernel that stores state sees a null pointer.
int launch(const ryd_batch_desc* d, const double* dp, int64_t n, int64_t ldp, double* ds, int64_t lds,
           double* dm, int64_t ldm, uint32_t* dstat, hipStream_t stream) {
  if (n == 0) return RYD_OK;
  const BatchPath path = batch_path(d);
  if (ds) return launch_kernels(path, d, dp, n, ldp, ds, lds, dm, ldm, dstat, stream);
  if (takes_twin(path)) return launch_kernels(path, d, dp, n, ldp, nullptr, 0, dm, ldm, dstat, stream);
  const int sw = ryd_state_width(d->evolution, d->dim);
  if (sw <= 0) return fail(RYD_ERR_INVALID, "bad evolution");
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  hipMemPool_t pool = jp_pool(dev);
  if (!pool) return fail(RYD_ERR_ALLOC, "scratch state pool creation failed");
  double* W = nullptr;
  HIPCHK(hipMallocFromPoolAsync((void**)&W, sizeof(double) * (size_t)sw * 4 * (size_t)n, pool, stream));
  const int rc = launch_kernels(path, d, dp, n, ldp, W, 4 * n, dm, ldm, dstat, stream);
  hipError_t ef = hipFreeAsync(W, stream);           // on the error path too
  if (rc) return rc;
  if (ef != hipSuccess) return fail(RYD_ERR_HIP, std::string("scratch state free: ") + hipGetErrorString(ef));
  return RYD_OK;
}

// ryd_run_schedule[_device]: the descriptor, the table pointer and the leading dimensions, all
// before any GPU call.  has_state = false: a summary-only call, whose ld_state is ignored.
int validate_schedule(const ryd_sched_desc* d, const double* sched, int64_t n, int64_t ldp, int64_t ldsc,
                      int64_t lds, int64_t ldm, bool has_state) {
  if (!d) return fail(RYD_ERR_INVALID, "desc is NULL");
  if (!sched) return fail(RYD_ERR_INVALID, "schedule table is NULL");
  if (d->abi_version != RYD_ABI_VERSION) return fail(RYD_ERR_INVALID, "abi_version mismatch");
  if (d->n_seg < 1 || d->n_seg > RYD_SCHED_MAX_SEG)
    return fail(RYD_ERR_INVALID, "n_seg must be 1 .. " + std::to_string(RYD_SCHED_MAX_SEG));
  if (d->flags & ~(RYD_FLAG_SYMMETRIC_ATOMS | RYD_SCHED_SHARED)) return fail(RYD_ERR_INVALID, "unknown flag bits");
  if (d->dim != 3) return fail(RYD_ERR_UNSUPPORTED, "pulse schedules run hilbert_space_dim 3 only");
  if (!(d->flags & RYD_FLAG_SYMMETRIC_ATOMS))
    return fail(RYD_ERR_UNSUPPORTED, "pulse schedules need identical atoms (RYD_FLAG_SYMMETRIC_ATOMS)");
  if (!(d->flags & RYD_SCHED_SHARED) && ldsc < (int64_t)RYD_SC_NFIELD * d->n_seg)
    return fail(RYD_ERR_INVALID, "ld_sched is smaller than 4 n_seg");
  if (n < 0) return fail(RYD_ERR_INVALID, "n < 0");
  if (ldp < n || (has_state && lds < 4 * n) || ldm < n) return fail(RYD_ERR_INVALID, "leading dimension too small");
  return RYD_OK;
}

// What the schedule launches share: nothing to do for n = 0, and `go(ld, n_seg, grid)` with the
// table's leading dimension as the kernels take it (a shared table is a per-point one of
// leading dimension 0) and the grid of `per_block` points per block.
template <typename Go>
int launch_sched(const ryd_sched_desc* d, int64_t n, int64_t ldsc, int per_block, Go&& go) {
  if (n == 0) return RYD_OK;
  return go((d->flags & RYD_SCHED_SHARED) ? (int64_t)0 : ldsc, (int)d->n_seg, (n + per_block - 1) / per_block);
}

// One schedule batch on `stream` (ryd_sched16.inc); ds = NULL takes the store-free twin.
int launch_schedule(const ryd_sched_desc* d, const double* dp, int64_t n, int64_t ldp, const double* dsc,
                    int64_t ldsc, double* ds, int64_t lds, double* dm, int64_t ldm, uint32_t* dstat,
                    hipStream_t stream) {
  if (!ds) lds = 0;
  // the output stores' 32-bit lane offsets, as launch_sym16 checks them
  const int st32 = sym16_store32_enabled() && lds >= 0 && ldm >= 0 && lds <= (0x1fffffffLL - 15) / 3 &&
                   ldm <= (0x1fffffffLL - 3) / 15;
  return launch_sched(d, n, ldsc, S16_PPW, [&](int64_t ld, int nseg, int64_t grid) {
    return launch_typed(ds ? lindblad_sched16_kernel<true> : lindblad_sched16_kernel<false>, grid, S16_BLOCK, 0,
                        stream, dp, n, ldp, dsc, ld, nseg, ds, lds, dm, ldm, dstat, st32);
  });
}

// ryd_run_schedule_kets[_device]: validate_schedule's rules (the descriptor first), then the
// Jacobian's leading dimension where a Jacobian is asked for
int validate_schedule_kets(const ryd_sched_desc* d, const double* sched, int64_t n, int64_t ldp, int64_t ldsc,
                           int64_t lds, int64_t ldm, bool has_state, int64_t ldj, bool has_jac) {
  if (int rc = validate_schedule(d, sched, n, ldp, ldsc, lds, ldm, has_state)) return rc;
  if (has_jac && ldj < (int64_t)RYD_SC_NFIELD * d->n_seg) return fail(RYD_ERR_INVALID, "ld_jac is smaller than 4 n_seg");
  return RYD_OK;
}

// One noise-free schedule batch as kets on `stream` (ryd_ket_sched.inc); ds = NULL takes the
// store-free twin.  ctl: the Jacobian of all four fields (ket_sched_ctl_kernel); else dj = NULL
// takes the forward kernel alone.
int launch_schedule_kets(bool ctl, const ryd_sched_desc* d, const double* dp, int64_t n, int64_t ldp,
                         const double* dsc, int64_t ldsc, double* ds, int64_t lds, double* dm, int64_t ldm,
                         double* dj, int64_t ldj, uint32_t* dstat, hipStream_t stream) {
  if (!ds) lds = 0;
  return launch_sched(d, n, ldsc, S16_PPW, [&](int64_t ld, int nseg, int64_t grid) {
    if (ctl)
      return launch_typed(ds ? ket_sched_ctl_kernel<true> : ket_sched_ctl_kernel<false>, grid, S16_BLOCK, 0, stream,
                          dp, n, ldp, dsc, ld, nseg, ds, lds, dm, ldm, dj, ldj, dstat);
    if (dj)
      return launch_typed(ds ? ket_sched_jac_kernel<true> : ket_sched_jac_kernel<false>, grid, S16_BLOCK, 0, stream,
                          dp, n, ldp, dsc, ld, nseg, ds, lds, dm, ldm, dj, ldj, dstat);
    return launch_typed(ds ? ket_sched_kernel<true> : ket_sched_kernel<false>, grid, S16_BLOCK, 0, stream, dp, n, ldp,
                        dsc, ld, nseg, ds, lds, dm, ldm, dstat);
  });
}

// ryd_run_schedule_kets_ctl[_device]: validate_schedule_kets' rules, with the Jacobian required
// and four fields wide
int validate_schedule_kets_ctl(const ryd_sched_desc* d, const double* sched, int64_t n, int64_t ldp, int64_t ldsc,
                               int64_t lds, int64_t ldm, bool has_state, const double* jac, int64_t ldj) {
  if (int rc = validate_schedule_kets(d, sched, n, ldp, ldsc, lds, ldm, has_state, 0, false)) return rc;
  if (!jac) return fail(RYD_ERR_INVALID, "the control Jacobian is NULL");
  if (ldj < 4 * (int64_t)RYD_SC_NFIELD * d->n_seg) return fail(RYD_ERR_INVALID, "ld_jac is smaller than 16 n_seg");
  return RYD_OK;
}

// RYD_COH_PROP=0 selects coherence_cheb_kernel for every protocol (A/B and cross-check runs)
bool coh_prop_enabled() { return !is_off(getenv("RYD_COH_PROP")); }

// The coherence sectors of one batch (one launch); status is cleared first and each
// sector ORs its bits in.  dim 4: the kernels of ryd_coh4_prop.inc.
int launch_coherences(const ryd_batch_desc* d, const double* dp, int64_t n, int64_t ldp, double* dc,
                      int64_t ldc, uint32_t* dstat, hipStream_t stream) {
  if (n == 0) return RYD_OK;
  HIPCHK(hipMemsetAsync(dstat, 0, sizeof(uint32_t) * n, stream));
  const bool dim4 = d->dim == 4;
  const int ns = d->n_steps, sh = d->shape;
  return with_protocol(d->protocol, [&](auto proto) {
    constexpr int P = decltype(proto)::value;
    if (P != RYD_PROTO_LP_SHAPED && coh_prop_enabled())   // one propagator per sector (ryd_coh_prop.inc)
      return launch_typed(dim4 ? coherence4_prop_kernel<P> : coherence_prop_kernel<P>, (n + CP_NR - 1) / CP_NR,
                          CP_BLOCK, 0, stream, dp, n, ldp, dc, ldc, dstat, ns, sh);
    const int64_t nb2 = (2 * n + BLOCK - 1) / BLOCK, nb1 = (n + BLOCK - 1) / BLOCK;
    const int64_t b0 = nb2, b1 = 2 * nb2, b2 = 2 * nb2 + nb1;
    return launch_typed(dim4 ? coherence4_cheb_kernel<P> : coherence_cheb_kernel<P>, 2 * nb2 + 2 * nb1, BLOCK, 0,
                        stream, dp, n, ldp, dc, ldc, dstat, ns, sh, b0, b1, b2);
  });
}

// ryd_run_schedule_coherences[_device]: validate_schedule's rules (the descriptor first), with
// the coherence rows' leading dimension in place of the state's and the summary's
int validate_schedule_coherences(const ryd_sched_desc* d, const double* sched, int64_t n, int64_t ldp,
                                 int64_t ldsc, int64_t ldc) {
  if (int rc = validate_schedule(d, sched, n, ldp, ldsc, 0, n, false)) return rc;
  if (ldc < n) return fail(RYD_ERR_INVALID, "leading dimension too small");
  return RYD_OK;
}

// The coherence sectors of one schedule batch (ryd_coh_sched.inc, one launch); status is cleared
// first, as launch_coherences does.
int launch_schedule_coherences(const ryd_sched_desc* d, const double* dp, int64_t n, int64_t ldp,
                               const double* dsc, int64_t ldsc, double* dc, int64_t ldc, uint32_t* dstat,
                               hipStream_t stream) {
  return launch_sched(d, n, ldsc, CP_NR, [&](int64_t ld, int nseg, int64_t grid) {
    HIPCHK(hipMemsetAsync(dstat, 0, sizeof(uint32_t) * n, stream));
    return launch_typed(coherence_sched_kernel, grid, CP_BLOCK, 0, stream, dp, n, ldp, dsc, ld, nseg, dc, ldc, dstat);
  });
}

int validate_coherences(const ryd_batch_desc* d, int64_t n, int64_t ldp, int64_t ldc) {
  if (!d) return fail(RYD_ERR_INVALID, "desc is NULL");
  if (d->dim != 3 && d->dim != 4) return fail(RYD_ERR_UNSUPPORTED, "process-map coherences: dim 3 or 4 only");
  ryd_batch_desc v = *d;                   // the Chebyshev vector method, Lindblad bookkeeping
  v.method = RYD_METHOD_CHEB_VECTOR;
  v.evolution = RYD_EVOL_LINDBLAD;
  int rc = validate(&v, n, ldp, 4 * n, n);
  if (rc) return rc;
  if (ldc < n) return fail(RYD_ERR_INVALID, "leading dimension too small");
  return RYD_OK;
}

// HIP events around one launch on a caller's stream (the *_device entry points);
// the destructor releases them on every path.
struct LaunchTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int start(hipStream_t s) {
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, s));
    return RYD_OK;
  }
  int stop(hipStream_t s, float* ms) {
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
    return RYD_OK;
  }
  ~LaunchTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// What the *_device entry points share: the slot check, the entry point's own validation
// (`check`), the slot's device, the caller's stream or else the slot's, and `go(stream)`
// between HIP events where elapsed_ms is asked for.
template <typename Check, typename Go>
int on_slot(ryd_handle* h, int slot, void* stream, float* elapsed_ms, Check&& check, Go&& go) {
  if (!h || slot < 0 || slot >= (int)h->dev.size()) return fail(RYD_ERR_INVALID, "bad handle/slot");
  int rc = check();
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->dev[slot]));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream[slot];
  LaunchTimer timer;
  if (elapsed_ms && (rc = timer.start(s))) return rc;
  if ((rc = go(s))) return rc;
  return elapsed_ms ? timer.stop(s, elapsed_ms) : RYD_OK;
}

// The ryd_stats of a host-form call: the timings, and the sums over the batch of the two
// summary rows that count iterations (summary = NULL: none, as for coherences).
void fill_stats(ryd_stats* st, const ryd_handle* h, double kms, double hms, double dms, const double* summary,
                int64_t ld, int64_t n, int row_useful, int row_exec) {
  if (!st) return;
  double u = 0.0, x = 0.0;
  for (int64_t i = 0; summary && i < n; ++i) {
    u += summary[(int64_t)row_useful * ld + i];
    x += summary[(int64_t)row_exec * ld + i];
  }
  *st = {kms, hms, dms, u, x, (int)h->dev.size(), 0};
}

// ryd_memcpy_h2d / ryd_memcpy_d2h: a blocking copy on the slot's stream
int slot_memcpy(ryd_handle* h, int slot, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (!h || slot < 0 || slot >= (int)h->dev.size()) return fail(RYD_ERR_INVALID, "bad args");
  HIPCHK(hipSetDevice(h->dev[slot]));
  // the slot's earlier work first: a copy to or from pageable memory is not reliably
  // ordered behind the kernels already on the stream
  HIPCHK(hipStreamSynchronize(h->stream[slot]));
  HIPCHK(hipMemcpyAsync(dst, src, bytes, kind, h->stream[slot]));
  HIPCHK(hipStreamSynchronize(h->stream[slot]));
  return RYD_OK;
}

// One output array of a partitioned run: `rows` rows of `per_point` doubles per point.
// stride > per_point (one row only): the caller's points are `stride` doubles apart (the
// Jacobian of ryd_run_schedule_kets with ld_jac > 4 n_seg); the device copy stays packed.
struct HostOut {
  double* host;
  int64_t ld;
  int rows;
  int per_point;
  int64_t stride = 0;
};

// A second per-point input of a partitioned run (the schedule table of ryd_run_schedule):
// `row` doubles per point at host + i ld, or one shared row.  A slot's rows are one contiguous
// block of the caller's table (the shared row: the row itself), staged and copied like the
// parameter columns; run_partitioned sets `dev` to the slot's copy before it calls launch_fn.
struct HostIn {
  const double* host;
  int64_t ld, row;
  bool shared;
  const double* dev = nullptr;
  size_t count(int64_t cnt) const { return (size_t)(shared ? row : (cnt - 1) * ld + row); }
};

// Host worker threads for staging copies: RYD_HOST_THREADS, else min(16, cores).
int host_threads() {
  const char* e = getenv("RYD_HOST_THREADS");
  int t = e ? atoi(e) : 0;
  if (t <= 0) t = std::min(16, (int)std::max(1u, std::thread::hardware_concurrency()));
  return t;
}

struct CopyTask {
  void* dst;
  const void* src;
  size_t bytes;
};

// Persistent host worker pool for the staging copies: created on the first large copy
// and kept for the life of the process (never joined: the workers sleep on a condition
// variable), so a call pays a wake-up, not a thread creation per worker.  One job at a
// time; the calling thread works on it too.
class HostPool {
 public:
  static HostPool& get() {
    static HostPool* p = new HostPool(host_threads() - 1);    // leaked on purpose (no exit-time join)
    return *p;
  }
  int workers() const { return (int)th_.size(); }
  // run every task of `tasks` on the caller + up to `helpers` workers; returns when done
  void run(const std::vector<CopyTask>& tasks, int helpers) {
    std::lock_guard<std::mutex> one(call_mu_);
    helpers = std::max(0, std::min(helpers, workers()));
    {
      std::lock_guard<std::mutex> lk(mu_);
      tasks_ = &tasks;
      next_.store(0);
      want_ = helpers;
      pending_ = helpers;
      ++gen_;
    }
    cv_.notify_all();
    drain(tasks);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return pending_ == 0; });
    tasks_ = nullptr;
  }

 private:
  explicit HostPool(int n) {
    for (int i = 0; i < n; ++i) th_.emplace_back([this, i] { loop(i); });
    for (auto& t : th_) t.detach();
  }
  void drain(const std::vector<CopyTask>& t) {
    for (size_t i; (i = next_.fetch_add(1)) < t.size();) memcpy(t[i].dst, t[i].src, t[i].bytes);
  }
  void loop(int id) {
    uint64_t seen = 0;
    for (;;) {
      const std::vector<CopyTask>* t;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (id >= want_) continue;               // not needed for this job
        t = tasks_;
      }
      drain(*t);
      std::lock_guard<std::mutex> lk(mu_);
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> th_;
  std::mutex call_mu_, mu_;
  std::condition_variable cv_, done_;
  const std::vector<CopyTask>* tasks_ = nullptr;
  std::atomic<size_t> next_{0};
  uint64_t gen_ = 0;
  int want_ = 0, pending_ = 0;
};

// memcpy a task list on the persistent pool (serial below 256 KiB); rows larger than
// 128 KiB are cut so the threads balance.
void parallel_copy(const std::vector<CopyTask>& in) {
  std::vector<CopyTask> tasks;
  size_t total = 0;
  const size_t cut = 128 << 10;
  for (const CopyTask& t : in) {
    total += t.bytes;
    for (size_t o = 0; o < t.bytes; o += cut)
      tasks.push_back({(char*)t.dst + o, (const char*)t.src + o, std::min(cut, t.bytes - o)});
  }
  const int helpers = (int)std::min<int64_t>(host_threads() - 1, (int64_t)tasks.size() - 1);
  if (total < (256u << 10) || helpers <= 0) {
    for (const CopyTask& t : tasks) memcpy(t.dst, t.src, t.bytes);
    return;
  }
  HostPool::get().run(tasks, helpers);
}

double host_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Grow slot k's device + pinned buffers to `bytes` and create its events (once).
int ensure_slot_work(ryd_handle* h, int k, size_t bytes) {
  ryd_slot_work& w = h->work[k];
  if (!w.ev_ok) {
    for (int j = 0; j < 4; ++j)
      if (!w.ev[j]) HIPCHK(hipEventCreate(&w.ev[j]));
    w.ev_ok = true;
  }
  if (w.dcap < bytes) {
    if (w.dbuf) HIPCHK(hipFree(w.dbuf));
    w.dbuf = nullptr;
    w.dcap = 0;
    const size_t cap = align256(bytes + bytes / 4);
    if (hipMalloc(&w.dbuf, cap) != hipSuccess) {
      w.dbuf = nullptr;
      return fail(RYD_ERR_ALLOC, "device workspace allocation failed");
    }
    w.dcap = cap;
  }
  if (w.hcap < bytes) {
    if (w.hbuf) HIPCHK(hipHostFree(w.hbuf));
    w.hbuf = nullptr;
    w.hcap = 0;
    const size_t cap = align256(bytes + bytes / 4);
    if (hipHostMalloc(&w.hbuf, cap, hipHostMallocPortable) != hipSuccess) {
      w.hbuf = nullptr;
      return fail(RYD_ERR_ALLOC, "pinned staging allocation failed");
    }
    w.hcap = cap;
  }
  return RYD_OK;
}

void release_slot_work(ryd_slot_work& w) {
  if (w.dbuf) (void)hipFree(w.dbuf);
  if (w.hbuf) (void)hipHostFree(w.hbuf);
  for (int j = 0; j < 4; ++j)
    if (w.ev[j]) (void)hipEventDestroy(w.ev[j]);
  for (int j = 0; j < 2; ++j)
    if (w.mark[j]) (void)hipEventDestroy(w.mark[j]);
  w = ryd_slot_work();
}

// Range-partition n points over the handle's devices (point i -> slot
// floor(nd*i/n)), one stream each, no inter-device traffic.
// Every slot's parameter columns are packed into its pinned staging buffer in one
// parallel pass first; then per slot, in order, H2D + `launch_fn(dp, cnt, ldp, off,
// dev_outs, dstat, stream)`; then every slot's D2H into staging -- all enqueued before the first wait, so devices
// (and same-device slots) overlap -- then wait slot by slot and unpack staging into
// the caller's strided buffers with host threads.  Device workspace and staging
// persist in the handle.  Device times are the max over slots; the per-slot event
// timeline and the host pack/unpack times go to h->timeline (ryd_last_timeline).
template <typename LaunchFn>
int run_partitioned(ryd_handle* h, const double* params, int64_t n, int64_t ld_params,
                    const std::vector<HostOut>& outs, uint32_t* out_status, LaunchFn launch_fn,
                    double& kms, double& hms, double& dms, HostIn* extra = nullptr) {
  std::lock_guard<std::mutex> lock(h->mu);
  const auto t_call = std::chrono::steady_clock::now();
  const int nd = (int)h->dev.size();
  const int no = (int)outs.size();
  if ((int)h->work.size() < nd) h->work.resize(nd);
  struct Part {
    int64_t off, cnt;
    size_t o_par, o_st, o_in = 0;
    std::vector<size_t> o_out;
    bool queued;
    double t_enq = 0.0, t_wait = 0.0;    // host ms since the call began: kernel enqueued, wait began
  };
  std::vector<Part> parts(nd);
  kms = hms = dms = 0.0;
  double pack_ms = 0.0, unpack_ms = 0.0;
  auto drain = [&](int upto) {   // error path: wait for what was already enqueued
    for (int k = 0; k < upto; ++k)
      if (parts[k].queued) {
        (void)hipSetDevice(h->dev[k]);
        (void)hipStreamSynchronize(h->stream[k]);
      }
  };
  // (1) partition + workspace for every slot, (2) pack every slot's parameter columns in
  // ONE parallel pass, (3) enqueue H2D + kernel slot by slot: slot k+1's H2D no longer
  // waits for slot k+1's pack behind slot k's enqueue.
  for (int k = 0; k < nd; ++k) {
    Part& P = parts[k];
    P.off = n * k / nd;
    P.cnt = n * (k + 1) / nd - P.off;
    P.queued = false;
    if (P.cnt == 0) continue;
    size_t at = 0;
    P.o_par = at;
    at = align256(at + sizeof(double) * RYD_NPARAM * P.cnt);
    P.o_out.resize(no);
    for (int j = 0; j < no; ++j) {
      P.o_out[j] = at;
      at = align256(at + sizeof(double) * outs[j].rows * outs[j].per_point * P.cnt);
    }
    P.o_st = at;
    at = align256(at + sizeof(uint32_t) * P.cnt);
    if (extra) {
      P.o_in = at;
      at = align256(at + sizeof(double) * extra->count(P.cnt));
    }
    hipError_t e = hipSetDevice(h->dev[k]);
    if (e != hipSuccess) return fail(RYD_ERR_HIP, std::string("set device: ") + hipGetErrorString(e));
    int rc = ensure_slot_work(h, k, at);
    if (rc) return rc;
  }
  {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<CopyTask> pack;
    for (int k = 0; k < nd; ++k) {
      const Part& P = parts[k];
      if (P.cnt == 0) continue;
      char* hb = (char*)h->work[k].hbuf;
      for (int c = 0; c < RYD_NPARAM; ++c)
        pack.push_back({hb + P.o_par + sizeof(double) * c * P.cnt, params + (int64_t)c * ld_params + P.off,
                        sizeof(double) * P.cnt});
      if (extra)
        pack.push_back({hb + P.o_in, extra->host + (extra->shared ? 0 : P.off * extra->ld),
                        sizeof(double) * extra->count(P.cnt)});
    }
    parallel_copy(pack);
    pack_ms = host_ms_since(t0);
  }
  for (int k = 0; k < nd; ++k) {
    Part& P = parts[k];
    if (P.cnt == 0) continue;
    hipError_t e = hipSetDevice(h->dev[k]);
    if (e != hipSuccess) {
      drain(k);
      return fail(RYD_ERR_HIP, std::string("set device: ") + hipGetErrorString(e));
    }
    ryd_slot_work& W = h->work[k];
    char* hb = (char*)W.hbuf;
    char* db = (char*)W.dbuf;
    hipStream_t s = h->stream[k];
    std::vector<double*> dout(no);
    for (int j = 0; j < no; ++j) dout[j] = (double*)(db + P.o_out[j]);
    e = hipEventRecord(W.ev[0], s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(db + P.o_par, hb + P.o_par, sizeof(double) * RYD_NPARAM * P.cnt,
                         hipMemcpyHostToDevice, s);
    if (e == hipSuccess && extra) {
      e = hipMemcpyAsync(db + P.o_in, hb + P.o_in, sizeof(double) * extra->count(P.cnt), hipMemcpyHostToDevice, s);
      extra->dev = (const double*)(db + P.o_in);
    }
    if (e == hipSuccess) e = hipEventRecord(W.ev[1], s);
    if (e != hipSuccess) {
      drain(k);
      (void)hipStreamSynchronize(s);
      return fail(RYD_ERR_HIP, std::string("h2d: ") + hipGetErrorString(e));
    }
    P.queued = true;
    int rc = launch_fn((const double*)(db + P.o_par), P.cnt, P.cnt, P.off, dout, (uint32_t*)(db + P.o_st), s);
    if (rc) {
      drain(k + 1);
      return rc;
    }
    e = hipEventRecord(W.ev[2], s);
    if (e != hipSuccess) {
      drain(k + 1);
      return fail(RYD_ERR_HIP, std::string("event: ") + hipGetErrorString(e));
    }
    P.t_enq = host_ms_since(t_call);
  }
  // D2Hs only after every slot's H2D: copies of one device's streams share its DMA
  // rings in submission order, so a D2H (waiting for its kernel) enqueued before the
  // next slot's H2D would hold that H2D back until the kernel ends.
  for (int k = 0; k < nd; ++k) {
    Part& P = parts[k];
    if (P.cnt == 0) continue;
    ryd_slot_work& W = h->work[k];
    (void)hipSetDevice(h->dev[k]);
    hipStream_t s = h->stream[k];
    // outputs + status are contiguous in the workspace: one D2H
    hipError_t e = hipMemcpyAsync((char*)W.hbuf + P.o_out.front(), (char*)W.dbuf + P.o_out.front(),
                                  P.o_st + sizeof(uint32_t) * P.cnt - P.o_out.front(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(W.ev[3], s);
    if (e != hipSuccess) {
      drain(nd);
      return fail(RYD_ERR_HIP, std::string("d2h: ") + hipGetErrorString(e));
    }
  }
  hipError_t err = hipSuccess;
  h->timeline.assign(RYD_TL_HEAD + RYD_TL_SLOT * (size_t)nd, 0.0);
  std::vector<hipEvent_t> origin(nd, nullptr);   // first slot's start event, per device
  for (int k = 0; k < nd; ++k) {
    Part& P = parts[k];
    double* tl = &h->timeline[RYD_TL_HEAD + RYD_TL_SLOT * (size_t)k];
    tl[0] = h->dev[k];
    tl[5] = (double)P.cnt;
    if (P.cnt == 0) continue;
    ryd_slot_work& W = h->work[k];
    (void)hipSetDevice(h->dev[k]);
    P.t_wait = host_ms_since(t_call);
    tl[6] = P.t_enq;
    tl[7] = P.t_wait;
    hipError_t e = hipStreamSynchronize(h->stream[k]);
    if (e != hipSuccess) {
      err = e;
      continue;
    }
    float t;
    if (hipEventElapsedTime(&t, W.ev[0], W.ev[1]) == hipSuccess) hms = std::max(hms, (double)t);
    if (hipEventElapsedTime(&t, W.ev[1], W.ev[2]) == hipSuccess) kms = std::max(kms, (double)t);
    if (hipEventElapsedTime(&t, W.ev[2], W.ev[3]) == hipSuccess) dms = std::max(dms, (double)t);
    hipEvent_t o = W.ev[0];
    for (int j = 0; j < k; ++j)
      if (h->dev[j] == h->dev[k] && parts[j].cnt > 0) {
        o = h->work[j].ev[0];
        break;
      }
    for (int j = 1; j < 4; ++j)
      if (hipEventElapsedTime(&t, o, W.ev[j - 1]) == hipSuccess) tl[j] = t;
    if (hipEventElapsedTime(&t, o, W.ev[3]) == hipSuccess) tl[4] = t;
    const auto t0 = std::chrono::steady_clock::now();
    const char* hb = (const char*)W.hbuf;
    std::vector<CopyTask> unpack;
    for (int j = 0; j < no; ++j) {
      const int64_t w = (int64_t)outs[j].per_point * P.cnt;
      if (outs[j].stride > outs[j].per_point) {          // point by point, the caller's padding untouched
        for (int64_t i = 0; i < P.cnt; ++i)
          unpack.push_back({outs[j].host + (P.off + i) * outs[j].stride,
                            hb + P.o_out[j] + sizeof(double) * i * outs[j].per_point,
                            sizeof(double) * outs[j].per_point});
        continue;
      }
      for (int r = 0; r < outs[j].rows; ++r)
        unpack.push_back({outs[j].host + (int64_t)r * outs[j].ld + (int64_t)outs[j].per_point * P.off,
                          hb + P.o_out[j] + sizeof(double) * r * w, sizeof(double) * w});
    }
    unpack.push_back({out_status + P.off, hb + P.o_st, sizeof(uint32_t) * P.cnt});
    parallel_copy(unpack);
    unpack_ms += host_ms_since(t0);
  }
  h->timeline[0] = nd;
  h->timeline[1] = pack_ms;
  h->timeline[2] = unpack_ms;
  h->timeline[3] = host_ms_since(t_call);
  if (err != hipSuccess) return fail(RYD_ERR_HIP, std::string("batch: ") + hipGetErrorString(err));
  return RYD_OK;
}

// The host-form entry points after their own validation: the handle and NULL checks (the last
// array of `outs` is the one every call requires: the summary, or the coherence rows),
// run_partitioned with the optional second input `tab`, and the stats.  counts: the last array
// is a summary whose iteration rows the stats sum.  The launch callable gets the slot's points
// and its device arrays in the order of `outs`: go(dp, cnt, ldp, o, dstat, stream).
template <typename Go>
int run_host(ryd_handle* h, const double* params, int64_t n, int64_t ld_params, const std::vector<HostOut>& outs,
             HostIn* tab, uint32_t* out_status, ryd_stats* stats, bool counts, Go&& go) {
  if (!h) return fail(RYD_ERR_INVALID, "handle is NULL");
  const HostOut& req = outs.back();
  if (n > 0 && (!params || !req.host || !out_status)) return fail(RYD_ERR_INVALID, "NULL buffer");
  double kms, hms, dms;
  int rc = run_partitioned(
      h, params, n, ld_params, outs, out_status,
      [&](const double* dp, int64_t cnt, int64_t ldp, int64_t, const std::vector<double*>& o, uint32_t* dst,
          hipStream_t s) { return go(dp, cnt, ldp, o, dst, s); },
      kms, hms, dms, tab);
  if (rc) return rc;
  fill_stats(stats, h, kms, hms, dms, counts ? req.host : nullptr, req.ld, n, RYD_S_NMV_USEFUL, RYD_S_NMV_EXEC);
  return RYD_OK;
}

// The caller's schedule table as run_partitioned's second input
HostIn sched_table_in(const ryd_sched_desc* d, const double* sched, int64_t ld_sched) {
  return {sched, ld_sched, (int64_t)RYD_SC_NFIELD * d->n_seg, (d->flags & RYD_SCHED_SHARED) != 0};
}

// The output list of a summary-carrying call: the state rows (out_state NULL: a summary-only
// call, whose device workspace, staging buffer, D2H and unpack carry no state rows), a Jacobian
// of jw doubles per point (packed on the device: its leading dimension there is jw; the caller's
// points are ld_jac apart, as the table's are on the way in), then the summary.
std::vector<HostOut> summary_outs(double* out_state, int64_t ld_state, int state_rows, double* out_summary,
                                  int64_t ld_summary, double* out_jac = nullptr, int jw = 0, int64_t ld_jac = 0) {
  std::vector<HostOut> outs;
  if (out_state) outs.push_back({out_state, ld_state, state_rows, 4});
  if (out_jac) outs.push_back({out_jac, 0, 1, jw, ld_jac});
  outs.push_back({out_summary, ld_summary, RYD_NSUMMARY, 1});
  return outs;
}

// ryd_run_schedule_kets and (ctl: the Jacobian four fields wide) ryd_run_schedule_kets_ctl after
// validation
int run_schedule_kets_host(bool ctl, ryd_handle* h, const ryd_sched_desc* desc, const double* params, int64_t n,
                           int64_t ld_params, const double* sched, int64_t ld_sched, double* out_state,
                           int64_t ld_state, double* out_summary, int64_t ld_summary, double* out_jac,
                           int64_t ld_jac, uint32_t* out_status, ryd_stats* stats) {
  const int jw = (ctl ? 4 : 1) * RYD_SC_NFIELD * desc->n_seg;
  HostIn tab = sched_table_in(desc, sched, ld_sched);
  return run_host(h, params, n, ld_params,
                  summary_outs(out_state, ld_state, ryd_state_width(RYD_EVOL_KET, 3), out_summary, ld_summary, out_jac,
                               jw, ld_jac),
                  &tab, out_status, stats, true,
                  [&](const double* dp, int64_t cnt, int64_t ldp, const std::vector<double*>& o, uint32_t* dst,
                      hipStream_t s) {
                    return launch_schedule_kets(ctl, desc, dp, cnt, ldp, tab.dev, ld_sched,
                                                out_state ? o[0] : nullptr, 4 * cnt, o.back(), cnt,
                                                out_jac ? o[out_state ? 1 : 0] : nullptr, jw, dst, s);
                  });
}

// three-atom quantum-jump trajectories (BASELINE configs[4])
#include "ryd_traj.inc"
#include "ryd_generic.inc"

// hot-path row a1 on the device: parameter derivation (ryd_derive)
#include "ryd_derive.inc"

// host epilogue: the reference's mixed-state controlled phase (ryd_mixed_phase)
#include "ryd_epilogue.inc"

}  // namespace

extern "C" {

int ryd_abi_version(void) { return RYD_ABI_VERSION; }
const char* ryd_last_error(void) { return g_err.c_str(); }
int ryd_param_count(void) { return RYD_NPARAM; }
int ryd_summary_width(void) { return RYD_NSUMMARY; }
int ryd_lp_unsquared(void) { return RYD_LP_UNSQUARED; }

int64_t ryd_sym16_balance_plan(int64_t n, int cus, int gpc_override, int64_t* head, int32_t* role, int64_t* job,
                               uint8_t* present, int64_t cap) {
  S16Plan pl;
  if (!head || !sym16_plan(n, cus, gpc_override, &pl)) return -1;
  head[0] = pl.groups;
  head[1] = pl.workgroups;
  head[2] = pl.waves;
  head[3] = pl.gpc;
  head[4] = pl.auto_on ? 1 : 0;
  const int64_t need = pl.workgroups * pl.waves;
  if (!role || !job || !present || cap < need) return need;
  for (int64_t b = 0; b < pl.workgroups; ++b)
    for (int w = 0; w < pl.waves; ++w) {
      const S16Role r = s16_bal_role(pl.gpc, w);
      const int64_t j = s16_bal_job(b, pl.workgroups, r.off);   // the kernel's own expressions
      role[b * pl.waves + w] = r.role;
      job[b * pl.waves + w] = j;
      present[b * pl.waves + w] = j < pl.groups ? 1 : 0;
    }
  return need;
}
int ryd_state_width(int evolution, int dim) {
  if (dim != 3 && dim != 4) return -1;
  if (evolution == RYD_EVOL_LINDBLAD) return dim == 3 ? 25 : 36;
  if (evolution == RYD_EVOL_KET) return dim == 3 ? 18 : 32;
  return -1;
}

int ryd_device_count(int* count) {
  if (!count) return fail(RYD_ERR_INVALID, "count is NULL");
  int c = 0;
  HIPCHK(hipGetDeviceCount(&c));
  *count = c;
  return RYD_OK;
}

int ryd_create(const int* device_ids, int n_devices, ryd_handle** out) {
  if (!out) return fail(RYD_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int avail = 0;
  HIPCHK(hipGetDeviceCount(&avail));
  ryd_handle* h = new ryd_handle();
  if (n_devices <= 0 || !device_ids) {
    h->dev.push_back(0);
  } else {
    for (int k = 0; k < n_devices; ++k) h->dev.push_back(device_ids[k]);
  }
  for (int d : h->dev) {
    if (d < 0 || d >= avail) {
      delete h;
      return fail(RYD_ERR_INVALID, "device id out of range");
    }
    hipStream_t s;
    hipError_t e = hipSetDevice(d);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) {
      for (size_t j = 0; j < h->stream.size(); ++j) (void)hipStreamDestroy(h->stream[j]);
      delete h;
      return fail(RYD_ERR_HIP, std::string("stream create: ") + hipGetErrorString(e));
    }
    h->stream.push_back(s);
  }
  *out = h;
  return RYD_OK;
}

int ryd_destroy(ryd_handle* h) {
  if (!h) return RYD_OK;
  for (size_t k = 0; k < h->dev.size(); ++k) {
    (void)hipSetDevice(h->dev[k]);
    (void)hipStreamSynchronize(h->stream[k]);
    if (k < h->work.size()) release_slot_work(h->work[k]);
    (void)hipStreamDestroy(h->stream[k]);
  }
  delete h;
  return RYD_OK;
}

int ryd_malloc(ryd_handle* h, int slot, size_t bytes, void** p) {
  if (!h || !p || slot < 0 || slot >= (int)h->dev.size()) return fail(RYD_ERR_INVALID, "bad args");
  HIPCHK(hipSetDevice(h->dev[slot]));
  hipError_t e = hipMalloc(p, bytes ? bytes : 16);
  if (e != hipSuccess) return fail(RYD_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
  return RYD_OK;
}

int ryd_free(ryd_handle* h, int slot, void* p) {
  if (!h || slot < 0 || slot >= (int)h->dev.size()) return fail(RYD_ERR_INVALID, "bad args");
  HIPCHK(hipSetDevice(h->dev[slot]));
  HIPCHK(hipFree(p));
  return RYD_OK;
}

int ryd_memcpy_h2d(ryd_handle* h, int slot, void* dst, const void* src, size_t bytes) {
  return slot_memcpy(h, slot, dst, src, bytes, hipMemcpyHostToDevice);
}

int ryd_memcpy_d2h(ryd_handle* h, int slot, void* dst, const void* src, size_t bytes) {
  return slot_memcpy(h, slot, dst, src, bytes, hipMemcpyDeviceToHost);
}

int ryd_last_timeline(ryd_handle* h, double* out, int64_t cap) {
  if (!h || !out) return fail(RYD_ERR_INVALID, "bad args");
  std::lock_guard<std::mutex> lock(h->mu);
  if (h->timeline.empty()) return fail(RYD_ERR_INVALID, "no host-buffer call on this handle yet");
  if (cap < (int64_t)h->timeline.size()) return fail(RYD_ERR_INVALID, "timeline buffer too small");
  memcpy(out, h->timeline.data(), sizeof(double) * h->timeline.size());
  return RYD_OK;
}

int ryd_mark(ryd_handle* h, int slot, int mark) {
  if (!h || slot < 0 || slot >= (int)h->dev.size() || mark < 0 || mark > 1) return fail(RYD_ERR_INVALID, "bad args");
  std::lock_guard<std::mutex> lock(h->mu);
  if ((int)h->work.size() < (int)h->dev.size()) h->work.resize(h->dev.size());
  ryd_slot_work& w = h->work[slot];
  HIPCHK(hipSetDevice(h->dev[slot]));
  if (!w.mark[mark]) HIPCHK(hipEventCreate(&w.mark[mark]));
  HIPCHK(hipEventRecord(w.mark[mark], h->stream[slot]));
  return RYD_OK;
}

int ryd_mark_elapsed(ryd_handle* h, int slot, float* ms) {
  if (!h || !ms || slot < 0 || slot >= (int)h->dev.size()) return fail(RYD_ERR_INVALID, "bad args");
  std::lock_guard<std::mutex> lock(h->mu);
  if ((int)h->work.size() <= slot || !h->work[slot].mark[0] || !h->work[slot].mark[1])
    return fail(RYD_ERR_INVALID, "ryd_mark 0 and 1 not recorded on this slot");
  ryd_slot_work& w = h->work[slot];
  HIPCHK(hipSetDevice(h->dev[slot]));
  HIPCHK(hipEventSynchronize(w.mark[1]));
  HIPCHK(hipEventElapsedTime(ms, w.mark[0], w.mark[1]));
  return RYD_OK;
}

int ryd_synchronize(ryd_handle* h) {
  if (!h) return fail(RYD_ERR_INVALID, "handle is NULL");
  for (size_t k = 0; k < h->dev.size(); ++k) {
    HIPCHK(hipSetDevice(h->dev[k]));
    HIPCHK(hipStreamSynchronize(h->stream[k]));
  }
  return RYD_OK;
}

int ryd_batch_path(const ryd_batch_desc* desc, int has_state) {
  if (int rc = validate(desc, 0, 0, 0, 0)) return rc;
  const BatchPath path = batch_path(desc);
  return !has_state && takes_twin(path) ? path | RYD_PATH_NOSTATE : path;
}

int ryd_run_batch_device(ryd_handle* h, int slot, const ryd_batch_desc* desc, const double* d_params,
                         int64_t n, int64_t ld_params, double* d_state, int64_t ld_state,
                         double* d_summary, int64_t ld_summary, uint32_t* d_status, void* stream,
                         float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms,
      [&] { return validate(desc, n, ld_params, ld_state, ld_summary, d_state != nullptr); },
      [&](hipStream_t s) {
        return launch(desc, d_params, n, ld_params, d_state, ld_state, d_summary, ld_summary, d_status, s);
      });
}

int ryd_run_batch(ryd_handle* h, const ryd_batch_desc* desc, const double* params, int64_t n,
                  int64_t ld_params, double* out_state, int64_t ld_state, double* out_summary,
                  int64_t ld_summary, uint32_t* out_status, ryd_stats* stats) {
  if (!h) return fail(RYD_ERR_INVALID, "handle is NULL");
  if (int rc = validate(desc, n, ld_params, ld_state, ld_summary, out_state != nullptr)) return rc;
  return run_host(h, params, n, ld_params,
                  summary_outs(out_state, ld_state, ryd_state_width(desc->evolution, desc->dim), out_summary, ld_summary),
                  nullptr, out_status, stats, true,
                  [&](const double* dp, int64_t cnt, int64_t ldp, const std::vector<double*>& o, uint32_t* dst,
                      hipStream_t s) {
                    return launch(desc, dp, cnt, ldp, out_state ? o[0] : nullptr, 4 * cnt, o.back(), cnt, dst, s);
                  });
}

int ryd_run_schedule_device(ryd_handle* h, int slot, const ryd_sched_desc* desc, const double* d_params,
                            int64_t n, int64_t ld_params, const double* d_sched, int64_t ld_sched,
                            double* d_state, int64_t ld_state, double* d_summary, int64_t ld_summary,
                            uint32_t* d_status, void* stream, float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms,
      [&] { return validate_schedule(desc, d_sched, n, ld_params, ld_sched, ld_state, ld_summary, d_state != nullptr); },
      [&](hipStream_t s) {
        return launch_schedule(desc, d_params, n, ld_params, d_sched, ld_sched, d_state, ld_state, d_summary,
                               ld_summary, d_status, s);
      });
}

int ryd_run_schedule(ryd_handle* h, const ryd_sched_desc* desc, const double* params, int64_t n,
                     int64_t ld_params, const double* sched, int64_t ld_sched, double* out_state,
                     int64_t ld_state, double* out_summary, int64_t ld_summary, uint32_t* out_status,
                     ryd_stats* stats) {
  // the descriptor first, so that each refusal reports its own reason with or without a handle
  // (so in every host-form schedule call)
  if (int rc = validate_schedule(desc, sched, n, ld_params, ld_sched, ld_state, ld_summary, out_state != nullptr))
    return rc;
  HostIn tab = sched_table_in(desc, sched, ld_sched);
  return run_host(h, params, n, ld_params, summary_outs(out_state, ld_state, NC, out_summary, ld_summary), &tab,
                  out_status, stats, true,
                  [&](const double* dp, int64_t cnt, int64_t ldp, const std::vector<double*>& o, uint32_t* dst,
                      hipStream_t s) {
                    return launch_schedule(desc, dp, cnt, ldp, tab.dev, ld_sched, out_state ? o[0] : nullptr, 4 * cnt,
                                           o.back(), cnt, dst, s);
                  });
}

int ryd_run_schedule_kets_device(ryd_handle* h, int slot, const ryd_sched_desc* desc, const double* d_params,
                                 int64_t n, int64_t ld_params, const double* d_sched, int64_t ld_sched,
                                 double* d_state, int64_t ld_state, double* d_summary, int64_t ld_summary,
                                 double* d_jac, int64_t ld_jac, uint32_t* d_status, void* stream,
                                 float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms,
      [&] {
        return validate_schedule_kets(desc, d_sched, n, ld_params, ld_sched, ld_state, ld_summary, d_state != nullptr,
                                      ld_jac, d_jac != nullptr);
      },
      [&](hipStream_t s) {
        return launch_schedule_kets(false, desc, d_params, n, ld_params, d_sched, ld_sched, d_state, ld_state,
                                    d_summary, ld_summary, d_jac, ld_jac, d_status, s);
      });
}

int ryd_run_schedule_kets(ryd_handle* h, const ryd_sched_desc* desc, const double* params, int64_t n,
                          int64_t ld_params, const double* sched, int64_t ld_sched, double* out_state,
                          int64_t ld_state, double* out_summary, int64_t ld_summary, double* out_jac,
                          int64_t ld_jac, uint32_t* out_status, ryd_stats* stats) {
  if (int rc = validate_schedule_kets(desc, sched, n, ld_params, ld_sched, ld_state, ld_summary,
                                      out_state != nullptr, ld_jac, out_jac != nullptr))
    return rc;
  return run_schedule_kets_host(false, h, desc, params, n, ld_params, sched, ld_sched, out_state, ld_state, out_summary,
                                ld_summary, out_jac, ld_jac, out_status, stats);
}

int ryd_run_schedule_kets_ctl_device(ryd_handle* h, int slot, const ryd_sched_desc* desc, const double* d_params,
                                     int64_t n, int64_t ld_params, const double* d_sched, int64_t ld_sched,
                                     double* d_state, int64_t ld_state, double* d_summary, int64_t ld_summary,
                                     double* d_jac, int64_t ld_jac, uint32_t* d_status, void* stream,
                                     float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms,
      [&] {
        return validate_schedule_kets_ctl(desc, d_sched, n, ld_params, ld_sched, ld_state, ld_summary,
                                          d_state != nullptr, d_jac, ld_jac);
      },
      [&](hipStream_t s) {
        return launch_schedule_kets(true, desc, d_params, n, ld_params, d_sched, ld_sched, d_state, ld_state,
                                    d_summary, ld_summary, d_jac, ld_jac, d_status, s);
      });
}

int ryd_run_schedule_kets_ctl(ryd_handle* h, const ryd_sched_desc* desc, const double* params, int64_t n,
                              int64_t ld_params, const double* sched, int64_t ld_sched, double* out_state,
                              int64_t ld_state, double* out_summary, int64_t ld_summary, double* out_jac,
                              int64_t ld_jac, uint32_t* out_status, ryd_stats* stats) {
  if (int rc = validate_schedule_kets_ctl(desc, sched, n, ld_params, ld_sched, ld_state, ld_summary,
                                          out_state != nullptr, out_jac, ld_jac))
    return rc;
  return run_schedule_kets_host(true, h, desc, params, n, ld_params, sched, ld_sched, out_state, ld_state, out_summary,
                                ld_summary, out_jac, ld_jac, out_status, stats);
}

int ryd_run_coherences(ryd_handle* h, const ryd_batch_desc* desc, const double* params, int64_t n,
                       int64_t ld_params, double* out_coh, int64_t ld_coh, uint32_t* out_status,
                       ryd_stats* stats) {
  if (!h) return fail(RYD_ERR_INVALID, "handle is NULL");
  if (int rc = validate_coherences(desc, n, ld_params, ld_coh)) return rc;
  return run_host(h, params, n, ld_params, {{out_coh, ld_coh, RYD_NCOH, 1}}, nullptr, out_status, stats, false,
                  [&](const double* dp, int64_t cnt, int64_t ldp, const std::vector<double*>& o, uint32_t* dst,
                      hipStream_t s) { return launch_coherences(desc, dp, cnt, ldp, o[0], cnt, dst, s); });
}

int ryd_run_schedule_coherences(ryd_handle* h, const ryd_sched_desc* desc, const double* params, int64_t n,
                                int64_t ld_params, const double* sched, int64_t ld_sched, double* out_coh,
                                int64_t ld_coh, uint32_t* out_status, ryd_stats* stats) {
  if (int rc = validate_schedule_coherences(desc, sched, n, ld_params, ld_sched, ld_coh)) return rc;
  HostIn tab = sched_table_in(desc, sched, ld_sched);
  return run_host(h, params, n, ld_params, {{out_coh, ld_coh, RYD_NCOH, 1}}, &tab, out_status, stats, false,
                  [&](const double* dp, int64_t cnt, int64_t ldp, const std::vector<double*>& o, uint32_t* dst,
                      hipStream_t s) {
                    return launch_schedule_coherences(desc, dp, cnt, ldp, tab.dev, ld_sched, o[0], cnt, dst, s);
                  });
}

int ryd_run_schedule_coherences_device(ryd_handle* h, int slot, const ryd_sched_desc* desc, const double* d_params,
                                       int64_t n, int64_t ld_params, const double* d_sched, int64_t ld_sched,
                                       double* d_coh, int64_t ld_coh, uint32_t* d_status, void* stream,
                                       float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms,
      [&] { return validate_schedule_coherences(desc, d_sched, n, ld_params, ld_sched, ld_coh); },
      [&](hipStream_t s) {
        return launch_schedule_coherences(desc, d_params, n, ld_params, d_sched, ld_sched, d_coh, ld_coh, d_status,
                                          s);
      });
}

int ryd_run_trajectories(ryd_handle* h, const ryd_traj_desc* desc, const double* params, int64_t n,
                         int64_t ld_params, double* out_rho, double* out_se, double* out_summary,
                         int64_t ld_summary, double* out_records, uint32_t* out_status, ryd_stats* stats) {
  if (!h) return fail(RYD_ERR_INVALID, "handle is NULL");
  int rc = validate_traj(desc, n, ld_params);
  if (rc) return rc;
  if (ld_summary < n) return fail(RYD_ERR_INVALID, "leading dimension too small");
  if (n > 0 && (!params || !out_rho || !out_se || !out_summary || !out_status))
    return fail(RYD_ERR_INVALID, "NULL buffer");
  // point-major rows: one "row" of width*cnt doubles per shard
  std::vector<HostOut> outs = {{out_rho, RYD_T_RHO_WIDTH, 1, RYD_T_RHO_WIDTH},
                               {out_se, RYD_T_SE_WIDTH, 1, RYD_T_SE_WIDTH},
                               {out_summary, ld_summary, RYD_T_NSUMMARY, 1}};
  if (out_records) outs.push_back({out_records, 0, 1, RYD_T_REC_WIDTH * desc->n_traj});
  double kms, hms, dms;
  rc = run_partitioned(
      h, params, n, ld_params, outs, out_status,
      [&](const double* dp, int64_t cnt, int64_t ldp, int64_t off, const std::vector<double*>& o,
          uint32_t* dst, hipStream_t s) {
        return launch_traj(desc, dp, cnt, ldp, off, o[0], RYD_T_RHO_WIDTH, o[1], RYD_T_SE_WIDTH, o[2], cnt,
                           out_records ? o[3] : nullptr, dst, s);
      },
      kms, hms, dms);
  if (rc) return rc;
  fill_stats(stats, h, kms, hms, dms, out_summary, ld_summary, n, RYD_TS_ITER_USEFUL, RYD_TS_ITER_EXEC);
  return RYD_OK;
}

int ryd_evolve_generic(ryd_handle* h, int dim, int n_seg, int n_ops, int64_t n, int ket, const double* H,
                       const double* dt, const double* ops, const double* state0, double* state_out,
                       uint32_t* status) {
  if (!h || h->dev.empty()) return fail(RYD_ERR_INVALID, "handle is NULL");
  if (dim < 1 || dim > GN_DMAX || n_seg < 1 || n_ops < 0 || n_ops > (GN_ROWS - 1) / GN_DMAX || n < 0)
    return fail(RYD_ERR_INVALID, "evolve_generic: need 1 <= dim <= 16, n_seg >= 1, 0 <= n_ops <= 32, n >= 0");
  if (ket && n_ops > 0)
    return fail(RYD_ERR_INVALID, "evolve_generic: kets evolve without jump operators (with them, pass rho)");
  if (n == 0) return RYD_OK;
  if (n > 0x7fffffffLL) return fail(RYD_ERR_INVALID, "evolve_generic: batch too large for one launch");
  if (!H || !dt || !state0 || !state_out || !status || (n_ops > 0 && !ops))
    return fail(RYD_ERR_INVALID, "evolve_generic: NULL buffer");
  return run_generic(h->dev[0], h->stream[0], dim, n_seg, n_ops, n, ket, H, dt, ops, state0, state_out, status);
}

int ryd_run_trajectories_device(ryd_handle* h, int slot, const ryd_traj_desc* desc, const double* d_params,
                                int64_t n, int64_t ld_params, int64_t point_offset, double* d_rho,
                                int64_t ld_rho, double* d_se, int64_t ld_se, double* d_summary,
                                int64_t ld_summary, double* d_records, uint32_t* d_status, void* stream,
                                float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms,
      [&] {
        if (int rc = validate_traj(desc, n, ld_params)) return rc;
        if (ld_rho < RYD_T_RHO_WIDTH || ld_se < RYD_T_SE_WIDTH || ld_summary < n || point_offset < 0)
          return fail(RYD_ERR_INVALID, "leading dimension too small or negative point_offset");
        return RYD_OK;
      },
      [&](hipStream_t s) {
        return launch_traj(desc, d_params, n, ld_params, point_offset, d_rho, ld_rho, d_se, ld_se, d_summary,
                           ld_summary, d_records, d_status, s);
      });
}

int ryd_run_coherences_device(ryd_handle* h, int slot, const ryd_batch_desc* desc, const double* d_params,
                              int64_t n, int64_t ld_params, double* d_coh, int64_t ld_coh,
                              uint32_t* d_status, void* stream, float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms, [&] { return validate_coherences(desc, n, ld_params, ld_coh); },
      [&](hipStream_t s) { return launch_coherences(desc, d_params, n, ld_params, d_coh, ld_coh, d_status, s); });
}

int ryd_derive_device(ryd_handle* h, int slot, const ryd_derive_desc* desc, const double* d_in, int64_t ld_in,
                      int64_t n, double* d_params, int64_t ld_params, uint32_t* d_warn, double* d_diag,
                      int64_t ld_diag, void* stream, float* elapsed_ms) {
  return on_slot(
      h, slot, stream, elapsed_ms, [] { return RYD_OK; },      // launch_derive validates
      [&](hipStream_t s) {
        return launch_derive(desc, d_in, ld_in, n, d_params, ld_params, d_warn, d_diag, ld_diag, s);
      });
}

int ryd_derive(ryd_handle* h, const ryd_derive_desc* desc, const double* in, int64_t n_cols, int64_t ld_in,
               int64_t n, double* params, int64_t ld_params, uint32_t* warn, double* diag, int64_t ld_diag) {
  if (!h || h->dev.empty() || !desc) return fail(RYD_ERR_INVALID, "derive: NULL handle/desc");
  if (n < 0 || n_cols < 0 || ld_params < n || (diag && ld_diag < n) || (n_cols > 0 && (!in || ld_in < n)))
    return fail(RYD_ERR_INVALID, "derive: bad sizes");
  for (int f = 0; f < RYD_DV_NFIELD; ++f)
    if (desc->col[f] >= n_cols) return fail(RYD_ERR_INVALID, "derive: a field's column is beyond n_cols");
  if (n == 0) return RYD_OK;
  if (!params || !warn) return fail(RYD_ERR_INVALID, "derive: NULL output");
  const int dev = h->dev[0];
  hipStream_t s = h->stream[0];
  HIPCHK(hipSetDevice(dev));
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t bIn = sizeof(double) * (size_t)n_cols * n, bP = sizeof(double) * RYD_NPARAM * (size_t)n,
               bW = sizeof(uint32_t) * (size_t)n, bD = diag ? sizeof(double) * RYD_DV_NDIAG * (size_t)n : 0;
  const size_t oP = al(bIn), oW = oP + al(bP), oD = oW + al(bW), tot = oD + al(bD) + 256;
  // a plain device allocation (host copies into the stream-ordered pool were observed to
  // return stale data for large blocks), stream-ordered copies, the stream synchronised
  // before the host reads anything
  char* buf = nullptr;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMalloc((void**)&buf, tot));
  hipError_t e = hipSuccess;
  for (int64_t c = 0; c < n_cols && e == hipSuccess; ++c)
    e = hipMemcpyAsync(buf + sizeof(double) * (size_t)c * n, in + c * ld_in, sizeof(double) * n,
                       hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  int rc = RYD_OK;
  if (e == hipSuccess)
    rc = launch_derive(desc, (const double*)buf, n, n, (double*)(buf + oP), n, (uint32_t*)(buf + oW),
                       diag ? (double*)(buf + oD) : nullptr, n, s);
  if (e == hipSuccess && rc == RYD_OK) e = hipStreamSynchronize(s);
  for (int f = 0; f < RYD_NPARAM && e == hipSuccess && rc == RYD_OK; ++f)
    e = hipMemcpyAsync(params + f * ld_params, buf + oP + sizeof(double) * (size_t)f * n, sizeof(double) * n,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && rc == RYD_OK) e = hipMemcpyAsync(warn, buf + oW, bW, hipMemcpyDeviceToHost, s);
  for (int k = 0; diag && k < RYD_DV_NDIAG && e == hipSuccess && rc == RYD_OK; ++k)
    e = hipMemcpyAsync(diag + k * ld_diag, buf + oD + sizeof(double) * (size_t)k * n, sizeof(double) * n,
                       hipMemcpyDeviceToHost, s);
  const hipError_t es = hipStreamSynchronize(s);
  const hipError_t ef = hipFree(buf);
  if (rc) return rc;
  if (e != hipSuccess) return fail(RYD_ERR_HIP, std::string("derive: ") + hipGetErrorString(e));
  if (ef != hipSuccess || es != hipSuccess) return fail(RYD_ERR_HIP, "derive: free/sync failed");
  return RYD_OK;
}

}  // extern "C"
#endif  // RYD_S16_BAL_TU
