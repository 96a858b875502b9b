// ryd_sched_table.inc -- how every custom-pulse-schedule kernel reads its table (included by
// ryd_engine.hip before ryd_sched16.inc; used by ryd_sched16.inc, ryd_ket_sched.inc and
// ryd_coh_sched.inc, the last of which drops the macros).  The protocol stands here only.
//
// Table.  Point-major, sched[i ld + f n_seg + s] (include/ryd_engine.h, "custom pulse
// schedules"); a shared table is the same address with ld = 0.  A point is one 16-lane DPP row
// of a wave.  A row past the batch reads point n - 1, and lanes past n_seg in the last chunk
// read segment n_seg - 1: with ld >= 4 n_seg (checked on the host) the largest index formed is
// (n - 1) ld + 4 n_seg - 1, the table's last element.  All of it is 64-bit arithmetic.
//
// Chunk.  The table is read 16 segments at a time: lane r of a row loads segment s0 + r of each
// of the four fields (one load instruction per field and chunk, 128 bytes per row), forms its
// segment's key (a Omega, delta Omega, x / Omega) -- the three products are formed the same way
// every time, so keys compare with == -- and the (cos, sin) of its phase, sixteen segments' worth
// per fast_sincos: the five per-lane values Ka, Kd, Kt, Pc, Ps.  A forward loop takes segment
// s0 + j from lane 0 of the row (row_bcast<0>) after j one-lane rotations, never from memory; a
// backward walk takes it from lane 15, a partial last chunk rotated up first.  The chunk of an
// invalid row is neutral: zero durations, phase 0, so that no NaN of the table reaches a state.
//
// Validity.  One pass before the first build: every entry finite, x >= 0, a >= 0, and the
// point's scalars as bang-bang checks them, without its segment count and without the ignored
// column RYD_P_DELTA (sched16_point_valid).
//
// What differs per kernel stays with the kernel: where Omega comes from, the step cap, and
// which LDS array parks the chunk across a build.
//
// The pass and the chunk are statement macros, not functions: a kernel that uses them compiles
// to the instructions it had with the statements written out, which an inlined function (the
// compiler optimises it on its own first) and a struct of the five values (promoted to
// registers in another order) do not give; make kernel-diff checks it.  They expand where the
// kernel declares `double Ka, Kd, Kt, Pc, Ps;`.

// lane r takes the value of lane (r + 1) mod 16 / (r - 1) mod 16 of its row: row_ror:15, row_ror:1
// (two 32-bit DPP moves each)
__device__ __forceinline__ double row_rol1(double v) { return dpp32x2<0x12F>(v); }
__device__ __forceinline__ double row_ror1(double v) { return dpp32x2<0x121>(v); }

// the scalars a schedule point reads (load_point's columns OMEGA, V, DELTA1 and the rates)
__device__ __forceinline__ bool sched16_point_valid(const PointP& q) {
  bool ok = q.Om > 0.0 && isfinite(q.Om) && isfinite(q.V) && isfinite(q.d1);
#pragma unroll
  for (int c = 0; c < 4; ++c) ok = ok && q.gA[c] >= 0.0 && q.gB[c] >= 0.0 && isfinite(q.gA[c]) && isfinite(q.gB[c]);
  return ok;
}

// field f of segment min(s0 + r, n_seg - 1) of the lane's row (row: the point's table row)
__device__ __forceinline__ double sched16_load(const double* __restrict__ row, int f, int n_seg, int s0, int r) {
  const int64_t s = (int64_t)s0 + r < (int64_t)n_seg ? (int64_t)s0 + r : (int64_t)n_seg - 1;
  return row[(int64_t)f * (int64_t)n_seg + s];
}

// valid &&= the table of row p of the wave (every lane of the wave takes part): lane r checks
// segments r, r + 16, ...; one ballot, the row's 16-bit slice
#define SCHED_TABLE_VALID(valid, row, n_seg, r, p)                                                        \
  {                                                                                                       \
    bool ok = true;                                                                                       \
    for (int s0 = 0; s0 < n_seg; s0 += 16) {                                                              \
      const double x = sched16_load(row, RYD_SC_X, n_seg, s0, r);                                         \
      const double a = sched16_load(row, RYD_SC_AMP, n_seg, s0, r);                                       \
      const double ph = sched16_load(row, RYD_SC_PHASE, n_seg, s0, r);                                    \
      const double d = sched16_load(row, RYD_SC_DELTA, n_seg, s0, r);                                     \
      ok = ok && x >= 0.0 && a >= 0.0 && isfinite(x) && isfinite(a) && isfinite(ph) && isfinite(d);       \
    }                                                                                                     \
    const uint64_t bad = __builtin_amdgcn_ballot_w64(!ok);                                                \
    valid = valid && ((bad >> (16 * p)) & 0xFFFFull) == 0;                                                \
  }

// the chunk at s0: lane r's segment s0 + r (clamped) of the row, on the point's Omega (a name)
#define SCHED_CHUNK_LOAD(row, n_seg, s0, r, Om)                      \
  const double x = sched16_load(row, RYD_SC_X, n_seg, s0, r);        \
  const double a = sched16_load(row, RYD_SC_AMP, n_seg, s0, r);      \
  const double ph = sched16_load(row, RYD_SC_PHASE, n_seg, s0, r);   \
  const double d = sched16_load(row, RYD_SC_DELTA, n_seg, s0, r);    \
  Ka = a * Om;                                                       \
  Kd = d * Om;                                                       \
  Kt = x / Om;                                                       \
  fast_sincos(ph, Ps, Pc);

// an invalid row takes part in nothing
#define SCHED_CHUNK_NEUTRAL() \
  Ka = Kd = Kt = 0.0;         \
  Pc = 1.0;                   \
  Ps = 0.0;

// one lane down (the next segment to lane 0) / one lane up (the segment before to lane 15)
#define SCHED_CHUNK_ROL1() \
  Ka = row_rol1(Ka);       \
  Kd = row_rol1(Kd);       \
  Kt = row_rol1(Kt);       \
  Pc = row_rol1(Pc);       \
  Ps = row_rol1(Ps);
#define SCHED_CHUNK_ROR1() \
  Ka = row_ror1(Ka);       \
  Kd = row_ror1(Kd);       \
  Kt = row_ror1(Kt);       \
  Pc = row_ror1(Pc);       \
  Ps = row_ror1(Ps);

// a partial chunk of cnt segments: its last segment up to lane 15
#define SCHED_CHUNK_TO_LANE15(cnt)   \
  for (int k = cnt; k < 16; ++k) {   \
    SCHED_CHUNK_ROR1()               \
  }
