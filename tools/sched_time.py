"""Custom pulse schedules (ryd_run_schedule_device, lindblad_sched16_kernel) on the C2 grid's
10,000 points, in one process:

  a  jp300           a 300-segment phase-only schedule (pulse_schedules.from_smooth_jp, the
                     smooth-JP defaults, one shared table) against the smooth-JP kernel
                     (Engine.run's "smooth_jp" on the sym16 path) on the same points, the two
                     alternating launch by launch
  b  shared/per_point  the same schedule as one shared table and as a copy per point
  c  amp300          300 segments with a different amplitude each: a build per segment
  a1 one segment     both kernels on ONE segment of the same length (tau / 300): the build and
                     the launch without the segment loop, so that (a - a1) / 299 is each kernel's
                     cost per further segment
  d  generic         100 of the points (400 states) through the generic seam
                     (Engine.evolve_generic, what evolve_state_batch calls) with the same 300
                     segments as dense Hamiltonians and 8 jump operators: wall time of the
                     blocking call, and that time scaled to 10,000 points

Per setting 3 warm-up launches, then median, min and max of 20 timed ones (HIP events around
the launch, inputs resident in HBM; d: 3 calls, host wall clock); three rounds.  Also checks
that the schedule run agrees with the smooth-JP kernel to 1e-10.  Prints one JSON line.

    python tools/sched_time.py
"""
import argparse
import json
import os
import sys
import time
import warnings

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import operators as OPS
from noisyquantumsimulator_amd import protocols as PR
from noisyquantumsimulator_amd import pulse_schedules as PS
from noisyquantumsimulator_amd import sweeps as SW

WARMUP, TIMED, ROUNDS = 3, 20, 3
NSEG = 300


def stats(ts, unit="ms"):
    return {f"median_{unit}": round(float(np.median(ts)), 5), f"min_{unit}": round(float(min(ts)), 5),
            f"max_{unit}": round(float(max(ts)), 5)}


def check(r, what):
    if np.any(r.status & N.STATUS_FAIL_MASK):
        raise SystemExit(f"{what}: the engine reported per-point failures")
    return r


def alternate(a, b):
    """WARMUP launches of each, then TIMED timed launches alternating a, b, a, b, ..."""
    for _ in range(WARMUP):
        a.launch()
        b.launch()
    a.synchronize()
    ta, tb = [], []
    for _ in range(TIMED):
        ta.append(a.launch(timed=True))
        tb.append(b.launch(timed=True))
    return ta, tb


def generic_case(eng, p, tab, m):
    """The first m points' 4 basis inputs as 4 m generic problems; returns wall seconds per call."""
    P = N.P
    H = np.zeros((4 * m, NSEG, 9, 9), complex)
    dt = np.zeros((4 * m, NSEG))
    ops = np.zeros((4 * m, 8, 9, 9), complex)
    rho0 = np.zeros((4 * m, 9, 9), complex)
    I3 = np.eye(3)
    unit = lambda i, j: np.outer(I3[i], I3[j]).astype(complex)
    chan = (("G1", unit(1, 2)), ("G0", unit(0, 2)), ("GPHI", unit(2, 2)), ("GSC", unit(1, 1)))
    for i in range(m):
        Om, V, d1 = p[P["OMEGA"], i], p[P["V"], i], p[P["DELTA1"], i]
        Hs = np.stack([OPS.hamiltonian(a * Om * np.exp(1j * ph), d * Om, V, 3, d1) for x, a, ph, d in tab.T])
        L = [np.sqrt(p[P[k + "_A"], i]) * np.kron(o, I3) for k, o in chan] + \
            [np.sqrt(p[P[k + "_B"], i]) * np.kron(I3, o) for k, o in chan]
        for k, idx in enumerate((0, 1, 3, 4)):
            H[4 * i + k], dt[4 * i + k], ops[4 * i + k] = Hs, tab[N.SC["X"]] / Om, L
            rho0[4 * i + k, idx, idx] = 1.0
    eng.evolve_generic(H, dt, rho0, ops)                        # warm-up
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        _, status = eng.evolve_generic(H, dt, rho0, ops)
        ts.append(time.perf_counter() - t0)
        if np.any(status & N.STATUS_FAIL_MASK):
            raise SystemExit("generic seam: per-problem failures")
    return ts


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-omega", type=int, default=100)
    ap.add_argument("--n-delta", type=int, default=100)
    ap.add_argument("--generic-points", type=int, default=100)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    eng = E.Engine()
    p = E.pack_params(SW.omega_delta_grid(args.n_omega, args.n_delta))
    n = p.shape[1]
    d = PR.SMOOTH_JP_DEFAULTS
    Om = p[N.P["OMEGA"]]
    dom = -abs(d["delta_over_omega"])
    p[N.P["DELTA"]], p[N.P["TAU"]] = dom * Om, d["omega_tau"] / Om
    p[N.P["A"]], p[N.P["OMEGA_MOD"]], p[N.P["PHI_OFF"]] = d["A"], d["omega_mod_ratio"] * Om, d["phi_offset"]
    tab = PS.from_smooth_jp(d["A"], d["omega_mod_ratio"], d["phi_offset"], d["omega_tau"], dom, NSEG)
    amp = tab.copy()
    amp[N.SC["AMP"]] = 0.4 + 0.6 * np.sin(np.pi * (np.arange(NSEG) + 0.5) / NSEG) ** 2 + 1e-6 * np.arange(NSEG)
    assert len(set(amp[N.SC["AMP"]])) == NSEG
    jp = E.DeviceBatch(eng, p, "smooth_jp", "lindblad", n_steps=NSEG)
    shared = E.ScheduleDeviceBatch(eng, p, tab)
    per = E.ScheduleDeviceBatch(eng, p, np.repeat(tab[None], n, axis=0))
    var = E.ScheduleDeviceBatch(eng, p, amp)
    p1 = p.copy()                                    # one segment of the 300: the same dt, the same build
    p1[N.P["TAU"]] = p[N.P["TAU"]] / NSEG
    jp1 = E.DeviceBatch(eng, p1, "smooth_jp", "lindblad", n_steps=1)
    one = E.ScheduleDeviceBatch(eng, p, tab[:, :1].copy())
    rounds = []
    try:
        for _ in range(ROUNDS):
            rec = {}
            t_jp, t_sh = alternate(jp, shared)
            rec["a_smooth_jp_kernel"], rec["a_schedule_shared"] = stats(t_jp), stats(t_sh)
            t_jp1, t_one = alternate(jp1, one)
            rec["a1_smooth_jp_kernel_1seg"], rec["a1_schedule_1seg"] = stats(t_jp1), stats(t_one)
            rec["per_segment_us"] = {
                "smooth_jp_kernel": round((np.median(t_jp) - np.median(t_jp1)) / (NSEG - 1) * 1e3, 4),
                "schedule": round((np.median(t_sh) - np.median(t_one)) / (NSEG - 1) * 1e3, 4)}
            t_sh2, t_pp = alternate(shared, per)
            rec["b_schedule_shared"], rec["b_schedule_per_point"] = stats(t_sh2), stats(t_pp)
            for _ in range(WARMUP):
                var.launch()
            var.synchronize()
            rec["c_schedule_amp300"] = stats([var.launch(timed=True) for _ in range(TIMED)])
            tg = generic_case(eng, p, tab, args.generic_points)
            rec["d_generic_seam"] = dict(points=args.generic_points, wall=stats(tg, "s"),
                                         scaled_to_n_s=round(float(np.median(tg)) * n / args.generic_points, 3))
            rounds.append(rec)
        r_jp, r_sh, r_pp, r_var = (check(b.fetch(), w) for b, w in ((jp, "smooth JP"), (shared, "shared"),
                                                                       (per, "per point"), (var, "amp300")))
    finally:
        for b in (jp, shared, per, var, jp1, one):
            b.free()
    agree = float(np.abs(r_sh.rho() - r_jp.rho()).max())
    if agree > 1e-10:
        raise SystemExit(f"schedule and smooth-JP kernel disagree: {agree:g}")
    same = bool(np.array_equal(r_sh.state, r_pp.state))
    print(json.dumps({"tool": "sched_time", "grid": "C2 omega_delta_grid", "points": int(n), "n_seg": NSEG,
                      "warmup": WARMUP, "timed": TIMED, "rounds": rounds,
                      "schedule_vs_smooth_jp_max_abs_drho": agree, "shared_equals_per_point_bits": same,
                      "nsquare_mean": {"jp300": float(r_sh.col("NSQUARE").mean()),
                                           "amp300": float(r_var.col("NSQUARE").mean())},
                      "table_bytes_per_point": int(8 * N.SC_NFIELD * NSEG)}))


if __name__ == "__main__":
    main()
