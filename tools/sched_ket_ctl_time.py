"""The control Jacobian of noise-free pulse schedules (ryd_run_schedule_kets_ctl_device:
ket_sched_ctl_kernel) against the phase-only Jacobian (ket_sched_jac_kernel) and the forward
kernel, in one process, on the cases of tools/sched_ket_time.py and by its method:

  a  jp300   the 300-segment phase-only shared table on the C2 grid's points, rates zero (one
             build per point and direction)
  b  amp300  300 segments with a different amplitude each (a build per segment and direction)
  d  small   a at n = 256 and n = 4096

Per case the control launch is alternated launch by launch with the phase-only launch, and
separately with the forward launch: 3 warm-up launches of each, then median, min and max of 20
timed ones (HIP events around the launch, inputs resident in HBM); three rounds.  Checks that
state, summary, status and the phase block of the control run are the phase-only run's bits.
Prints one JSON line and writes it to --out.

    python tools/sched_ket_ctl_time.py
"""
import argparse
import json
import os
import sys
import warnings

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import protocols as PR
from noisyquantumsimulator_amd import pulse_schedules as PS
from noisyquantumsimulator_amd import sweeps as SW
from tools.sched_ket_time import NSEG, ROUNDS, SMALL, TIMED, WARMUP, alternate, check


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-omega", type=int, default=100)
    ap.add_argument("--n-delta", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "sched_ket_ctl", "sched_ket_ctl_time.json"))
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    eng = E.Engine()
    p = E.pack_params(SW.omega_delta_grid(args.n_omega, args.n_delta))
    n = p.shape[1]
    d = PR.SMOOTH_JP_DEFAULTS
    Om = p[N.P["OMEGA"]]
    dom = -abs(d["delta_over_omega"])
    p[N.P["G1_A"]:N.P["GSC_B"] + 1] = 0.0
    p[N.P["GMJ_A"]:] = 0.0
    p[N.P["DELTA"]], p[N.P["TAU"]] = dom * Om, d["omega_tau"] / Om
    p[N.P["A"]], p[N.P["OMEGA_MOD"]], p[N.P["PHI_OFF"]] = d["A"], d["omega_mod_ratio"] * Om, d["phi_offset"]
    tab = PS.from_smooth_jp(d["A"], d["omega_mod_ratio"], d["phi_offset"], d["omega_tau"], dom, NSEG)
    amp = tab.copy()
    amp[N.SC["AMP"]] = 0.4 + 0.6 * np.sin(np.pi * (np.arange(NSEG) + 0.5) / NSEG) ** 2 + 1e-6 * np.arange(NSEG)
    cases = {"a_jp300": (p, tab), "b_amp300": (p, amp)}
    for m in SMALL:
        cases[f"d_jp300_n{m}"] = (np.ascontiguousarray(p[:, np.linspace(0, n - 1, m).astype(int)]), tab)
    B = {}
    for k, (pp, tt) in cases.items():
        B[k] = {"ctl": E.ScheduleKetDeviceBatch(eng, pp, tt, jacobian="controls"),
                "jac": E.ScheduleKetDeviceBatch(eng, pp, tt, jacobian=True),
                "fwd": E.ScheduleKetDeviceBatch(eng, pp, tt)}
    rounds, same = [], {}
    try:
        for _ in range(ROUNDS):
            rec = {}
            for k, b in B.items():
                c1, j = alternate(b["ctl"], b["jac"])
                c2, f = alternate(b["ctl"], b["fwd"])
                rec[k] = {"controls": c1, "phase_only": j, "controls_beside_forward": c2, "forward": f,
                          "controls_over_phase_only": round(c1["median_ms"] / j["median_ms"], 3),
                          "controls_over_forward": round(c2["median_ms"] / f["median_ms"], 3)}
            rounds.append(rec)
        for k, b in B.items():
            rc, rj = check(b["ctl"].fetch(), k), check(b["jac"].fetch(), k)
            same[k] = bool(np.array_equal(rc.state, rj.state) and
                           np.array_equal(rc.summary.view(np.uint64), rj.summary.view(np.uint64)) and
                           np.array_equal(rc.status, rj.status) and
                           np.array_equal(rc.phase_jacobian.view(np.float64).view(np.uint64),
                                          rj.phase_jacobian.view(np.float64).view(np.uint64)))
    finally:
        for b in B.values():
            for x in b.values():
                x.free()
    if not all(same.values()):
        raise SystemExit(f"the control run's bits differ from the phase-only run's: {same}")
    line = json.dumps({"tool": "sched_ket_ctl_time", "grid": "C2 omega_delta_grid, rates zero", "points": int(n),
                       "n_seg": NSEG, "warmup": WARMUP, "timed": TIMED, "rounds": rounds,
                       "phase_only_run_same_bits": same,
                       "jacobian_bytes_per_point": int(8 * 4 * N.SC_NFIELD * NSEG)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
