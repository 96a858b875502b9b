"""Noise-free custom pulse schedules as kets (ryd_run_schedule_kets_device: ket_sched_kernel,
ket_sched_jac_kernel) on the C2 grid's points with every rate zero, in one process, by the
method of tools/sched_time.py:

  a  jp300     the 300-segment phase-only shared table of pulse_schedules.from_smooth_jp (one
               build per point): the forward ket kernel alternated launch by launch with
               lindblad_sched16_kernel on the same points and table -- the only route a
               noise-free schedule had -- and, separately, with ket_block_kernel
               (Engine.run's "smooth_jp", "ket", n_steps = 300: one lane per point)
  b  amp300    300 segments with a different amplitude each (a build per segment), the forward
               ket kernel alternated with lindblad_sched16_kernel
  c  jacobian  a and b with the Jacobian (ket_sched_jac_kernel) alternated with the forward kernel
  d  small     a at n = 256 and n = 4096, forward alone and with the Jacobian, alternated

Per pair 3 warm-up launches of each, then median, min and max of 20 timed ones (HIP events
around the launch, inputs resident in HBM); three rounds.  Also checks that the ket run agrees
with the Lindblad schedule run (rho = |psi><psi|) and with ket_block_kernel to 1e-10.  Prints
one JSON line.

    python tools/sched_ket_time.py
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

WARMUP, TIMED, ROUNDS = 3, 20, 3
NSEG = 300
SMALL = (256, 4096)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 5), "min_ms": round(float(min(ts)), 5),
            "max_ms": round(float(max(ts)), 5)}


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
    return stats(ta), stats(tb)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-omega", type=int, default=100)
    ap.add_argument("--n-delta", type=int, default=100)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    eng = E.Engine()
    p = E.pack_params(SW.omega_delta_grid(args.n_omega, args.n_delta))
    n = p.shape[1]
    d = PR.SMOOTH_JP_DEFAULTS
    Om = p[N.P["OMEGA"]]
    dom = -abs(d["delta_over_omega"])
    p[N.P["G1_A"]:N.P["GSC_B"] + 1] = 0.0            # noise-free: the Lindblad route at zero rates
    p[N.P["GMJ_A"]:] = 0.0
    p[N.P["DELTA"]], p[N.P["TAU"]] = dom * Om, d["omega_tau"] / Om
    p[N.P["A"]], p[N.P["OMEGA_MOD"]], p[N.P["PHI_OFF"]] = d["A"], d["omega_mod_ratio"] * Om, d["phi_offset"]
    tab = PS.from_smooth_jp(d["A"], d["omega_mod_ratio"], d["phi_offset"], d["omega_tau"], dom, NSEG)
    amp = tab.copy()
    amp[N.SC["AMP"]] = 0.4 + 0.6 * np.sin(np.pi * (np.arange(NSEG) + 0.5) / NSEG) ** 2 + 1e-6 * np.arange(NSEG)
    assert len(set(amp[N.SC["AMP"]])) == NSEG
    B = {
        "ket_jp": E.ScheduleKetDeviceBatch(eng, p, tab),
        "ket_jp_jac": E.ScheduleKetDeviceBatch(eng, p, tab, jacobian=True),
        "lind_jp": E.ScheduleDeviceBatch(eng, p, tab),
        "block_jp": E.DeviceBatch(eng, p, "smooth_jp", "ket", n_steps=NSEG),
        "ket_amp": E.ScheduleKetDeviceBatch(eng, p, amp),
        "ket_amp_jac": E.ScheduleKetDeviceBatch(eng, p, amp, jacobian=True),
        "lind_amp": E.ScheduleDeviceBatch(eng, p, amp),
    }
    for m in SMALL:
        sub = np.ascontiguousarray(p[:, np.linspace(0, n - 1, m).astype(int)])
        B[f"ket_jp_{m}"] = E.ScheduleKetDeviceBatch(eng, sub, tab)
        B[f"ket_jp_jac_{m}"] = E.ScheduleKetDeviceBatch(eng, sub, tab, jacobian=True)
    rounds = []
    try:
        for _ in range(ROUNDS):
            rec = {}
            rec["a_ket_forward"], rec["a_lindblad_zero_rates"] = alternate(B["ket_jp"], B["lind_jp"])
            rec["a2_ket_forward"], rec["a2_ket_block_kernel"] = alternate(B["ket_jp"], B["block_jp"])
            rec["b_ket_forward_amp300"], rec["b_lindblad_zero_rates_amp300"] = alternate(B["ket_amp"], B["lind_amp"])
            rec["c_ket_jacobian"], rec["c_ket_forward"] = alternate(B["ket_jp_jac"], B["ket_jp"])
            rec["c_ket_jacobian_amp300"], rec["c_ket_forward_amp300"] = alternate(B["ket_amp_jac"], B["ket_amp"])
            for m in SMALL:
                rec[f"d_ket_forward_n{m}"], rec[f"d_ket_jacobian_n{m}"] = alternate(B[f"ket_jp_{m}"],
                                                                                    B[f"ket_jp_jac_{m}"])
            rec["a_forward_median_below_lindblad_min"] = \
                rec["a_ket_forward"]["median_ms"] < rec["a_lindblad_zero_rates"]["min_ms"]
            rec["b_forward_median_below_lindblad_min"] = \
                rec["b_ket_forward_amp300"]["median_ms"] < rec["b_lindblad_zero_rates_amp300"]["min_ms"]
            rounds.append(rec)
        R = {k: check(b.fetch(), k) for k, b in B.items()}
    finally:
        for b in B.values():
            b.free()
    agree = {}
    for k, l in (("ket_jp", "lind_jp"), ("ket_amp", "lind_amp")):
        psi = R[k].kets()
        agree[f"{l}_rho_vs_{k}"] = float(np.abs(R[l].rho() - np.einsum("nki,nkj->nkij", psi, psi.conj())).max())
    agree["block_jp_vs_ket_jp"] = float(np.abs(R["block_jp"].kets() - R["ket_jp"].kets()).max())
    if max(agree.values()) > 1e-10:
        raise SystemExit(f"the routes disagree: {agree}")
    same = all(np.array_equal(R[k].state, R[k + "_jac"].state) and
               np.array_equal(R[k].summary.view(np.uint64), R[k + "_jac"].summary.view(np.uint64))
               for k in ("ket_jp", "ket_amp"))
    print(json.dumps({"tool": "sched_ket_time", "grid": "C2 omega_delta_grid, rates zero", "points": int(n),
                      "n_seg": NSEG, "warmup": WARMUP, "timed": TIMED, "rounds": rounds, "max_abs_disagreement": agree,
                      "jacobian_run_same_bits": bool(same),
                      "nsquare_mean": {"jp300": float(R["ket_jp"].col("NSQUARE").mean()),
                                       "amp300": float(R["ket_amp"].col("NSQUARE").mean())},
                      "gauge_sum_max": float(np.abs(R["ket_jp_jac"].phase_jacobian.sum(axis=2)).max()),
                      "jacobian_bytes_per_point": int(8 * N.SC_NFIELD * NSEG)}))


if __name__ == "__main__":
    main()
