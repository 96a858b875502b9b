"""Process-map coherences of a custom pulse schedule (ryd_run_schedule_coherences_device,
coherence_sched_kernel) on the C2 grid's 10,000 points with the smooth-JP defaults, in one
process, by the method of tools/sched_time.py:

  a  jp300           coherence_prop_kernel<SMOOTH_JP> (CoherenceDeviceBatch "smooth_jp", 300
                     steps) against the same pulse as one shared 300-segment phase-only table
                     (pulse_schedules.from_smooth_jp) in the schedule kernel, the two alternating
                     launch by launch
  b  shared/per_point  the same table shared and as a copy per point
  c  amp300          300 segments with a different amplitude each: a build per segment in both
                     sector groups
  d  process map     ryd_run_schedule_device + ryd_run_schedule_coherences_device for (a): the
                     two launches back to back, the sum of their device times

Per setting 3 warm-up launches, then median, min and max of 20 timed ones (HIP events around
the launch, inputs resident in HBM); three rounds; the range of the rounds' medians is reported.
Also checks that the schedule coherences agree with coherence_prop_kernel to 1e-10 and that the
shared and per-point tables give the same bits.  Writes one JSON document.

    python tools/sched_coh_time.py [--out profiles/sched_coh/sched_coh_time.json]
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
GENERIC_SEAM_S = 101.0                       # 10,000 points x 300 segments, recorded


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 5), "min_ms": round(float(min(ts)), 5),
            "max_ms": round(float(max(ts)), 5)}


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


def clean(got, what):
    coh, st = got
    if np.any(st & N.STATUS_FAIL_MASK):
        raise SystemExit(f"{what}: the engine reported per-point failures")
    return coh


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-omega", type=int, default=100)
    ap.add_argument("--n-delta", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "sched_coh", "sched_coh_time.json"))
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
    jp = E.CoherenceDeviceBatch(eng, p, "smooth_jp", n_steps=NSEG)
    shared = E.ScheduleCoherenceDeviceBatch(eng, p, tab)
    per = E.ScheduleCoherenceDeviceBatch(eng, p, np.repeat(tab[None], n, axis=0))
    var = E.ScheduleCoherenceDeviceBatch(eng, p, amp)
    states = E.ScheduleDeviceBatch(eng, p, tab)
    rounds = []
    try:
        for _ in range(ROUNDS):
            rec = {}
            t_jp, t_sh = alternate(jp, shared)
            rec["a_coherence_prop_smooth_jp"], rec["a_schedule_shared"] = stats(t_jp), stats(t_sh)
            rec["a_ratio"] = round(float(np.median(t_sh) / np.median(t_jp)), 4)
            t_sh2, t_pp = alternate(shared, per)
            rec["b_schedule_shared"], rec["b_schedule_per_point"] = stats(t_sh2), stats(t_pp)
            for _ in range(WARMUP):
                var.launch()
            var.synchronize()
            rec["c_schedule_amp300"] = stats([var.launch(timed=True) for _ in range(TIMED)])
            t_st, t_co = alternate(states, shared)
            rec["d_states"], rec["d_coherences"] = stats(t_st), stats(t_co)
            rec["d_process_map"] = stats([a + b for a, b in zip(t_st, t_co)])
            rounds.append(rec)
        c_jp, c_sh, c_pp = clean(jp.fetch(), "smooth JP"), clean(shared.fetch(), "shared"), clean(per.fetch(), "per point")
        clean(var.fetch(), "amp300")
    finally:
        for b in (jp, shared, per, var, states):
            b.free()
    agree = float(np.abs(c_sh - c_jp).max())
    if agree > 1e-10:
        raise SystemExit(f"schedule coherences and coherence_prop_kernel disagree: {agree:g}")
    keys = ("a_coherence_prop_smooth_jp", "a_schedule_shared", "b_schedule_shared", "b_schedule_per_point",
            "c_schedule_amp300", "d_process_map")
    med = {k: [r[k]["median_ms"] for r in rounds] for k in keys}
    doc = {"tool": "sched_coh_time", "grid": "C2 omega_delta_grid", "points": int(n), "n_seg": NSEG,
           "warmup": WARMUP, "timed": TIMED, "rounds": rounds,
           "median_of_medians_ms": {k: round(float(np.median(v)), 5) for k, v in med.items()},
           "range_of_medians_ms": {k: [min(v), max(v)] for k, v in med.items()},
           "a_ratio_range": [min(r["a_ratio"] for r in rounds), max(r["a_ratio"] for r in rounds)],
           "schedule_vs_coherence_prop_max_abs": agree,
           "shared_equals_per_point_bits": bool(np.array_equal(c_sh, c_pp)),
           "generic_seam_recorded_s_per_10000_points": GENERIC_SEAM_S,
           "table_bytes_per_point": int(8 * N.SC_NFIELD * NSEG)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
