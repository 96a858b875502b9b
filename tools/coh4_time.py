"""Kernel time of the process-map coherence pass on the C2 (Omega, Delta) grid: the dim-3
coherence_prop_kernel (the yardstick), the dim-4 coherence4_prop_kernel on the same grid
derived with hilbert_space_dim=4, and coherence4_cheb_kernel (RYD_COH_PROP=0), in one
process.  Per input 3 warm-up launches, then the median of 20 timed ones (HIP events around
the launch, inputs resident in HBM).  Prints one JSON line.

    python tools/coh4_time.py [--n-omega 100 --n-delta 100]
"""
import argparse
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import sweeps as SW

WARMUP, TIMED = 3, 20


def median_ms(eng, params, dim):
    db = E.CoherenceDeviceBatch(eng, params, "lp_square", dim=dim)
    try:
        for _ in range(WARMUP):
            db.launch()
        db.synchronize()
        ts = [db.launch(timed=True) for _ in range(TIMED)]
        coh, st = db.fetch()
    finally:
        db.free()
    if np.any(st & N.STATUS_FAIL_MASK) or not np.all(np.isfinite(coh)):
        raise SystemExit(f"dim {dim}: the engine reported per-point failures")
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-omega", type=int, default=100)
    ap.add_argument("--n-delta", type=int, default=100)
    args = ap.parse_args()
    eng = E.Engine()
    p3 = E.pack_params(SW.omega_delta_grid(args.n_omega, args.n_delta, hilbert_space_dim=3))
    p4 = E.pack_params(SW.omega_delta_grid(args.n_omega, args.n_delta, hilbert_space_dim=4))
    old = os.environ.pop("RYD_COH_PROP", None)
    try:
        d3 = median_ms(eng, p3, 3)
        d4 = median_ms(eng, p4, 4)
        os.environ["RYD_COH_PROP"] = "0"
        d4c = median_ms(eng, p4, 4)
    finally:
        os.environ.pop("RYD_COH_PROP", None)
        if old is not None:
            os.environ["RYD_COH_PROP"] = old
    key = lambda t: dict(median_ms=round(t[0], 4), min_ms=round(t[1], 4), max_ms=round(t[2], 4))
    print(json.dumps({
        "tool": "coh4_time", "grid": "C2 omega_delta_grid", "points": int(p3.shape[1]), "protocol": "lp_square",
        "warmup": WARMUP, "timed": TIMED,
        "dim3_coherence_prop_kernel": key(d3), "dim4_coherence4_prop_kernel": key(d4),
        "dim4_coherence4_cheb_kernel": key(d4c),
        "dim4_over_dim3": round(d4[0] / d3[0], 3), "dim4_cheb_over_prop": round(d4c[0] / d4[0], 2)}))


if __name__ == "__main__":
    main()
