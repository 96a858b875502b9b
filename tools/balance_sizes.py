"""Kernel time of the sym16 LP-square kernel's two launch forms against the batch size: the
one-wave kernel (RYD_S16_BALANCE=0) and the CU-balanced form (RYD_S16_BALANCE=2), alternating
in one process on the C2 parameter ranges (HIP events around 50 launches, best and median of
5 rounds).  The automatic rule's choice for each n is printed beside them.
    python tools/balance_sizes.py [n ...]
"""
import os
import sys
import warnings

import numpy as np

from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import sweeps as SW

warnings.simplefilter("ignore")
ns = [int(a) for a in sys.argv[1:]] or [4096, 5000, 6000, 7000, 8192, 9000, 10000, 11000, 12288, 13000, 14000, 16384]
full = E.pack_params(SW.omega_delta_grid(200, 200))              # 40k points, C2 ranges
c2 = E.pack_params(SW.omega_delta_grid(100, 100))                # the bench batch itself at n = 10000
eng = E.Engine()
rng = np.random.default_rng(0)
REPS, ROUNDS = 50, 5


def timed(db, mode):
    os.environ["RYD_S16_BALANCE"] = mode
    db.launch()
    db.synchronize()
    db.mark(0)
    for _ in range(REPS):
        db.launch()
    db.mark(1)
    return db.mark_elapsed() / REPS * 1e3


for n in ns:
    prm = c2 if n == 10000 else full[:, np.sort(rng.choice(full.shape[1], n, replace=False))].copy()
    db = E.DeviceBatch(eng, prm, "lp_square", "lindblad")
    t = {"0": [], "2": []}
    for _ in range(ROUNDS):
        for mode in ("0", "2"):
            t[mode].append(timed(db, mode))
    db.free()
    pl = E.sym16_balance_plan(n, 256)
    a, b = np.array(t["0"]), np.array(t["2"])
    print(f"n={n:6d} gpc={pl['gpc']:2d} waves/wg={pl['waves']:2d} auto={int(pl['auto'])}  one-wave {np.median(a):7.2f} us "
          f"(min {a.min():7.2f})  balanced {np.median(b):7.2f} us (min {b.min():7.2f})  "
          f"balanced/one-wave {np.median(b) / np.median(a):.3f}", flush=True)
os.environ.pop("RYD_S16_BALANCE", None)
