"""Per-wave phase timeline of lindblad_sym16_kernel from the RYD_S16_PROF build variant
(build/libryd_prof.so: shader-clock timestamps written to the summary's unused Lindblad
columns).  Usage on the GPU box:
    RYD_ENGINE_LIB=$PWD/build/libryd_prof.so python tools/phase_prof.py [c2|c3] [n ...]
When the launch took the LP-square kernel's CU-balanced form (RYD_S16_BALANCE, ryd_sym16.inc)
the PROF build also records each wave's role and polls and the producer's stamps: the tool
then adds the cycles per role, the distribution of wave end times, the consumers that polled
more than once or fell back, and per workgroup the SIMD every role ran on.
For both forms the 'load' phase is split at the PROF build's start-up stamps (the workgroup
roles known and the consumer's flag cleared, the parameter column loads issued, their values in hand), and the waves' span
from the first start to the last end is set against the kernel's time: what is left is
dispatch before the first wave and drain after the last.
"""
import os
import sys
import warnings
from collections import defaultdict

import numpy as np

from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import sweeps as SW

warnings.simplefilter("ignore")
w = sys.argv[1] if len(sys.argv) > 1 else "c2"
ns = [int(a) for a in sys.argv[2:]] or [4096, 10000]
if w == "c2":
    full = E.pack_params(SW.omega_delta_grid(200, 200))
    proto, nst = "lp_square", None
else:
    full = SW.c3_four_op_params(SW.pareto_tgate_grid(400, 100))
    proto, nst = "smooth_jp", 300
eng = E.Engine()
names = ["load", "cheb", "square", "transpose", "segments", "epilogue"]
for n in ns:
    idx = np.linspace(0, full.shape[1] - 1, n).round().astype(int) if n != 10000 or w != "c2" else None
    prm = E.pack_params(SW.omega_delta_grid(100, 100)) if idx is None else full[:, idx].copy()
    db = E.DeviceBatch(eng, prm, proto, "lindblad", n_steps=nst)
    for _ in range(3):
        db.launch()
    db.synchronize()
    ms = db.launch(timed=True)
    r = db.fetch()
    S = r.summary
    cyc = S[4:10, ::4]                       # per wave (first point of each wave)
    t0 = S[10, ::4]
    t1 = S[11, ::4]
    hw = S[13, ::4].astype(np.int64)
    xcc = np.zeros_like(hw)                  # (the XCC column carries the staging timestamp)
    stage = S[14, ::4] - S[8, ::4]
    d = np.diff(np.vstack([np.zeros(cyc.shape[1]), cyc]), axis=0)
    print(f"== {w} n={n} waves={n // 4} kernel {ms * 1e3:.1f} us (HIP events)")
    for k, nm in enumerate(names):
        print(f"  {nm:10s} mean {d[k].mean():9.0f} cyc  p10 {np.percentile(d[k], 10):9.0f}  "
              f"p90 {np.percentile(d[k], 90):9.0f}  max {d[k].max():9.0f}")
    # the start-up in four parts (the PROF build's extra stamps, cycles from entry, in the
    # counter columns 17-19): the barrier (balanced form only) and the issue of the column
    # loads come in either order, values in hand = the first s_waitcnt vmcnt(0) returned
    bar, iss, hand = S[17, ::4], S[18, ::4], S[19, ::4]
    def dist(nm, x):
        print(f"    {nm:38s} mean {x.mean():7.0f} cyc  p10 {np.percentile(x, 10):7.0f}  p90 "
              f"{np.percentile(x, 90):7.0f}  max {x.max():7.0f}")
    print("  'load' in parts:")
    if np.all(bar > 0) and np.all(bar <= iss):                   # barrier first
        dist("entry -> roles known (no barrier)", bar)
        dist("roles known -> column loads issued", iss - bar)
        dist("column loads issued -> values in hand", hand - iss)
    elif np.all(bar > 0):                                        # loads first
        dist("entry -> column loads issued", iss)
        dist("column loads issued -> barrier passed", bar - iss)
        dist("barrier passed -> values in hand", hand - bar)
    else:                                                        # one-wave kernel: no barrier
        dist("entry -> column loads issued", iss)
        dist("column loads issued -> values in hand", hand - iss)
    dist("values in hand -> point_valid done", cyc[0] - hand)
    print(f"  (epilogue: rotate + LDS staging + state stores {stage.mean():.0f} cyc, summary "
          f"{(cyc[5] - S[14, ::4]).mean():.0f} cyc)")
    tot = cyc[-1]
    print(f"  total      mean {tot.mean():9.0f} cyc  max {tot.max():9.0f}")
    rt0 = (t0 - t0.min()) * 0.01             # 100 MHz -> us
    rt1 = (t1 - t0.min()) * 0.01
    print(f"  wall: start p50 {np.median(rt0):.2f} us max {rt0.max():.2f}; end p50 {np.median(rt1):.2f} "
          f"max {rt1.max():.2f}; wave duration p50 {np.median(rt1 - rt0):.2f} us max {(rt1 - rt0).max():.2f}")
    span = rt1.max()
    print(f"  wave span (first start to last end) {span:.2f} us of the kernel's {ms * 1e3:.2f} us: "
          f"{ms * 1e3 - span:.2f} us outside the waves")
    print(f"  clock: {np.median(tot / np.maximum(rt1 - rt0, 1e-3)) / 1e3:.2f} GHz (cycles / wall)")
    simd = defaultdict(list)
    for k in range(len(hw)):
        key = (int(xcc[k]), (int(hw[k]) >> 13) & 7, (int(hw[k]) >> 12) & 1, (int(hw[k]) >> 8) & 15,
               (int(hw[k]) >> 4) & 3)
        simd[key].append((rt0[k], rt1[k]))
    cnt = np.array([len(v) for v in simd.values()])
    print(f"  SIMDs used {len(simd)}  waves/SIMD min {cnt.min()} max {cnt.max()} "
          f"hist {np.bincount(cnt).tolist()}")
    conc = []
    for v in simd.values():
        ev = sorted([(a, 1) for a, b in v] + [(b, -1) for a, b in v])
        c = m = 0
        for _, e in ev:
            c += e
            m = max(m, c)
        conc.append(m)
    print(f"  max concurrent waves per SIMD hist {np.bincount(conc).tolist()}")
    late = rt0 > 2.0
    if late.any():
        print(f"  waves starting > 2 us after the first: {late.sum()}  (start p50 {np.median(rt0[late]):.2f} us)")
    db.free()
    code = S[12, ::4]
    if proto != "lp_square" or not (np.all(code == np.round(code)) and np.any(np.abs(code) >= 1)):
        continue                             # the one-wave kernel ran: column 12 is AVG_POP
    # ---- the balanced form: role, workgroup wave index, polls; the producer's stamps
    pl = E.sym16_balance_plan(n, 256, int(os.environ.get("RYD_S16_BALANCE_GPC", "0")))
    gpc = pl["gpc"]
    low = np.mod(code, 64).astype(int)
    polls = ((code - low) / 64).astype(int)
    role, wv = (low - 1) % 4, (low - 1) // 4
    wg = np.zeros(len(code), dtype=int)      # job -> its workgroup (the consumer's entry for a split job)
    for b, w in zip(*np.nonzero(pl["present"] & (pl["role"] != 1))):
        wg[pl["job"][b, w]] = b
    pst = S[15, ::4]
    pcyc, psimd = np.mod(pst, 1048576.0), (pst // 1048576.0).astype(int)
    simd_of = (hw >> 4) & 3
    cu_of = [((int(h) >> 13) & 7, (int(h) >> 12) & 1, (int(h) >> 8) & 15) for h in hw]
    print(f"== balanced form: gpc {gpc}, {pl['workgroups']} workgroups of {pl['waves']} waves")
    for rl, nm in ((0, "whole job"), (2, "consumer")):
        m = role == rl
        if not m.any():
            continue
        print(f"  {nm:9s} waves {m.sum():5d}: " + "  ".join(
            f"{names[k]} {d[k][m].mean():.0f}" for k in range(6)) + f"  total {tot[m].mean():.0f} (max {tot[m].max():.0f}) cyc")
    cons = role == 2
    if cons.any():
        got = cons & (polls > 0)
        print(f"  producers (from their consumers' slots): cycles to handoff mean {pcyc[got].mean():.0f} "
              f"p90 {np.percentile(pcyc[got], 90):.0f} max {pcyc[got].max():.0f}")
        print(f"  consumers {cons.sum()}: polled once {(cons & (polls == 1)).sum()}, more than once "
              f"{(cons & (polls > 1)).sum()} (max {polls[cons].max()} polls), fell back {(cons & (polls <= 0)).sum()}")
        print(f"  consumer wait (its 'cheb' phase, start to columns in hand): mean {d[1][cons].mean():.0f} "
              f"p90 {np.percentile(d[1][cons], 90):.0f} max {d[1][cons].max():.0f} cyc")
    pct = [10, 50, 90, 99, 100]
    print("  wave end times (us after the first start) " + "  ".join(
        f"p{q} {np.percentile(rt1, q):.2f}" for q in pct))
    for rl, nm in ((0, "whole job"), (2, "consumer")):
        if (role == rl).any():
            print(f"    {nm:9s} end " + "  ".join(f"p{q} {np.percentile(rt1[role == rl], q):.2f}" for q in pct))
    # placement: per workgroup, the SIMD of each role in wave order; the CU(s) it ran on
    pat = defaultdict(int)
    cus = defaultdict(set)
    lines = []
    for b in range(pl["workgroups"]):
        m = np.flatnonzero(wg == b)
        m = m[np.argsort(wv[m])]
        wh = [int(simd_of[k]) for k in m if role[k] == 0]
        co = [int(simd_of[k]) for k in m if role[k] == 2]
        pr = [int(psimd[k]) if polls[k] > 0 else -1 for k in m if role[k] == 2]
        where = sorted({cu_of[k] for k in m})
        for c in where:
            cus[c].add(b)
        key = (tuple(wh), tuple(pr), tuple(co))
        pat[key] += 1
        lines.append(f"  wg {b:3d} cu {where}: whole {wh} producer {pr} consumer {co}")
    print(f"  placement patterns (SIMD of whole jobs | producers | consumers, by wave index): {len(pat)} distinct")
    for key, c in sorted(pat.items(), key=lambda kv: -kv[1])[:8]:
        print(f"    {c:4d} x  {list(key[0])} | {list(key[1])} | {list(key[2])}")
    print(f"  (SE, SH, CU) ids seen {len(cus)}; workgroups sharing an id with another: "
          f"{sum(len(v) > 1 for v in cus.values())} ids (the id does not carry the XCD)")
    per_simd = np.array([np.bincount([int(simd_of[k]) for k in np.flatnonzero(wg == b)], minlength=4)
                         for b in range(pl["workgroups"])])
    print(f"  resident waves per SIMD (whole + consumer), mean over workgroups: {per_simd.mean(axis=0).round(2).tolist()}")
    print("\n".join(lines))
