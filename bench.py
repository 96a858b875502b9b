"""Benchmark: Lindblad parameter points/s on the C2 sweep (BASELINE.json configs[1]).

    python bench.py [--gpus N --steps K --warmup W] [--workload c1|c2|c3|c4|c5|shaped|dim4|ket|coherence|opt_lp|opt_smooth]

A step = one propagation of this rank's 10,000-point LP-square (Omega, Delta)
sweep -- every point's 4 basis density matrices through both pulses, noise
rates from the reference formulas -- with inputs resident in HBM.  ``--workload
c3`` runs the 100k-point smooth-JP (Omega, Omega*tau) Pareto sweep instead
(300 reference segments per point); ``--workload c4`` the 1M-point species x
temperature x tweezer-power LP-square grid (BASELINE configs[3]), range-sharded
over the ranks (strong scaling: the global grid is fixed); ``--workload c5`` the
4096-point three-atom blockade grid with 256 quantum-jump trajectories per point
(BASELINE configs[4]), strong-scaled the same way.  ``shaped`` / ``dim4`` / ``ket`` /
``coherence`` time the other kernels (shaped LP, dim 4, noise-free kets, process-map
coherences) on their own grids; ``opt_lp`` / ``opt_smooth`` run the reference's
published optimiser workloads (demo notebook settings) end to end.  These are
secondary lines, not the metric.  With N > 1
ranks (one process per GPU: under torch.distributed.run, or started by this script
itself when ``--gpus N`` is given without WORLD_SIZE in the environment) the global sweep is N x 10k
points range-partitioned by Delta/Omega; no collective touches the data path
(weak scaling); a gloo barrier brackets the timed region and the max time over
ranks is reported.  Rank 0 prints one JSON line.

A plain run sets up, warms up, times the K steps and prints the line (headline fields,
configuration and the roofline of the timed launches themselves).  ``--full`` adds every
measurement that takes runs of its own: isolated launches (``kernel_ms_isolated``), the
host-buffer boundary (``host_path``), ``end_to_end``, ``pipelined`` and the CPU baseline
(``cpu_baseline``; ``--no-cpu-baseline`` leaves that one out of a full run).
``--dump-outputs DIR`` writes what the last timed step left in HBM -- the arrays a caller
of the timed path fetches -- as ``DIR/<name>.npy`` (float64, at most 64 MB: beyond that a
fixed seeded sample of the points, their indices in ``points.npy``; summary rows that
the evolution does not define are left out, ``summary_rows.npy`` names the rest).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md chip table (spec)
FP64_PEAK_TFLOPS = 78.6    # MI355X FP64 vector (spec)
# FLOPs per generator application (one 25-vector): apply_A 75 + apply_B 75 + V 12 + Clenshaw 25 FMAs
FLOP_PER_MATVEC = 2 * (75 + 75 + 12 + 25)
# identical atoms: the symmetric column on its 15-entry triangle (apply_Lsym): every
# output (i <= j) costs row i + row j of M (1, 3, 3, 4, 4 ops), V 6, Clenshaw 15
FLOP_PER_MATVEC_SYM = 2 * (6 * (1 + 3 + 3 + 4 + 4) + 6 + 15)
# the 16-lane DPP-row kernel builds phase-0 propagators only (real Rabi frequency, hy = 0):
# rows 0-4 of M cost 1, 2, 2, 2 FMAs and 3 FMAs + 1 subtraction (2, 4, 4, 4, 7 flops) per
# output, V 6 FMAs, the unit start vector's Clenshaw term 1 add on the lane's own coordinate
FLOP_PER_MATVEC_SYM16 = 6 * (2 + 4 + 4 + 4 + 7) + 2 * 6 + 1
FLOP_PER_SQUARING = 2 * 25 ** 3          # one 25x25 real matrix product
# identical atoms: only the block-triangular symmetric block [[B, C], [0, D]] (5 + 10):
# B^2 (125) + BC + CD (250 + 500) + D^2 (1000) FMAs
FLOP_PER_SQUARING_SYM = 2 * (5 ** 3 + 5 * 5 * 10 + 5 * 10 * 10 + 10 ** 3)
# R_k <- U R_k for the 4 inputs per segment, each on its invariant support only (|00>: 1x1,
# |01>/|10>: 5x5, |11>: 25x25); identical atoms: |10> is the atom-swap mirror of |01>
FLOP_PER_STATE_UPDATE = 2 * (1 + 25 + 25 + 625)
FLOP_PER_STATE_UPDATE_SYM = 2 * (1 + 25 + 625)
# the 16-lane DPP-row kernel (csrc/ryd_sym16.inc) keeps |11> on its 15-coordinate exchange-
# symmetric triangle: 15 x 15 + the single-atom 5 x 5 (|01>, |10> its mirror) + |00>
FLOP_PER_STATE_UPDATE_SYM16 = 2 * (1 + 25 + 225)
N_OMEGA, N_DELTA = 100, 100
# PMC-measured HBM bytes per launch of the dominant kernel (rocprofv3 --pmc FETCH_SIZE /
# WRITE_SIZE in separate passes, FETCH_SIZE x2 per MI355X_MICROARCH.md), committed under
# profiles/ by tools/pmc_traffic.py; matched on workload + method + points per launch.
TRAFFIC_FILE = os.path.join(REPO, "profiles", "pmc_traffic.json")


def _measured_traffic(workload: str, method: str, n: int, kernel: str):
    """The committed PMC HBM-traffic row (tools/pmc_traffic.py) for this workload, size
    and dominant kernel, or None."""
    try:
        with open(TRAFFIC_FILE) as f:
            rows = json.load(f)
    except (OSError, ValueError):
        return None
    for r in rows:
        if (r.get("workload") == workload and r.get("method") == method and r.get("n") == n
                and r.get("kernel") == kernel):
            return r
    return None


DUMP_MAX_BYTES = 64 * 10 ** 6    # --dump-outputs: all files of one rank together
DUMP_SEED = 20260215
DUMP_RESERVE = 8192               # the .npy headers and summary_rows


def dump_outputs(dirname: str, rank: int, ws: int, n: int, arrays: dict) -> None:
    """--dump-outputs: ``arrays`` maps a name to (array, point axis, entries per point along
    that axis; point p owns p * g ... p * g + g - 1).  Everything goes out as float64
    ``<name>.npy`` (``<name>.rank<r>.npy`` with more than one rank), with the point indices
    in ``points``; if the full arrays exceed DUMP_MAX_BYTES, a sorted sample of the points
    drawn from a fixed seed is written instead (the same points in every run).  A summary
    row the kernel does not compute for this evolution (NaN at every point: the overlaps,
    controlled phase and penalty of a Lindblad run) is left out, the rows written are
    named in ``summary_rows``; any other non-finite value is an error."""
    arrays = dict(arrays)
    sfx = f".rank{rank}" if ws > 1 else ""
    os.makedirs(dirname, exist_ok=True)
    if "summary" in arrays:
        a, axis, g = arrays["summary"]
        rows = np.flatnonzero(~np.isnan(a).all(axis=1))
        arrays["summary"] = (a[rows], axis, g)
        np.save(os.path.join(dirname, f"summary_rows{sfx}.npy"), rows.astype(np.float64))
    for name, (a, _, _) in arrays.items():
        if not np.isfinite(a).all():
            raise ValueError(f"--dump-outputs: {name} holds non-finite values")
    per_point = 8 + sum(8 * (a.size // n) for a, _, _ in arrays.values())
    keep = (DUMP_MAX_BYTES - DUMP_RESERVE) // per_point
    pts = np.arange(n)
    if n > keep:
        pts = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=keep, replace=False))
    for name, (a, axis, g) in arrays.items():
        if n > keep:
            a = np.take(a, (pts[:, None] * g + np.arange(g)).ravel(), axis=axis)
        np.save(os.path.join(dirname, f"{name}{sfx}.npy"), np.ascontiguousarray(a, dtype=np.float64))
    np.save(os.path.join(dirname, f"points{sfx}.npy"), pts.astype(np.float64))


def _dist():
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    pg = None
    if ws > 1:
        import torch.distributed as dist   # CPU gloo: barrier + max only, never on the data path
        dist.init_process_group("gloo")
        pg = dist
    return ws, rank, local, pg


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int, argv, timeout_s: float = 0.0) -> int:
    """``--gpus N`` without a launcher around us: start N rank processes of this script
    (one per GPU) and wait for them.  The parent makes no GPU call (it never imports the
    engine or torch), so nothing here initialises HIP before the children start; each
    child is a fresh interpreter with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, maps
    LOCAL_RANK -> device LOCAL_RANK % device_count, and rank 0 prints the JSON line on the
    inherited stdout.  If any rank fails the others are stopped (they would wait at the
    barrier forever) and the first failing exit code is returned."""
    import subprocess
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__), *argv], env=env))
    t0 = time.monotonic()
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
        if rc != 0 or (timeout_s > 0 and time.monotonic() - t0 > timeout_s):
            for p in live:              # our own children, by PID
                p.terminate()
            for p in live:
                try:
                    p.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            if rc == 0:
                rc = 124
            break
        time.sleep(0.05)
    return rc


def _rank_device(local: int) -> int:
    """LOCAL_RANK -> HIP device: LOCAL_RANK % visible devices (ranks share a device when
    N exceeds the devices: a functional run, not a scaling point)."""
    from noisyquantumsimulator_amd import engine as E
    return local % E.device_count()


def _placement(ws: int, local: int, dev: int) -> dict:
    from noisyquantumsimulator_amd import engine as E
    cnt = E.device_count()
    shared = ws > cnt
    return {"device": dev, "visible_devices": cnt, "ranks_share_devices": shared,
            "note": ("ranks share devices (N > visible GPUs): functional check of the N-rank path, "
                     "not a scaling point") if shared else "one rank per GPU"}


def run_stub(ws, rank, local, pg):
    """GPU-free rank body for the launcher test: every rank reports its environment, rank
    0 prints them as one JSON line after a barrier."""
    info = {k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR")}
    info["pid"] = os.getpid()
    if os.environ.get("RYD_BENCH_STUB_FAIL_RANK") == str(rank):
        sys.exit(3)          # launcher test: a failing rank must fail the job
    ranks = [info]
    if pg is not None:
        ranks = [None] * ws
        pg.all_gather_object(ranks, info)
        _barrier(pg)
    if rank == 0:
        print(json.dumps({"stub": True, "n_ranks": ws, "ranks": ranks}), flush=True)
    if pg is not None:
        pg.destroy_process_group()


def _barrier(pg):
    if pg is not None:
        pg.barrier()


def _max_over_ranks(pg, x: float) -> float:
    if pg is None:
        return x
    import torch
    t = torch.tensor([x], dtype=torch.float64)
    pg.all_reduce(t, op=pg.ReduceOp.MAX)
    return float(t.item())


def cpu_baseline(sample: int, procs: int, workload: str = "c2"):
    """QuTiP-like CPU restatement timed on the host cores (oracle/cpu_baseline.py),
    in a clean child process with single-threaded BLAS."""
    import subprocess
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "oracle.cpu_baseline", "--sample", str(sample),
                          "--procs", str(procs), "--workload", workload], cwd=REPO, env=env, check=True,
                         capture_output=True, text=True, timeout=600)
    res = json.loads(out.stdout.strip().splitlines()[-1])
    # `cores` = worker processes actually used; the box's visible CPUs beside it
    res["host_cpus_visible"] = os.cpu_count()
    res["cpu_share"] = ("one-GPU box share: OMP_NUM_THREADS=" + os.environ.get("OMP_NUM_THREADS", "?")
                        + "; os.cpu_count() counts the whole machine")
    res["per_core"] = res["value"] / max(1, res["cores"])
    return res


def cpu_procs() -> int:
    """Worker processes for the CPU baseline: the CPU share of this box
    (OMP_NUM_THREADS, 16 on the GPU box), capped by the visible CPUs."""
    share = int(os.environ.get("OMP_NUM_THREADS", "16") or 16)
    return max(1, min(share, os.cpu_count() or 1))


def pipelined_c2(params, protocol, n_steps, args, dev, n):
    """The same C2 steps as `value`, alternated over two streams of the device (two engine
    slots, each its own copy of the inputs and outputs): step k+1's waves fill the SIMDs that
    step k's launch leaves idle at its tail (2500 waves on 1024 SIMDs: 452 hold three, the
    rest two).  Reported beside `value`, never as it: the steps overlap, so this is the
    throughput of a sweep of many 10k-point batches, not of one batch per launch."""
    from noisyquantumsimulator_amd import engine as E
    eng2 = E.Engine(devices=[dev, dev])
    dbs = [E.DeviceBatch(eng2, params, protocol, "lindblad", n_steps=n_steps, method=args.method, slot=k)
           for k in range(2)]
    for _ in range(max(args.warmup, 2)):
        for db in dbs:
            db.launch()
    dbs[0].synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        dbs[k & 1].launch()
    dbs[0].synchronize()
    dt = time.perf_counter() - t0
    for db in dbs:
        r = db.fetch()
        assert np.all(r.status == 0), "engine reported per-point failures"
    return {"streams": 2, "points_per_s": n * args.steps / dt, "ms_per_step": dt * 1e3 / args.steps,
            "note": "steps alternated over two streams of one device (overlapping launches); "
                    "a many-batch sweep's throughput, not the per-launch metric"}


def end_to_end_c4(args, eng, host_params, t_host_derive):
    """C4 end to end with the derivation on the device (hot-path row a1, ryd_derive): the
    sweep's varying columns (species index, T, P_tweezer: 24 B per point) go to HBM once,
    then each step derives the parameter block in HBM and propagates it.  Reported beside
    the host derivation the kernel-only line starts from (physics.derive_batch +
    pack_params, timed once) and checked against it at 1e-13 relative."""
    from noisyquantumsimulator_amd import engine as E
    from noisyquantumsimulator_amd import sweeps as SW
    ws_, rk = (args.c4_shards, args.c4_rank) if args.c4_shards else (int(os.environ.get("WORLD_SIZE", 1)),
                                                                   int(os.environ.get("RANK", 0)))
    t0 = time.perf_counter()
    inp = SW.c4_rank_inputs(rk, ws_)
    t_cols = time.perf_counter() - t0
    sw = E.DeviceSweep(eng, inp)
    n = sw.n
    ups = []
    for _ in range(3):
        t0 = time.perf_counter()
        sw.upload()
        ups.append(time.perf_counter() - t0)
    for _ in range(max(args.warmup, 2)):
        sw.launch()
    sw.synchronize()
    d_ms = float(np.mean([sw.derive(timed=True) for _ in range(5)]))
    p_ms = float(np.mean([sw.propagate(timed=True) for _ in range(3)]))
    sw.mark(0)
    for _ in range(args.steps):
        sw.launch()
    sw.mark(1)
    step_ms = sw.mark_elapsed() / args.steps
    # with the inputs' H2D inside each step (host columns -> HBM -> derive -> engine)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sw.upload()
        sw.launch()
    sw.synchronize()
    wh_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    pd, warn = sw.fetch_params()
    rel = np.abs(pd - host_params) / np.maximum(np.abs(host_params), 1e-300)
    rel[(pd == host_params)] = 0.0
    res = sw.fetch()
    assert np.all((res.status & E.N.STATUS_FAIL_MASK) == 0), "engine reported per-point failures"
    sw.free()
    return {"points": n, "derive_ms": d_ms, "engine_ms": p_ms, "derive_plus_engine_ms": step_ms,
            "points_per_s": n / (step_ms * 1e-3),
            "with_input_h2d_ms": wh_ms, "input_h2d_ms": float(np.median(ups)) * 1e3,
            "input_bytes": int(inp.cols.nbytes), "host_columns_ms": t_cols * 1e3,
            "host_derive_ms": t_host_derive * 1e3,
            "device_vs_host_params_max_rel": float(rel.max()),
            "note": ("derive_plus_engine_ms: ryd_derive_device + ryd_run_batch_device back to back on one "
                     "stream, HIP events over K steps, inputs resident; with_input_h2d_ms adds the H2D of "
                     "the varying columns each step (wall clock); host_derive_ms: the vectorised host "
                     "derivation (physics.derive_batch) this replaces, one call")}


def host_path_c(eng, params, protocol, n_steps, args, n):
    """The host-buffer form of the boundary (ryd_run_batch: params H2D, kernel, state +
    summary D2H) -- PCIe-inclusive, reported beside `value`, never as it."""
    from noisyquantumsimulator_amd import engine as E
    t_h = time.perf_counter()
    rh = eng.run(params, protocol, "lindblad", n_steps=n_steps, method=args.method)
    t_h = time.perf_counter() - t_h
    assert np.all(rh.status == 0)
    # warm calls (device workspace and pinned staging reused): the median of 5
    hp = []
    for _ in range(5):
        t_h = time.perf_counter()
        rh = eng.run(params, protocol, "lindblad", n_steps=n_steps, method=args.method)
        t_h = time.perf_counter() - t_h
        assert np.all(rh.status == 0)
        hp.append((t_h, rh, eng.last_timeline()))
    t_h, rh, tl = sorted(hp, key=lambda x: x[0])[len(hp) // 2]
    bytes_d2h = 8 * (25 * 4 + E.N.NSUMMARY) * n + 4 * n
    return {"points_per_s": n / t_h, "wall_ms": t_h * 1e3, "h2d_ms": rh.h2d_ms,
            "kernel_ms": rh.kernel_ms, "d2h_ms": rh.d2h_ms, "bytes_d2h": bytes_d2h,
            "d2h_gbs": bytes_d2h / (rh.d2h_ms * 1e-3) / 1e9 if rh.d2h_ms > 0 else None,
            "host_pack_ms": tl["pack_ms"], "host_unpack_ms": tl["unpack_ms"],
            "host_pack_gbs": 8 * 38 * n / (tl["pack_ms"] * 1e-3) / 1e9,
            "host_unpack_gbs": bytes_d2h / (tl["unpack_ms"] * 1e-3) / 1e9, "calls": "median of 5 warm calls",
            "staging": "persistent device workspace + pinned staging per handle slot; "
                       "unpack into the caller's strided numpy arrays on host threads"}


def end_to_end_c2():
    """simulate_CZ_gate_batch on the C2 grid: derivation (host) + engine (host-buffer
    boundary) + the reference-penalty epilogue (zheevr on host threads, the batch call's
    default gauge check) -- the whole Python drop-in call, wall clock: one warm-up call, then
    the median of five (min and max beside it; the stage timings are the median call's)."""
    from noisyquantumsimulator_amd import simulation as S
    from noisyquantumsimulator_amd import sweeps as SW
    si, n, kw = SW.omega_delta_call()
    out = {}
    for gauge in (True, False):
        S.simulate_CZ_gate_batch(si, n, gauge_check=gauge, **kw)
        runs = []
        for _ in range(5):
            t0 = time.perf_counter()
            br = S.simulate_CZ_gate_batch(si, n, gauge_check=gauge, **kw)
            runs.append((time.perf_counter() - t0, br))
        assert all(b.ok.all() for _, b in runs)
        runs.sort(key=lambda x: x[0])
        dt, br = runs[2]
        key = "gauge_check" if gauge else "no_gauge_check"
        out[key] = dict(points_per_s=n / dt, wall_ms=dt * 1e3, wall_ms_min=runs[0][0] * 1e3,
                        wall_ms_max=runs[-1][0] * 1e3,
                        **{k: round(v, 3) for k, v in br.timings.items()},
                        gauge_unstable=int(br.gauge_unstable.sum()))
    out["points"] = n
    out["call"] = "simulate_CZ_gate_batch(LPSimulationInputs(medium), 10000, overrides=C2 grid)"
    return out


# C5 (three-atom trajectories) accounting, per include/ryd_engine.h RYD_TS_*:
# one ladder step = block matvec (124 complex MACs = 992 flops) + norm (108 flops);
# one block squaring = 8 + 64 + 512 complex MACs (4672 flops) + 168 adds;
# on-chip reduction = 378 elements x 14 flops per trajectory.
FLOP_PER_LADDER_STEP = 8 * 124 + 2 * 54
FLOP_PER_BLOCK_SQUARING = 8 * (8 + 64 + 512) + 2 * 84
FLOP_PER_TRAJ_REDUCTION = 378 * 14
# the exchange-symmetry-adapted kernel (traj3s_kernel, the default): a ladder step is the
# quadratic form x^dag G_l x over the 12 block instances (86 complex-pair terms: 344
# flops); an accepted step applies (I + X_l) (66 complex MACs + the norm: 636 flops); one
# ladder level is 71 complex MACs + 46 adds (squaring) + 71 complex MACs (its Gram level)
FLOP_PER_SYM_STEP = 344
FLOP_PER_SYM_APPLY = 8 * 66 + 2 * 54
FLOP_PER_SYM_LEVEL = 8 * 71 + 92 + 8 * 71
# the exact-jump-time kernel (traj3e_kernel, ladder_levels = 0): one evaluation of psi(t) is
# 12 complex exponentials (counted as their 2 scaling multiplies, not as flops of their own),
# 26 complex scalings, the 66-MAC block product and the norm + decay sums (27 x 4); a
# change to eigen-coordinates (segment start, after each jump) is another 66 complex MACs
FLOP_PER_EIG_EVAL = 2 * 12 + 6 * 26 + 8 * 66 + 4 * 27
FLOP_PER_EIG_COEFFS = 8 * 66
C5_BYTES_PER_POINT = 8 * 15 + 8 * (1458 + 729 + 10) + 4   # params read; rho, se, summary, status


def _c1_hamiltonian(Om: complex, Dl: float, V: float) -> np.ndarray:
    """The two-atom dim-3 H of RG/hamiltonians.py:584-1274 for the generic-seam timing:
    sum_atoms [(Om/2)|r><1| + h.c. - Dl P_r] + V P_rr (levels 0, 1, r)."""
    h1 = np.zeros((3, 3), complex)
    h1[2, 1] = Om / 2
    h1[1, 2] = np.conj(Om) / 2
    h1[2, 2] = -Dl
    I = np.eye(3)
    prr = np.zeros((9, 9))
    prr[8, 8] = 1.0
    return np.kron(h1, I) + np.kron(I, h1) + V * prr


def run_c1(args, ws, rank, local, pg):
    """C1: ONE dim-3 LP-square point with one collapse operator, as a
    single-point latency -- what every unmodified per-point caller of the reference
    (examples/research_parameter_sweeps.py:119, RG/optimize_cz_gate.py:1117,
    RG/optimization.py:531) sees per simulate_CZ_gate call.  Reported: the engine path on
    the exact C1 inputs (host-buffer ryd_run_batch + the reference phase epilogue), the
    drop-in simulate_CZ_gate on the reference's default noisy LP configuration (derive +
    engine + epilogue + SimulationResult), each the median of warm calls, and the oracle's
    ZVODE CPU path on the C1 point beside them."""
    from noisyquantumsimulator_amd import configurations as CF
    from noisyquantumsimulator_amd import engine as E
    from noisyquantumsimulator_amd import simulation as SIM
    from noisyquantumsimulator_amd import sweeps as SW
    dev = _rank_device(local)
    eng = E.Engine(devices=[dev])
    prm = SW.c1_params()
    reps = max(args.steps, 20)

    def engine_call():
        t0 = time.perf_counter()
        r = eng.run(prm, "lp_square", "lindblad")
        t1 = time.perf_counter()
        ph, fl = E.mixed_phase(r.state, 1, 3, gauge_check=True)
        cp, pen = SIM._cp_penalty(ph)
        pops = r.populations()[0]
        avg = float((pops[0] + pops[1] + pops[2] + pops[3] * pen[0]) / 4.0)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, r.kernel_ms, avg, int(r.status[0] | fl[0])
    for _ in range(max(args.warmup, 3)):
        engine_call()
    runs = [engine_call() for _ in range(reps)]
    eng_ms = [x[0] for x in runs]
    epi_ms = [x[1] for x in runs]
    k_ms = [x[2] for x in runs]
    tot = [x[0] + x[1] for x in runs]
    avg_f, st = runs[-1][3], runs[-1][4]
    # the drop-in per-point call on the reference's default noisy LP configuration
    si = CF.LPSimulationInputs()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(3):
            SIM.simulate_CZ_gate(si, include_noise=True)
        dt = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = SIM.simulate_CZ_gate(si, include_noise=True)
            dt.append((time.perf_counter() - t0) * 1e3)
        parts = []
        for _ in range(reps):
            br = SIM.simulate_CZ_gate_batch(si, 1, include_noise=True, return_states=True)
            parts.append(br.timings)
    med = lambda v: float(np.median(v))
    # the generic evolve_state seam on the same C1 point (the reference's two mesolve calls
    # per basis input, H1 then H2 = H(Omega xi), one collapse operator): 4 problems, 2 segments
    c1 = SW.c1_point()
    H1 = _c1_hamiltonian(c1["Omega"], c1["Delta"], c1["V"])
    H2 = _c1_hamiltonian(c1["Omega"] * c1["xi"], c1["Delta"], c1["V"])
    cop = np.zeros((9, 9), complex)
    for b in range(3):
        cop[3 + b, 6 + b] = np.sqrt(c1["gamma"])                  # |1><r| (x) I
    kets = np.zeros((4, 9), complex)
    for k, idx in enumerate((0, 1, 3, 4)):
        kets[k, idx] = 1.0
    Hs = np.broadcast_to(np.stack([H1, H2])[None], (4, 2, 9, 9))
    Ts = np.full((4, 2), c1["tau"])
    for _ in range(3):
        SIM.evolve_state_batch(Hs, kets, Ts, [[cop]] * 4, devices=[dev])
    gen_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        SIM.evolve_state_batch(Hs, kets, Ts, [[cop]] * 4, devices=[dev])
        gen_ms.append((time.perf_counter() - t0) * 1e3)
    dropin = {k: med([p[k] for p in parts]) for k in ("derive_ms", "engine_ms", "epilogue_ms", "total_ms")}
    dropin["simulate_CZ_gate_ms"] = med(dt)
    dropin["result_assembly_ms"] = med(dt) - dropin["total_ms"]
    dropin["avg_fidelity"] = float(res.avg_fidelity)
    out = {
        "metric": "C1 single-point latency (one 2-atom 3-level Rydberg CZ point, 1 collapse op)",
        "value": med(tot), "unit": "ms", "n_gpus": 1, "steps": reps, "warmup": max(args.warmup, 3),
        "ms_per_step": med(tot), "higher_is_better": False, "scaling": "none", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "C1: dim 3, LP square, Omega = 2 pi 5 MHz, V/Omega = 100, Delta/Omega = 0.377371, "
                               "Omega tau = 4.29268, xi from compute_phase_shift_xi, one c_op sqrt(1/140 us) |1><r| (x) I",
                   "placement": _placement(1, local, dev)},
        "engine_path": {"engine_call_ms": med(eng_ms), "kernel_ms": med(k_ms), "epilogue_ms": med(epi_ms),
                        "avg_fidelity": avg_f, "status": st,
                        "note": "host-buffer ryd_run_batch (pack, H2D, kernel, D2H) + ryd_mixed_phase with the "
                                "16-probe gauge check"},
        "generic_evolve_state": {"ms": med(gen_ms),
                                 "note": "simulation.evolve_state_batch (ryd_evolve_generic): the C1 point as dense "
                                         "9x9 H1, H2 and one jump operator, 4 basis inputs x 2 segments, host arrays in "
                                         "and out (the reference's evolve_state seam, RG/simulation.py:647-690)"},
        "dropin_default_lp": dict(dropin, note="simulate_CZ_gate(LPSimulationInputs(), include_noise=True): the "
                                               "reference's default noisy LP point (14 c_ops collapsed to 8 channels); "
                                               "breakdown from simulate_CZ_gate_batch(n=1) timings"),
    }
    if args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(10, 1, "c1")
        out["cpu_over_gpu"] = out["cpu_baseline"]["value"] / out["value"]
    print(json.dumps(out), flush=True)
    eng.close()


def run_c5(args, ws, rank, local, pg):
    """C5: 4096-point (Omega, V/Omega) three-atom blockade grid, 256 quantum-jump
    trajectories per point, strong-scaled over the ranks (range shards keyed by their
    global point offset, so the random streams do not depend on N)."""
    from noisyquantumsimulator_amd import engine as E
    from noisyquantumsimulator_amd import sweeps as SW
    from noisyquantumsimulator_amd import trajectories as TR
    # --c5-shards: one GPU, one rank's shard of an N-way split (the scaling proxy);
    # --c5-order strided: rank r takes points r, r + N, ... of the Omega-major grid
    r_, ws_ = (args.c5_rank, args.c5_shards) if args.c5_shards else (rank, ws)
    stride = 1
    if args.c5_order == "strided":
        batch, off, stride = SW.c5_strided_shard(r_, ws_)
    else:
        batch, off = SW.c5_rank_shard(r_, ws_, order=args.c5_order)
    params = E.pack_params(batch)
    n = batch.n
    dev = _rank_device(local)
    eng = E.Engine(devices=[dev])
    db = TR.TrajectoryDeviceBatch(eng, params, "lp_square", TR.plus_state(), n_traj=args.n_traj,
                                  ladder_levels=args.ladder if args.ladder >= 0 else TR.DEFAULT_LADDER,
                                  seed=20260215, point_offset=off, kernel=args.c5_kernel, point_stride=stride)
    for _ in range(args.warmup):
        db.launch()
    db.synchronize()
    _barrier(pg)
    db.synchronize()
    t0 = time.perf_counter()
    db.mark(0)
    for _ in range(args.steps):
        db.launch()
    db.mark(1)
    db.synchronize()
    _barrier(pg)
    dt = time.perf_counter() - t0
    dt_max = _max_over_ranks(pg, dt)
    # the dominant kernel's average launch duration: HIP events on its stream over the
    # timed region (back-to-back launches; the only work on that stream)
    k_ms = db.mark_elapsed() / args.steps
    res = db.fetch()
    assert np.all(res.status == 0), "engine reported per-point failures"
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, ws, n,
                     {"rho_re": (res.rho.real, 0, 1), "rho_im": (res.rho.imag, 0, 1), "se": (res.se, 0, 1),
                      "summary": (res.summary, 1, 1), "status": (res.status, 0, 1)})
    # --full: one launch at a time, events around each (includes event/sync overhead)
    k_iso = (float(np.mean([db.launch(timed=True) for _ in range(max(3, min(args.steps, 10)))]))
             if args.full else None)
    it_use = float(res.col("ITER_USEFUL").sum())
    it_exec = float(res.col("ITER_EXEC").sum())
    napply = float(res.col("RESERVED").sum())
    exact = db.desc.ladder_levels == TR.N.T["EXACT"]
    wg = os.environ.get("RYD_T_WG", "0") == "1"
    rows = (args.c5_kernel == "rows" or (args.c5_kernel == "auto" and os.environ.get("RYD_T_ROWS", "0") != "0"))
    kernel = (("traj3w_kernel" if wg else ("traj3r_kernel" if rows else "traj3e_kernel")) if exact
              else ("traj3s_kernel" if napply > 0 else "traj3_kernel"))
    if exact:                                       # traj3e_kernel: evaluations + basis changes
        ntr = args.n_traj
        ncoef = float((res.col("MEAN_JUMPS") * ntr + 2.0 * res.col("FRAC_JUMPED") * ntr + 2.0).sum())
        flops = it_use * FLOP_PER_EIG_EVAL + ncoef * FLOP_PER_EIG_COEFFS + n * ntr * FLOP_PER_TRAJ_REDUCTION
    elif napply > 0:                                # traj3s_kernel (adapted basis)
        flops = (it_use * FLOP_PER_SYM_STEP + napply * FLOP_PER_SYM_APPLY
                 + float(res.col("NSQUARE").sum()) * FLOP_PER_SYM_LEVEL + n * args.n_traj * FLOP_PER_TRAJ_REDUCTION)
    else:                                           # traj3_kernel (RYD_T_SYM=0)
        flops = (it_use * FLOP_PER_LADDER_STEP + float(res.col("NSQUARE").sum()) * FLOP_PER_BLOCK_SQUARING
                 + n * args.n_traj * FLOP_PER_TRAJ_REDUCTION)
    achieved_tf = flops / (k_ms * 1e-3) / 1e12
    achieved_gbs = C5_BYTES_PER_POINT * n / (k_ms * 1e-3) / 1e9
    tr = (_measured_traffic("c5", "mcwf", n, kernel)
          if args.n_traj == 256 else None)
    traffic = tr["bytes_per_launch"] if tr else None
    total = (n if args.c5_shards else SW.C5_POINTS) * args.steps
    out = {
        "metric": "Lindblad param-points/sec (2-atom Rydberg CZ sweep); achieved HBM GB/s vs peak",
        "value": total / dt_max, "unit": "points/s", "n_gpus": ws, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": ("C5: 4096-point (Omega 1-10 MHz x V/Omega 10-1000) three-atom "
                                f"blockade grid, LP square, {args.n_traj} quantum-jump trajectories "
                                "per point (Philox4x32-10), |+++> input, medium-apparatus rates"),
                   "points_per_gpu": n, "global_points": SW.C5_POINTS, "trajectories_per_point": args.n_traj,
                   "shard": (f"rank {args.c5_rank} of {args.c5_shards} (1-GPU scaling proxy)" if args.c5_shards
                             else None),
                   "trajectories_per_s": total * args.n_traj / dt_max,
                   "parallelism": f"range-shard x{ws}", "method": ("MCWF, exact jump times (Newton on the eigen-decomposed H_eff)" if exact
                              else "MCWF, binary expm1 ladder in LDS"),
                   "ladder_levels": db.desc.ladder_levels, "placement": _placement(ws, local, dev)},
        "roofline": {"bound": "fp64", "achieved": achieved_tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": achieved_tf / FP64_PEAK_TFLOPS, "traffic": traffic, "kernel": kernel,
                     "kernel_ms": k_ms, "kernel_ms_isolated": k_iso,
                     "flops_per_launch": flops, "exec_over_useful": it_exec / max(it_use, 1.0),
                     "mean_jumps": float(res.col("MEAN_JUMPS").mean())},
        "roofline_hbm": {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved_gbs / HBM_PEAK_GBS, "traffic": traffic,
                         "bytes_per_launch": C5_BYTES_PER_POINT * n},
    }
    if rank == 0 and ws == 1 and args.full and not args.no_cpu_baseline:
        procs = cpu_procs()
        out["cpu_baseline"] = cpu_baseline(min(args.cpu_sample, 64), procs, "c5")
    if rank == 0:
        print(json.dumps(out), flush=True)
    db.free()
    eng.close()
    if pg is not None:
        pg.destroy_process_group()


# secondary kernels: flops per Chebyshev term per lane, from the source
# (ryd_engine.hip): ket_cheb_kernel apply_K 48 FMA + 18 mul + 18 add + Clenshaw 18 FMA;
# lindblad4_cheb_kernel apply4_one x2 (2 x 6 x (16 FMA + 3 add)) + apply4_V 16 FMA +
# Clenshaw 36 FMA; coherence_cheb_kernel per point (2 + 2 lanes of 20 doubles, 2 of 8):
# KIND 0/1 4 m0_apply (13 FMA + 2 sub) + 20 CMAC (80 FMA) + 10 FMA + Clenshaw 20 FMA = 332,
# KIND 2 64 + 2 FMA + Clenshaw 8 FMA = 148, KIND 3 64 + 8 FMA = 144 -> 2*332 + 2*332 + 148 + 144.
FLOP_PER_KET_TERM = 2 * 48 + 18 + 18 + 2 * 18
# ket_block_kernel (the default ket method): per segment the 2x2 block in its frame (2
# complex mults for the phase, 4 + 2 adds: 40 flops) and the 3x3 symmetric block (4
# complex mults, 9 complex MACs, the double angle: 99 flops); per propagator build the
# 3x3 Jacobi (18 rotations x ~30 flops), the 2x2 closed form and U = Q E Q^T (~650 flops;
# the sincos / sqrt / divisions are not counted)
FLOP_PER_KET_BLOCK_SEG = 40 + 99
FLOP_PER_KET_BLOCK_BUILD = 650
FLOP_PER_DIM4_TERM = 2 * 6 * (2 * 16 + 3) + 2 * 16 + 2 * 36
FLOP_PER_COH_POINT_TERM = 2 * 332 + 2 * 332 + 148 + 144
# lindblad4_prop_kernel (ryd_dim4_prop.inc): one triangle-generator application (apply_Lsym4:
# the single-atom rows twice per output, 7 x (3+7+8+7+7+4) = 252 flops, the V term 32, the
# Clenshaw add 21) per term of each of the 15 D columns, one 6-vector column term (36 + 12)
# per term of each of the 6 B columns, one block-triangular squaring (round 5: the useful
# products only -- D D 15^3, B C + C D 6 x 6 x 15 + 6 x 15^2, B B 6^3 = 5481 FMA), one
# segment (21^2 + 6^2 FMA + the frames)
FLOP_PER_D4_APPLY = 252 + 32 + 21
# lindblad_shaped16_kernel (ryd_shaped16.inc), per series term of a point: the triangle
# generator (apply_Lsym: 95 FMAs), the single-atom 5-vector (13 FMAs + 2 subtractions) and the
# Clenshaw update of the 20 coordinates (a_k v + ... + b2: one FMA and one add each)
FLOP_PER_SHAPED16_TERM = 2 * 95 + 2 * 13 + 2 + 4 * 20
FLOP_PER_D4_SQUARING = 2 * (15 ** 3 + 6 * 6 * 15 + 6 * 15 ** 2 + 6 ** 3)
FLOP_PER_D4_SEGMENT = 2 * 21 ** 2 + 4 * 21 + 2 * 6 ** 2 + 8
FLOP_PER_D4_VEC_TERM = 36 + 12


def coh_prop_flops(params: np.ndarray, protocol: str) -> float:
    """Algorithmic flops of coherence_prop_kernel (ryd_coh_prop.inc) on a batch: per sector
    built (the (0,-1) sector, n = 10; (-1,-1) and (-1,+1), n = 4; (-1,0) too when the atoms
    differ) n Chebyshev columns x the series terms at x / 2^s (332 / 148 / 144 flops per
    term and column, as coherence_cheb_kernel's applications) + s squarings (the useful
    complex MACs of one squaring: 680 for n = 10, whose 2 invariant columns take 4 products
    each and the other 8 columns 84; 64 for n = 4) + per segment the inputs' n^2 complex
    MACs.  The kernel's own omega and s, restated (h_bounds + the rate sum;
    s = ceil(log2(x / CP_XS)), CP_XS = 0.5, terms = cheb_terms_small + 1); LP square and
    smooth JP build once."""
    from noisyquantumsimulator_amd import _native as N
    P = N.P
    Om, Dl, V, d1 = params[P["OMEGA"]], params[P["DELTA"]], params[P["V"]], params[P["DELTA1"]]
    tau = params[P["TAU"]]
    nseg, dt = (2, tau) if protocol == "lp_square" else (300, tau / 300)
    Dl = Dl if protocol != "bangbang" else 0.0 * Dl
    w = 0.5 * np.abs(Om)
    e = [np.zeros_like(Om), d1, -Dl]
    emin, emax = np.full_like(Om, np.inf), np.full_like(Om, -np.inf)
    for a1 in range(3):
        for a2 in range(a1, 3):
            E = e[a1] + e[a2] + (V if a1 == a2 == 2 else 0.0)
            r = w * ((a1 > 0) + (a2 > 0))
            emin, emax = np.minimum(emin, E - r), np.maximum(emax, E + r)
    rsum = np.abs(params[P["G1_A"]:P["GSC_A"] + 1]).sum(0) + np.abs(params[P["G1_B"]:P["GSC_B"] + 1]).sum(0)
    x = (emax - emin + rsum) * dt
    s = np.where(x > CP_XS, np.ceil(np.log2(np.maximum(x, 1e-300) / CP_XS)), 0.0)
    xs = x / 2.0 ** s
    terms = np.array([_cheb_terms_small(v) + 1 for v in xs], float)
    sym = np.all(params[P["G1_A"]:P["GSC_A"] + 1] == params[P["G1_B"]:P["GSC_B"] + 1], axis=0)
    f = 0.0
    for n, per_term, sq_macs, nin, on in ((10, 332, 680, 2, np.ones_like(sym)), (10, 332, 680, 2, ~sym),
                                          (4, 148, 64, 1, np.ones_like(sym)), (4, 144, 64, 1, np.ones_like(sym))):
        f += float((on * (n * terms * per_term + s * sq_macs * 8 + nseg * nin * n * n * 8)).sum())
    return f


CP_XS = 0.5                      # ryd_coh_prop.inc
# ryd_sym16.inc cheb_terms_small: the smallest doubles h = x / 2 whose j-th term reaches 1e-17
_TH_SMALL = (1e-17, 4.4721359549995795e-09, 3.914867641168864e-06, 0.00012446659545769568,
             0.0010371372893366482, 0.004394290351366487, 0.0125993232817844, 0.02822864716464555,
             0.05356271212458357, 0.09036001686117834, 0.1398168813097236, 0.20262580209060138,
             0.2790704614462359, 0.36912378048400807, 0.47253426642798413, 0.5888961629494429,
             0.7177037357024775)


def _cheb_terms_small(x: float) -> int:
    h = 0.5 * x
    return 1 + sum(1 for t in _TH_SMALL if h >= t)


def _cheb_terms(x: float) -> int:
    """ryd_engine.hip cheb_terms: series terms for tail < 1e-17."""
    if x < 24.0:
        t, k = 1.0, 0
        while True:
            k += 1
            t *= 0.5 * x / k
            if t < 1e-18 and k > x:
                return k
    return int(np.ceil(x + 12.0 * np.cbrt(x) + 10.0))
AUX = {
    # name: (kernel, state rows per input (0: coherence), bytes per point, description)
    "shaped": ("lindblad_shaped16_kernel", 25, 8 * 16 + 8 * 100 + 8 * 19 + 4,
               "C2 (Omega, Delta) grid with the cosine-shaped LP pulse (RG/simulation.py:2099-2231: 2 x 499 "
               "segments of tau/500, envelope sin^2, area correction 2), full reference noise, 25-dim sector "
               "(RYD_SHAPED16=0: lindblad_cheb_kernel, the per-lane Chebyshev cross-check)"),
    "dim4": ("lindblad4_cheb_kernel", 36, 8 * 17 + 8 * 144 + 8 * 19 + 4,
             "C2 (Omega, Delta) grid, LP square, hilbert_space_dim=4 (mJ sublevels r+/r-, mJ mixing; "
             "RG/hamiltonians.py:490-853), full reference noise, 36-dim sector"),
    "ket": ("ket_block_kernel", 18, 8 * 15 + 8 * 72 + 8 * 19 + 4,
            "C3 (Omega, Omega*tau) smooth-JP grid, 100k points x 300 segments, noise-free "
            "(kets: the optimiser's path, RG/simulation.py:683-690), exact block propagators"),
    "ket_cheb": ("ket_cheb_kernel", 18, 8 * 15 + 8 * 72 + 8 * 19 + 4,
                 "C3 (Omega, Omega*tau) smooth-JP grid, 100k points x 300 segments, noise-free, the "
                 "Chebyshev state-vector ket kernel (method cheb_vector, the cross-check)"),
    "coherence": ("coherence_prop_kernel", 0, 8 * 15 + 8 * 20 + 4 + 4,
                  "C2 (Omega, Delta) grid, LP square, full reference noise: the 6 upper qubit coherences "
                  "of the process map (noise_models Kraus/CPTP); one launch, one propagator per sector and "
                  "point (RYD_COH_PROP=0: coherence_cheb_kernel, the per-lane Chebyshev over the pulse)"),
}


def run_aux(args, ws, rank, local, pg):
    """Secondary kernels on their own workloads (HBM-resident inputs, HIP events on the
    launch stream): shaped LP, dim 4, kets, process-map coherences."""
    from noisyquantumsimulator_amd import engine as E
    from noisyquantumsimulator_amd import sweeps as SW
    kernel, width, bpp, desc = AUX[args.workload]
    if args.workload in ("ket", "ket_cheb"):
        batch = SW.c3_rank_shard(rank, ws, include_noise=False)
        protocol, evolution, n_steps, shape, dim = "smooth_jp", "ket", 300, "square", 3
    else:
        batch = SW.c2_rank_shard(rank, ws) if args.workload == "coherence" else SW.omega_delta_grid(
            100, 100 * ws, delta_slice=slice(rank * 100, (rank + 1) * 100),
            pulse_shape="cosine" if args.workload == "shaped" else "square",
            hilbert_space_dim=4 if args.workload == "dim4" else 3)
        protocol = E.protocol_key(batch)
        evolution, shape, dim = "lindblad", batch.pulse_shape.lower(), batch.dim
        n_steps = None
    params = E.pack_params(batch)
    n = batch.n
    dev = _rank_device(local)
    eng = E.Engine(devices=[dev])
    if args.workload == "coherence":
        db = E.CoherenceDeviceBatch(eng, params, protocol)
    else:
        db = E.DeviceBatch(eng, params, protocol, evolution, n_steps=n_steps, shape=shape,
                           method="chebyshev" if args.workload in ("ket", "shaped") or dim == 4 else "cheb_vector", dim=dim)
    for _ in range(args.warmup):
        db.launch()
    db.synchronize()
    _barrier(pg)
    db.synchronize()
    t0 = time.perf_counter()
    db.mark(0)
    for _ in range(args.steps):
        db.launch()
    db.mark(1)
    db.synchronize()
    _barrier(pg)
    dt = time.perf_counter() - t0
    dt_max = _max_over_ranks(pg, dt)
    k_ms = db.mark_elapsed() / args.steps
    if args.workload == "coherence":
        coh, st = db.fetch()
        assert np.all(st == 0), "engine reported per-point failures"
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rank, ws, n, {"coherences": (coh, 1, 1), "status": (st, 0, 1)})
        if os.environ.get("RYD_COH_PROP", "1") != "0":
            kernel = "coherence_prop_kernel"
            flops = coh_prop_flops(params, protocol)
            useful_exec = None
        else:
            # per-lane Chebyshev terms = those of the 25-dim vector kernel on the same segments
            # (same omega * dt per segment): its NMV_USEFUL / 4 per point
            kernel = "coherence_cheb_kernel"
            rv = eng.run(params, protocol, "lindblad", method="cheb_vector")
            terms = float(rv.col("NMV_USEFUL").sum()) / 4.0
            flops = terms * FLOP_PER_COH_POINT_TERM
            useful_exec = float(rv.col("NMV_EXEC").sum()) / max(float(rv.col("NMV_USEFUL").sum()), 1.0)
    else:
        res = db.fetch()
        assert np.all(res.status == 0), "engine reported per-point failures"
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rank, ws, n, {"state": (res.state, 1, 4), "summary": (res.summary, 1, 1),
                                                          "status": (res.status, 0, 1)})
        if args.workload == "ket":
            flops = (res.matvec_useful * FLOP_PER_KET_BLOCK_SEG
                     + float(res.col("NSQUARE").sum()) * FLOP_PER_KET_BLOCK_BUILD)
        elif args.workload == "shaped" and os.environ.get("RYD_SHAPED16", "1") != "0":
            kernel = "lindblad_shaped16_kernel"        # NMV_USEFUL: series terms per point
            flops = float(res.col("NMV_USEFUL").sum()) * FLOP_PER_SHAPED16_TERM
        elif args.workload == "dim4" and os.environ.get("RYD_DIM4_PROP", "1") != "0":
            kernel = "lindblad4_prop_kernel"           # NMV_USEFUL / NMV_EXEC: terms per triangle / 6-vector column
            nseg = 2
            flops = (float(res.col("NMV_USEFUL").sum()) * (15 * FLOP_PER_D4_APPLY + 6 * FLOP_PER_D4_VEC_TERM)
                     + float(res.col("NSQUARE").sum()) * FLOP_PER_D4_SQUARING
                     + n * nseg * FLOP_PER_D4_SEGMENT)
        else:
            if args.workload == "shaped":
                kernel = "lindblad_cheb_kernel"            # RYD_SHAPED16=0
            per = {"shaped": FLOP_PER_MATVEC, "dim4": FLOP_PER_DIM4_TERM, "ket_cheb": FLOP_PER_KET_TERM}[args.workload]
            flops = res.matvec_useful * per
        useful_exec = (res.matvec_exec / max(res.matvec_useful, 1.0)
                       if kernel != "lindblad4_prop_kernel" else None)
    achieved_tf = flops / (k_ms * 1e-3) / 1e12
    achieved_gbs = bpp * n / (k_ms * 1e-3) / 1e9
    tr = _measured_traffic(args.workload, "aux", n, kernel)
    out = {
        "metric": f"{args.workload}: param-points/sec of {kernel} (secondary line, not the headline metric)",
        "value": n * ws * args.steps / dt_max, "unit": "points/s", "n_gpus": ws, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": desc, "points_per_gpu": n, "global_points": n * ws,
                   "parallelism": f"range-shard x{ws}", "placement": _placement(ws, local, dev)},
        "roofline": {"bound": "fp64", "achieved": achieved_tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": achieved_tf / FP64_PEAK_TFLOPS, "traffic": tr["bytes_per_launch"] if tr else None,
                     "kernel": kernel, "kernel_ms": k_ms, "flops_per_launch": flops,
                     "flops_per_point": flops / n, "exec_over_useful": useful_exec},
        "roofline_hbm": {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved_gbs / HBM_PEAK_GBS, "bytes_per_launch": bpp * n},
    }
    if rank == 0:
        print(json.dumps(out), flush=True)
    db.free()
    eng.close()
    if pg is not None:
        pg.destroy_process_group()


# RG/cz_gate_optimization_demo.ipynb cell 10: noise-free, spacing optimised in (2.0, 5.5);
# the notebook printed "Evaluations: 2974, Runtime: 24.2 s, Cache hits: 149" for LP
# (:825-827; 2825 simulations -> 117 sims/s) and 7297 / 1359.3 s / 9 for smooth JP (:966-968)
OPT_PUBLISHED = {"opt_lp": dict(protocol="lp", maxiter=80, popsize=15, evaluations=2974, runtime_s=24.2,
                                cache_hits=149, lines="RG/cz_gate_optimization_demo.ipynb:825-827"),
                 "opt_smooth": dict(protocol="smooth_jp", maxiter=80, popsize=15, evaluations=7297,
                                    runtime_s=1359.3, cache_hits=9,
                                    lines="RG/cz_gate_optimization_demo.ipynb:966-968")}


def run_opt(args, ws, rank, local, pg):
    """The reference's published optimiser workloads: optimize_cz_gate at the demo
    notebook's settings through the batched drop-in (one engine pass per DE generation),
    wall clock of the whole run, against the notebook's printed evaluations/s."""
    import importlib
    import warnings
    OC = importlib.import_module("noisyquantumsimulator_amd.optimize_cz_gate")
    from noisyquantumsimulator_amd import simulation as SIM
    pub = OPT_PUBLISHED[args.workload]
    stats = dict(kernel_ms=0.0, calls=0, points=0, derive_ms=0.0, engine_ms=0.0, epilogue_ms=0.0)

    def evaluator(si, n, include_noise, overrides, **app):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            br = SIM.simulate_CZ_gate_batch(si, n, include_noise=include_noise, overrides=overrides, **app)
        stats["kernel_ms"] += br.kernel_ms
        stats["calls"] += 1
        stats["points"] += n
        for k in ("derive_ms", "engine_ms", "epilogue_ms"):
            stats[k] += br.timings[k]
        m = OC.extract_metrics_batch(br)
        m["_batch"] = br.batch
        return m, br.ok

    a = OC.ApparatusConstraints()
    kw = dict(include_noise=False, optimize_spacing=True, spacing_bounds=(2.0, 5.5), maxiter=pub["maxiter"],
              popsize=pub["popsize"], verbose=False, evaluator=evaluator)
    OC.optimize_cz_gate(pub["protocol"], a, cache=OC.SimulationCache(), **dict(kw, maxiter=2))   # warm-up
    for k in stats:
        stats[k] = 0 if isinstance(stats[k], int) else 0.0
    t0 = time.perf_counter()
    r = OC.optimize_cz_gate(pub["protocol"], a, cache=OC.SimulationCache(), **kw)
    dt = time.perf_counter() - t0
    sims = r.n_evaluations - r.cache_hits
    ref_sims_s = (pub["evaluations"] - pub["cache_hits"]) / pub["runtime_s"]
    out = {
        "metric": f"{args.workload}: optimize_cz_gate simulations/s (the reference's published timing)",
        "value": sims / dt, "unit": "simulations/s", "n_gpus": 1, "steps": 1, "warmup": 1,
        "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "none",
        "vs_baseline": (sims / dt) / ref_sims_s, "dtype": "f64", "data": "synthetic",
        "config": {"workload": (f"optimize_cz_gate('{pub['protocol']}', ApparatusConstraints() medium, "
                                f"include_noise=False, optimize_spacing=True, spacing_bounds=(2.0, 5.5), "
                                f"maxiter={pub['maxiter']}, popsize={pub['popsize']}) -- demo notebook cell 10"),
                   "evaluations": r.n_evaluations, "cache_hits": r.cache_hits, "simulations": sims,
                   "engine_batches": r.n_batches, "best_avg_fidelity": r.best_metrics.get("avg_fidelity"),
                   "published": dict(pub, sims_per_s=ref_sims_s, hardware="the author's laptop (QuTiP, CPU)"),
                   "vs_baseline_note": "value / published sims/s (different hardware: a CPU laptop)",
                   "host_ms": {k: round(v, 3) for k, v in stats.items() if k.endswith("_ms")},
                   "ket_kernel_ms_total": stats["kernel_ms"], "engine_calls": stats["calls"]},
    }
    if rank == 0:
        print(json.dumps(out), flush=True)
    if pg is not None:
        pg.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (isolated launches, host-buffer path, "
                         "end to end, pipelined, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/<name>.npy (float64, at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-sample", type=int, default=1024)
    ap.add_argument("--method", default="chebyshev",
                    choices=["chebyshev", "cheb_squaring", "cheb_vector"])
    ap.add_argument("--workload", default="c2",
                    choices=["c1", "c2", "c3", "c4", "c5", *AUX, *OPT_PUBLISHED])
    ap.add_argument("--n-traj", type=int, default=256, help="C5 trajectories per point")
    ap.add_argument("--c5-shards", type=int, default=0,
                    help="C5: time rank --c5-rank's shard of an N-way split on this one GPU (0: off)")
    ap.add_argument("--c5-rank", type=int, default=0)
    ap.add_argument("--c5-kernel", default="auto", choices=["auto", "rows", "lanes"],
                    help="C5 exact-mode kernel: rows (traj3p + traj3r, 16-lane DPP rows), lanes (traj3e)")
    ap.add_argument("--c4-shards", type=int, default=0,
                    help="C4: time rank --c4-rank's shard of an N-way split on this one GPU (0: off)")
    ap.add_argument("--c4-rank", type=int, default=0)
    ap.add_argument("--c5-order", default="omega", choices=["omega", "blocked", "balanced", "strided"],
                    help="C5 grid point order (sweeps.blockade_grid_3atom); strided: the Omega-major "
                         "grid split over the ranks by point index mod N (sweeps.c5_strided_shard)")
    ap.add_argument("--ladder", type=int, default=-1,
                    help="C5 ladder levels (0: exact jump times; -1: trajectories.DEFAULT_LADDER)")
    ap.add_argument("--stub", action="store_true", help=argparse.SUPPRESS)   # launcher test: no GPU
    args = ap.parse_args()
    if args.dump_outputs and args.workload in ("c1", *OPT_PUBLISHED):
        ap.error(f"--dump-outputs: the {args.workload} line times whole calls, not a resident batch")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no torchrun around us: start the N ranks ourselves (before any GPU call)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    ws, rank, local, pg = _dist()
    if args.stub:
        return run_stub(ws, rank, local, pg)
    if args.workload == "c5":
        return run_c5(args, ws, rank, local, pg)
    if args.workload == "c1":
        return run_c1(args, ws, rank, local, pg)
    if args.workload in AUX:
        return run_aux(args, ws, rank, local, pg)
    if args.workload in OPT_PUBLISHED:
        return run_opt(args, ws, rank, local, pg)
    from noisyquantumsimulator_amd import engine as E
    from noisyquantumsimulator_amd import sweeps as SW

    if args.workload == "c2":
        # this rank's contiguous shard of the global N x 10k sweep (Delta/Omega partitioned)
        batch = SW.c2_rank_shard(rank, ws, N_DELTA, N_OMEGA)
        protocol, n_steps, n_seg = "lp_square", None, 2
        workload = ("C2: 10k-point (Omega, Delta) LP-square CZ sweep per GPU, medium apparatus, "
                    "full reference noise model (8 Lindblad channels)")
    elif args.workload == "c3":
        batch = SW.c3_rank_shard(rank, ws)
        protocol, n_steps, n_seg = "smooth_jp", 300, 300
        workload = ("C3: 100k-point (Omega, Omega*tau) smooth-JP Pareto sweep per GPU, 300 "
                    "reference segments, medium apparatus, 4 collapse ops (sqrt(gamma_r)|1><r| and "
                    "sqrt(gamma_phi) P_r per atom, gamma_r = 1/140 us, gamma_phi = 2pi x 10 kHz)")
    else:
        # with --c4-shards: one rank's shard of an N-way split on this one GPU (the 1-GPU
        # strong-scaling proxy, as --c5-shards)
        t_host_derive = time.perf_counter()
        batch = (SW.c4_rank_shard(args.c4_rank, args.c4_shards) if args.c4_shards
                 else SW.c4_rank_shard(rank, ws))
        t_host_derive = time.perf_counter() - t_host_derive
        protocol, n_steps, n_seg = "lp_square", None, 2
        workload = ("C4: 1M-point species {Rb87, Cs133} x T logspace(1-100 uK, 1000) x P_tweezer "
                    "logspace(1-100 mW, 500) LP-square grid, range-sharded over the ranks, "
                    "medium apparatus, full reference noise model")
    params = SW.c3_four_op_params(batch) if args.workload == "c3" else E.pack_params(batch)
    n = batch.n
    dev = _rank_device(local)
    eng = E.Engine(devices=[dev])
    db = E.DeviceBatch(eng, params, protocol, "lindblad", n_steps=n_steps, method=args.method)

    for _ in range(args.warmup):
        db.launch()
    db.synchronize()
    _barrier(pg)
    db.synchronize()
    t0 = time.perf_counter()
    db.mark(0)
    for _ in range(args.steps):
        db.launch()
    db.mark(1)
    db.synchronize()
    _barrier(pg)
    dt = time.perf_counter() - t0
    dt_max = _max_over_ranks(pg, dt)
    # the dominant kernel's average launch duration: HIP events on its stream over the
    # timed region (back-to-back launches; the only work on that stream)
    k_ms = db.mark_elapsed() / args.steps

    res = db.fetch()
    assert np.all(res.status == 0), "engine reported per-point failures"
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, ws, n, {"state": (res.state, 1, 4), "summary": (res.summary, 1, 1),
                                                      "status": (res.status, 0, 1)})
    # --full: one launch at a time, events around each (includes event/sync overhead)
    k_iso = (float(np.mean([db.launch(timed=True) for _ in range(max(3, min(args.steps, 10)))]))
             if args.full else None)
    # algorithmic bytes per launch: 15 param columns read, 25x4 state + 19 summary doubles
    # + 1 status word written per point
    bytes_per_point = 8 * 15 + 8 * 100 + 8 * 19 + 4
    achieved_gbs = bytes_per_point * n / (k_ms * 1e-3) / 1e9
    nsq = float(res.col("NSQUARE").sum())
    prop_kernel = args.method in ("cheb_squaring", "chebyshev")   # both workloads: auto -> prop
    sq_flops = FLOP_PER_SQUARING_SYM if E.symmetric_atoms(params) else FLOP_PER_SQUARING
    mv_flops = FLOP_PER_MATVEC_SYM if E.symmetric_atoms(params) else FLOP_PER_MATVEC
    flops = res.matvec_useful * mv_flops + nsq * sq_flops
    sym16 = (args.method == "chebyshev" and E.symmetric_atoms(params)
             and os.environ.get("RYD_SYM16", "1") != "0")
    if sym16:
        # LP square leaves the last min(s, K) squaring levels to the states: per point
        # s - min(s, K) squarings and 2^min(s, K) state updates per segment (one build)
        sd = res.col("NSQUARE")
        rep = np.minimum(sd, eng.lib.ryd_lp_unsquared()) if protocol == "lp_square" else np.zeros(n)
        flops = (res.matvec_useful * FLOP_PER_MATVEC_SYM16 + float((sd - rep).sum()) * sq_flops
                 + n_seg * float(np.exp2(rep).sum()) * FLOP_PER_STATE_UPDATE_SYM16)
    elif prop_kernel:
        upd = FLOP_PER_STATE_UPDATE_SYM if E.symmetric_atoms(params) else FLOP_PER_STATE_UPDATE
        flops += n_seg * n * upd                         # R <- U R once per reference segment
    achieved_tf = flops / (k_ms * 1e-3) / 1e12
    if sym16:
        dom_kernel = "lindblad_sym16_kernel"
    elif args.workload == "c3" and prop_kernel:
        dom_kernel = "jp_frame_kernel"
    else:
        dom_kernel = "lindblad_prop_kernel" if prop_kernel else "lindblad_cheb_kernel"
    tr = _measured_traffic(args.workload, args.method, n, dom_kernel)
    traffic = tr["bytes_per_launch"] if tr else None

    host_path = out_e2e = pipelined = None
    if args.full:
        host_path = host_path_c(eng, params, protocol, n_steps, args, n)
    if args.full and args.workload == "c2" and ws == 1:
        out_e2e = end_to_end_c2()
        pipelined = pipelined_c2(params, protocol, n_steps, args, dev, n)
    if args.full and args.workload == "c4":
        out_e2e = end_to_end_c4(args, eng, params, t_host_derive)
    strong = args.workload == "c4"
    proxy = strong and args.c4_shards > 0
    global_points = n if proxy else (SW.C4_POINTS if strong else n * ws)
    total_points = global_points * args.steps
    value = total_points / dt_max
    out = {
        "metric": "Lindblad param-points/sec (2-atom Rydberg CZ sweep); achieved HBM GB/s vs peak",
        "value": value, "unit": "points/s", "n_gpus": ws, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt_max / args.steps * 1e3,
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": workload, "points_per_gpu": n, "global_points": global_points,
                   "parallelism": f"range-shard x{ws}", "placement": _placement(ws, local, dev),
                   "shard": (f"rank {args.c4_rank} of {args.c4_shards} (1-GPU strong-scaling proxy: value "
                             f"counts this shard's points only)" if proxy else None),
                   "method": args.method + ((" (auto: 16-lane DPP-row propagator kernel, phase frame)"
                                             if sym16 else " (auto: propagator kernel, phase frame)")
                                            if args.method == "chebyshev" else "")},
        # The binding roof is FP64 arithmetic (MI355X dense FP64: 78.6 TF, the same for the
        # matrix cores and the VALU; these kernels run on the FP64 VALU); the HBM view is
        # kept beside it: the kernel moves ~1 kB per point against ~1 MFLOP.
        "roofline": {"bound": "fp64", "achieved": achieved_tf, "peak": FP64_PEAK_TFLOPS,
                     "unit": "TFLOP/s", "frac": achieved_tf / FP64_PEAK_TFLOPS,
                     "traffic": traffic, "kernel": dom_kernel, "kernel_ms": k_ms, "kernel_ms_isolated": k_iso,
                     "flops_per_launch": flops,
                     "exec_over_useful": res.matvec_exec / max(res.matvec_useful, 1)},
        "host_path": host_path,
        "end_to_end": out_e2e,
        "pipelined": pipelined,
        "roofline_hbm": {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved_gbs / HBM_PEAK_GBS, "traffic": traffic,
                         "bytes_per_launch": bytes_per_point * n},
    }
    if rank == 0 and ws == 1 and args.full and not args.no_cpu_baseline:
        procs = cpu_procs()
        # C3 points cost ~6 core-seconds each on the CPU path: a smaller sample
        sample = args.cpu_sample if args.workload != "c3" else min(args.cpu_sample, 32)
        out["cpu_baseline"] = cpu_baseline(sample, procs, args.workload)
    if rank == 0:
        print(json.dumps(out), flush=True)
    db.free()
    eng.close()
    if pg is not None:
        pg.destroy_process_group()


if __name__ == "__main__":
    main()
