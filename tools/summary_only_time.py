"""Summary-only runs against full runs, in one process: `storing` (a state buffer is passed),
`store_free` (NULL state pointer: the descriptor's store-free kernel where the library has one,
the scratch-buffer path otherwise) and `scratch` (NULL state pointer under RYD_NOSTATE=0: the
storing kernel into a pool buffer), for

  c2_lindblad   the C2 (Omega, Delta) grid, LP square, Lindblad (sym16, balanced form)
  c2_ket        the same grid noise-free, as kets (ket_block_kernel)
  c2_shaped     the grid with the cosine envelope at n_steps = 500 (shaped16; no store-free
                kernel in the library: profiles/summary_only/README.md)
  c2_dim4       the grid derived with hilbert_space_dim = 4 (lindblad4_prop_kernel; none either)

and, end to end,

  host_call     Engine.run on C2 with states True / False: wall time, d2h_ms, D2H bytes
  c4_shard      DeviceSweep on rank 0's 125k-point shard of C4 with states True / False:
                derive + engine (device time between two marks), then the D2H of summary and
                status (and, with states, of the state rows), with the bytes of each.

Per setting 3 warm-up launches, then median, min and max of 20 timed ones (HIP events around
the launch, inputs resident in HBM); the settings are cycled through three times.  A store-free
kernel "wins" a round when its median lies below the storing kernel's min-max range of that
round.  Prints one JSON line.

    python tools/summary_only_time.py
"""
import argparse
import contextlib
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
from noisyquantumsimulator_amd import sweeps as SW

WARMUP, TIMED, ROUNDS = 3, 20, 3


@contextlib.contextmanager
def nostate_env(value):
    old = os.environ.pop("RYD_NOSTATE", None)
    if value is not None:
        os.environ["RYD_NOSTATE"] = value
    try:
        yield
    finally:
        os.environ.pop("RYD_NOSTATE", None)
        if old is not None:
            os.environ["RYD_NOSTATE"] = old


def stats(ts, unit="ms"):
    return {f"median_{unit}": round(float(np.median(ts)), 5), f"min_{unit}": round(float(min(ts)), 5),
            f"max_{unit}": round(float(max(ts)), 5)}


def kernel_case(eng, params, protocol, evolution, **desc):
    """One round of the three variants on one batch; returns {variant: stats} and checks that
    the three summaries and status words are the same bits."""
    out, ref = {}, None
    for variant, states, env in (("storing", True, None), ("store_free", False, None), ("scratch", False, "0")):
        db = E.DeviceBatch(eng, params, protocol, evolution, states=states, **desc)
        try:
            with nostate_env(env):
                for _ in range(WARMUP):
                    db.launch()
                db.synchronize()
                ts = [db.launch(timed=True) for _ in range(TIMED)]
            r = db.fetch()
        finally:
            db.free()
        if np.any(r.status & N.STATUS_FAIL_MASK):
            raise SystemExit(f"{protocol}/{evolution} {variant}: the engine reported per-point failures")
        if ref is None:
            ref = r
        elif not (np.array_equal(r.summary.view(np.uint64), ref.summary.view(np.uint64)) and
                  np.array_equal(r.status, ref.status)):
            raise SystemExit(f"{protocol}/{evolution} {variant}: summary or status differs from the storing kernel")
        out[variant] = stats(ts)
    out["store_free_wins"] = out["store_free"]["median_ms"] < out["storing"]["min_ms"]
    return out


def host_call(eng, params):
    out = {}
    n = params.shape[1]
    for states in (True, False):
        for _ in range(WARMUP):
            eng.run(params, "lp_square", "lindblad", states=states)
        wall, d2h, kern = [], [], []
        for _ in range(TIMED):
            t0 = time.perf_counter()
            r = eng.run(params, "lp_square", "lindblad", states=states)
            wall.append((time.perf_counter() - t0) * 1e3)
            d2h.append(r.d2h_ms)
            kern.append(r.kernel_ms)
        nbytes = 8 * N.NSUMMARY * n + 4 * n + (8 * 25 * 4 * n if states else 0)
        out["states" if states else "summary_only"] = dict(
            d2h_bytes=nbytes, wall=stats(wall), d2h=stats(d2h), kernel=stats(kern))
    return out


def c4_shard(eng, inp):
    out = {}
    lib, h = eng.lib, eng.handle
    for states in (True, False):
        sw = E.DeviceSweep(eng, inp, states=states)
        try:
            n = sw.n
            summ = np.zeros((N.NSUMMARY, n))
            status = np.zeros(n, dtype=np.uint32)
            state = np.zeros((sw.width, 4 * n)) if states else None
            for _ in range(WARMUP):
                sw.launch()
            sw.synchronize()
            dev, d2h, d2h_state = [], [], []
            for _ in range(TIMED):
                sw.mark(0)
                sw.launch()
                sw.mark(1)
                dev.append(sw.mark_elapsed())
                t0 = time.perf_counter()
                N.check(lib.ryd_memcpy_d2h(h, sw.slot, summ.ctypes.data, sw.d_summary, summ.nbytes))
                N.check(lib.ryd_memcpy_d2h(h, sw.slot, status.ctypes.data, sw.d_status, status.nbytes))
                d2h.append((time.perf_counter() - t0) * 1e3)
                if states:
                    t0 = time.perf_counter()
                    N.check(lib.ryd_memcpy_d2h(h, sw.slot, state.ctypes.data, sw.d_state, state.nbytes))
                    d2h_state.append((time.perf_counter() - t0) * 1e3)
            if np.any(status & N.STATUS_FAIL_MASK):
                raise SystemExit("C4 shard: the engine reported per-point failures")
            rec = dict(points=n, state_alloc_bytes=8 * sw.width * 4 * n if states else 0,
                       derive_engine=stats(dev), d2h_summary_status_bytes=summ.nbytes + status.nbytes,
                       d2h_summary_status=stats(d2h))
            if states:
                rec.update(d2h_state_bytes=state.nbytes, d2h_state=stats(d2h_state))
            out["states" if states else "summary_only"] = rec
        finally:
            sw.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-omega", type=int, default=100)
    ap.add_argument("--n-delta", type=int, default=100)
    ap.add_argument("--c4-ranks", type=int, default=8, help="the C4 shard is rank 0 of this many")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    eng = E.Engine()
    g = lambda **kw: E.pack_params(SW.omega_delta_grid(args.n_omega, args.n_delta, **kw))
    cases = {
        "c2_lindblad": (g(), "lp_square", "lindblad", {}),
        "c2_ket": (g(include_noise=False), "lp_square", "ket", {}),
        "c2_shaped": (g(pulse_shape="cosine"), "lp_shaped", "lindblad", dict(shape="cosine", n_steps=500)),
        "c2_dim4": (g(hilbert_space_dim=4), "lp_square", "lindblad", dict(dim=4)),
    }
    c4 = SW.c4_rank_inputs(0, args.c4_ranks)
    rounds = []
    for _ in range(ROUNDS):
        rec = {name: kernel_case(eng, p, proto, evol, **desc) for name, (p, proto, evol, desc) in cases.items()}
        rec["host_call"] = host_call(eng, cases["c2_lindblad"][0])
        rec["c4_shard"] = c4_shard(eng, c4)
        rounds.append(rec)
    keep = {name: all(r[name]["store_free_wins"] for r in rounds) for name in cases}
    print(json.dumps({"tool": "summary_only_time", "grid": "C2 omega_delta_grid",
                      "points": int(cases["c2_lindblad"][0].shape[1]), "warmup": WARMUP, "timed": TIMED,
                      "rounds": rounds, "store_free_wins_every_round": keep}))


if __name__ == "__main__":
    main()
