"""Test batches for the pulse-schedule path (ryd_run_schedule) and their CPU oracle.

The oracle side is composed from oracle.lindblad_oracle only: ``two_atom_hamiltonian`` and
``collapse_operators`` per segment, ``evolve_state(method="expm")`` chained over the segments
from ``initial_kets``.  A chain costs ~4 ms per (segment, input) on one core, a minute for all
the batches below, so the GPU tests read the chains' results from tests/golden/sched_oracle.npz
(written by ``python -m tests.sched_points``) and tests/test_sched_points_cpu.py recomputes
every chain and compares it with the file.

Every batch is a dict: ``params`` (NPARAM, n) with equal atom-A and atom-B rates, ``sched``
(n, 4, n_seg) per-point tables, and for the protocol batches ``protocol`` / ``n_steps``, the
``Engine.run`` call the table restates (``params`` carries that protocol's columns too).
"""
from __future__ import annotations

import os
from functools import lru_cache
from typing import Dict

import numpy as np

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import pulse_schedules as PS
from oracle import lindblad_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sched_oracle.npz")
CHUNK_NSEG = (1, 15, 16, 17, 32, 33)


def random_params(rng, n: int) -> np.ndarray:
    """Omega 1-10 MHz, V/Omega 10-1000 and the rate ranges of test_gpu_parity._random_points,
    the two atoms alike; G0 >= G1 so that the oracle's rate keys reproduce the channels."""
    p = np.zeros((N.NPARAM, n))
    Om = 2 * np.pi * rng.uniform(1e6, 10e6, n)
    p[N.P["OMEGA"]] = Om
    p[N.P["V"]] = Om * 10 ** rng.uniform(1, 3, n)
    p[N.P["DELTA1"]] = 2 * np.pi * rng.uniform(0, 3e5, n)
    g1 = rng.uniform(0, 2e4, n)
    rates = dict(G1=g1, G0=g1 + rng.uniform(0, 3e4, n), GPHI=rng.uniform(0, 1e5, n), GSC=rng.uniform(0, 5e5, n))
    for k, g in rates.items():
        p[N.P[k + "_A"]] = g
        p[N.P[k + "_B"]] = g
    return p


def c_ops_of(p: np.ndarray, i: int):
    """The oracle's collapse operators for the channel rates of point i: gamma_r = 2 G1 gives
    G1 on |1><r| and on |0><r| (branching 1/2), gamma_bbr the rest of G0."""
    g1, g0 = p[N.P["G1_A"], i], p[N.P["G0_A"], i]
    return O.collapse_operators(dict(gamma_r=2 * g1, gamma_bbr=g0 - g1, gamma_phi_laser=p[N.P["GPHI_A"], i],
                                     gamma_scatter_intermediate=p[N.P["GSC_A"], i]))


def oracle_chain(p: np.ndarray, sched: np.ndarray) -> np.ndarray:
    """rho[n, 4, 9, 9] of the schedule(s) ``sched`` ((4, n_seg) or (n, 4, n_seg)) on ``p``."""
    n = p.shape[1]
    out = np.zeros((n, 4, 9, 9), complex)
    for i in range(n):
        tab = sched if sched.ndim == 2 else sched[i]
        Om, V, d1 = p[N.P["OMEGA"], i], p[N.P["V"], i], p[N.P["DELTA1"], i]
        c_ops = c_ops_of(p, i)
        segs = []
        for x, a, ph, d in tab.T:
            if x == 0.0:
                continue
            H = O.two_atom_hamiltonian(a * Om * np.exp(1j * ph), d * Om, V, 3, delta_zeeman=d1)
            segs.append((H, np.array([0.0, x / Om])))
        for k, lab in enumerate(O.LABELS):
            psi = O.initial_kets()[lab]
            s = np.outer(psi, psi.conj())
            for H, t in segs:
                s = O.evolve_state(H, s, t, c_ops, method="expm")
            out[i, k] = s
    return out


def _random_batch() -> Dict:
    rng = np.random.default_rng(20261020)
    n, ns = 13, 20
    p = random_params(rng, n)
    s = PS.assemble(rng.uniform(0.05, 3.0, (n, ns)), rng.uniform(0.0, 1.2, (n, ns)),
                    -rng.uniform(-np.pi, np.pi, (n, ns)), rng.uniform(-0.5, 0.5, (n, ns)))
    for i in range(n):                           # one exact-zero x and one a = 0 gap per point
        z, g = rng.choice(ns, 2, replace=False)
        s[i, N.SC["X"], z] = 0.0
        s[i, N.SC["AMP"], g] = 0.0
    return dict(params=p, sched=s)


def _protocol_batch(protocol: str) -> Dict:
    rng = np.random.default_rng({"lp_square": 11, "bangbang": 12, "smooth_jp": 13}[protocol])
    n = 9
    p = random_params(rng, n)
    Om = p[N.P["OMEGA"]]
    if protocol == "lp_square":
        dom, ot = rng.uniform(0.3, 0.45, n), np.full(n, 4.29268)
        xi = np.exp(1j * rng.uniform(0, 2 * np.pi, n))
        p[N.P["DELTA"]], p[N.P["TAU"]] = dom * Om, ot / Om
        p[N.P["XI_RE"]], p[N.P["XI_IM"]] = xi.real, xi.imag
        return dict(params=p, sched=PS.from_lp_square(dom, ot, xi), protocol=protocol, n_steps=None,
                    dom=dom, omega_tau=ot, xi=xi)
    if protocol == "bangbang":
        st = np.sort(rng.uniform(0, 22.08, (n, 4)), axis=1)
        st[:, 1] = st[:, 0]                      # a zero-length segment
        ph = rng.uniform(-np.pi, np.pi, (n, 5))
        p[N.P["OMEGA_TAU"]], p[N.P["NSEG"]] = 22.08, 5
        p[N.P["SWT0"]:N.P["SWT0"] + 4] = st.T
        p[N.P["PHI0"]:N.P["PHI0"] + 5] = ph.T
        return dict(params=p, sched=PS.from_bangbang(st, ph, 22.08), protocol=protocol, n_steps=5,
                    switching_times=st, phases=ph, omega_tau=22.08)
    A, omr, pho, dom, ot = 0.311 * np.pi, 1.242, 4.696, -0.0205, rng.uniform(5, 12, n)
    p[N.P["DELTA"]], p[N.P["TAU"]] = dom * Om, ot / Om
    p[N.P["A"]], p[N.P["OMEGA_MOD"]], p[N.P["PHI_OFF"]] = A, omr * Om, pho
    return dict(params=p, sched=PS.from_smooth_jp(A, omr, pho, ot, dom, 300), protocol=protocol, n_steps=300,
                A=A, omega_mod_ratio=omr, phi_offset=pho, delta_over_omega=dom, omega_tau=ot)


def _chunk_batch(ns: int) -> Dict:
    rng = np.random.default_rng(3000 + ns)
    n = 5
    p = random_params(rng, n)
    s = PS.assemble(np.full((n, ns), 0.35), 1.0, -rng.uniform(-np.pi, np.pi, (n, ns)),
                    rng.uniform(-0.1, 0.1, (n, 1)) + np.zeros((n, ns)))
    return dict(params=p, sched=s)


NAN_ROW = 2


def nan_last_segment(name: str = "chunk17"):
    """Batch ``name`` with a NaN in the last segment of point NAN_ROW's table -- the segment that
    the lanes past n_seg of a partial last chunk read too -- between untouched neighbours:
    (params, sched, good), ``good`` the other points, whose oracle rows are the batch's own."""
    b = batch(name)
    s = b["sched"].copy()
    s[NAN_ROW, N.SC["DELTA"], -1] = np.nan
    return b["params"], s, [i for i in range(s.shape[0]) if i != NAN_ROW]


NAMES = ("random", "lp_square", "bangbang", "smooth_jp") + tuple(f"chunk{ns}" for ns in CHUNK_NSEG)


@lru_cache(maxsize=None)
def batch(name: str) -> Dict:
    if name == "random":
        return _random_batch()
    if name.startswith("chunk"):
        return _chunk_batch(int(name[5:]))
    return _protocol_batch(name)


@lru_cache(maxsize=None)
def golden(name: str) -> np.ndarray:
    """The recorded oracle chain of batch ``name``: rho[n, 4, 9, 9]."""
    with np.load(GOLDEN) as f:
        return f[name]


if __name__ == "__main__":
    from threadpoolctl import threadpool_limits
    threadpool_limits(1)                         # 81 x 81 matrices: threaded BLAS only thrashes (tests/conftest.py)
    np.savez_compressed(GOLDEN, **{name: oracle_chain(batch(name)["params"], batch(name)["sched"]) for name in NAMES})
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
