"""Test batches for the schedule coherence path (ryd_run_schedule_coherences) and their CPU
oracle: the full 16 x 16 qubit map of every point.

The batches of tests/sched_points.py are taken unchanged; two more walk the memo of
coherence_sched_kernel: ``aba`` (a key that returns to an earlier value) and ``step16`` (one
change of key, on the first segment of the second chunk of 16).

The oracle is composed from oracle.lindblad_oracle alone.  Per segment of positive length:
``expm(liouvillian(two_atom_hamiltonian(...), c_ops_of(...)) x / Omega)``; the 16 qubit matrix
units are chained through the segments and projected on QUBIT_INDEX, as ``process_map`` does,
S[4c+d, 4a+b] = <c| E(|a><b|) |d>.  All batches take ~10 s on one core, so the GPU tests read
the maps from tests/golden/sched_maps.npz (written by ``python -m tests.sched_coh_points``) and
tests/test_sched_coh_points_cpu.py recomputes every map and compares it with the file.
"""
from __future__ import annotations

import os
from functools import lru_cache
from typing import Dict

import numpy as np
import scipy.linalg as sla

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import pulse_schedules as PS
from oracle import lindblad_oracle as O
from tests import sched_points as SP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sched_maps.npz")
OWN = ("aba", "step16")
NAMES = SP.NAMES + OWN
X_CAP = 2.0e6                                    # csrc/ryd_engine.hip: the build argument's cap
QI = O.QUBIT_INDEX


def _aba_batch() -> Dict:
    """5 points, 6 segments whose amplitudes go A, B, A, B, A, A (random phases; duration and
    detuning constant per point): five builds, three of them of a key seen before."""
    rng = np.random.default_rng(20261021)
    n, ns = 5, 6
    p = SP.random_params(rng, n)
    A, B = rng.uniform(0.6, 1.2, (n, 1)), rng.uniform(0.2, 0.5, (n, 1))
    amp = np.where(np.array([1, 0, 1, 0, 1, 1], bool)[None], A, B)
    s = PS.assemble(np.full((n, ns), 0.4), amp, rng.uniform(-np.pi, np.pi, (n, ns)),
                    rng.uniform(-0.3, 0.3, (n, 1)) + np.zeros((n, ns)))
    return dict(params=p, sched=s)


def _step16_batch() -> Dict:
    """4 points, 33 segments whose amplitude changes once, at segment 16: the second build is
    asked for by the first segment of the second chunk."""
    rng = np.random.default_rng(20261022)
    n, ns = 4, 33
    p = SP.random_params(rng, n)
    a0, a1 = rng.uniform(0.8, 1.2, (n, 1)), rng.uniform(0.3, 0.7, (n, 1))
    amp = np.where(np.arange(ns)[None] < 16, a0, a1)
    s = PS.assemble(np.full((n, ns), 0.3), amp, rng.uniform(-np.pi, np.pi, (n, ns)),
                    rng.uniform(-0.1, 0.1, (n, 1)) + np.zeros((n, ns)))
    return dict(params=p, sched=s)


@lru_cache(maxsize=None)
def batch(name: str) -> Dict:
    if name == "aba":
        return _aba_batch()
    if name == "step16":
        return _step16_batch()
    return SP.batch(name)


def oracle_maps(p: np.ndarray, sched: np.ndarray) -> np.ndarray:
    """S[n, 16, 16] of the schedule(s) ``sched`` ((4, n_seg) or (n, 4, n_seg)) on ``p``."""
    n, D = p.shape[1], 9
    units = np.zeros((D * D, 16), complex)       # column 4a+b: vec(|a><b|), column-stacked
    for a in range(4):
        for b in range(4):
            units[QI[a] + D * QI[b], 4 * a + b] = 1.0
    rows = [QI[c] + D * QI[d] for c in range(4) for d in range(4)]
    out = np.zeros((n, 16, 16), complex)
    for i in range(n):
        tab = sched if sched.ndim == 2 else sched[i]
        Om, V, d1 = p[N.P["OMEGA"], i], p[N.P["V"], i], p[N.P["DELTA1"], i]
        c_ops = SP.c_ops_of(p, i)
        v = units.copy()
        for x, a, ph, d in tab.T:
            if x == 0.0:
                continue
            H = O.two_atom_hamiltonian(a * Om * np.exp(1j * ph), d * Om, V, 3, delta_zeeman=d1)
            v = sla.expm(O.liouvillian(H, c_ops) * (x / Om)) @ v
        out[i] = v[rows]
    return out


@lru_cache(maxsize=None)
def golden(name: str) -> np.ndarray:
    """The recorded oracle maps of batch ``name``: S[n, 16, 16]."""
    with np.load(GOLDEN) as f:
        return f[name]


def diagonal_block(S: np.ndarray) -> np.ndarray:
    """rho[n, 4, 4, 4] on the qubit block for the 4 basis inputs |a><a|, from the maps."""
    return np.stack([S[:, :, 5 * a].reshape(-1, 4, 4) for a in range(4)], axis=1)


def build_argument(p: np.ndarray, i: int, a: float, d: float, x: float, with_v: bool = True) -> float:
    """The argument coherence_sched_kernel's build of the key (a Omega, d Omega, x / Omega) is
    scaled by on point i: (Gershgorin width of the two-atom H + the eight rates) dt, as
    tests/coh_points.py's bounds; ``with_v`` False is the (-1,+1) bank's, which leaves V out."""
    Om, V, d1 = p[N.P["OMEGA"], i], p[N.P["V"], i] if with_v else 0.0, p[N.P["DELTA1"], i]
    w, e = 0.5 * a * Om, (0.0, d1, -d * Om)
    lo, hi = [], []
    for a1 in range(3):
        for a2 in range(a1, 3):
            E = e[a1] + e[a2] + (V if a1 == a2 == 2 else 0.0)
            r = w * ((a1 > 0) + (a2 > 0))
            lo.append(E - r)
            hi.append(E + r)
    rates = sum(abs(p[N.P[k + s], i]) for k in ("G1", "G0", "GPHI", "GSC") for s in ("_A", "_B"))
    return ((max(hi) - min(lo)) + rates) * x / Om


def capped_segment(p: np.ndarray, i: int, a: float = 1.0, d: float = 0.0) -> float:
    """x of a segment whose build argument on point i is 3e6 > X_CAP (the construction of
    tests/coh_points.py's capped row: tau = 3e6 / omega, here x = 3e6 Omega / omega)."""
    return 3e6 / build_argument(p, i, a, d, 1.0)


if __name__ == "__main__":
    from threadpoolctl import threadpool_limits
    threadpool_limits(1)                         # 81 x 81 matrices: threaded BLAS only thrashes (tests/conftest.py)
    np.savez_compressed(GOLDEN, **{name: oracle_maps(batch(name)["params"], batch(name)["sched"]) for name in NAMES})
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
