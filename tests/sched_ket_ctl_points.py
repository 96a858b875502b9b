"""CPU oracle of the control Jacobian of the noise-free schedule path
(ryd_run_schedule_kets_ctl): the derivatives of the two diagonal overlaps with respect to every
segment's duration, amplitude, phase and detuning, on the 9-dimensional two-atom space.

It extends ``tests.sched_ket_points.chain`` (whose kets, overlaps and phase Jacobian it keeps) from
the same oracle pieces plus ``scipy.linalg.expm_frechet``.  With H_s = H0 + a_s Ha(phi_s) +
delta_s Hd the Hamiltonian of segment s (Ha, Hd: the oracle's Hamiltonian of the drive alone and
of a detuning Omega alone, so that they are its derivatives in the table's units),
dt = x_s / Omega, b_s = U_s .. U_1 e and lambda_s^T = e^T U_N .. U_{s+1}:

    d a / d x_s     = lambda_s^T (-i H_s / Omega) b_s          (also at x_s = 0: the one-sided value)
    d a / d a_s     = lambda_s^T L(-i H_s dt, -i Ha dt) b_{s-1}
    d a / d delta_s = lambda_s^T L(-i H_s dt, -i Hd dt) b_{s-1}

L the Frechet derivative of expm.  A segment of zero duration has zeros in a, phi and delta.

The batches are those of tests/sched_points.py (by import) and two small ones of this file:
``degenerate`` (exactly and nearly degenerate blocks, eigenvalue gaps on both sides of the
kernel's sinc switch) and ``zero_x`` (zero-duration segments first, last, adjacent, at a chunk
edge, with phases of their own).
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict

import numpy as np
from scipy.linalg import expm_frechet

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import pulse_schedules as PS
from oracle import lindblad_oracle as O
from tests import sched_ket_points as KP
from tests import sched_points as SP

SC = N.SC
NEW = ("degenerate", "zero_x")
SINC_SWITCH = 1e-3          # the kernel's |(lambda_k - lambda_l) dt / 2| below which sinc is a series


def hamiltonian_parts(p: np.ndarray, i: int, ph: float):
    """(H0, Ha, Hd) of point i at laser phase ph: H = H0 + a Ha + delta Hd."""
    Om, V, d1 = p[N.P["OMEGA"], i], p[N.P["V"], i], p[N.P["DELTA1"], i]
    H0 = O.two_atom_hamiltonian(0.0, 0.0, V, 3, delta_zeeman=d1)
    Ha = O.two_atom_hamiltonian(Om * np.exp(1j * ph), 0.0, 0.0, 3, delta_zeeman=0.0)
    Hd = O.two_atom_hamiltonian(0.0, Om, 0.0, 3, delta_zeeman=0.0)
    return H0, Ha, Hd


def chain(p: np.ndarray, sched: np.ndarray) -> Dict[str, np.ndarray]:
    """``tests.sched_ket_points.chain`` plus ``C`` (n, 4, 2, n_seg): d a01 and d a11 with respect
    to x_s, a_s, phi_s, delta_s (first index ``_native.SC``)."""
    out = KP.chain(p, sched)
    n, n_seg = p.shape[1], sched.shape[-1]
    C = np.zeros((n, N.SC_NFIELD, 2, n_seg), complex)
    C[:, SC["PHASE"]] = out["J"]
    eye = np.eye(9, dtype=complex)
    for i in range(n):
        tab = sched if sched.ndim == 2 else sched[i]
        Om = p[N.P["OMEGA"], i]
        Us = KP.segment_unitaries(p, i, tab)
        Hs, dUa, dUd = [], [], []
        for s, (x, a, ph, d) in enumerate(tab.T):
            H0, Ha, Hd = hamiltonian_parts(p, i, ph)
            H = H0 + a * Ha + d * Hd
            Hs.append(H)
            if x == 0.0:
                dUa.append(None)
                dUd.append(None)
                continue
            dt = x / Om
            dUa.append(expm_frechet(-1j * H * dt, -1j * Ha * dt, compute_expm=False))
            dUd.append(expm_frechet(-1j * H * dt, -1j * Hd * dt, compute_expm=False))
        for c, e in enumerate((KP.IN01, KP.IN11)):
            b = [eye[e]]
            for U in Us:
                b.append(b[-1] if U is None else U @ b[-1])
            lam = eye[e]
            for s in range(n_seg - 1, -1, -1):
                C[i, SC["X"], c, s] = lam @ (-1j * Hs[s] / Om) @ b[s + 1]
                if Us[s] is None:
                    continue
                C[i, SC["AMP"], c, s] = lam @ dUa[s] @ b[s]
                C[i, SC["DELTA"], c, s] = lam @ dUd[s] @ b[s]
                lam = Us[s].T @ lam
    out["C"] = C
    return out


def _degenerate_batch() -> Dict:
    """17 segments per point; per point, among ordinary segments:
    a = 0 with delta = -d1 / Omega (the 2 x 2 block fully degenerate), a = 0 with
    delta = -d1 / Omega again gives 2 d1 = d1 - Delta (the 3 x 3 block's degenerate pair: the same
    condition), a = 1e-9 at that detuning (a gap of 1e-9 Omega), and four segments whose 2 x 2
    gap times dt / 2 is 0.5, 0.999, 1.001 and 2 times the sinc switch."""
    rng = np.random.default_rng(7101)
    n, ns = 5, 17
    p = SP.random_params(rng, n)
    Om, d1 = p[N.P["OMEGA"]], p[N.P["DELTA1"]]
    s = PS.assemble(rng.uniform(0.2, 1.5, (n, ns)), rng.uniform(0.3, 1.2, (n, ns)),
                    -rng.uniform(-np.pi, np.pi, (n, ns)), rng.uniform(-0.5, 0.5, (n, ns)))
    dres = -d1 / Om                                # d1 + Delta = 0
    for i in range(n):
        s[i, SC["AMP"], 1], s[i, SC["DELTA"], 1] = 0.0, dres[i]
        s[i, SC["AMP"], 5], s[i, SC["DELTA"], 5] = 0.0, dres[i]
        s[i, SC["X"], 5] = 2.5
        s[i, SC["AMP"], 8], s[i, SC["DELTA"], 8] = 1e-9, dres[i]
        # at resonance the 2 x 2 gap is a Omega: gap dt / 2 = a x / 2 = f SINC_SWITCH
        for seg, f in zip((10, 11, 12, 13), (0.5, 0.999, 1.001, 2.0)):
            s[i, SC["DELTA"], seg] = dres[i]
            s[i, SC["AMP"], seg] = 2.0 * f * SINC_SWITCH / s[i, SC["X"], seg]
    return dict(params=p, sched=s)


def _zero_x_batch() -> Dict:
    """17 segments per point, every field different from segment to segment, with zero-duration
    segments first, last, adjacent (6, 7), on both sides of the chunk edge (15, 16)."""
    rng = np.random.default_rng(7102)
    n, ns = 5, 17
    p = SP.random_params(rng, n)
    s = PS.assemble(rng.uniform(0.2, 1.5, (n, ns)), rng.uniform(0.3, 1.2, (n, ns)),
                    -rng.uniform(-np.pi, np.pi, (n, ns)), rng.uniform(-0.5, 0.5, (n, ns)))
    zeros = ([0], [16], [6, 7], [15], [0, 6, 7, 15, 16])
    for i in range(n):
        s[i, SC["X"], zeros[i]] = 0.0
    return dict(params=p, sched=s)


@lru_cache(maxsize=None)
def batch(name: str) -> Dict:
    if name == "degenerate":
        return _degenerate_batch()
    if name == "zero_x":
        return _zero_x_batch()
    return SP.batch(name)


NAMES = SP.NAMES + NEW


@lru_cache(maxsize=None)
def reference(name: str) -> Dict[str, np.ndarray]:
    """The chain of batch ``name``, computed once per process; the arrays are read-only."""
    b = batch(name)
    out = chain(b["params"], b["sched"])
    for v in out.values():
        v.setflags(write=False)
    return out
