"""Pulse-schedule tables for ``Engine.run_schedule`` / ``PulseScheduleInputs``.

A schedule is a float64 array of shape ``(4, n_seg)`` (one table for every point) or
``(n, 4, n_seg)`` (one per point); its rows are the fields of include/ryd_engine.h
(``_native.SC``), all in units of the point's own two-photon Rabi frequency Omega:

    X      x_s     = Omega dt_s  >= 0   (duration; the convention of the bang-bang switching times)
    AMP    a_s     = Omega_s / Omega >= 0
    PHASE  phi_s   radians
    DELTA  delta_s = Delta_s / Omega, signed

so that segment s is H(Omega_s = a_s Omega e^{i phi_s}, Delta_s = delta_s Omega) for x_s / Omega.
The ``from_*`` builders restate the engine's own protocols as tables (and are tested against
the oracle's segment lists); ``from_functions`` samples any a(u), phi(u), delta(u), u = Omega t.
Scalar arguments give a shared ``(4, n_seg)`` table, arrays of length n an ``(n, 4, n_seg)`` one.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Union

import numpy as np

from ._native import S, SC, SC_NFIELD, SCHED_MAX_SEG

ArrayLike = Union[float, Sequence[float], np.ndarray]


def validate_schedule(sched: np.ndarray, n: Optional[int] = None) -> np.ndarray:
    """The table as a C-contiguous float64 array, or ValueError: shape (4, n_seg) or
    (n, 4, n_seg) with 1 <= n_seg <= 4096, every entry finite, x >= 0, a >= 0."""
    s = np.ascontiguousarray(sched, dtype=np.float64)
    if s.ndim not in (2, 3) or s.shape[-2] != SC_NFIELD:
        raise ValueError(f"a schedule has shape (4, n_seg) or (n, 4, n_seg), not {s.shape}")
    if not 1 <= s.shape[-1] <= SCHED_MAX_SEG:
        raise ValueError(f"a schedule has 1 .. {SCHED_MAX_SEG} segments, not {s.shape[-1]}")
    if s.ndim == 3 and n is not None and s.shape[0] != n:
        raise ValueError(f"a per-point schedule for {n} points has shape ({n}, 4, n_seg), not {s.shape}")
    if not np.all(np.isfinite(s)):
        raise ValueError("schedule entries must be finite")
    if np.any(s[..., SC["X"], :] < 0):
        raise ValueError("segment durations x = Omega dt must be >= 0")
    if np.any(s[..., SC["AMP"], :] < 0):
        raise ValueError("segment amplitudes a = Omega_s / Omega must be >= 0 (a sign belongs in the phase)")
    return s


def assemble(x: ArrayLike, amp: ArrayLike, phase: ArrayLike, delta: ArrayLike) -> np.ndarray:
    """Four arrays of shape (n_seg,) or (n, n_seg) (scalars broadcast) -> a table."""
    parts = [np.asarray(v, dtype=np.float64) for v in (x, amp, phase, delta)]
    shape = np.broadcast_shapes(*(p.shape for p in parts))
    if len(shape) not in (1, 2):
        raise ValueError(f"x, amp, phase, delta must have shape (n_seg,) or (n, n_seg), not {shape}")
    return np.ascontiguousarray(np.stack([np.broadcast_to(p, shape) for p in parts], axis=-2))


def _col(v: ArrayLike) -> np.ndarray:
    """A scalar stays a scalar, an array of n values becomes a column that broadcasts
    against the segment axis."""
    a = np.asarray(v, dtype=np.float64)
    if a.ndim > 1:
        raise ValueError("per-point arguments are 1-D")
    return a[..., None] if a.ndim else a


def from_lp_square(delta_over_omega: ArrayLike, omega_tau: ArrayLike, xi: Union[complex, np.ndarray]) -> np.ndarray:
    """Levine-Pichler square pulses: two segments of duration omega_tau, the second with the
    drive multiplied by xi (amplitude |xi|, phase arg xi), both at detuning delta_over_omega."""
    xi = np.asarray(xi, dtype=np.complex128)
    one = np.ones(2)
    mag = np.stack([np.ones_like(xi.real), np.abs(xi)], axis=-1)
    arg = np.stack([np.zeros_like(xi.real), np.angle(xi)], axis=-1)
    return assemble(_col(omega_tau) * one, mag, arg, _col(delta_over_omega) * one)


def from_bangbang(switching_times: ArrayLike, phases: ArrayLike, omega_tau: ArrayLike) -> np.ndarray:
    """Bang-bang: len(phases) = len(switching_times) + 1 segments between the bounds
    0, switching_times..., omega_tau (dimensionless), amplitude 1, detuning 0.  Equal bounds
    give a segment of zero length, which the engine skips."""
    st = np.asarray(switching_times, dtype=np.float64)
    ph = np.asarray(phases, dtype=np.float64)
    if ph.shape[-1] != st.shape[-1] + 1:
        raise ValueError(f"need len(phases) = len(switching_times) + 1, got {ph.shape[-1]} and {st.shape[-1]}")
    ot = np.asarray(omega_tau, dtype=np.float64)
    lead = np.broadcast_shapes(st.shape[:-1], ph.shape[:-1], ot.shape)
    st = np.broadcast_to(st, lead + st.shape[-1:])
    bounds = np.concatenate([np.zeros(lead + (1,)), st, np.broadcast_to(ot[..., None], lead + (1,))], axis=-1)
    return assemble(np.diff(bounds, axis=-1), 1.0, np.broadcast_to(ph, lead + ph.shape[-1:]), 0.0)


def from_smooth_jp(A: ArrayLike, omega_mod_ratio: ArrayLike, phi_offset: ArrayLike, omega_tau: ArrayLike,
                   delta_over_omega: ArrayLike, n_steps: int = 300) -> np.ndarray:
    """Smooth Jandura-Pupillo: n_steps equal segments, phase A cos(omega_mod t - phi_offset)
    at each segment's midpoint (omega_mod = omega_mod_ratio Omega), amplitude 1, the signed
    two-photon detuning delta_over_omega."""
    if n_steps < 1:
        raise ValueError("n_steps must be >= 1")
    ot = _col(omega_tau)
    k = np.arange(n_steps, dtype=np.float64)
    x = ot / n_steps + 0.0 * k
    # the midpoints as the evolver forms them: linspace(0, tau, n + 1)[i] + dt / 2
    mid = k * (ot / n_steps) + (ot / n_steps) / 2
    phase = _col(A) * np.cos(_col(omega_mod_ratio) * mid - _col(phi_offset))
    return assemble(x, 1.0, phase, _col(delta_over_omega) + 0.0 * k)


def from_functions(amp: Union[float, Callable], phase: Union[float, Callable], delta: Union[float, Callable],
                   omega_tau: float, n_seg: int) -> np.ndarray:
    """n_seg equal segments over u = Omega t in [0, omega_tau]; ``amp``, ``phase`` and
    ``delta`` are numbers or callables of u (arrays in, arrays out), sampled at the segment
    midpoints.  A shared (4, n_seg) table."""
    if n_seg < 1:
        raise ValueError("n_seg must be >= 1")
    du = float(omega_tau) / n_seg
    mid = (np.arange(n_seg, dtype=np.float64) + 0.5) * du

    def sample(f):
        v = f(mid) if callable(f) else f
        return np.broadcast_to(np.asarray(v, dtype=np.float64), (n_seg,))
    return validate_schedule(assemble(np.full(n_seg, du), sample(amp), sample(phase), sample(delta)))


# ---- the table as an optimiser's parameterisation: phase gradients of the noise-free gate
def overlaps(summary: np.ndarray):
    """(a01, a11), complex (n,), from the summary rows of a ket run: a01 = <01|psi_01> is input
    1 of OV_RE0 / OV_IM0, a11 = <11|psi_11> input 3."""
    re, im = S["OV_RE0"], S["OV_IM0"]
    return summary[re + 1] + 1j * summary[im + 1], summary[re + 3] + 1j * summary[im + 3]


def gate_fidelity_and_gradient(a01: np.ndarray, a11: np.ndarray, J: np.ndarray, which: str = "avg_gate"):
    """``noise_models.gate_fidelity`` of a noise-free identical-atom gate from its two diagonal
    overlaps a01 = <01|psi_01> (= <10|psi_10>) and a11 = <11|psi_11> (complex, shape (n,)), and
    its derivative with respect to every segment's phase from ``J`` (complex (n, 2, n_seg),
    ``EngineResult.phase_jacobian``: d a01 / d phi_s, d a11 / d phi_s).  ``which``: "process"
    or "avg_gate".  Returns (F (n,), dF/dphi (n, n_seg)).  ``J`` of shape (n, 4, 2, n_seg)
    (``EngineResult.control_jacobian``) gives dF (n, 4, n_seg) with respect to every field of the
    table, indexed by ``SC``.

    With the local-Z phases (alpha, beta) that ``cz_phase_fit`` returns,
    T = 1 + a01 (e^{-i beta} + e^{-i alpha}) - a11 e^{-i (alpha + beta)}, F_pro = |T|^2 / 16,
    survival = (1 + 2 |a01|^2 + |a11|^2) / 4 and F_avg = (4 F_pro + survival) / 5.  The fitted
    phases maximise F_pro, a stationary point, so the partial derivative at fixed (alpha, beta)
    is the whole derivative."""
    from . import noise_models as NM
    if which not in ("process", "avg_gate"):
        raise ValueError(f'which must be "process" or "avg_gate", not {which!r}')
    a01 = np.atleast_1d(np.asarray(a01, dtype=np.complex128))
    a11 = np.atleast_1d(np.asarray(a11, dtype=np.complex128))
    J = np.asarray(J, dtype=np.complex128)
    n = a01.shape[0]
    if J.ndim == 4:                              # every field: each one as the phase alone, stacked
        if a11.shape != (n,) or J.shape[:3] != (n, SC_NFIELD, 2):
            raise ValueError(f"need a01 (n,), a11 (n,) and J (n, 4, 2, n_seg), got {a01.shape}, {a11.shape}, "
                             f"{J.shape}")
        parts = [gate_fidelity_and_gradient(a01, a11, J[:, f], which) for f in range(SC_NFIELD)]
        return parts[0][0], np.stack([dF for _, dF in parts], axis=1)
    if a11.shape != (n,) or J.ndim != 3 or J.shape[:2] != (n, 2):
        raise ValueError(f"need a01 (n,), a11 (n,) and J (n, 2, n_seg) or (n, 4, 2, n_seg), got {a01.shape}, "
                         f"{a11.shape}, {J.shape}")
    # the qubit block of the four output kets: only the diagonal amplitudes are in it
    psi = np.zeros((n, 4, 9), dtype=np.complex128)
    psi[:, 0, 0] = 1.0
    psi[:, 1, 1] = a01
    psi[:, 2, 3] = a01
    psi[:, 3, 4] = a11
    al, be = NM.cz_phase_fit(NM.ket_maps(psi))
    w01 = np.exp(-1j * be) + np.exp(-1j * al)
    w11 = -np.exp(-1j * (al + be))
    T = 1.0 + a01 * w01 + a11 * w11
    fpro = np.abs(T) ** 2 / 16
    dT = w01[:, None] * J[:, 0] + w11[:, None] * J[:, 1]
    dpro = 2.0 * np.real(np.conj(T)[:, None] * dT) / 16
    if which == "process":
        return fpro, dpro
    surv = (1.0 + 2.0 * np.abs(a01) ** 2 + np.abs(a11) ** 2) / 4
    dsurv = (4.0 * np.real(np.conj(a01)[:, None] * J[:, 0]) + 2.0 * np.real(np.conj(a11)[:, None] * J[:, 1])) / 4
    return (4 * fpro + surv) / 5, (4 * dpro + dsurv) / 5


def optimize_phases(params: np.ndarray, sched0: np.ndarray, *, which: str = "avg_gate", maxiter: int = 200,
                    engine=None) -> dict:
    """Optimise the phase field of noise-free schedules by L-BFGS-B on exact gradients.

    Every point of ``params`` (NPARAM, n) is its own start, with its own parameters and its own
    table (``sched0``: (n, 4, n_seg), or (4, n_seg) copied to every point); only the phases
    move.  The starts are optimised together, as ONE problem: the objective is the separable
    sum of the points' infidelities 1 - F (``gate_fidelity_and_gradient``) over the
    concatenated n n_seg phases, and every function evaluation is exactly one
    ``Engine.run_schedule_kets(..., states=False, jacobian=True)`` call for all the starts.
    The sum is separable but the optimiser is not: one line search, one step length and one
    L-BFGS history serve all the starts, so a start's path depends on its companions, and the
    run ends on the sum's criteria, not on each start's own.  (Per-start optimiser state is
    not kept.)

    Returns a dict: ``sched`` (n, 4, n_seg) the final tables, ``F_start`` and ``F_final`` (n,)
    the fidelity ``which`` of every point at ``sched0`` and at ``sched``, ``nfev``,
    ``engine_calls``, ``nit``, ``success`` and ``message`` (scipy's)."""
    import hashlib

    from scipy.optimize import minimize

    from . import engine as E
    params = np.ascontiguousarray(params, dtype=np.float64)
    n = params.shape[1]
    tab = validate_schedule(sched0, n if np.ndim(sched0) == 3 else None)
    if tab.ndim == 2:
        tab = np.ascontiguousarray(np.broadcast_to(tab, (n,) + tab.shape))
    tab = tab.copy()
    n_seg = tab.shape[-1]
    eng = engine if engine is not None else E.Engine()
    calls = [0]
    seen = {}                                # digest of an evaluated phase vector -> its F (n,)
    first = []

    def fun(phi):
        tab[:, SC["PHASE"], :] = phi.reshape(n, n_seg)
        r = eng.run_schedule_kets(params, tab, states=False, jacobian=True)
        calls[0] += 1
        a01, a11 = overlaps(r.summary)
        F, dF = gate_fidelity_and_gradient(a01, a11, r.phase_jacobian, which)
        if not first:
            first.append(F)
        seen[hashlib.sha1(phi.tobytes()).digest()] = F
        return float(np.sum(1.0 - F)), -dF.reshape(-1)

    res = minimize(fun, tab[:, SC["PHASE"], :].reshape(-1).copy(), jac=True, method="L-BFGS-B",
                   options=dict(maxiter=maxiter))
    # the returned point is one of those evaluated: its F needs no further engine call
    x = np.ascontiguousarray(res.x, dtype=np.float64)
    tab[:, SC["PHASE"], :] = x.reshape(n, n_seg)
    F_final = seen[hashlib.sha1(x.tobytes()).digest()]
    return dict(sched=tab, F_start=first[0], F_final=F_final, nfev=int(res.nfev), engine_calls=calls[0],
                nit=int(res.nit), success=bool(res.success), message=str(res.message))


FIELDS = {"x": SC["X"], "amp": SC["AMP"], "phase": SC["PHASE"], "delta": SC["DELTA"]}


def optimize_schedule(params: np.ndarray, sched0: np.ndarray, *, free: Sequence[str] = ("phase",),
                      amp_max: Optional[float] = None, duration_weight: float = 0.0, which: str = "avg_gate",
                      maxiter: int = 200, engine=None) -> dict:
    """Optimise chosen fields of noise-free schedules by L-BFGS-B on exact gradients.

    ``optimize_phases`` with the moving fields chosen: ``free`` names them, any of "x", "amp",
    "phase", "delta" (``FIELDS``), and the other fields stay as ``sched0`` has them.  The bounds
    are x >= 0 and 0 <= a <= ``amp_max`` (None: no upper bound); phase and detuning are free.
    The objective is sum_points (1 - F) + ``duration_weight`` sum_points sum_s x_s, so a positive
    weight with "x" free trades fidelity against pulse length.  As in ``optimize_phases`` the
    starts are one problem, and every function evaluation is exactly one
    ``Engine.run_schedule_kets(..., states=False, jacobian="controls")`` call for all of them.

    Returns the dict of ``optimize_phases``: ``sched``, ``F_start``, ``F_final`` (the fidelity
    ``which``, without the duration term), ``nfev``, ``engine_calls``, ``nit``, ``success``,
    ``message``."""
    import hashlib

    from scipy.optimize import minimize

    from . import engine as E
    free = tuple(free)
    if not free or len(set(free)) != len(free) or any(f not in FIELDS for f in free):
        raise ValueError(f"free must name distinct fields out of {tuple(FIELDS)}, not {free!r}")
    if which not in ("process", "avg_gate"):
        raise ValueError(f'which must be "process" or "avg_gate", not {which!r}')
    if amp_max is not None and not (np.isfinite(amp_max) and amp_max > 0):
        raise ValueError(f"amp_max must be a positive number or None, not {amp_max!r}")
    if not (np.isfinite(duration_weight) and duration_weight >= 0):
        raise ValueError(f"duration_weight must be >= 0, not {duration_weight!r}")
    params = np.ascontiguousarray(params, dtype=np.float64)
    n = params.shape[1]
    tab = validate_schedule(sched0, n if np.ndim(sched0) == 3 else None)
    if tab.ndim == 2:
        tab = np.ascontiguousarray(np.broadcast_to(tab, (n,) + tab.shape))
    tab = tab.copy()
    if "amp" in free and amp_max is not None and np.any(tab[:, SC["AMP"]] > amp_max):
        raise ValueError("sched0 has amplitudes above amp_max")
    n_seg = tab.shape[-1]
    idx = [FIELDS[f] for f in free]
    lo = {"x": 0.0, "amp": 0.0}
    hi = {"amp": amp_max}
    bounds = [(lo.get(f), hi.get(f)) for f in free for _ in range(n * n_seg)]
    eng = engine if engine is not None else E.Engine()
    calls = [0]
    seen = {}                                    # digest of an evaluated vector -> its F (n,)
    first = []

    def put(v):
        tab[:, idx, :] = v.reshape(len(idx), n, n_seg).transpose(1, 0, 2)

    def fun(v):
        put(v)
        r = eng.run_schedule_kets(params, tab, states=False, jacobian="controls")
        calls[0] += 1
        a01, a11 = overlaps(r.summary)
        F, dF = gate_fidelity_and_gradient(a01, a11, r.control_jacobian, which)
        if not first:
            first.append(F)
        seen[hashlib.sha1(v.tobytes()).digest()] = F
        grad = -dF[:, idx, :]
        if "x" in free:
            grad[:, free.index("x"), :] += duration_weight
        cost = float(np.sum(1.0 - F)) + duration_weight * float(np.sum(tab[:, SC["X"], :]))
        return cost, np.ascontiguousarray(grad.transpose(1, 0, 2)).reshape(-1)

    v0 = np.ascontiguousarray(tab[:, idx, :].transpose(1, 0, 2)).reshape(-1)
    res = minimize(fun, v0, jac=True, method="L-BFGS-B", bounds=bounds, options=dict(maxiter=maxiter))
    # the returned point is one of those evaluated: its F needs no further engine call
    v = np.ascontiguousarray(res.x, dtype=np.float64)
    put(v)
    F_final = seen[hashlib.sha1(v.tobytes()).digest()]
    return dict(sched=tab, F_start=first[0], F_final=F_final, nfev=int(res.nfev), engine_calls=calls[0],
                nit=int(res.nit), success=bool(res.success), message=str(res.message))
