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

from ._native import SC, SC_NFIELD, SCHED_MAX_SEG

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
