"""Batched evolution engine: the host side of the ryd_engine C-ABI.

``Engine.run`` is the batched replacement for every ``evolve_state`` /
``qutip.mesolve`` call the reference evolvers make
(RG/simulation.py:647-2231): one call propagates all 4 computational-basis
inputs of every parameter point through every segment of the protocol.

State rows come back in the compact sector form of include/ryd_engine.h;
``expand_rho`` / ``expand_ket`` rebuild the QuTiP-layout 9x9 density matrices
(structural zeros exact) and kets for the fidelity epilogue and callers that
want ``SimulationResult.results``.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Any, Dict, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native as N
from .physics import DerivedBatch

def _sector_basis(d: int) -> np.ndarray:
    """Single-atom Hermitian basis of the sector: e00, e11, err, ex, ey (dim 3), plus
    e-- = |r-><r-| (dim 4, where r = r+)."""
    E = np.zeros((5 if d == 3 else 6, d, d), dtype=complex)
    E[0, 0, 0] = E[1, 1, 1] = E[2, 2, 2] = 1
    E[3, 1, 2] = E[3, 2, 1] = 1
    E[4, 1, 2], E[4, 2, 1] = 1j, -1j
    if d == 4:
        E[5, 3, 3] = 1
    # B[k i + j] = e_i (x) e_j  (atom 1 = slow index, as qutip.tensor)
    k = E.shape[0]
    return np.stack([np.kron(E[i], E[j]) for i in range(k) for j in range(k)]).reshape(k * k, d ** 4)


_BFLAT = {3: _sector_basis(3), 4: _sector_basis(4)}


def expand_rho(state: np.ndarray, n: int, dim: int = 3) -> np.ndarray:
    """Compact Lindblad rows (25 or 36, >=4n) -> rho[n, 4, D, D] (complex128), D = dim^2."""
    B = _BFLAT[dim]
    R = np.ascontiguousarray(state[:B.shape[0], :4 * n].T)     # (4n, 25 | 36)
    D = dim * dim
    return (R @ B).reshape(n, 4, D, D)


def expand_ket(state: np.ndarray, n: int, dim: int = 3) -> np.ndarray:
    """Ket rows (2 D, >=4n) -> psi[n, 4, D] (complex128)."""
    D = dim * dim
    s = state[:2 * D, :4 * n]
    return (s[0::2] + 1j * s[1::2]).T.reshape(n, 4, D)


GAUGE_REL_EPS = 1e-12       # relative perturbation of the sector coordinates (gauge check)
GAUGE_TOL = 1e-9            # penalty change that flags RYD_STATUS_GAUGE_UNSTABLE
GAUGE_COPIES = 16          # probes (an unstable point usually stops after a few); see ryd_mixed_phase


def mixed_phase(state: np.ndarray, n: int, dim: int = 3, gauge_check: bool = True,
                n_threads: int = 0, rel_eps: float = GAUGE_REL_EPS, tol: float = GAUGE_TOL,
                copies: int = GAUGE_COPIES) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's mixed-state controlled phase (RG/simulation.py:424-452) for every
    point of a Lindblad state block (sector rows, >= 4n columns), through the C-ABI host
    epilogue ryd_mixed_phase on scipy's own LAPACK zheevr (so each phase equals
    scipy.linalg.eigh's -- QuTiP 5's eigensolver -- on the same rho).  Returns
    (phases[n, 4], flags[n]): phi_x = np.angle(<x|v_max>) exactly as the reference forms
    it, and RYD_STATUS_GAUGE_UNSTABLE where the penalty is not a function of rho at
    relative precision rel_eps."""
    lib = N.load()
    if n_threads <= 0:          # the GPU box's CPU share is 16 cores per GPU (os.cpu_count() shows more)
        n_threads = int(os.environ.get("RYD_HOST_THREADS", min(16, os.cpu_count() or 1)))
    pool = N.lapack_pool_copies(n_threads)
    if n_threads > 1 and n >= 64 and pool > 1:
        N.scipy_lapack_pool(pool)
    st = np.ascontiguousarray(state, dtype=np.float64)
    out = np.zeros((N.MP_WIDTH, max(n, 1)), dtype=np.float64)
    flags = np.zeros(max(n, 1), dtype=np.uint32)
    dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    N.check(lib.ryd_mixed_phase(N.scipy_zheevr(), dim, dptr(st), n, st.shape[1],
                                copies if gauge_check else 0, rel_eps, tol, n_threads,
                                dptr(out), out.shape[1], flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
    v = out[N.MP["V0"]:N.MP["V0"] + 8:2, :n] + 1j * out[N.MP["V0"] + 1:N.MP["V0"] + 8:2, :n]
    return np.angle(v).T.copy(), flags[:n]


@dataclass
class EngineResult:
    evolution: str
    n: int
    state: Optional[np.ndarray]   # (width, 4n); None after a summary-only run (states=False)
    summary: np.ndarray     # (NSUMMARY, n)
    status: np.ndarray      # (n,) uint32
    kernel_ms: float
    h2d_ms: float
    d2h_ms: float
    matvec_useful: float
    matvec_exec: float
    # run_schedule_kets(jacobian="controls"): d a01 and d a11 with respect to every field of every
    # segment, complex (n, 4, 2, n_seg), first index _native.SC.  By keyword only: positional
    # construction, which ends with dim and phase_jacobian, stays as it was.
    control_jacobian: Optional[np.ndarray] = field(default=None, kw_only=True)
    dim: int = 3
    # run_schedule_kets(jacobian=True): d a01 / d phi_s and d a11 / d phi_s, complex (n, 2, n_seg)
    phase_jacobian: Optional[np.ndarray] = None

    def col(self, name: str) -> np.ndarray:
        return self.summary[N.S[name]]

    def populations(self) -> np.ndarray:
        return self.summary[N.S["POP0"]:N.S["POP0"] + 4].T

    def _need_state(self, what: str) -> None:
        if self.state is None:
            raise ValueError(f"{what}: the run was summary-only (states=False), no state rows were kept")

    def rho(self) -> np.ndarray:
        assert self.evolution == "lindblad"
        self._need_state("rho()")
        return expand_rho(self.state, self.n, self.dim)

    def kets(self) -> np.ndarray:
        assert self.evolution == "ket"
        self._need_state("kets()")
        return expand_ket(self.state, self.n, self.dim)


def protocol_key(batch: DerivedBatch) -> str:
    if batch.protocol == "levine_pichler":
        shape = batch.pulse_shape.lower()
        if shape == "square":
            return "lp_square"
        if shape == "drag":
            # RG/simulation.py:2170 -> area_correction_factor('drag') -> envelope without Delta_leak
            raise TypeError("pulse_envelope_drag() missing 1 required positional argument: 'Delta_leak'")
        if shape not in N.SHAPE:
            raise ValueError(f"Unknown pulse shape: {batch.pulse_shape}. "
                             f"Available shapes: ['square', 'gaussian', 'cosine', 'blackman', 'drag']")
        return "lp_shaped"
    if batch.protocol == "smooth_jp":
        return "smooth_jp"
    if batch.protocol == "pulse_schedule":
        return "schedule"                    # Engine.run_schedule: not a protocol of Engine.run
    return "bangbang"


def pack_params(batch: DerivedBatch, idx: Optional[np.ndarray] = None) -> np.ndarray:
    """DerivedBatch -> SoA parameter block (NPARAM, n) for the kernel."""
    sel = slice(None) if idx is None else idx
    c = batch.cols
    n = batch.n if idx is None else len(idx)
    p = np.zeros((N.NPARAM, n), dtype=np.float64)
    P = N.P
    p[P["OMEGA"]] = c["Omega"][sel]
    p[P["DELTA"]] = c["Delta_seg"][sel]
    p[P["V"]] = c["V"][sel]
    p[P["DELTA1"]] = (c["delta_zeeman"] + (c["delta_stark"] if batch.trap_laser_on else 0.0))[sel]
    g1, g0, gphi, gsc = (g[sel] for g in batch.channel_rates())
    for key, g in (("G1", g1), ("G0", g0), ("GPHI", gphi), ("GSC", gsc)):
        p[P[key + "_A"]] = g
        p[P[key + "_B"]] = g
    if batch.dim == 4:
        gm = batch.mj_rate()[sel]
        p[P["GMJ_A"]] = gm
        p[P["GMJ_B"]] = gm
    key = protocol_key(batch)
    if key in ("lp_square", "lp_shaped"):
        p[P["TAU"]] = c["tau_single"][sel]
        p[P["XI_RE"]] = c["xi_re"][sel]
        p[P["XI_IM"]] = c["xi_im"][sel]
        if key == "lp_shaped":
            from .physics import area_correction_factor
            p[P["AREA_CORR"]] = area_correction_factor(batch.pulse_shape.lower(), c["tau_single"][sel])
    elif key == "smooth_jp":
        p[P["TAU"]] = c["tau_total"][sel]
        p[P["A"]] = c["A"][sel]
        p[P["OMEGA_MOD"]] = c["omega_mod"][sel]
        p[P["PHI_OFF"]] = c["phi_offset"][sel]
    elif key == "schedule":
        pass                                 # the table carries the pulse; the protocol columns stay 0
    else:
        t = batch.bangbang_times[sel]
        ph = batch.bangbang_phases[sel]
        nseg = ph.shape[1]
        if nseg > 8:
            raise ValueError("bang-bang schedules with more than 8 segments are not supported")
        p[P["OMEGA_TAU"]] = c["omega_tau"][sel]
        p[P["NSEG"]] = nseg
        p[P["SWT0"]:P["SWT0"] + nseg - 1] = t.T
        p[P["PHI0"]:P["PHI0"] + nseg] = ph.T
    return p


def make_desc(protocol: str, evolution: str, n_steps: int = 0, shape: str = "square",
              symmetric: bool = True, method: str = "chebyshev", dim: int = 3,
              rtol: float = 1e-10, atol: float = 1e-12, max_steps: int = 10 ** 7) -> N.BatchDesc:
    d = N.BatchDesc()
    d.abi_version = N.RYD_ABI_VERSION
    d.dim = dim
    d.protocol = N.PROTO[protocol]
    d.evolution = N.EVOL[evolution]
    d.method = N.METHOD[method]
    d.shape = N.SHAPE[shape]
    d.n_steps = n_steps
    d.flags = N.FLAG_SYMMETRIC_ATOMS if symmetric else 0
    d.rtol, d.atol, d.max_steps = rtol, atol, max_steps
    return d


def default_n_steps(protocol: str, params: np.ndarray) -> int:
    if protocol == "smooth_jp":
        return 300                       # RG/simulation.py:3496
    if protocol == "lp_shaped":
        return 500                       # evolve_shaped_pulse n_time_steps (:2113)
    if protocol == "bangbang":
        return int(params[N.P["NSEG"]].max()) if params.shape[1] else 1
    return 0


def symmetric_atoms(params: np.ndarray) -> bool:
    P = N.P
    return all(np.array_equal(params[P[k + "_A"]], params[P[k + "_B"]])
               for k in ("G1", "G0", "GPHI", "GSC", "GMJ"))


def schedule_desc(params: np.ndarray, sched: np.ndarray) -> Tuple[N.SchedDesc, np.ndarray, int]:
    """(descriptor, contiguous table, ld_sched) of a schedule run on ``params`` (NPARAM, n):
    the table is checked (``pulse_schedules.validate_schedule``) except for its values, which
    the kernel checks per point (status BAD_INPUT), and unequal atoms are refused."""
    n = params.shape[1]
    tab = np.ascontiguousarray(sched, dtype=np.float64)
    if tab.ndim not in (2, 3) or tab.shape[-2] != N.SC_NFIELD or (tab.ndim == 3 and tab.shape[0] != n):
        raise ValueError(f"sched must have shape ({n}, 4, n_seg) or (4, n_seg), not {tab.shape}")
    if not 1 <= tab.shape[-1] <= N.SCHED_MAX_SEG:
        raise ValueError(f"a schedule has 1 .. {N.SCHED_MAX_SEG} segments, not {tab.shape[-1]}")
    if not symmetric_atoms(params):
        raise ValueError("pulse schedules run identical atoms only: the atom-A and atom-B rate columns differ")
    d = N.SchedDesc()
    d.abi_version = N.RYD_ABI_VERSION
    d.dim = 3
    d.n_seg = tab.shape[-1]
    d.flags = N.FLAG_SYMMETRIC_ATOMS | (N.RYD_SCHED_SHARED if tab.ndim == 2 else 0)
    return d, tab, N.SC_NFIELD * tab.shape[-1]


def complex_jacobian(jac: Optional[np.ndarray]) -> Optional[np.ndarray]:
    """The library's Jacobian rows (n, 4, n_seg) -- Re, Im of d a01, Re, Im of d a11 -- as the
    complex (n, 2, n_seg) of ``EngineResult.phase_jacobian``; None stays None."""
    return None if jac is None else jac[:, 0::2] + 1j * jac[:, 1::2]


def complex_control_jacobian(jac: np.ndarray) -> np.ndarray:
    """The library's control-Jacobian rows (n, 4 fields, 4, n_seg) -- per field Re, Im of d a01,
    Re, Im of d a11 -- as the complex (n, 4, 2, n_seg) of ``EngineResult.control_jacobian``."""
    return jac[:, :, 0::2] + 1j * jac[:, :, 1::2]


def jacobian_mode(jacobian) -> bool:
    """``jacobian`` of the schedule-ket calls: True / False (the phase Jacobian or none) give
    False, "controls" gives True; anything else is a ValueError."""
    if isinstance(jacobian, (bool, np.bool_)):
        return False
    if jacobian == "controls":
        return True
    raise ValueError(f'jacobian must be True, False or "controls", not {jacobian!r}')


def check_coherence_dim(params: np.ndarray, dim: int) -> None:
    """The process-map coherence kernels exist for dim 3 and 4; dim 3 has no mJ channel, so
    a ``params`` with nonzero GMJ columns would have them silently ignored: refuse it."""
    if dim not in (3, 4):
        raise ValueError(f"process-map coherences: dim must be 3 or 4, not {dim}")
    if dim == 3 and (np.any(params[N.P["GMJ_A"]] != 0) or np.any(params[N.P["GMJ_B"]] != 0)):
        raise ValueError("params carry mJ leakage rates (GMJ_A / GMJ_B) that dim=3 would ignore; pass dim=4")


def schedule_coherence_inputs(params: np.ndarray,
                              sched: np.ndarray) -> Tuple[np.ndarray, N.SchedDesc, np.ndarray, int]:
    """(contiguous params, descriptor, contiguous table, ld_sched) of a schedule coherence run:
    ``schedule_desc``'s checks (table form, segment count, identical atoms) and, as for every
    dim-3 coherence run, nonzero GMJ columns refused rather than ignored."""
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.ndim != 2 or params.shape[0] != N.NPARAM:
        raise ValueError(f"params must have shape ({N.NPARAM}, n)")
    check_coherence_dim(params, 3)
    desc, tab, ld = schedule_desc(params, sched)
    return params, desc, tab, ld


def param_block(params: np.ndarray) -> np.ndarray:
    """``params`` as the contiguous float64 (NPARAM, n) block the library reads."""
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.shape[0] != N.NPARAM:
        raise ValueError(f"params must have shape ({N.NPARAM}, n)")
    return params


def jacobian_shape(n: int, n_seg: int, controls: bool) -> Tuple[int, ...]:
    """The library's Jacobian rows of a schedule-ket run: phases alone, or all four fields."""
    return (n, N.SC_NFIELD, 4, n_seg) if controls else (n, N.SC_NFIELD, n_seg)


def summary_result(evolution: str, n: int, state: Optional[np.ndarray], summ: np.ndarray, status: np.ndarray,
                   dim: int, st: Optional[N.Stats] = None, jac: Optional[np.ndarray] = None,
                   controls: bool = False) -> EngineResult:
    """The EngineResult of a summary-carrying run: timings and iteration counts from the call's
    stats, or (a device-resident batch, ``st`` None) no timings and the counts summed here;
    ``jac`` the library's Jacobian rows of a schedule-ket run (``jacobian_shape``), or None."""
    times = (st.kernel_ms, st.h2d_ms, st.d2h_ms, st.matvec_useful, st.matvec_exec) if st is not None else (
        0.0, 0.0, 0.0, summ[N.S["NMV_USEFUL"]].sum(), summ[N.S["NMV_EXEC"]].sum())
    if controls:
        cj = complex_control_jacobian(jac)
        return EngineResult(evolution, n, state, summ, status, *times, dim,
                            np.ascontiguousarray(cj[:, N.SC["PHASE"]]), control_jacobian=cj)
    return EngineResult(evolution, n, state, summ, status, *times, dim, complex_jacobian(jac))


def _dptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def sym16_balance_plan(n: int, cus: int = 256, gpc: int = 0) -> Dict[str, Any]:
    """The static plan of the sym16 LP-square kernel's CU-balanced launch form for ``n`` points
    on ``cus`` compute units (``gpc`` > 0 overrides the groups per workgroup): ``groups``,
    ``workgroups``, ``waves``, ``gpc``, ``auto`` (the automatic rule picks the form) and, per
    (workgroup, wave), ``role`` (0 whole job, 1 producer, 2 consumer), ``job`` and ``present``.
    Host code only: no device is touched."""
    lib = N.load()
    i64p = ctypes.POINTER(ctypes.c_int64)
    head = np.zeros(5, dtype=np.int64)
    need = lib.ryd_sym16_balance_plan(n, cus, gpc, head.ctypes.data_as(i64p), None, None, None, 0)
    if need < 0:
        raise ValueError(f"no balanced plan for n={n}, cus={cus}, gpc={gpc}")
    role = np.zeros(need, dtype=np.int32)
    job = np.zeros(need, dtype=np.int64)
    present = np.zeros(need, dtype=np.uint8)
    lib.ryd_sym16_balance_plan(n, cus, gpc, head.ctypes.data_as(i64p),
                               role.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), job.ctypes.data_as(i64p),
                               present.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), need)
    shape = (int(head[1]), int(head[2]))
    return dict(groups=int(head[0]), workgroups=shape[0], waves=shape[1], gpc=int(head[3]), auto=bool(head[4]),
                role=role.reshape(shape), job=job.reshape(shape), present=present.reshape(shape).astype(bool))


def batch_path(desc: N.BatchDesc, states: bool = True) -> int:
    """The kernel family a batch call launches for ``desc`` (``N.PATH``), under the environment
    switches as they stand now; ``states=False`` asks about a summary-only call, and
    ``N.PATH["NOSTATE"]`` is then OR-ed in where it runs the store-free twin.  Host code only."""
    rc = N.load().ryd_batch_path(ctypes.byref(desc), 1 if states else 0)
    if rc < 0:
        N.check(rc)
    return rc


def device_count() -> int:
    """GPUs visible to the HIP runtime (ryd_device_count)."""
    lib = N.load()
    cnt = ctypes.c_int(0)
    N.check(lib.ryd_device_count(ctypes.byref(cnt)))
    return cnt.value


class Engine:
    """A handle on one or more GPUs (points are range-partitioned across them)."""

    def __init__(self, devices: Optional[Sequence[int]] = None):
        self.lib = N.load()
        cnt = ctypes.c_int(0)
        N.check(self.lib.ryd_device_count(ctypes.byref(cnt)))
        if cnt.value == 0:
            raise N.EngineError("no GPU visible to the HIP runtime")
        devs = list(devices) if devices is not None else [0]
        arr = (ctypes.c_int * len(devs))(*devs)
        h = ctypes.c_void_p()
        N.check(self.lib.ryd_create(arr, len(devs), ctypes.byref(h)))
        self.handle = h
        self.devices = devs

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ryd_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, desc, params: np.ndarray, outs, table=()) -> Tuple[np.ndarray, N.Stats]:
        """One host-buffer entry point on ``params`` (NPARAM, n): ``table`` is the (pointer,
        leading dimension) of a schedule table or nothing, ``outs`` the (array or None, leading
        dimension) pairs in the entry point's order.  Returns (status (n,), the call's stats)."""
        n = params.shape[1]
        status = np.zeros(n, dtype=np.uint32)
        st = N.Stats()
        N.check(fn(self.handle, ctypes.byref(desc), _dptr(params), n, n, *table,
                   *(x for arr, ld in outs for x in (_dptr(arr), ld)),
                   status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(st)))
        return status, st

    def _summary_run(self, fn, desc, params: np.ndarray, evolution: str, dim: int, states: bool, table=(),
                     jac: Optional[np.ndarray] = None, jac_arg: bool = False,
                     controls: bool = False) -> EngineResult:
        """A summary-carrying entry point and its EngineResult.  ``jac_arg``: the entry point takes
        a Jacobian (``jac``, or NULL) after the summary."""
        n = params.shape[1]
        # every kernel writes every state row and summary column of every point, so the
        # outputs need no zero fill (np.zeros of the 8 MB C2 state costs ~0.3 ms of page
        # zeroing per call; tools/unpack_probe.py)
        state = np.empty((N.STATE_WIDTH_DIM[dim][evolution], 4 * n), dtype=np.float64) if states else None
        summ = np.empty((N.NSUMMARY, n), dtype=np.float64)
        outs = [(state, 4 * n), (summ, n)]
        if jac_arg:
            outs.append((jac, (4 if controls else 1) * N.SC_NFIELD * desc.n_seg))
        status, st = self._call(fn, desc, params, outs, table)
        return summary_result(evolution, n, state, summ, status, dim, st, jac, controls)

    def run(self, params: np.ndarray, protocol: str, evolution: str, n_steps: Optional[int] = None,
            shape: str = "square", method: str = "chebyshev", rtol: float = 1e-10,
            atol: float = 1e-12, max_steps: int = 10 ** 7, dim: int = 3,
            states: bool = True) -> EngineResult:
        """``states=False`` is a summary-only run: no state array is allocated, the library
        gets a NULL state pointer (no state rows cross the bus) and ``EngineResult.state`` is
        None; summary and status are those of the full run bit for bit."""
        params = param_block(params)
        if n_steps is None:
            n_steps = default_n_steps(protocol, params)
        desc = make_desc(protocol, evolution, n_steps, shape, symmetric_atoms(params), method,
                         dim=dim, rtol=rtol, atol=atol, max_steps=max_steps)
        return self._summary_run(self.lib.ryd_run_batch, desc, params, evolution, dim, states)

    def run_schedule(self, params: np.ndarray, sched: np.ndarray, *, states: bool = True) -> EngineResult:
        """The caller's own pulse (ryd_run_schedule): ``sched`` is a table of piecewise-constant
        segments, shape ``(n, 4, n_seg)`` per point or ``(4, n_seg)`` shared by every point
        (``pulse_schedules``; fields ``_native.SC``).  Lindblad, dim 3, identical atoms: unequal
        atom-A / atom-B rate columns are refused.  The result is that of ``run(...,
        "lindblad")``; ``states=False`` is a summary-only run."""
        params = param_block(params)
        desc, tab, ld = schedule_desc(params, sched)
        return self._summary_run(self.lib.ryd_run_schedule, desc, params, "lindblad", 3, states, (_dptr(tab), ld))

    def run_schedule_kets(self, params: np.ndarray, sched: np.ndarray, *, states: bool = True,
                          jacobian: Union[bool, str] = False) -> EngineResult:
        """The caller's own pulse without noise, as kets (ryd_run_schedule_kets): ``sched`` as
        ``run_schedule`` takes it; the rate columns of ``params`` are checked and otherwise
        ignored.  The result is that of ``run(..., "ket")``.  With ``jacobian`` its
        ``phase_jacobian`` is the complex array (n, 2, n_seg) of d a01 / d phi_s (index 0) and
        d a11 / d phi_s (index 1), a01 = <01|psi_01>, a11 = <11|psi_11>
        (``pulse_schedules.overlaps(result.summary)``); state, summary and status do not depend on it.
        ``jacobian="controls"`` (ryd_run_schedule_kets_ctl) gives ``control_jacobian`` too, the
        complex (n, 4, 2, n_seg) of the derivatives with respect to x_s, a_s, phi_s and delta_s
        (first index ``_native.SC``, the table's units); ``phase_jacobian`` is then its
        ``SC["PHASE"]`` slice.  ``states=False`` is a summary-only run."""
        controls = jacobian_mode(jacobian)
        params = param_block(params)
        desc, tab, ld = schedule_desc(params, sched)
        n = params.shape[1]
        jac = np.empty(jacobian_shape(n, desc.n_seg, controls), dtype=np.float64) if jacobian else None
        fn = self.lib.ryd_run_schedule_kets_ctl if controls else self.lib.ryd_run_schedule_kets
        return self._summary_run(fn, desc, params, "ket", 3, states, (_dptr(tab), ld), jac, True, controls)

    def last_timeline(self) -> Dict[str, Any]:
        """ryd_last_timeline: host staging times and the per-slot HIP-event timeline of the
        last host-buffer call (ms; slot times relative to the first slot on its device)."""
        buf = np.zeros(N.TL_HEAD + N.TL_SLOT * len(self.devices))
        N.check(self.lib.ryd_last_timeline(self.handle, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                           buf.size))
        slots = []
        for k in range(int(buf[0])):
            t = buf[N.TL_HEAD + N.TL_SLOT * k: N.TL_HEAD + N.TL_SLOT * (k + 1)]
            slots.append(dict(device=int(t[0]), h2d_start=t[1], kernel_start=t[2], kernel_end=t[3],
                              d2h_end=t[4], points=int(t[5]), host_enqueued=t[6], host_wait=t[7]))
        return dict(pack_ms=buf[1], unpack_ms=buf[2], wall_ms=buf[3], slots=slots)

    def run_coherences(self, params: np.ndarray, protocol: str, n_steps: Optional[int] = None,
                       shape: str = "square", dim: int = 3) -> Tuple[np.ndarray, np.ndarray]:
        """The 6 upper off-diagonal qubit matrix units through the gate
        (ryd_run_coherences): returns (coh (NCOH, n) float64, status (n,) uint32).  The rows
        mean the same for ``dim`` 3 and 4 (the qubit block has the same support)."""
        params = param_block(params)
        check_coherence_dim(params, dim)
        n = params.shape[1]
        if n_steps is None:
            n_steps = default_n_steps(protocol, params)
        desc = make_desc(protocol, "lindblad", n_steps, shape, symmetric_atoms(params), "cheb_vector", dim=dim)
        coh = np.zeros((N.NCOH, n), dtype=np.float64)
        status, _ = self._call(self.lib.ryd_run_coherences, desc, params, [(coh, n)])
        return coh, status

    def run_schedule_coherences(self, params: np.ndarray, sched: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """The coherence rows of ``run_coherences`` for the caller's own pulse
        (ryd_run_schedule_coherences): ``sched`` as ``run_schedule`` takes it.  With the states of
        ``run_schedule`` on the same inputs they make the process map
        (``noise_models.schedule_process_maps``).  Returns (coh (NCOH, n), status (n,))."""
        params, desc, tab, ld = schedule_coherence_inputs(params, sched)
        n = params.shape[1]
        coh = np.zeros((N.NCOH, n), dtype=np.float64)
        status, _ = self._call(self.lib.ryd_run_schedule_coherences, desc, params, [(coh, n)], (_dptr(tab), ld))
        return coh, status

    def derive(self, inp, diag: bool = False) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """Hot-path row a1 on the GPU (ryd_derive): ``physics.derive_inputs(...)`` ->
        (params (NPARAM, n) as pack_params builds them, warning bits (n,) uint32, and with
        ``diag`` the (DV_NDIAG, n) derived columns named by _native.DV_DIAG)."""
        n = inp.n
        cols = np.ascontiguousarray(inp.cols, dtype=np.float64)
        params = np.empty((N.NPARAM, n), dtype=np.float64)
        warn = np.zeros(n, dtype=np.uint32)
        dg = np.empty((N.DV_NDIAG, n), dtype=np.float64) if diag else None
        dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        N.check(self.lib.ryd_derive(self.handle, ctypes.byref(inp.desc), dptr(cols) if cols.shape[0] else None,
                                    cols.shape[0], n, n, dptr(params), n,
                                    warn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                    dptr(dg) if diag else None, n))
        return params, warn, dg

    def evolve_generic(self, H: np.ndarray, dt: np.ndarray, state0: np.ndarray,
                       ops: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The generic evolve_state seam (ryd_evolve_generic; RG/simulation.py:647-690) for
        a batch: H (n, n_seg, d, d) piecewise-constant Hamiltonians, dt (n, n_seg), state0
        (n, d) kets or (n, d, d) density matrices, ops (n, K, d, d) jump operators (kets
        only without them).  Returns (final states, status (n,) uint32)."""
        H = np.ascontiguousarray(H, dtype=np.complex128)
        if H.ndim != 4 or H.shape[2] != H.shape[3]:
            raise ValueError("H must have shape (n, n_seg, d, d)")
        n, n_seg, d = H.shape[0], H.shape[1], H.shape[2]
        dt = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, dtype=np.float64), (n, n_seg)))
        state0 = np.ascontiguousarray(state0, dtype=np.complex128)
        ket = state0.shape == (n, d)
        if not ket and state0.shape != (n, d, d):
            raise ValueError("state0 must have shape (n, d) or (n, d, d)")
        K = 0
        if ops is not None:
            ops = np.ascontiguousarray(ops, dtype=np.complex128)
            if ops.ndim != 4 or ops.shape[0] != n or ops.shape[2:] != (d, d):
                raise ValueError("ops must have shape (n, K, d, d)")
            K = ops.shape[1]
        out = np.zeros_like(state0)
        status = np.zeros(n, dtype=np.uint32)
        dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        N.check(self.lib.ryd_evolve_generic(
            self.handle, d, n_seg, K, n, 1 if ket else 0, dptr(H), dptr(dt),
            dptr(ops) if K > 0 else None, dptr(state0), dptr(out),
            status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out, status


class _DeviceBuffers:
    """What every device-resident batch shares: buffers on one device slot (allocated with a
    16-byte floor, freed together), uploads and downloads through the slot's stream, the two
    HIP-event marks, and the timing of a ``*_device`` call.  A subclass keeps its constructor
    arguments, its ``launch`` and what ``fetch`` assembles."""

    def __init__(self, engine: Engine, slot: int):
        self.eng, self.slot = engine, slot
        self._bufs = []

    def _alloc(self, nbytes: int) -> ctypes.c_void_p:
        p = ctypes.c_void_p()
        N.check(self.eng.lib.ryd_malloc(self.eng.handle, self.slot, max(nbytes, 16), ctypes.byref(p)))
        self._bufs.append(p)
        return p

    def _upload(self, array: np.ndarray, d_ptr: Optional[ctypes.c_void_p] = None) -> ctypes.c_void_p:
        """H2D of a contiguous array, into a new buffer of its size unless ``d_ptr`` is given."""
        if d_ptr is None:
            d_ptr = self._alloc(array.nbytes)
        N.check(self.eng.lib.ryd_memcpy_h2d(self.eng.handle, self.slot, d_ptr, array.ctypes.data, array.nbytes))
        return d_ptr

    def _download(self, array: np.ndarray, d_ptr: ctypes.c_void_p) -> np.ndarray:
        N.check(self.eng.lib.ryd_memcpy_d2h(self.eng.handle, self.slot, array.ctypes.data, d_ptr, array.nbytes))
        return array

    def _timed(self, call, timed: bool) -> float:
        """``call(elapsed_ms)`` with a float pointer when ``timed`` (the library then waits and
        reports the device time between HIP events on the launch stream), else NULL."""
        ms = ctypes.c_float(0.0)
        N.check(call(ctypes.byref(ms) if timed else None))
        return float(ms.value)

    def _alloc_summary_run(self, n: int, states: bool) -> None:
        """The outputs of a summary-carrying run; ``states`` False: summary-only, no d_state
        (NULL is passed)."""
        self.states = states
        self.d_state = self._alloc(8 * self.width * 4 * n) if states else None
        self.d_summary = self._alloc(8 * N.NSUMMARY * n)
        self.d_status = self._alloc(4 * n)

    def _fetch_summary_run(self, evolution: str, dim: int, status_or=0, jac: Optional[np.ndarray] = None,
                           controls: bool = False) -> EngineResult:
        state = self._download(np.zeros((self.width, 4 * self.n)), self.d_state) if self.states else None
        summ = self._download(np.zeros((N.NSUMMARY, self.n)), self.d_summary)
        status = self._download(np.zeros(self.n, dtype=np.uint32), self.d_status)
        return summary_result(evolution, self.n, state, summ, status | status_or, dim, None, jac, controls)

    def _fetch_coherences(self) -> Tuple[np.ndarray, np.ndarray]:
        return (self._download(np.zeros((N.NCOH, self.n)), self.d_coh),
                self._download(np.zeros(self.n, dtype=np.uint32), self.d_status))

    def mark(self, which: int):
        """Record HIP event `which` (0 = region start, 1 = region end) on the launch stream."""
        N.check(self.eng.lib.ryd_mark(self.eng.handle, self.slot, which))

    def mark_elapsed(self) -> float:
        """Device ms between marks 0 and 1 (waits for mark 1)."""
        return self._timed(lambda ms: self.eng.lib.ryd_mark_elapsed(self.eng.handle, self.slot, ms), True)

    def synchronize(self):
        N.check(self.eng.lib.ryd_synchronize(self.eng.handle))

    def free(self):
        for p in self._bufs:
            self.eng.lib.ryd_free(self.eng.handle, self.slot, p)
        self._bufs = []


class DeviceBatch(_DeviceBuffers):
    """Inputs resident in HBM on one device slot, for timed re-runs (bench.py)."""

    def __init__(self, engine: Engine, params: np.ndarray, protocol: str, evolution: str,
                 n_steps: Optional[int] = None, shape: str = "square", slot: int = 0,
                 method: str = "chebyshev", dim: int = 3, states: bool = True):
        super().__init__(engine, slot)
        params = np.ascontiguousarray(params, dtype=np.float64)
        self.n = n = params.shape[1]
        if n_steps is None:
            n_steps = default_n_steps(protocol, params)
        self.desc = make_desc(protocol, evolution, n_steps, shape, symmetric_atoms(params), method, dim=dim)
        self.dim = dim
        self.width = N.STATE_WIDTH_DIM[dim][evolution]
        self.evolution = evolution
        self.d_params = self._upload(params)
        self._alloc_summary_run(n, states)

    def launch(self, timed: bool = False) -> float:
        """Enqueue one propagation of the whole batch; with ``timed`` wait and return
        the kernel's device time (HIP events on the launch stream)."""
        return self._timed(lambda ms: self.eng.lib.ryd_run_batch_device(
            self.eng.handle, self.slot, ctypes.byref(self.desc), self.d_params, self.n, self.n,
            self.d_state, 4 * self.n, self.d_summary, self.n, self.d_status, None, ms), timed)

    def fetch(self) -> EngineResult:
        return self._fetch_summary_run(self.evolution, self.dim)


class ScheduleDeviceBatch(_DeviceBuffers):
    """A schedule run (ryd_run_schedule_device) with parameters and table resident in HBM on
    one device slot, for timed re-runs; ``sched`` as ``Engine.run_schedule`` takes it."""

    def __init__(self, engine: Engine, params: np.ndarray, sched: np.ndarray, slot: int = 0,
                 states: bool = True):
        super().__init__(engine, slot)
        params = param_block(params)
        self.n = n = params.shape[1]
        self.desc, tab, self.ld_sched = schedule_desc(params, sched)
        self.width = N.STATE_WIDTH["lindblad"]
        self.d_params = self._upload(params)
        self.d_sched = self._upload(tab)
        self._alloc_summary_run(n, states)

    def launch(self, timed: bool = False) -> float:
        """Enqueue one propagation of the whole batch; with ``timed`` wait and return the
        kernel's device time (HIP events on the launch stream)."""
        return self._timed(lambda ms: self.eng.lib.ryd_run_schedule_device(
            self.eng.handle, self.slot, ctypes.byref(self.desc), self.d_params, self.n, self.n,
            self.d_sched, self.ld_sched, self.d_state, 4 * self.n, self.d_summary, self.n, self.d_status, None,
            ms), timed)

    def fetch(self) -> EngineResult:
        return self._fetch_summary_run("lindblad", 3)


class ScheduleKetDeviceBatch(_DeviceBuffers):
    """A noise-free schedule run as kets (ryd_run_schedule_kets_device) with parameters and table
    resident in HBM on one device slot, for timed re-runs, in the manner of
    ``ScheduleDeviceBatch``; ``sched``, ``states`` and ``jacobian`` as
    ``Engine.run_schedule_kets`` takes them."""

    def __init__(self, engine: Engine, params: np.ndarray, sched: np.ndarray, slot: int = 0,
                 states: bool = True, jacobian: Union[bool, str] = False):
        super().__init__(engine, slot)
        self.controls = jacobian_mode(jacobian)         # "controls": ryd_run_schedule_kets_ctl_device
        self.jacobian = jacobian                        # False: no buffer, NULL is passed
        params = param_block(params)
        self.n = n = params.shape[1]
        self.desc, tab, self.ld_sched = schedule_desc(params, sched)
        self.width = N.STATE_WIDTH["ket"]
        self.ld_jac = (4 if self.controls else 1) * N.SC_NFIELD * self.desc.n_seg
        self.d_params = self._upload(params)
        self.d_sched = self._upload(tab)
        self._alloc_summary_run(n, states)
        self.d_jac = self._alloc(8 * self.ld_jac * n) if jacobian else None

    def launch(self, timed: bool = False) -> float:
        """Enqueue one propagation of the whole batch; with ``timed`` wait and return the
        kernel's device time (HIP events on the launch stream)."""
        lib = self.eng.lib
        fn = lib.ryd_run_schedule_kets_ctl_device if self.controls else lib.ryd_run_schedule_kets_device
        return self._timed(lambda ms: fn(
            self.eng.handle, self.slot, ctypes.byref(self.desc), self.d_params, self.n, self.n,
            self.d_sched, self.ld_sched, self.d_state, 4 * self.n, self.d_summary, self.n,
            self.d_jac, self.ld_jac, self.d_status, None, ms), timed)

    def fetch(self) -> EngineResult:
        jac = None
        if self.jacobian:
            jac = self._download(np.zeros(jacobian_shape(self.n, self.desc.n_seg, self.controls)), self.d_jac)
        return self._fetch_summary_run("ket", 3, jac=jac, controls=self.controls)


class DeviceSweep(_DeviceBuffers):
    """A sweep whose parameters never exist on the host: its varying input fields are
    resident on one device slot (``upload``), ``ryd_derive_device`` writes the parameter
    block in HBM and the propagation kernel reads it there (C4: 1M species x T x
    P_tweezer points -> derive + engine on the device).  ``launch`` enqueues derive then
    engine on the slot's stream."""

    def __init__(self, engine: Engine, inp, evolution: str = "lindblad", slot: int = 0,
                 n_steps: Optional[int] = None, method: str = "chebyshev", states: bool = True):
        super().__init__(engine, slot)
        self.inp = inp
        self.n = n = inp.n
        self.dim = inp.dim
        self.width = N.STATE_WIDTH_DIM[inp.dim][evolution]
        self.evolution = evolution
        if n_steps is None:
            n_steps = {"smooth_jp": 300, "lp_shaped": 500}.get(inp.protocol, 0)
            if inp.protocol == "bangbang":
                n_steps = int(inp.desc.bb_nseg)
        # every shared rate is equal on both atoms (the derivation writes atom B = atom A)
        self.desc = make_desc(inp.protocol, evolution, n_steps, inp.shape, True, method, dim=inp.dim)
        self.k = inp.cols.shape[0]
        self.d_in = self._alloc(8 * self.k * n)
        self.d_params = self._alloc(8 * N.NPARAM * n)
        self.d_warn = self._alloc(4 * n)
        self._alloc_summary_run(n, states)
        self.upload()

    def upload(self):
        """H2D of the varying input fields (the only per-point host data)."""
        if self.k:
            self._upload(np.ascontiguousarray(self.inp.cols, dtype=np.float64), self.d_in)

    def derive(self, timed: bool = False) -> float:
        return self._timed(lambda ms: self.eng.lib.ryd_derive_device(
            self.eng.handle, self.slot, ctypes.byref(self.inp.desc), self.d_in if self.k else None, self.n,
            self.n, self.d_params, self.n, self.d_warn, None, self.n, None, ms), timed)

    def propagate(self, timed: bool = False) -> float:
        return self._timed(lambda ms: self.eng.lib.ryd_run_batch_device(
            self.eng.handle, self.slot, ctypes.byref(self.desc), self.d_params, self.n, self.n,
            self.d_state, 4 * self.n, self.d_summary, self.n, self.d_status, None, ms), timed)

    def launch(self):
        self.derive()
        self.propagate()

    def fetch_params(self) -> Tuple[np.ndarray, np.ndarray]:
        return (self._download(np.zeros((N.NPARAM, self.n)), self.d_params),
                self._download(np.zeros(self.n, dtype=np.uint32), self.d_warn))

    def fetch(self) -> EngineResult:
        _, warn = self.fetch_params()
        return self._fetch_summary_run(self.evolution, self.dim, status_or=warn)


class CoherenceDeviceBatch(_DeviceBuffers):
    """Process-map coherence sectors (ryd_run_coherences_device: one launch of the dim-3 or
    dim-4 coherence kernel) with inputs resident in HBM, for timed re-runs."""

    def __init__(self, engine: Engine, params: np.ndarray, protocol: str, n_steps: Optional[int] = None,
                 shape: str = "square", slot: int = 0, dim: int = 3):
        super().__init__(engine, slot)
        params = np.ascontiguousarray(params, dtype=np.float64)
        check_coherence_dim(params, dim)
        self.dim = dim
        self.n = n = params.shape[1]
        if n_steps is None:
            n_steps = default_n_steps(protocol, params)
        self.desc = make_desc(protocol, "lindblad", n_steps, shape, symmetric_atoms(params), "cheb_vector",
                              dim=dim)
        self.d_params = self._upload(params)
        self.d_coh = self._alloc(8 * N.NCOH * n)
        self.d_status = self._alloc(4 * n)

    def launch(self, timed: bool = False) -> float:
        return self._timed(lambda ms: self.eng.lib.ryd_run_coherences_device(
            self.eng.handle, self.slot, ctypes.byref(self.desc), self.d_params, self.n, self.n,
            self.d_coh, self.n, self.d_status, None, ms), timed)

    def fetch(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._fetch_coherences()


class ScheduleCoherenceDeviceBatch(_DeviceBuffers):
    """The coherence sectors of a schedule (ryd_run_schedule_coherences_device) with parameters
    and table resident in HBM on one device slot, for timed re-runs: the interface of
    ``CoherenceDeviceBatch``, ``sched`` as ``Engine.run_schedule_coherences`` takes it."""

    def __init__(self, engine: Engine, params: np.ndarray, sched: np.ndarray, slot: int = 0):
        super().__init__(engine, slot)
        params, self.desc, tab, self.ld_sched = schedule_coherence_inputs(params, sched)
        self.dim = 3
        self.n = n = params.shape[1]
        self.d_params = self._upload(params)
        self.d_sched = self._upload(tab)
        self.d_coh = self._alloc(8 * N.NCOH * n)
        self.d_status = self._alloc(4 * n)

    def launch(self, timed: bool = False) -> float:
        return self._timed(lambda ms: self.eng.lib.ryd_run_schedule_coherences_device(
            self.eng.handle, self.slot, ctypes.byref(self.desc), self.d_params, self.n, self.n,
            self.d_sched, self.ld_sched, self.d_coh, self.n, self.d_status, None, ms), timed)

    def fetch(self) -> Tuple[np.ndarray, np.ndarray]:
        return self._fetch_coherences()
