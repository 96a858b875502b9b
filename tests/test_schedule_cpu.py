"""CPU side of the pulse-schedule path: the C-ABI names and refusals (no device is touched),
the table builders against the oracle's own segment lists, and derive_batch on
PulseScheduleInputs."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import configurations as CF
from noisyquantumsimulator_amd import physics as PH
from noisyquantumsimulator_amd import pulse_schedules as PS
from oracle import lindblad_oracle as O
from tests import sched_points as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3


def test_header_binding_and_symbols():
    with open(os.path.join(REPO, "include", "ryd_engine.h")) as f:
        h = f.read()
    defs = dict(re.findall(r"#define\s+(RYD_[A-Z0-9_]+)\s+(-?\d+)u?", h))
    for k, v in N.SC.items():
        assert int(defs["RYD_SC_" + k]) == v
    assert int(defs["RYD_SC_NFIELD"]) == N.SC_NFIELD == len(N.SC)
    assert int(defs["RYD_SCHED_SHARED"]) == N.RYD_SCHED_SHARED
    assert int(defs["RYD_SCHED_MAX_SEG"]) == N.SCHED_MAX_SEG == 4096
    assert N.RYD_SCHED_SHARED & N.FLAG_SYMMETRIC_ATOMS == 0
    assert int(defs["RYD_ABI_VERSION"]) == 5                      # additive: the version stays
    assert ctypes.sizeof(N.SchedDesc) == 16 and ctypes.sizeof(N.BatchDesc) == 56
    m = re.search(r"typedef struct ryd_sched_desc \{(.*?)\} ryd_sched_desc;", h, re.S)
    assert re.findall(r"u?int32_t\s+(\w+);", m.group(1)) == [f[0] for f in N.SchedDesc._fields_]
    lib = N.load()
    for name in ("ryd_run_schedule", "ryd_run_schedule_device"):
        assert name in N.EXPORTED and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, h)


def _call(lib, n_seg=2, dim=3, flags=N.FLAG_SYMMETRIC_ATOMS, ld=None, abi=N.RYD_ABI_VERSION, table=True, desc=True):
    d = N.SchedDesc(abi, dim, n_seg, flags)
    tab = np.zeros(4 * 4097)
    dp = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = lib.ryd_run_schedule(None, ctypes.byref(d) if desc else None, None, 1, 1, dp if table else None,
                              4 * n_seg if ld is None else ld, None, 4, None, 1, None, None)
    return rc, lib.ryd_last_error().decode()


def test_refusals_need_no_device():
    lib = N.load()
    assert _call(lib)[0] == INVALID and "handle" in _call(lib)[1]            # everything else in order
    assert _call(lib, desc=False)[0] == INVALID
    assert _call(lib, table=False)[0] == INVALID
    assert _call(lib, abi=4)[0] == INVALID
    for n_seg in (0, -1, 4097):
        rc, msg = _call(lib, n_seg=n_seg, ld=4 * 4097)
        assert rc == INVALID and "n_seg" in msg
    assert _call(lib, n_seg=4096)[0] == INVALID and "handle" in _call(lib, n_seg=4096)[1]
    rc, msg = _call(lib, n_seg=5, ld=19)
    assert rc == INVALID and "ld_sched" in msg
    # a shared table ignores ld_sched
    assert "handle" in _call(lib, n_seg=5, ld=0, flags=N.FLAG_SYMMETRIC_ATOMS | N.RYD_SCHED_SHARED)[1]
    assert _call(lib, flags=N.FLAG_SYMMETRIC_ATOMS | 4)[0] == INVALID
    rc, msg = _call(lib, dim=4)
    assert rc == UNSUPPORTED and "dim" in msg
    rc, msg = _call(lib, flags=0)
    assert rc == UNSUPPORTED and "identical atoms" in msg
    d = N.SchedDesc(N.RYD_ABI_VERSION, 4, 2, N.FLAG_SYMMETRIC_ATOMS)
    assert lib.ryd_run_schedule_device(None, 0, ctypes.byref(d), None, 1, 1, None, 8, None, 4, None, 1, None, None,
                                       None) == INVALID                       # handle / slot first, as the other *_device calls
    # the batch entry points still refuse protocol values above 3
    bd = N.BatchDesc(N.RYD_ABI_VERSION, 3, 4, 0, 0, 0, 1, 1, 1e-10, 1e-12, 10)
    assert lib.ryd_batch_path(ctypes.byref(bd), 1) == INVALID


# ---- the builders against oracle.segments()
OM, V, D1 = 2 * np.pi * 3.7e6, 2 * np.pi * 3.7e6 * 41.3, 2 * np.pi * 1.3e5


def _check_table(tab, spec, what, t_scale, angle_scale=np.pi):
    """Every segment of positive length against the oracle's list, each quantity to 1e-15
    relative to the scale the oracle itself rounded it at: the diagonal of H and |Omega_s|
    element by element; the duration against `t_scale`, the largest time of the pulse (the
    oracle's bang-bang dt is a difference of bounds, each rounded at its own size); the drive's
    phase against `angle_scale`, the largest angle that enters it (smooth JP: the modulation
    angle omega_mod t - phi_offset, whose product is rounded at up to omega_mod tau, ~14 rad,
    before the cosine; a table in units of Omega cannot repeat that rounding).  Measured with
    every denominator the element itself: 1.7e-15 on smooth JP's phases (17 steps), below
    3e-16 everywhere else."""
    segs = O.segments(spec)
    live = [c for c in tab.T if c[0] != 0.0]
    assert len(live) == len(segs), what
    worst_d = worst_m = worst_p = worst_t = 0.0
    off = ~np.eye(9, dtype=bool)
    for (x, a, ph, d), (H, t, _) in zip(live, segs):
        Ht = O.two_atom_hamiltonian(a * OM * np.exp(1j * ph), d * OM, V, 3, delta_zeeman=D1)
        nz = H != 0
        assert np.array_equal(nz, Ht != 0), what
        dg = np.diag(nz)
        worst_d = max(worst_d, float((np.abs(np.diag(Ht - H))[dg] / np.abs(np.diag(H))[dg]).max()))
        ratio = Ht[nz & off] / H[nz & off]
        worst_m = max(worst_m, float(np.abs(np.abs(ratio) - 1).max()))
        worst_p = max(worst_p, float(np.abs(np.angle(ratio)).max()) / angle_scale)
        worst_t = max(worst_t, abs(x / OM - (t[-1] - t[0])) / t_scale)
    print(f"{what}: diagonal {worst_d:.2e}, |Omega| {worst_m:.2e}, phase {worst_p:.2e}, dt {worst_t:.2e}")
    assert max(worst_d, worst_m, worst_p, worst_t) <= 1e-15, (what, worst_d, worst_m, worst_p, worst_t)


def test_from_lp_square_reproduces_segments():
    dom, ot, xi = 0.377371, 4.29268, np.exp(2.38j)
    tab = PS.from_lp_square(dom, ot, xi)
    assert tab.shape == (4, 2)
    spec = O.PointSpec(protocol="lp_square", Omega=OM, V=V, Delta=dom * OM, tau=ot / OM, xi=xi, delta_zeeman=D1)
    _check_table(tab, spec, "lp_square", ot / OM)


def test_from_bangbang_reproduces_segments():
    st, ph, ot = [3.1, 7.9, 7.9, 15.2], [0.3, -1.1, 0.7, 2.9, -2.2], 22.08
    tab = PS.from_bangbang(st, ph, ot)
    assert tab.shape == (4, 5) and tab[N.SC["X"], 2] == 0.0               # the zero-length segment
    spec = O.PointSpec(protocol="bangbang", Omega=OM, V=V, omega_tau=ot, switching_times=st, phases=ph,
                       delta_zeeman=D1)
    _check_table(tab, spec, "bangbang", ot / OM)
    with pytest.raises(ValueError):
        PS.from_bangbang(st, ph[:-1], ot)


@pytest.mark.parametrize("n_steps", [1, 17, 300])
def test_from_smooth_jp_reproduces_segments(n_steps):
    A, omr, pho, ot, dom = 0.311 * np.pi, 1.242, 4.696, 7.61, -0.0205
    tab = PS.from_smooth_jp(A, omr, pho, ot, dom, n_steps)
    assert tab.shape == (4, n_steps)
    spec = O.PointSpec(protocol="smooth_jp", Omega=OM, V=V, Delta=dom * OM, tau=ot / OM, A=A, omega_mod=omr * OM,
                       phi_offset=pho, n_steps=n_steps, delta_zeeman=D1)
    _check_table(tab, spec, f"smooth_jp {n_steps}", ot / OM, angle_scale=omr * ot + pho)


def test_builders_broadcast_and_validate():
    t = PS.from_smooth_jp(0.9, 1.2, np.array([4.6, 4.7, 4.8]), 7.6, -0.02, 17)
    assert t.shape == (3, 4, 17)
    np.testing.assert_array_equal(t[1], PS.from_smooth_jp(0.9, 1.2, 4.7, 7.6, -0.02, 17))
    f = PS.from_functions(lambda u: np.sin(np.pi * u / 6.0) ** 2, 0.25, lambda u: 0.1 * (u - 3.0), 6.0, 12)
    assert f.shape == (4, 12) and np.allclose(f[N.SC["X"]].sum(), 6.0)
    np.testing.assert_allclose(f[N.SC["AMP"], 0], np.sin(np.pi * 0.25 / 6.0) ** 2, rtol=1e-15)
    assert np.all(f[N.SC["PHASE"]] == 0.25)
    for bad in (np.zeros((3, 5)), np.zeros((4, 0)), np.zeros((4, 4097)), np.full((4, 2), np.nan)):
        with pytest.raises(ValueError):
            PS.validate_schedule(bad)
    neg = PS.assemble([1.0, 1.0], 1.0, 0.0, 0.0)
    for field in ("X", "AMP"):
        s = neg.copy()
        s[N.SC[field], 1] = -1e-9
        with pytest.raises(ValueError):
            PS.validate_schedule(s)
    with pytest.raises(ValueError):
        PS.validate_schedule(np.zeros((2, 4, 3)), n=3)


# ---- derive_batch(PulseScheduleInputs)
def test_derive_batch_schedule():
    warnings.simplefilter("ignore")
    kw = dict(temperature=np.linspace(1e-6, 4e-6, 4), include_noise=True)
    x = np.array([0.5, 0.0, 1.25, 2.0])
    bs = PH.derive_batch(CF.PulseScheduleInputs(x=x, amp=[1, 0.5, 0, 1], phase=0.3, delta=-0.1), **kw)
    bj = PH.derive_batch(CF.JPSimulationInputs(omega_tau=float(x.sum())), **kw)
    assert bs.protocol == "pulse_schedule" and bs.n == 4 and bs.schedule.shape == (4, 4)
    # the same formulas: everything but the protocol's own columns
    for k, v in bj.cols.items():
        np.testing.assert_array_equal(bs.cols[k], v, err_msg=k)
    np.testing.assert_array_equal(bs.cols["tau_total"], x.sum() / bs.cols["Omega"])
    np.testing.assert_array_equal(bs.status_bits, bj.status_bits)
    # per-point tables: n from the table, tau_total per point
    xp = np.array([[0.5, 1.0], [2.0, 3.0], [0.25, 0.25]])
    bp = PH.derive_batch(CF.PulseScheduleInputs(x=xp))
    assert bp.n == 3 and bp.schedule.shape == (3, 4, 2)
    np.testing.assert_array_equal(bp.cols["tau_total"], xp.sum(axis=1) / bp.cols["Omega"])
    np.testing.assert_array_equal(bp.schedule[:, N.SC["AMP"]], 1.0)
    t = PS.from_smooth_jp(0.9, 1.2, 4.7, 7.6, -0.02, 17)
    np.testing.assert_array_equal(PH.derive_batch(CF.PulseScheduleInputs.from_table(t)).schedule, t)
    from noisyquantumsimulator_amd import engine as E
    prm = E.pack_params(bs)
    assert prm.shape == (N.NPARAM, 4) and E.symmetric_atoms(prm) and np.all(prm[N.P["TAU"]:N.P["GMJ_A"]] == 0)
    for bad in (dict(x=None), dict(x=[1.0, -1.0]), dict(x=[1.0], amp=[-0.5]), dict(x=[1.0], phase=[np.inf]),
                dict(x=np.ones((2, 3, 4)))):
        with pytest.raises(ValueError):
            PH.derive_batch(CF.PulseScheduleInputs(**bad))
    with pytest.raises(ValueError):
        PH.derive_batch(CF.PulseScheduleInputs(x=xp), 5)
    with pytest.raises(TypeError, match="simulation_inputs must be LPSimulationInputs"):
        PH.derive_batch(object())


def test_public_names():
    import noisyquantumsimulator_amd as Q
    assert Q.PulseScheduleInputs is CF.PulseScheduleInputs and Q.pulse_schedules is PS
    assert "PulseScheduleInputs" in Q.__all__ and "pulse_schedules" in Q.__all__
    assert hasattr(Q.Engine, "run_schedule")
    from noisyquantumsimulator_amd import engine as E
    assert hasattr(E, "ScheduleDeviceBatch")
