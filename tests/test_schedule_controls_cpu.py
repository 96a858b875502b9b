"""CPU side of the control Jacobian (ryd_run_schedule_kets_ctl): the C-ABI names and refusals, none
of which touches a device, the result type's new field, and the argument checks of
``gate_fidelity_and_gradient`` and ``optimize_schedule``."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import pulse_schedules as PS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
NAMES = ("ryd_run_schedule_kets_ctl", "ryd_run_schedule_kets_ctl_device")


def test_header_binding_and_symbols():
    with open(os.path.join(REPO, "include", "ryd_engine.h")) as f:
        h = f.read()
    defs = dict(re.findall(r"#define\s+(RYD_[A-Z0-9_]+)\s+(-?\d+)u?", h))
    assert int(defs["RYD_ABI_VERSION"]) == N.RYD_ABI_VERSION == 5     # additive: the version stays
    assert [int(defs["RYD_SC_" + f]) for f in ("X", "AMP", "PHASE", "DELTA")] == [0, 1, 2, 3]
    lib = N.load()
    for name, base in zip(NAMES, ("ryd_run_schedule_kets", "ryd_run_schedule_kets_device")):
        assert name in N.EXPORTED and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, h)
        # the arguments of the phase-only entry point, in its order
        proto = re.search(r"\b%s\s*\((.*?)\);" % name, h, re.S).group(1)
        old = re.search(r"\b%s\s*\((.*?)\);" % base, h, re.S).group(1)
        assert [a.split() for a in proto.split(",")] == [a.split() for a in old.split(",")]
        assert list(getattr(lib, name).argtypes) == list(getattr(lib, base).argtypes)


def _call(lib, n_seg=2, dim=3, flags=N.FLAG_SYMMETRIC_ATOMS, ld=None, abi=N.RYD_ABI_VERSION, table=True, desc=True,
          jac=True, ld_jac=None):
    d = N.SchedDesc(abi, dim, n_seg, flags)
    tab = np.zeros(4 * 4097)
    dp = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    jb = np.zeros(16)
    jp = jb.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = lib.ryd_run_schedule_kets_ctl(None, ctypes.byref(d) if desc else None, None, 1, 1, dp if table else None,
                                       4 * n_seg if ld is None else ld, None, 4, None, 1, jp if jac else None,
                                       16 * n_seg if ld_jac is None else ld_jac, None, None)
    return rc, lib.ryd_last_error().decode()


def test_refusals_need_no_device():
    lib = N.load()
    assert _call(lib)[0] == INVALID and "handle" in _call(lib)[1]            # everything else in order
    # validate_schedule_kets' rules, the descriptor first
    assert _call(lib, desc=False)[0] == INVALID and "desc" in _call(lib, desc=False)[1]
    assert _call(lib, table=False)[0] == INVALID and "table" in _call(lib, table=False)[1]
    assert _call(lib, abi=4)[0] == INVALID and "abi_version" in _call(lib, abi=4)[1]
    for n_seg in (0, -1, 4097):
        rc, msg = _call(lib, n_seg=n_seg, ld=4 * 4097)
        assert rc == INVALID and "n_seg" in msg
    assert "handle" in _call(lib, n_seg=4096)[1]
    rc, msg = _call(lib, n_seg=5, ld=19)
    assert rc == INVALID and "ld_sched" in msg
    assert "handle" in _call(lib, n_seg=5, ld=0, flags=N.FLAG_SYMMETRIC_ATOMS | N.RYD_SCHED_SHARED)[1]
    rc, msg = _call(lib, flags=N.FLAG_SYMMETRIC_ATOMS | 4)
    assert rc == INVALID and "flag" in msg
    rc, msg = _call(lib, dim=4)
    assert rc == UNSUPPORTED and "dim" in msg
    rc, msg = _call(lib, flags=0)
    assert rc == UNSUPPORTED and "identical atoms" in msg


def test_jacobian_is_required_and_sixteen_wide():
    lib = N.load()
    rc, msg = _call(lib, n_seg=5, jac=False)
    assert rc == INVALID and "Jacobian is NULL" in msg
    for ld_jac in (79, 20, 0, -1):                       # 4 n_seg, the phase-only width, is too small
        rc, msg = _call(lib, n_seg=5, ld_jac=ld_jac)
        assert rc == INVALID and "ld_jac" in msg and "16" in msg, ld_jac
    assert "handle" in _call(lib, n_seg=5, ld_jac=80)[1]
    assert "handle" in _call(lib, n_seg=5, ld_jac=83)[1]
    # the descriptor's own reason comes before the Jacobian's
    rc, msg = _call(lib, n_seg=0, jac=False)
    assert rc == INVALID and "n_seg" in msg
    # a shared table does not excuse the Jacobian's leading dimension
    rc, msg = _call(lib, n_seg=5, ld=0, flags=N.FLAG_SYMMETRIC_ATOMS | N.RYD_SCHED_SHARED, ld_jac=79)
    assert rc == INVALID and "ld_jac" in msg


def test_leading_dimensions():
    lib = N.load()
    d = N.SchedDesc(N.RYD_ABI_VERSION, 3, 2, N.FLAG_SYMMETRIC_ATOMS)
    buf = np.zeros(64)
    dp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call(n=2, ldp=2, lds=8, ldm=2, state=True):
        rc = lib.ryd_run_schedule_kets_ctl(None, ctypes.byref(d), None, n, ldp, dp, 8, dp if state else None, lds,
                                           None, ldm, dp, 32, None, None)
        return rc, lib.ryd_last_error().decode()
    assert "handle" in call()[1]
    for kw in (dict(n=-1), dict(ldp=1), dict(lds=7), dict(ldm=1)):
        rc, msg = call(**kw)
        assert rc == INVALID and "handle" not in msg, kw
    assert "handle" in call(lds=0, state=False)[1]       # summary-only: ld_state is ignored


def test_device_form_refuses_handle_and_slot_first():
    lib = N.load()
    d = N.SchedDesc(N.RYD_ABI_VERSION, 4, 2, N.FLAG_SYMMETRIC_ATOMS)          # dim 4 would be UNSUPPORTED
    rc = lib.ryd_run_schedule_kets_ctl_device(None, 0, ctypes.byref(d), None, 1, 1, None, 8, None, 4, None, 1, None,
                                              0, None, None, None)
    assert rc == INVALID and "handle" in lib.ryd_last_error().decode()


def test_engine_result_still_constructs_positionally():
    z = np.zeros((N.NSUMMARY, 1))
    r = E.EngineResult("ket", 1, None, z, np.zeros(1, np.uint32), 0.0, 0.0, 0.0, 0.0, 0.0)
    assert r.dim == 3 and r.phase_jacobian is None and r.control_jacobian is None
    J = np.zeros((1, 2, 3), complex)
    r = E.EngineResult("ket", 1, None, z, np.zeros(1, np.uint32), 0.0, 0.0, 0.0, 0.0, 0.0, 3, J)
    assert r.dim == 3 and r.phase_jacobian is J and r.control_jacobian is None
    C = np.zeros((1, 4, 2, 3), complex)
    r = E.EngineResult("ket", 1, None, z, np.zeros(1, np.uint32), 0.0, 0.0, 0.0, 0.0, 0.0, 3, J, control_jacobian=C)
    assert r.control_jacobian is C
    raw = np.arange(2 * 4 * 4 * 3.0).reshape(2, 4, 4, 3)
    c = E.complex_control_jacobian(raw)
    assert c.shape == (2, 4, 2, 3) and c[1, 3, 1, 2] == raw[1, 3, 2, 2] + 1j * raw[1, 3, 3, 2]
    # a field's block is the phase-only layout
    np.testing.assert_array_equal(c[:, N.SC["PHASE"]], E.complex_jacobian(raw[:, N.SC["PHASE"]]))


def test_public_names_and_modes():
    import noisyquantumsimulator_amd as Q
    assert Q.pulse_schedules.optimize_schedule is PS.optimize_schedule
    assert E.jacobian_mode(False) is False and E.jacobian_mode(True) is False and E.jacobian_mode("controls") is True
    for bad in ("phase", "control", None, 2):
        with pytest.raises(ValueError, match="controls"):
            E.jacobian_mode(bad)
    sig = inspect.signature(PS.optimize_schedule)
    kw = {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY}
    assert kw == dict(free=("phase",), amp_max=None, duration_weight=0.0, which="avg_gate", maxiter=200, engine=None)
    assert list(sig.parameters)[:2] == ["params", "sched0"]
    assert PS.FIELDS == dict(x=N.SC["X"], amp=N.SC["AMP"], phase=N.SC["PHASE"], delta=N.SC["DELTA"])
    # optimize_phases is as it was
    sig = inspect.signature(PS.optimize_phases)
    assert sig.parameters["which"].default == "avg_gate" and sig.parameters["maxiter"].default == 200


def test_gate_fidelity_and_gradient_shapes():
    rng = np.random.default_rng(3)
    a01 = 0.9 * np.exp(1j * rng.uniform(-3, 3, 4))
    a11 = 0.8 * np.exp(1j * rng.uniform(-3, 3, 4))
    C = rng.normal(size=(4, 4, 2, 6)) + 1j * rng.normal(size=(4, 4, 2, 6))
    F, dF = PS.gate_fidelity_and_gradient(a01, a11, C)
    assert F.shape == (4,) and dF.shape == (4, 4, 6)
    for f in range(4):
        Ff, dFf = PS.gate_fidelity_and_gradient(a01, a11, C[:, f])
        np.testing.assert_array_equal(F, Ff)
        np.testing.assert_array_equal(dF[:, f], dFf)
    for bad in (C[:, :3], C[:, :, :1], C[:3], C[0, :3], np.zeros((4, 4, 2, 6, 1))):
        with pytest.raises(ValueError, match="need a01"):
            PS.gate_fidelity_and_gradient(a01, a11, bad)
    with pytest.raises(ValueError, match="which"):
        PS.gate_fidelity_and_gradient(a01, a11, C, "state")


class _NoEngine:
    def run_schedule_kets(self, *a, **k):
        raise AssertionError("an argument error must come before any engine call")


def test_optimize_schedule_argument_errors():
    p = np.zeros((N.NPARAM, 2))
    s = PS.assemble(np.full(3, 0.5), 1.0, 0.0, 0.0)
    eng = _NoEngine()
    for free in ((), ("phase", "phase"), ("omega",), ("phase", "X"), "phase"):
        with pytest.raises(ValueError, match="free"):
            PS.optimize_schedule(p, s, free=free, engine=eng)
    for amp_max in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="amp_max"):
            PS.optimize_schedule(p, s, free=("amp",), amp_max=amp_max, engine=eng)
    with pytest.raises(ValueError, match="above amp_max"):
        PS.optimize_schedule(p, s, free=("amp",), amp_max=0.5, engine=eng)
    for w in (-1e-3, np.nan):
        with pytest.raises(ValueError, match="duration_weight"):
            PS.optimize_schedule(p, s, free=("x",), duration_weight=w, engine=eng)
    with pytest.raises(ValueError, match="which"):
        PS.optimize_schedule(p, s, which="state", engine=eng)
    with pytest.raises(ValueError):                      # the table's own checks
        PS.optimize_schedule(p, np.zeros((3, 4, 3)), engine=eng)
    with pytest.raises(AssertionError):                  # and a good call reaches the engine
        PS.optimize_schedule(p, s, free=("phase", "amp", "delta", "x"), amp_max=1.0, engine=eng)
