"""CPU side of the noise-free schedule path (ryd_run_schedule_kets): the C-ABI names and its
refusals, none of which touches a device, and the result type's new optional field."""
import ctypes
import inspect
import os
import re

import numpy as np

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import pulse_schedules as PS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
NAMES = ("ryd_run_schedule_kets", "ryd_run_schedule_kets_device")


def test_header_binding_and_symbols():
    with open(os.path.join(REPO, "include", "ryd_engine.h")) as f:
        h = f.read()
    defs = dict(re.findall(r"#define\s+(RYD_[A-Z0-9_]+)\s+(-?\d+)u?", h))
    assert int(defs["RYD_ABI_VERSION"]) == N.RYD_ABI_VERSION == 5     # additive: the version stays
    lib = N.load()
    for name in NAMES:
        assert name in N.EXPORTED and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, h)
        assert getattr(lib, name).argtypes is not None
    # (jac, ld_jac) sit between the summary and the status in both forms
    for name in NAMES:
        proto = re.search(r"\b%s\s*\((.*?)\);" % name, h, re.S).group(1)
        args = [a.split()[-1].lstrip("*") for a in proto.split(",")]
        i = args.index("ld_summary")
        assert args[i + 1].endswith("jac") and args[i + 2] == "ld_jac" and args[i + 3].endswith("status")
        assert len(getattr(lib, name).argtypes) == len(args)


def _call(lib, n_seg=2, dim=3, flags=N.FLAG_SYMMETRIC_ATOMS, ld=None, abi=N.RYD_ABI_VERSION, table=True, desc=True,
          jac=False, ld_jac=0):
    d = N.SchedDesc(abi, dim, n_seg, flags)
    tab = np.zeros(4 * 4097)
    dp = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    jb = np.zeros(4 * 4097)
    jp = jb.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = lib.ryd_run_schedule_kets(None, ctypes.byref(d) if desc else None, None, 1, 1, dp if table else None,
                                   4 * n_seg if ld is None else ld, None, 4, None, 1, jp if jac else None, ld_jac,
                                   None, None)
    return rc, lib.ryd_last_error().decode()


def test_refusals_need_no_device():
    lib = N.load()
    assert _call(lib)[0] == INVALID and "handle" in _call(lib)[1]            # everything else in order
    # every rule of validate_schedule, the descriptor first
    assert _call(lib, desc=False)[0] == INVALID and "desc" in _call(lib, desc=False)[1]
    assert _call(lib, table=False)[0] == INVALID and "table" in _call(lib, table=False)[1]
    assert _call(lib, abi=4)[0] == INVALID and "abi_version" in _call(lib, abi=4)[1]
    for n_seg in (0, -1, 4097):
        rc, msg = _call(lib, n_seg=n_seg, ld=4 * 4097)
        assert rc == INVALID and "n_seg" in msg
    assert _call(lib, n_seg=4096)[0] == INVALID and "handle" in _call(lib, n_seg=4096)[1]
    rc, msg = _call(lib, n_seg=5, ld=19)
    assert rc == INVALID and "ld_sched" in msg
    # a shared table ignores ld_sched
    assert "handle" in _call(lib, n_seg=5, ld=0, flags=N.FLAG_SYMMETRIC_ATOMS | N.RYD_SCHED_SHARED)[1]
    rc, msg = _call(lib, flags=N.FLAG_SYMMETRIC_ATOMS | 4)
    assert rc == INVALID and "flag" in msg
    rc, msg = _call(lib, dim=4)
    assert rc == UNSUPPORTED and "dim" in msg
    rc, msg = _call(lib, flags=0)
    assert rc == UNSUPPORTED and "identical atoms" in msg


def test_leading_dimensions():
    lib = N.load()
    d = N.SchedDesc(N.RYD_ABI_VERSION, 3, 2, N.FLAG_SYMMETRIC_ATOMS)
    buf = np.zeros(64)
    dp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call(n=2, ldp=2, lds=8, ldm=2, state=True):
        rc = lib.ryd_run_schedule_kets(None, ctypes.byref(d), None, n, ldp, dp, 8, dp if state else None, lds, None,
                                       ldm, None, 0, None, None)
        return rc, lib.ryd_last_error().decode()
    assert "handle" in call()[1]
    for kw in (dict(n=-1), dict(ldp=1), dict(lds=7), dict(ldm=1)):
        rc, msg = call(**kw)
        assert rc == INVALID and "handle" not in msg, kw
    assert "handle" in call(lds=0, state=False)[1]       # summary-only: ld_state is ignored


def test_ld_jac_is_checked_only_with_a_jacobian():
    lib = N.load()
    rc, msg = _call(lib, n_seg=5, jac=True, ld_jac=19)
    assert rc == INVALID and "ld_jac" in msg
    assert "handle" in _call(lib, n_seg=5, jac=True, ld_jac=20)[1]
    assert "handle" in _call(lib, n_seg=5, jac=False, ld_jac=0)[1]
    assert "handle" in _call(lib, n_seg=5, jac=False, ld_jac=-7)[1]
    # the descriptor's own reason comes before the Jacobian's
    rc, msg = _call(lib, n_seg=0, jac=True, ld_jac=0)
    assert rc == INVALID and "n_seg" in msg
    # a shared table does not excuse the Jacobian's leading dimension
    rc, msg = _call(lib, n_seg=5, ld=0, flags=N.FLAG_SYMMETRIC_ATOMS | N.RYD_SCHED_SHARED, jac=True, ld_jac=19)
    assert rc == INVALID and "ld_jac" in msg


def test_device_form_refuses_handle_and_slot_first():
    lib = N.load()
    d = N.SchedDesc(N.RYD_ABI_VERSION, 4, 2, N.FLAG_SYMMETRIC_ATOMS)          # dim 4 would be UNSUPPORTED
    rc = lib.ryd_run_schedule_kets_device(None, 0, ctypes.byref(d), None, 1, 1, None, 8, None, 4, None, 1, None, 0,
                                          None, None, None)
    assert rc == INVALID and "handle" in lib.ryd_last_error().decode()


def test_engine_result_constructs_positionally():
    z = np.zeros((N.NSUMMARY, 1))
    r = E.EngineResult("ket", 1, None, z, np.zeros(1, np.uint32), 0.0, 0.0, 0.0, 0.0, 0.0)
    assert r.dim == 3 and r.phase_jacobian is None
    r = E.EngineResult("ket", 1, None, z, np.zeros(1, np.uint32), 0.0, 0.0, 0.0, 0.0, 0.0, 3)
    assert r.phase_jacobian is None
    names = [f for f in E.EngineResult.__dataclass_fields__]
    assert names[-2:] == ["dim", "phase_jacobian"]                             # the new field is the last
    J = np.arange(24.0).reshape(2, 4, 3)
    c = E.complex_jacobian(J)
    assert c.shape == (2, 2, 3) and c[1, 1, 2] == J[1, 2, 2] + 1j * J[1, 3, 2] and E.complex_jacobian(None) is None


def test_public_names():
    import noisyquantumsimulator_amd as Q
    assert Q.ScheduleKetDeviceBatch is E.ScheduleKetDeviceBatch and "ScheduleKetDeviceBatch" in Q.__all__
    sig = inspect.signature(E.Engine.run_schedule_kets)
    assert [(k, v.default) for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY] == \
        [("states", True), ("jacobian", False)]
    sig = inspect.signature(E.ScheduleKetDeviceBatch.__init__)
    assert list(sig.parameters)[1:] == ["engine", "params", "sched", "slot", "states", "jacobian"]
    assert sig.parameters["slot"].default == 0 and sig.parameters["jacobian"].default is False
    sig = inspect.signature(PS.optimize_phases)
    assert sig.parameters["which"].default == "avg_gate" and sig.parameters["maxiter"].default == 200
    assert inspect.signature(PS.gate_fidelity_and_gradient).parameters["which"].default == "avg_gate"
