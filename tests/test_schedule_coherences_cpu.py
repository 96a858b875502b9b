"""CPU side of the schedule coherence path: the C-ABI names, the refusals that come before any
GPU call (through ctypes with a NULL handle: each reports its own reason), the Python names and
the input checks that precede the engine call.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from tests import sched_points as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
NAMES = ("ryd_run_schedule_coherences", "ryd_run_schedule_coherences_device")


def test_names_in_header_binding_and_library():
    with open(os.path.join(REPO, "include", "ryd_engine.h")) as f:
        h = f.read()
    lib = N.load()
    for name in NAMES:
        assert name in N.EXPORTED and hasattr(lib, name) and re.search(r"\bint %s\s*\(" % name, h)
    assert int(re.search(r"#define\s+RYD_ABI_VERSION\s+(\d+)", h).group(1)) == N.RYD_ABI_VERSION == 5
    # the argument lists: those of the schedule entry points with the coherence outputs
    assert len(lib.ryd_run_schedule_coherences.argtypes) == 11
    assert len(lib.ryd_run_schedule_coherences_device.argtypes) == 13


def _call(lib, n_seg=2, dim=3, flags=N.FLAG_SYMMETRIC_ATOMS, ld=None, abi=N.RYD_ABI_VERSION, table=True, desc=True,
          ld_coh=1):
    d = N.SchedDesc(abi, dim, n_seg, flags)
    tab = np.zeros(4 * 4097)
    dp = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = lib.ryd_run_schedule_coherences(None, ctypes.byref(d) if desc else None, None, 1, 1, dp if table else None,
                                         4 * n_seg if ld is None else ld, None, ld_coh, None, None)
    return rc, lib.ryd_last_error().decode()


def test_refusals_need_no_device():
    lib = N.load()
    rc, msg = _call(lib)                             # everything else in order: the handle is what is missing
    assert rc == INVALID and "handle" in msg
    rc, msg = _call(lib, desc=False)
    assert rc == INVALID and "desc" in msg
    rc, msg = _call(lib, table=False)
    assert rc == INVALID and "table" in msg
    rc, msg = _call(lib, abi=4)
    assert rc == INVALID and "abi_version" in msg
    for n_seg in (0, 4097):
        rc, msg = _call(lib, n_seg=n_seg, ld=4 * 4097)
        assert rc == INVALID and "n_seg" in msg
    assert "handle" in _call(lib, n_seg=4096)[1]
    rc, msg = _call(lib, flags=N.FLAG_SYMMETRIC_ATOMS | 4)
    assert rc == INVALID and "flag" in msg
    rc, msg = _call(lib, dim=4)
    assert rc == UNSUPPORTED and "dim" in msg
    rc, msg = _call(lib, flags=0)
    assert rc == UNSUPPORTED and "identical atoms" in msg
    rc, msg = _call(lib, n_seg=5, ld=19)
    assert rc == INVALID and "ld_sched" in msg
    assert "handle" in _call(lib, n_seg=5, ld=0, flags=N.FLAG_SYMMETRIC_ATOMS | N.RYD_SCHED_SHARED)[1]
    rc, msg = _call(lib, ld_coh=0)
    assert rc == INVALID and "leading dimension" in msg
    # the descriptor before the leading dimension: dim = 4 with ld_coh too small is "dim"
    assert "dim" in _call(lib, dim=4, ld_coh=0)[1]
    # the device form: handle / slot first, as the other *_device calls
    d = N.SchedDesc(N.RYD_ABI_VERSION, 3, 2, N.FLAG_SYMMETRIC_ATOMS)
    assert lib.ryd_run_schedule_coherences_device(None, 0, ctypes.byref(d), None, 1, 1, None, 8, None, 1, None, None,
                                                  None) == INVALID


def test_public_names():
    import noisyquantumsimulator_amd as Q
    from noisyquantumsimulator_amd import noise_models as NM
    assert Q.schedule_process_maps is NM.schedule_process_maps and "schedule_process_maps" in Q.__all__
    assert Q.ScheduleCoherenceDeviceBatch is E.ScheduleCoherenceDeviceBatch
    assert "ScheduleCoherenceDeviceBatch" in Q.__all__
    assert hasattr(Q.Engine, "run_schedule_coherences")
    for m in ("launch", "mark", "mark_elapsed", "synchronize", "fetch", "free"):    # CoherenceDeviceBatch's
        assert hasattr(E.CoherenceDeviceBatch, m) and hasattr(E.ScheduleCoherenceDeviceBatch, m)


def test_input_checks_before_the_engine_call():
    """What Engine.run_schedule_coherences and ScheduleCoherenceDeviceBatch check before they
    call the library (engine.schedule_coherence_inputs; Engine() itself needs a GPU)."""
    b = SP.batch("random")
    p, s = b["params"], b["sched"]
    prm, desc, tab, ld = E.schedule_coherence_inputs(p, s)
    assert prm.shape == p.shape and tab.shape == s.shape and ld == 4 * s.shape[-1]
    assert desc.dim == 3 and desc.n_seg == s.shape[-1] and desc.flags == N.FLAG_SYMMETRIC_ATOMS
    assert E.schedule_coherence_inputs(p, s[0])[1].flags == N.FLAG_SYMMETRIC_ATOMS | N.RYD_SCHED_SHARED
    for bad in (s[:5], s[:, :3], np.zeros((4, 0)), np.zeros((4, 4097)), s[0, 0]):    # table shape
        with pytest.raises(ValueError):
            E.schedule_coherence_inputs(p, bad)
    with pytest.raises(ValueError):
        E.schedule_coherence_inputs(p[:-1], s)
    q = p.copy()
    q[N.P["GSC_B"], 2] *= 2
    with pytest.raises(ValueError, match="identical atoms"):
        E.schedule_coherence_inputs(q, s)
    for col in ("GMJ_A", "GMJ_B"):
        q = p.copy()
        q[N.P["GMJ_A"], 1] = q[N.P["GMJ_B"], 1] = 10.0          # equal atoms, nonzero mJ rates
        with pytest.raises(ValueError, match="GMJ"):
            E.schedule_coherence_inputs(q, s)
        q[N.P[col], 1] = 0.0
        with pytest.raises(ValueError):
            E.schedule_coherence_inputs(q, s)
