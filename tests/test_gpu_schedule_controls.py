"""The control Jacobian of noise-free pulse schedules on the GPU (ryd_run_schedule_kets_ctl;
ket_sched_ctl_kernel): the derivatives of the two diagonal overlaps with respect to every
segment's duration, amplitude, phase and detuning against the CPU oracle
(tests/sched_ket_ctl_points.py: chained 9 x 9 ``expm`` and ``expm_frechet``), against the
phase-only and forward runs bit for bit, and the kernel's edges (the memo in both directions, rows
of a wave, launch shapes, refused rows, the step cap), then ``optimize_schedule`` on top.

Tolerance: the project's 1e-10 (tests/test_gpu_parity.py) on every element of the Jacobian in the
table's units; the measured maxima are printed.  Bit-for-bit comparisons between differently
composed waves leave out NMV_EXEC, as tests/test_gpu_schedule_kets.py does.
"""
import ctypes

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import pulse_schedules as PS
from tests import sched_ket_ctl_points as CP
from tests import sched_points as SP

pytestmark = pytest.mark.gpu

TOL = 1e-10
SC = N.SC
OWN = [i for name, i in N.S.items() if name != "NMV_EXEC"]
BAD, CAP = N.STATUS_BAD_INPUT, N.STATUS_STEP_CAP
FIELDS = ("X", "AMP", "PHASE", "DELTA")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype != np.complex128 else a.view(np.float64).view(np.uint64)


def _same(a, b, ia=slice(None), ib=slice(None), cols=OWN, what="", state=True):
    """Rows ia of run a and ib of run b: ket rows, summary columns `cols`, status, the phase
    Jacobian and (where both have one) the control Jacobian, bit for bit."""
    ia, ib = np.arange(a.n)[ia], np.arange(b.n)[ib]
    la = (4 * ia[:, None] + np.arange(4)).ravel()
    lb = (4 * ib[:, None] + np.arange(4)).ravel()
    if state:
        np.testing.assert_array_equal(_bits(a.state[:, la]), _bits(b.state[:, lb]), err_msg=f"{what}: state")
    for c in cols:
        np.testing.assert_array_equal(_bits(a.summary[c, ia]), _bits(b.summary[c, ib]),
                                      err_msg=f"{what}: summary column {c}")
    np.testing.assert_array_equal(a.status[ia], b.status[ib], err_msg=f"{what}: status")
    if a.phase_jacobian is not None and b.phase_jacobian is not None:
        np.testing.assert_array_equal(_bits(a.phase_jacobian[ia]), _bits(b.phase_jacobian[ib]),
                                      err_msg=f"{what}: phase Jacobian")
    if a.control_jacobian is not None and b.control_jacobian is not None:
        np.testing.assert_array_equal(_bits(a.control_jacobian[ia]), _bits(b.control_jacobian[ib]),
                                      err_msg=f"{what}: control Jacobian")


def _ctl(eng, p, s, **kw):
    r = eng.run_schedule_kets(p, s, jacobian="controls", **kw)
    assert r.control_jacobian.shape == (p.shape[1], 4, 2, s.shape[-1])
    np.testing.assert_array_equal(_bits(r.phase_jacobian), _bits(r.control_jacobian[:, SC["PHASE"]]))
    return r


def _field_errors(C, ref):
    return {f: float(np.abs(C[:, SC[f]] - ref[:, SC[f]]).max()) for f in FIELDS}


# ---- 1. against the oracle
@pytest.mark.parametrize("name", ("random", "lp_square", "bangbang", "smooth_jp") +
                         tuple(f"chunk{ns}" for ns in SP.CHUNK_NSEG) + CP.NEW)
def test_against_oracle(eng, name):
    b, ref = CP.batch(name), CP.reference(name)
    r = _ctl(eng, b["params"], b["sched"])
    assert np.all(r.status == 0), r.status
    kerr = float(np.abs(r.kets() - ref["kets"]).max())
    errs = _field_errors(r.control_jacobian, ref["C"])
    mags = {f: float(np.abs(ref["C"][:, SC[f]]).max()) for f in FIELDS}
    print(f"{name}: max|dpsi| = {kerr:.3e}, " +
          ", ".join(f"max|dJ_{f}| = {errs[f]:.3e} (of {mags[f]:.2g})" for f in FIELDS))
    assert kerr < TOL and max(errs.values()) < TOL, (name, kerr, errs)
    zero = b["sched"][:, SC["X"]] == 0.0                 # zero duration: exact zeros but in x
    for f in ("AMP", "PHASE", "DELTA"):
        sel = np.broadcast_to(zero[:, None], r.control_jacobian[:, SC[f]].shape)
        np.testing.assert_array_equal(_bits(r.control_jacobian[:, SC[f]][sel]), 0, err_msg=f"{name}: {f}")


# ---- 2. the same bits as the phase-only and the forward runs, in every form
def test_same_bits_across_forms(eng):
    b = CP.batch("random")
    p, s = np.ascontiguousarray(b["params"]), np.ascontiguousarray(b["sched"])
    n, ns = p.shape[1], s.shape[-1]
    ctl = _ctl(eng, p, s)
    jac = eng.run_schedule_kets(p, s, jacobian=True)
    fwd = eng.run_schedule_kets(p, s)
    assert jac.control_jacobian is None and fwd.control_jacobian is None
    _same(ctl, jac, cols=range(N.NSUMMARY), what="controls / phase only")
    _same(ctl, fwd, cols=range(N.NSUMMARY), what="controls / forward")
    lean = _ctl(eng, p, s, states=False)
    assert lean.state is None
    _same(lean, ctl, cols=range(N.NSUMMARY), what="summary-only", state=False)
    for states in (True, False):
        db = E.ScheduleKetDeviceBatch(eng, p, s, states=states, jacobian="controls")
        try:
            assert db.launch(timed=True) > 0.0
            got = db.fetch()
        finally:
            db.free()
        assert (got.state is None) == (not states)
        _same(got, ctl, cols=range(N.NSUMMARY), what=f"device-resident {states}", state=states)
    # the host form with padded Jacobian rows: the same numbers, the padding untouched
    desc, tab, ld = E.schedule_desc(p, s)
    ldj = 16 * ns + 5
    raw = np.full((n, ldj), -7.0)
    summ = np.empty((N.NSUMMARY, n))
    status = np.zeros(n, dtype=np.uint32)
    dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    N.check(eng.lib.ryd_run_schedule_kets_ctl(eng.handle, ctypes.byref(desc), dptr(p), n, n, dptr(tab), ld, None, 0,
                                              dptr(summ), n, dptr(raw), ldj,
                                              status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None))
    assert np.all(raw[:, 16 * ns:] == -7.0)
    got = E.complex_control_jacobian(raw[:, :16 * ns].reshape(n, 4, 4, ns))
    np.testing.assert_array_equal(_bits(got), _bits(ctl.control_jacobian))
    np.testing.assert_array_equal(_bits(summ), _bits(ctl.summary))
    np.testing.assert_array_equal(status, ctl.status)


# ---- 3. the memo
def test_memo(eng):
    rng = np.random.default_rng(404)                     # the cases of test_memo_counts_builds
    p = SP.random_params(rng, 1)
    ns = 33
    amps = rng.uniform(0.5, 1.2, ns)
    ph = -rng.uniform(-np.pi, np.pi, ns)
    aba = np.where((np.arange(ns) // 5) % 2 == 0, amps[0], amps[1])      # A, B, A, ... in runs of five
    for what, a, want in (("equal", np.full(ns, amps[0]), 1),
                          ("one step", np.where(np.arange(ns) < 16, amps[0], amps[1]), 2),
                          ("all different", amps, ns), ("A B A", aba, 7)):
        s = PS.assemble(np.full(ns, 0.35), a, ph, 0.07)
        r = _ctl(eng, p, s)
        assert r.status[0] == 0
        assert r.col("NSQUARE")[0] == want and r.col("NMV_USEFUL")[0] == ns, what
        errs = _field_errors(r.control_jacobian, CP.chain(p, s)["C"])
        print(what, r.col("NSQUARE")[0], errs)
        assert max(errs.values()) < TOL, (what, errs)


# ---- 4. rows independent of their wave and of the forward loop it takes
def test_rows_independent_of_wave(eng):
    b = CP.batch("random")
    p, s = b["params"][:, :4].copy(), b["sched"][:4].copy()
    wave = _ctl(eng, p, s)
    rev = _ctl(eng, p[:, ::-1].copy(), s[::-1].copy())
    assert np.all(wave.status == 0)
    for i in range(4):
        alone = _ctl(eng, p[:, i:i + 1].copy(), s[i:i + 1].copy())
        _same(alone, wave, [0], [i], what=f"point {i} alone / in its wave")
        _same(rev, wave, [3 - i], [i], what=f"point {i} reversed wave")


def test_rows_independent_of_the_loop_their_wave_takes(eng):
    """The 40-segment case of tests/test_gpu_schedule_kets.py: a phase-only point alone (plain
    forward chunks) and beside two points that put the wave on the general loop."""
    rng = np.random.default_rng(505)
    ns = 40
    p = SP.random_params(rng, 3)
    s = PS.assemble(np.full((3, ns), 0.3), 1.0, rng.uniform(-3, 3, (3, ns)), 0.05)
    s[1, SC["AMP"]] = rng.uniform(0.5, 1.2, ns)
    s[2, SC["X"], [3, 20, 37]] = 0.0
    wave = _ctl(eng, p, s)
    assert np.all(wave.status == 0) and wave.col("NSQUARE").tolist() == [1, ns, 1]
    for i in range(3):
        alone = _ctl(eng, p[:, i:i + 1].copy(), s[i:i + 1].copy())
        _same(alone, wave, [0], [i], what=f"point {i} alone / in a mixed wave")
    errs = _field_errors(wave.control_jacobian, CP.chain(p, s)["C"])
    print("plain and general chunks:", errs)
    assert max(errs.values()) < TOL


# ---- 5. launch shapes, 6. shared against per-point table
@pytest.fixture(scope="module")
def shapes(eng):
    rng = np.random.default_rng(606)
    n, ns = 149, 7
    p = SP.random_params(rng, n)
    s = PS.assemble(rng.uniform(0.05, 1.0, (n, ns)), rng.uniform(0.0, 1.2, (n, ns)),
                    rng.uniform(-3, 3, (n, ns)), rng.uniform(-0.5, 0.5, (n, ns)))
    return p, s, _ctl(eng, p, s)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 37])
def test_launch_shapes(eng, shapes, n):
    p, s, full = shapes
    assert np.all(full.status == 0) and full.n == 149
    r = _ctl(eng, p[:, :n].copy(), s[:n].copy())
    _same(r, full, slice(None), slice(0, n), what=f"n = {n}")


def test_shared_against_per_point(eng, shapes):
    p, s, _ = shapes
    per = _ctl(eng, p, np.repeat(s[:1], p.shape[1], axis=0))
    sh = _ctl(eng, p, s[0])
    assert np.all(sh.status == 0) and all(np.any(sh.control_jacobian[:, SC[f]] != 0) for f in FIELDS)
    _same(sh, per, cols=range(N.NSUMMARY), what="shared table")


# ---- 7. refused rows, the step cap
def _spoil(p, s, i, kind):
    if kind == "nan":
        s[i, SC["DELTA"], 3] = np.nan
    elif kind == "a<0":
        s[i, SC["AMP"], 5] = -1e-3
    else:
        p[N.P["OMEGA"], i] = 0.0


@pytest.mark.parametrize("kind", ("nan", "a<0", "omega=0"))
def test_refused_rows(eng, shapes, kind):
    p0, s0, _ = shapes
    p0, s0 = p0[:, :12].copy(), s0[:12].copy()
    base = _ctl(eng, p0, s0)
    for rows in ([4], [5], [6], [7], [4, 5, 6, 7]):
        p, s = p0.copy(), s0.copy()
        for i in rows:
            _spoil(p, s, i, kind)
        r = _ctl(eng, p, s)
        good = [i for i in range(12) if i not in rows]
        np.testing.assert_array_equal(r.status[rows], BAD)
        _same(r, base, good, good, what=f"{kind} at {rows}: neighbours")
        for i in rows:
            np.testing.assert_array_equal(_bits(r.control_jacobian[i]), 0, err_msg=f"{kind}: Jacobian row {i}")


def test_nan_in_the_last_segment(eng):
    """n_seg = 17: the NaN sits alone in the partial second chunk, where every lane past it reads
    it again and where the backward walk starts.  Its row is refused; the neighbours are the
    oracle's, as in test_against_oracle."""
    p, s, good = SP.nan_last_segment()
    r = _ctl(eng, p, s)
    ref = CP.reference("chunk17")
    np.testing.assert_array_equal(r.status, np.where(np.arange(5) == SP.NAN_ROW, BAD, 0))
    kerr = float(np.abs(r.kets()[good] - ref["kets"][good]).max())
    errs = _field_errors(r.control_jacobian[good], ref["C"][good])
    print(f"NaN in the last segment: neighbours max|dpsi| = {kerr:.3e}, " +
          ", ".join(f"max|dJ_{f}| = {errs[f]:.3e}" for f in FIELDS))
    assert kerr < TOL and max(errs.values()) < TOL
    np.testing.assert_array_equal(_bits(r.control_jacobian[SP.NAN_ROW]), 0)


def test_step_cap(eng, shapes):
    p0, s0, _ = shapes
    p, s = p0[:, :8].copy(), s0[:8].copy()
    base = _ctl(eng, p, s)
    s[5, SC["X"], 3] = 1e7                               # beyond the ket build's argument cap
    r = _ctl(eng, p, s)
    good = [i for i in range(8) if i != 5]
    np.testing.assert_array_equal(r.status[5], CAP)
    _same(r, base, good, good, what="step cap: neighbours")
    C = r.control_jacobian[5]
    np.testing.assert_array_equal(_bits(C[:, :, 3]), 0)  # all four fields of the capped segment
    assert np.all(np.isfinite(C)) and np.any(C[:, :, [0, 1, 2, 4, 5, 6]] != 0)
    # the other segments: the schedule without that one (whose zero duration has a value in x only)
    t = s[5:6].copy()
    t[0, SC["X"], 3] = 0.0
    q = _ctl(eng, p[:, 5:6].copy(), t)
    assert q.status[0] == 0
    keep = [0, 1, 2, 4, 5, 6]
    np.testing.assert_array_equal(_bits(q.control_jacobian[0][:, :, keep]), _bits(C[:, :, keep]))
    np.testing.assert_array_equal(_bits(q.state), _bits(r.state[:, 20:24]))


# ---- 8. the optimiser
@pytest.mark.parametrize("free, kw", ((("phase", "amp", "delta"), dict(amp_max=1.1)),
                                      (("phase", "x"), dict(duration_weight=1e-3))))
def test_optimize_schedule(eng, free, kw):
    rng = np.random.default_rng(909)
    n, ns = 3, 24
    p = SP.random_params(rng, n)
    s0 = PS.assemble(np.full((n, ns), 7.612 / ns), 1.0, rng.uniform(-0.5, 0.5, (n, ns)), 0.0)

    class Counting:
        def __init__(self):
            self.calls = 0

        def run_schedule_kets(self, params, sched, *, states=True, jacobian=False):
            assert states is False and jacobian == "controls"
            self.calls += 1
            return eng.run_schedule_kets(params, sched, states=states, jacobian=jacobian)

    c = Counting()
    out = PS.optimize_schedule(p, s0, free=free, maxiter=30, engine=c, **kw)
    print(free, "F start", out["F_start"], "F final", out["F_final"], "nfev", out["nfev"], out["message"])
    assert out["engine_calls"] == out["nfev"] == c.calls
    tab = out["sched"]
    w = kw.get("duration_weight", 0.0)
    cost = lambda F, t: np.sum(1.0 - F) + w * np.sum(t[:, SC["X"]])
    assert np.all(out["F_final"] >= out["F_start"])
    assert cost(out["F_final"], tab) <= cost(out["F_start"], s0)      # the objective, duration term included
    for f, name in PS.FIELDS.items():                    # only the free fields moved
        if f not in free:
            np.testing.assert_array_equal(tab[:, name], s0[:, name])
    assert np.all(tab[:, SC["X"]] >= 0.0) and np.all(tab[:, SC["AMP"]] >= 0.0)
    if "amp_max" in kw:
        assert np.all(tab[:, SC["AMP"]] <= kw["amp_max"])
    PS.validate_schedule(tab, n)
    k = 1                                                # avg_gate
    F_ref = NM.gate_fidelity(NM.ket_maps(CP.KP.chain(p, tab)["kets"]))[k]
    F0_ref = NM.gate_fidelity(NM.ket_maps(CP.KP.chain(p, s0)["kets"]))[k]
    err = float(np.abs(out["F_final"] - F_ref).max())
    err0 = float(np.abs(out["F_start"] - F0_ref).max())
    print(f"optimize_schedule {free}: |F_final - oracle| = {err:.3e}, |F_start - oracle| = {err0:.3e}")
    assert err < TOL and err0 < TOL
    again = PS.optimize_schedule(p, s0, free=free, maxiter=30, engine=eng, **kw)
    np.testing.assert_array_equal(_bits(again["sched"]), _bits(tab))
    np.testing.assert_array_equal(_bits(again["F_final"]), _bits(out["F_final"]))
