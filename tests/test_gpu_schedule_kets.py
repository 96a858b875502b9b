"""Noise-free custom pulse schedules as kets, with phase gradients, on the GPU
(ryd_run_schedule_kets; ket_sched_kernel, ket_sched_jac_kernel): against the CPU oracle's
chained 9 x 9 ``expm`` and its analytic Jacobian (tests/sched_ket_points.py), against the
engine's own neighbouring paths, and the kernels' edges (chunks of 16 segments walked forwards
and backwards, the propagator memo, rows of a wave, launch shapes, refused rows, the step cap),
then the phase optimiser on top.

Tolerance: the project's 1e-10 (tests/test_gpu_parity.py) on ket amplitudes, overlaps,
populations, TRACE11 and the Jacobian's elements; the measured maxima are printed.
Bit-for-bit comparisons between differently composed waves leave out NMV_EXEC, as
tests/test_gpu_schedule.py does.
"""
import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import pulse_schedules as PS
from tests import sched_ket_points as KP
from tests import sched_points as SP

pytestmark = pytest.mark.gpu

TOL = 1e-10
OWN = [i for name, i in N.S.items() if name != "NMV_EXEC"]
BAD, CAP = N.STATUS_BAD_INPUT, N.STATUS_STEP_CAP
PROTOCOLS = ("lp_square", "bangbang", "smooth_jp")


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype != np.complex128 else a.view(np.float64).view(np.uint64)


def _same(a, b, ia=slice(None), ib=slice(None), cols=OWN, what="", state=True):
    """Rows ia of run a and ib of run b: ket rows, summary columns `cols`, status and (where
    both have one) the Jacobian, bit for bit."""
    ia, ib = np.arange(a.n)[ia], np.arange(b.n)[ib]
    la = (4 * ia[:, None] + np.arange(4)).ravel()
    lb = (4 * ib[:, None] + np.arange(4)).ravel()
    if state:
        np.testing.assert_array_equal(_bits(a.state[:, la]), _bits(b.state[:, lb]), err_msg=f"{what}: state")
    for c in cols:                                   # (NaN columns: equal as bit patterns)
        np.testing.assert_array_equal(_bits(a.summary[c, ia]), _bits(b.summary[c, ib]),
                                      err_msg=f"{what}: summary column {c}")
    np.testing.assert_array_equal(a.status[ia], b.status[ib], err_msg=f"{what}: status")
    if a.phase_jacobian is not None and b.phase_jacobian is not None:
        np.testing.assert_array_equal(_bits(a.phase_jacobian[ia]), _bits(b.phase_jacobian[ib]),
                                      err_msg=f"{what}: Jacobian")


def _against_oracle(r, ref, what):
    assert np.all(r.status == 0), (what, r.status)
    kets = ref["kets"]
    err = float(np.abs(r.kets() - kets).max())
    a01, a11 = PS.overlaps(r.summary)
    ov = np.stack([np.ones_like(ref["a01"]), ref["a01"], ref["a01"], ref["a11"]])
    got = r.summary[N.S["OV_RE0"]:N.S["OV_RE0"] + 4] + 1j * r.summary[N.S["OV_IM0"]:N.S["OV_IM0"] + 4]
    oerr = float(np.abs(got - ov).max())
    assert np.array_equal(a01, got[1]) and np.array_equal(a11, got[3])
    perr = float(np.abs(r.populations() - (np.abs(ov) ** 2).T).max())
    terr = float(np.abs(r.col("TRACE11") - np.sum(np.abs(kets[:, 3]) ** 2, axis=1)).max())
    jerr = float(np.abs(r.phase_jacobian - ref["J"]).max())
    gerr = float(np.abs(r.phase_jacobian.sum(axis=2)).max())
    print(f"{what}: max|dpsi| = {err:.3e}, max|doverlap| = {oerr:.3e}, max|dpop| = {perr:.3e}, "
          f"max|dTr11| = {terr:.3e}, max|dJ| = {jerr:.3e}, max|sum_s J| = {gerr:.3e}")
    assert max(err, oerr, perr, terr, jerr, gerr) < TOL, (what, err, oerr, perr, terr, jerr, gerr)


# ---- 1. against the oracle
@pytest.mark.parametrize("name", ("random",) + PROTOCOLS + tuple(f"chunk{ns}" for ns in SP.CHUNK_NSEG))
def test_against_oracle(eng, name):
    """Kets, overlaps, populations, TRACE11, the Jacobian and its gauge sum.  The chunk batches
    (n_seg = 1, 15, 16, 17, 32, 33) walk the reverse pass across chunk edges and start it in a
    partial last chunk."""
    b = SP.batch(name)
    r = eng.run_schedule_kets(b["params"], b["sched"], jacobian=True)
    assert r.evolution == "ket" and r.phase_jacobian.shape == (b["params"].shape[1], 2, b["sched"].shape[-1])
    _against_oracle(r, KP.reference(name), name)


# ---- 2. against the neighbouring paths
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_tables_against_protocol_kets(eng, protocol):
    b = SP.batch(protocol)
    r = eng.run_schedule_kets(b["params"], b["sched"])
    assert r.phase_jacobian is None
    rp = eng.run(b["params"], protocol, "ket", n_steps=b["n_steps"])
    assert np.all(r.status == 0) and np.all(rp.status == 0)
    err = float(np.abs(r.kets() - rp.kets()).max())
    print(f"{protocol}: table against Engine.run kets max|dpsi| = {err:.3e}")
    assert err < TOL


def test_against_lindblad_schedule_at_zero_rates(eng):
    b = SP.batch("random")
    p = b["params"].copy()
    p[N.P["G1_A"]:N.P["GSC_B"] + 1] = 0.0          # every rate column (the mJ columns are zero already)
    assert not np.any(p[N.P["GMJ_A"]:]) and np.all(p[:4] == b["params"][:4])
    r = eng.run_schedule_kets(p, b["sched"])
    rl = eng.run_schedule(p, b["sched"])
    assert np.all(r.status == 0) and np.all(rl.status == 0)
    psi = r.kets()
    err = float(np.abs(rl.rho() - np.einsum("nki,nkj->nkij", psi, psi.conj())).max())
    print(f"zero rates: Lindblad schedule rho against |psi><psi| max = {err:.3e}")
    assert err < TOL


# ---- 3. the memo
def test_memo_counts_builds(eng):
    rng = np.random.default_rng(404)
    p = SP.random_params(rng, 1)
    ns = 33
    amps = rng.uniform(0.5, 1.2, ns)
    ph = -rng.uniform(-np.pi, np.pi, ns)
    for what, a, want in (("equal", np.full(ns, amps[0]), 1),
                          ("one step", np.where(np.arange(ns) < 16, amps[0], amps[1]), 2),
                          ("all different", amps, ns)):
        for jac in (False, True):
            r = eng.run_schedule_kets(p, PS.assemble(np.full(ns, 0.35), a, ph, 0.07), jacobian=jac)
            print(what, jac, r.col("NSQUARE")[0], r.col("NMV_USEFUL")[0])
            assert r.status[0] == 0
            assert r.col("NSQUARE")[0] == want and r.col("NMV_USEFUL")[0] == ns, (what, jac)


# ---- 4. same bits with and without the Jacobian, the states, the host
def test_same_bits_across_forms(eng):
    b = SP.batch("random")
    p, s = b["params"], b["sched"]
    full = eng.run_schedule_kets(p, s, jacobian=True)
    fwd = eng.run_schedule_kets(p, s)
    _same(full, fwd, cols=range(N.NSUMMARY), what="with / without the Jacobian")
    for jac in (True, False):
        lean = eng.run_schedule_kets(p, s, states=False, jacobian=jac)
        assert lean.state is None
        _same(lean, full, cols=range(N.NSUMMARY), what=f"summary-only, jacobian={jac}", state=False)
        for states in (True, False):
            db = E.ScheduleKetDeviceBatch(eng, p, s, states=states, jacobian=jac)
            try:
                assert db.launch(timed=True) > 0.0
                got = db.fetch()
            finally:
                db.free()
            assert (got.state is None) == (not states) and (got.phase_jacobian is None) == (not jac)
            _same(got, full, cols=range(N.NSUMMARY), what=f"device-resident {states} {jac}", state=states)


# ---- 5. rows independent of their wave
def test_rows_independent_of_wave(eng):
    b = SP.batch("random")
    p, s = b["params"][:, :4].copy(), b["sched"][:4].copy()
    wave = eng.run_schedule_kets(p, s, jacobian=True)
    rev = eng.run_schedule_kets(p[:, ::-1].copy(), s[::-1].copy(), jacobian=True)
    assert np.all(wave.status == 0)
    for i in range(4):
        alone = eng.run_schedule_kets(p[:, i:i + 1].copy(), s[i:i + 1].copy(), jacobian=True)
        _same(alone, wave, [0], [i], what=f"point {i} alone / in its wave")
        _same(rev, wave, [3 - i], [i], what=f"point {i} reversed wave")


def test_rows_independent_of_the_loop_their_wave_takes(eng):
    """A chunk whose 16 segments all run on the row's current propagator takes the kernel's
    broadcast loop, but only if that holds for every row of the wave.  A phase-only point of 40
    segments (chunks 2 and 3 plain; the last one partial) alone, and beside a point whose
    amplitude changes every segment and a point with a zero-length segment in every chunk,
    which put the whole wave on the general loop: the same bits, Jacobian included."""
    rng = np.random.default_rng(505)
    ns = 40
    p = SP.random_params(rng, 3)
    s = PS.assemble(np.full((3, ns), 0.3), 1.0, rng.uniform(-3, 3, (3, ns)), 0.05)
    s[1, N.SC["AMP"]] = rng.uniform(0.5, 1.2, ns)
    s[2, N.SC["X"], [3, 20, 37]] = 0.0
    wave = eng.run_schedule_kets(p, s, jacobian=True)
    assert np.all(wave.status == 0) and wave.col("NSQUARE").tolist() == [1, ns, 1]
    assert wave.col("NMV_USEFUL").tolist() == [ns, ns, ns - 3]
    for i in range(3):
        alone = eng.run_schedule_kets(p[:, i:i + 1].copy(), s[i:i + 1].copy(), jacobian=True)
        _same(alone, wave, [0], [i], what=f"point {i} alone / in a mixed wave")
    ref = KP.chain(p, s)
    err = float(np.abs(wave.kets() - ref["kets"]).max())
    jerr = float(np.abs(wave.phase_jacobian - ref["J"]).max())
    print(f"plain and general chunks: max|dpsi| = {err:.3e}, max|dJ| = {jerr:.3e}")
    assert err < TOL and jerr < TOL


# ---- 6. launch shapes
@pytest.fixture(scope="module")
def shapes(eng):
    rng = np.random.default_rng(606)
    n, ns = 149, 7
    p = SP.random_params(rng, n)
    s = PS.assemble(rng.uniform(0.05, 1.0, (n, ns)), rng.uniform(0.0, 1.2, (n, ns)),
                    rng.uniform(-3, 3, (n, ns)), rng.uniform(-0.5, 0.5, (n, ns)))
    return p, s, eng.run_schedule_kets(p, s, jacobian=True)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 37])
def test_launch_shapes(eng, shapes, n):
    p, s, full = shapes
    assert np.all(full.status == 0)
    r = eng.run_schedule_kets(p[:, :n].copy(), s[:n].copy(), jacobian=True)
    _same(r, full, slice(None), slice(0, n), what=f"n = {n}")


# ---- 7. shared against per-point table
def test_shared_against_per_point(eng, shapes):
    p, s, _ = shapes
    per = eng.run_schedule_kets(p, np.repeat(s[:1], p.shape[1], axis=0), jacobian=True)
    sh = eng.run_schedule_kets(p, s[0], jacobian=True)
    assert np.all(sh.status == 0) and np.any(sh.phase_jacobian != 0)
    _same(sh, per, cols=range(N.NSUMMARY), what="shared table")


# ---- 8. refused rows, the step cap
DEFECTS = ("nan", "x<0", "a<0", "omega=0", "rate<0")


def _spoil(p, s, i, kind):
    if kind == "nan":
        s[i, N.SC["DELTA"], 3] = np.nan
    elif kind == "x<0":
        s[i, N.SC["X"], 2] = -0.1
    elif kind == "a<0":
        s[i, N.SC["AMP"], 5] = -1e-3
    elif kind == "omega=0":
        p[N.P["OMEGA"], i] = 0.0
    else:
        p[N.P["GPHI_A"], i] = p[N.P["GPHI_B"], i] = -1.0


@pytest.mark.parametrize("kind", DEFECTS)
def test_refused_rows(eng, shapes, kind):
    p0, s0, _ = shapes
    p0, s0 = p0[:, :12].copy(), s0[:12].copy()
    base = eng.run_schedule_kets(p0, s0, jacobian=True)
    basis = np.zeros((4, 9), complex)                # the untouched basis kets
    basis[0, 0] = basis[1, 1] = basis[2, 3] = basis[3, 4] = 1.0
    for rows in ([4], [5], [6], [7], [4, 5, 6, 7]):
        p, s = p0.copy(), s0.copy()
        for i in rows:
            _spoil(p, s, i, kind)
        r = eng.run_schedule_kets(p, s, jacobian=True)
        good = [i for i in range(12) if i not in rows]
        np.testing.assert_array_equal(r.status[rows], BAD)
        _same(r, base, good, good, what=f"{kind} at {rows}: neighbours")
        psi = r.kets()
        for i in rows:
            np.testing.assert_array_equal(_bits(psi[i]), _bits(basis), err_msg=f"{kind}: row {i}")
            np.testing.assert_array_equal(_bits(r.phase_jacobian[i]), 0, err_msg=f"{kind}: Jacobian row {i}")


def test_nan_in_the_last_segment(eng):
    """n_seg = 17: the NaN sits alone in the partial second chunk, where every lane past it reads
    it again and where the backward walk starts.  Its row is refused; the neighbours are the
    oracle's, as in test_against_oracle."""
    p, s, good = SP.nan_last_segment()
    r = eng.run_schedule_kets(p, s, jacobian=True)
    ref = KP.reference("chunk17")
    np.testing.assert_array_equal(r.status, np.where(np.arange(5) == SP.NAN_ROW, BAD, 0))
    err = float(np.abs(r.kets()[good] - ref["kets"][good]).max())
    jerr = float(np.abs(r.phase_jacobian[good] - ref["J"][good]).max())
    print(f"NaN in the last segment: neighbours max|dpsi| = {err:.3e}, max|dJ| = {jerr:.3e}")
    assert max(err, jerr) < TOL
    basis = np.zeros((4, 9), complex)
    basis[0, 0] = basis[1, 1] = basis[2, 3] = basis[3, 4] = 1.0
    np.testing.assert_array_equal(_bits(r.kets()[SP.NAN_ROW]), _bits(basis))
    np.testing.assert_array_equal(_bits(r.phase_jacobian[SP.NAN_ROW]), 0)


def test_step_cap(eng, shapes):
    p0, s0, _ = shapes
    p, s = p0[:, :8].copy(), s0[:8].copy()
    base = eng.run_schedule_kets(p, s, jacobian=True)
    s[5, N.SC["X"], 3] = 1e7                         # half the spectral width times dt >= 5 x / Omega V/Omega > X_CAP
    r = eng.run_schedule_kets(p, s, jacobian=True)
    good = [i for i in range(8) if i != 5]
    np.testing.assert_array_equal(r.status[5], CAP)
    _same(r, base, good, good, what="step cap: neighbours")
    J = r.phase_jacobian[5]
    np.testing.assert_array_equal(_bits(J[:, 3]), 0)
    assert np.all(np.isfinite(r.kets()[5])) and np.all(np.isfinite(J)) and np.all(np.isfinite(r.summary[:, 5]))
    assert np.any(J[:, [0, 1, 2, 4, 5, 6]] != 0)
    assert r.col("NMV_USEFUL")[5] == s.shape[-1] - 1
    # the rest of the point is the schedule without that segment
    t = s[5:6].copy()
    t[0, N.SC["X"], 3] = 0.0
    q = eng.run_schedule_kets(p[:, 5:6].copy(), t, jacobian=True)
    assert q.status[0] == 0
    np.testing.assert_array_equal(_bits(q.state), _bits(r.state[:, 20:24]))
    np.testing.assert_array_equal(_bits(q.phase_jacobian[0]), _bits(J))


def test_padded_jacobian_rows(eng):
    """The C-ABI's host form with ld_jac > 4 n_seg: the same numbers, the caller's padding untouched."""
    import ctypes
    b = SP.batch("chunk17")
    p, s = np.ascontiguousarray(b["params"]), np.ascontiguousarray(b["sched"])
    n, ns = p.shape[1], s.shape[-1]
    tight = eng.run_schedule_kets(p, s, states=False, jacobian=True)
    desc, tab, ld = E.schedule_desc(p, s)
    ldj = 4 * ns + 3
    jac = np.full((n, ldj), -7.0)
    summ = np.empty((N.NSUMMARY, n))
    status = np.zeros(n, dtype=np.uint32)
    dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    N.check(eng.lib.ryd_run_schedule_kets(eng.handle, ctypes.byref(desc), dptr(p), n, n, dptr(tab), ld, None, 0,
                                          dptr(summ), n, dptr(jac), ldj,
                                          status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None))
    assert np.all(jac[:, 4 * ns:] == -7.0)
    got = E.complex_jacobian(jac[:, :4 * ns].reshape(n, 4, ns))
    np.testing.assert_array_equal(_bits(got), _bits(tight.phase_jacobian))
    np.testing.assert_array_equal(_bits(summ), _bits(tight.summary))


def test_unequal_atoms_refused(eng):
    b = SP.batch("random")
    p = b["params"].copy()
    p[N.P["GSC_B"], 2] *= 2
    with pytest.raises(ValueError, match="identical atoms"):
        eng.run_schedule_kets(p, b["sched"])


# ---- 9. the phase optimiser
def test_optimize_phases(eng):
    rng = np.random.default_rng(909)
    n, ns = 3, 24
    p = SP.random_params(rng, n)
    s0 = PS.assemble(np.full((n, ns), 7.612 / ns), 1.0, rng.uniform(-0.5, 0.5, (n, ns)), 0.0)

    class Counting:
        """The engine, counting its schedule-ket calls and their arguments' form."""
        def __init__(self):
            self.calls = 0

        def run_schedule_kets(self, params, sched, *, states=True, jacobian=False):
            assert states is False and jacobian is True
            self.calls += 1
            return eng.run_schedule_kets(params, sched, states=states, jacobian=jacobian)

    c = Counting()
    out = PS.optimize_phases(p, s0, maxiter=30, engine=c)
    print("F start", out["F_start"], "F final", out["F_final"], "nfev", out["nfev"], out["message"])
    assert np.all(out["F_final"] > out["F_start"])
    assert out["engine_calls"] == out["nfev"] == c.calls
    tab = out["sched"]
    for f in ("X", "AMP", "DELTA"):                  # only the phase field moved
        np.testing.assert_array_equal(tab[:, N.SC[f]], s0[:, N.SC[f]])
    ref = KP.chain(p, tab)
    F_ref = NM.gate_fidelity(NM.ket_maps(ref["kets"]))[1]
    F0_ref = NM.gate_fidelity(NM.ket_maps(KP.chain(p, s0)["kets"]))[1]
    err = float(np.abs(out["F_final"] - F_ref).max())
    err0 = float(np.abs(out["F_start"] - F0_ref).max())
    print(f"optimize_phases: |F_final - oracle| = {err:.3e}, |F_start - oracle| = {err0:.3e}")
    assert err < TOL and err0 < TOL
    again = PS.optimize_phases(p, s0, maxiter=30, engine=eng)
    np.testing.assert_array_equal(_bits(again["sched"]), _bits(tab))
    np.testing.assert_array_equal(_bits(again["F_final"]), _bits(out["F_final"]))
