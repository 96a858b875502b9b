"""Custom pulse schedules on the GPU (ryd_run_schedule, lindblad_sched16_kernel): against the
CPU oracle's chained segments, against the protocols the builders restate, and the kernel's
own edges (chunks of 16 segments, the propagator memo, rows of a wave, launch shapes, refused
rows, summary-only runs, the product path).

Tolerance: the project's 1e-10 on rho elements and populations (tests/test_gpu_parity.py); the
measured maxima are printed.  Bit-for-bit comparisons between differently composed waves
leave out NMV_EXEC, which counts what the point's WAVE executed (include/ryd_engine.h: "wave-
uniform"; tests/test_gpu_sym16_build.py does the same) -- every other column, the state rows
and the status are compared.
"""
import warnings

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import configurations as CF
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import physics as PH
from noisyquantumsimulator_amd import protocols as PR
from noisyquantumsimulator_amd import pulse_schedules as PS
from noisyquantumsimulator_amd import simulation as SIM
from tests import sched_points as SP

pytestmark = pytest.mark.gpu

TOL = 1e-10
OWN = [i for name, i in N.S.items() if name != "NMV_EXEC"]
BAD = N.STATUS_BAD_INPUT


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _same(a, b, ia=slice(None), ib=slice(None), cols=OWN, what=""):
    """Rows ia of run a and ib of run b: state rows, summary columns `cols`, status, bit for bit."""
    ia, ib = np.arange(a.n)[ia], np.arange(b.n)[ib]
    la = (4 * ia[:, None] + np.arange(4)).ravel()
    lb = (4 * ib[:, None] + np.arange(4)).ravel()
    np.testing.assert_array_equal(a.state[:, la], b.state[:, lb], err_msg=f"{what}: state")
    for c in cols:                                   # (NaN columns: equal as bit patterns)
        np.testing.assert_array_equal(a.summary[c, ia].view(np.uint64), b.summary[c, ib].view(np.uint64),
                                      err_msg=f"{what}: summary column {c}")
    np.testing.assert_array_equal(a.status[ia], b.status[ib], err_msg=f"{what}: status")


def _against_oracle(r, ref, what):
    assert np.all(r.status == 0), (what, r.status)
    rho = r.rho()
    err = float(np.abs(rho - ref).max())
    pops = np.real(np.stack([ref[:, k, i, i] for k, i in enumerate((0, 1, 3, 4))], axis=1))
    perr = float(np.abs(r.populations() - pops).max())
    tr = np.real(np.trace(ref[:, 3], axis1=1, axis2=2))
    terr = float(np.abs(r.col("TRACE11") - tr).max())
    print(f"{what}: max|drho| = {err:.3e}, max|dpop| = {perr:.3e}, max|dTr rho_11| = {terr:.3e}")
    assert err < TOL and perr < TOL and terr < TOL, (what, err, perr, terr)


# ---- 1. against the oracle
def test_random_schedules_against_oracle(eng):
    """13 points, 20 random segments each (one of zero length, one with a = 0), per-point tables."""
    b = SP.batch("random")
    _against_oracle(eng.run_schedule(b["params"], b["sched"]), SP.golden("random"), "random schedules")


# ---- 2. against the existing protocols
@pytest.mark.parametrize("protocol", ["lp_square", "bangbang", "smooth_jp"])
def test_builders_against_protocols(eng, protocol):
    b = SP.batch(protocol)
    r = eng.run_schedule(b["params"], b["sched"])
    _against_oracle(r, SP.golden(protocol), f"{protocol} as a table")
    rp = eng.run(b["params"], protocol, "lindblad", n_steps=b["n_steps"])
    assert np.all(rp.status == 0)
    err = float(np.abs(r.rho() - rp.rho()).max())
    print(f"{protocol}: table against Engine.run max|drho| = {err:.3e}")
    assert err < TOL
    if protocol == "smooth_jp":                      # equal segments: one build, as smooth JP
        np.testing.assert_array_equal(r.col("NSQUARE"), rp.col("NSQUARE"))


# ---- 3. chunk edges
@pytest.mark.parametrize("ns", SP.CHUNK_NSEG)
def test_chunk_edges(eng, ns):
    b = SP.batch(f"chunk{ns}")
    _against_oracle(eng.run_schedule(b["params"], b["sched"]), SP.golden(f"chunk{ns}"), f"n_seg = {ns}")


# ---- 4. the memo
def test_memo_counts_builds(eng):
    rng = np.random.default_rng(404)
    p = SP.random_params(rng, 1)
    ns = 33
    amps = rng.uniform(0.5, 1.2, ns)
    one = lambda a: PS.assemble([0.35], [a], [0.0], [0.07])
    # the one-segment schedule of every amplitude, one point each
    singles = eng.run_schedule(np.repeat(p, ns, axis=1), np.stack([one(a) for a in amps]))
    assert np.all(singles.status == 0) and np.all(singles.col("NSQUARE") > 0)
    ph = -rng.uniform(-np.pi, np.pi, ns)
    for what, a, want in (("equal", np.full(ns, amps[0]), [0]),
                          ("one step", np.where(np.arange(ns) < 16, amps[0], amps[1]), [0, 1]),
                          ("all different", amps, list(range(ns)))):
        r = eng.run_schedule(p, PS.assemble(np.full(ns, 0.35), a, ph, 0.07))
        assert r.status[0] == 0
        for col in ("NSQUARE", "NMV_USEFUL"):
            print(what, col, r.col(col)[0], singles.col(col)[want].sum())
            assert r.col(col)[0] == singles.col(col)[want].sum(), (what, col)


# ---- 5. rows independent of their wave
def test_rows_independent_of_wave(eng):
    b = SP.batch("random")
    p, s = b["params"][:, :4].copy(), b["sched"][:4].copy()
    wave = eng.run_schedule(p, s)
    rev = eng.run_schedule(p[:, ::-1].copy(), s[::-1].copy())
    assert np.all(wave.status == 0)
    for i in range(4):
        alone = eng.run_schedule(p[:, i:i + 1].copy(), s[i:i + 1].copy())
        _same(alone, wave, [0], [i], what=f"point {i} alone / in its wave")
        _same(rev, wave, [3 - i], [i], what=f"point {i} reversed wave")


# ---- 6. launch shapes
@pytest.fixture(scope="module")
def shapes(eng):
    rng = np.random.default_rng(606)
    n, ns = 149, 7
    p = SP.random_params(rng, n)
    s = PS.assemble(rng.uniform(0.05, 1.0, (n, ns)), rng.uniform(0.0, 1.2, (n, ns)),
                    rng.uniform(-3, 3, (n, ns)), rng.uniform(-0.5, 0.5, (n, ns)))
    return p, s, eng.run_schedule(p, s)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 37, 149])
def test_launch_shapes(eng, shapes, n):
    p, s, full = shapes
    assert np.all(full.status == 0)
    r = eng.run_schedule(p[:, :n].copy(), s[:n].copy())
    _same(r, full, slice(None), slice(0, n), what=f"n = {n}")


def test_shared_against_per_point(eng, shapes):
    p, s, _ = shapes
    per = eng.run_schedule(p, np.repeat(s[:1], p.shape[1], axis=0))
    sh = eng.run_schedule(p, s[0])
    _same(sh, per, cols=range(N.NSUMMARY), what="shared table")


# ---- 7. refused rows
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
    base = eng.run_schedule(p0, s0)
    inputs = np.zeros((25, 4))                      # the untouched basis states, sector rows
    inputs[0, 0] = inputs[1, 1] = inputs[5, 2] = inputs[6, 3] = 1.0
    for rows in ([4], [5], [6], [7], [4, 5, 6, 7]):
        p, s = p0.copy(), s0.copy()
        for i in rows:
            _spoil(p, s, i, kind)
        r = eng.run_schedule(p, s)
        good = [i for i in range(12) if i not in rows]
        np.testing.assert_array_equal(r.status[rows], BAD)
        _same(r, base, good, good, what=f"{kind} at {rows}: neighbours")
        for i in rows:
            np.testing.assert_array_equal(r.state[:, 4 * i:4 * i + 4], inputs, err_msg=f"{kind}: row {i}")


def test_nan_in_the_last_segment(eng):
    """n_seg = 17: the NaN sits alone in the partial second chunk, where every lane past it reads
    it again.  Its row is refused; the neighbours are the oracle's, as in test_chunk_edges."""
    p, s, good = SP.nan_last_segment()
    r = eng.run_schedule(p, s)
    np.testing.assert_array_equal(r.status, np.where(np.arange(5) == SP.NAN_ROW, BAD, 0))
    err = float(np.abs(r.rho()[good] - SP.golden("chunk17")[good]).max())
    print(f"NaN in the last segment: neighbours max|drho| = {err:.3e}")
    assert err < TOL
    inputs = np.zeros((25, 4))
    inputs[0, 0] = inputs[1, 1] = inputs[5, 2] = inputs[6, 3] = 1.0
    np.testing.assert_array_equal(r.state[:, 4 * SP.NAN_ROW:4 * SP.NAN_ROW + 4], inputs)


# ---- 8. summary-only, device-resident
def test_summary_only_and_device_batch(eng):
    b = SP.batch("random")
    full = eng.run_schedule(b["params"], b["sched"])
    lean = eng.run_schedule(b["params"], b["sched"], states=False)
    assert lean.state is None
    np.testing.assert_array_equal(lean.summary.view(np.uint64), full.summary.view(np.uint64))
    np.testing.assert_array_equal(lean.status, full.status)
    for states in (True, False):
        db = E.ScheduleDeviceBatch(eng, b["params"], b["sched"], states=states)
        try:
            assert db.launch(timed=True) > 0.0
            got = db.fetch()
        finally:
            db.free()
        if states:
            np.testing.assert_array_equal(got.state, full.state)
        np.testing.assert_array_equal(got.summary.view(np.uint64), full.summary.view(np.uint64))
        np.testing.assert_array_equal(got.status, full.status)
    sh = E.ScheduleDeviceBatch(eng, b["params"], b["sched"][0])
    try:
        sh.launch()
        got = sh.fetch()
    finally:
        sh.free()
    _same(got, eng.run_schedule(b["params"], b["sched"][0]), cols=range(N.NSUMMARY), what="shared, device-resident")


def test_unequal_atoms_refused(eng):
    b = SP.batch("random")
    p = b["params"].copy()
    p[N.P["GSC_B"], 2] *= 2
    with pytest.raises(ValueError, match="identical atoms"):
        eng.run_schedule(p, b["sched"])


# ---- 9. the product path
def test_product_path_against_smooth_jp():
    """simulate_CZ_gate_batch on the table from_smooth_jp builds of the smooth-JP defaults
    against the same call with SmoothJPSimulationInputs.  No rate is excluded: "schedule" and
    "smooth_sinusoidal" take the same ("other") branch of the leakage spectral factor, and
    tau_total = sum x / Omega equals omega_tau / Omega to rounding."""
    warnings.simplefilter("ignore")
    kw = dict(temperature=np.linspace(1e-6, 5e-6, 5), include_noise=True, return_states=True)
    ref = SIM.simulate_CZ_gate_batch(CF.SmoothJPSimulationInputs(), **kw)
    d = PR.SMOOTH_JP_DEFAULTS
    sdom = ref.batch.cols["smooth_delta_over_omega"]
    tab = PS.from_smooth_jp(d["A"], d["omega_mod_ratio"], d["phi_offset"], d["omega_tau"], sdom, 300)
    got = SIM.simulate_CZ_gate_batch(CF.PulseScheduleInputs.from_table(tab), **kw)
    assert np.all(got.is_mixed) and np.all(ref.is_mixed) and np.all(got.ok)
    for k in PH.RATE_FIELDS:
        np.testing.assert_allclose(got.batch.cols[k], ref.batch.cols[k], rtol=1e-12, atol=0, err_msg=k)
    perr = float(np.abs(got.populations - ref.populations).max())
    err = float(np.abs(got.states["rho"] - ref.states["rho"]).max())
    print(f"product path: max|dpop| = {perr:.3e}, max|drho| = {err:.3e}")
    assert perr < TOL and err < TOL
    with pytest.raises(ValueError, match="coherence"):
        SIM.simulate_CZ_gate_batch(CF.PulseScheduleInputs.from_table(tab), process_fidelity=True, **kw)
