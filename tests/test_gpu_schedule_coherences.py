"""Process-map coherences of a custom pulse schedule on the GPU (ryd_run_schedule_coherences,
coherence_sched_kernel): against the CPU oracle's full maps, against the coherence kernel of
the protocols the builders restate, the join with the state kernel into one map, and the
kernel's own edges (chunks of 16 segments, the propagator memo, rows of a wave, launch shapes,
refused and capped rows, the product path).

Tolerance: the project's 1e-10 on coherence rows (tests/test_gpu_process_map.py); the measured
maxima are printed.  Bit-for-bit comparisons cover every coherence row and the status.
"""
import json
import warnings

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import calibration as CAL
from noisyquantumsimulator_amd import configurations as CF
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import physics as PH
from noisyquantumsimulator_amd import protocols as PR
from noisyquantumsimulator_amd import pulse_schedules as PS
from oracle import lindblad_oracle as O
from tests import sched_coh_points as SC
from tests import sched_points as SP
from tests.process_map_util import rows_from_map

pytestmark = pytest.mark.gpu

TOL = 1e-10
BAD, CAP = N.STATUS_BAD_INPUT, N.STATUS_STEP_CAP
IDENTITY = rows_from_map(np.eye(16, dtype=complex))[1][:, 0]     # E(|a><b|) = |a><b|


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _golden_rows(name):
    return np.stack([rows_from_map(S)[1][:, 0] for S in SC.golden(name)], axis=1)      # (NCOH, n)


def _against_oracle(eng, name):
    b = SC.batch(name)
    coh, st = eng.run_schedule_coherences(b["params"], b["sched"])
    assert coh.shape == (N.NCOH, b["params"].shape[1]) and np.all(st == 0), (name, st)
    err = np.abs(coh - _golden_rows(name)).max(axis=1)
    print(f"{name}: max|d coh| over the 20 rows = {err.max():.3e} (row {int(err.argmax())})")
    assert err.max() < TOL, (name, err)
    return coh


# ---- 1. against the oracle
@pytest.mark.parametrize("name", ["random", "aba", "step16"])
def test_schedules_against_oracle(eng, name):
    """random: 13 x 20 with a zero-length and an a = 0 segment per point; aba: a key that
    returns; step16: the second build asked for by the first segment of the second chunk."""
    _against_oracle(eng, name)


# ---- 2. against the existing protocols
@pytest.mark.parametrize("protocol", ["lp_square", "bangbang", "smooth_jp"])
def test_builders_against_protocols(eng, protocol):
    coh = _against_oracle(eng, protocol)
    b = SC.batch(protocol)
    ref, st = eng.run_coherences(b["params"], protocol, n_steps=b["n_steps"])
    assert np.all(st == 0)
    err = float(np.abs(coh - ref).max())
    print(f"{protocol}: table against Engine.run_coherences max|d coh| = {err:.3e}")
    assert err < TOL


# ---- 3. chunk edges
@pytest.mark.parametrize("ns", SP.CHUNK_NSEG)
def test_chunk_edges(eng, ns):
    _against_oracle(eng, f"chunk{ns}")


# ---- 4. states and coherences join into one map
def test_joint_map_is_a_channel(eng):
    """The state kernel's diagonal inputs and this kernel's coherences in one Choi matrix: were
    the two carried in different frames, the oracle comparison of the whole map, the positivity
    and the PTM's first row would all fail."""
    b = SC.batch("random")
    pm = NM.schedule_process_maps(b["params"], b["sched"], engine=eng)
    assert np.all(pm.status == 0)
    ref = SC.golden("random")
    err = float(np.abs(pm.S - ref).max())
    w = float(np.linalg.eigvalsh(pm.choi).min())
    print(f"joint map: max|dS| = {err:.3e}, smallest Choi eigenvalue {w:.3e}, min leakage {pm.leakage.min():.3e}")
    assert err < TOL
    assert w >= -1e-10 and np.all(pm.leakage >= -1e-10)
    # R[0, j] = Tr E(P_j) / 4: the identity's entry is the surviving trace 1 - leakage as analyse
    # defines it, the row is the oracle map's
    np.testing.assert_allclose(pm.ptm[:, 0, 0], 1.0 - pm.leakage, atol=1e-12, rtol=0)
    row0 = np.stack([O.pauli_transfer_matrix(S)[0] for S in ref])
    np.testing.assert_allclose(pm.ptm[:, 0, :], row0, atol=TOL, rtol=0)


# ---- 5. rows independent of their wave
def test_rows_independent_of_wave(eng):
    b = SC.batch("random")
    p, s = b["params"][:, :4].copy(), b["sched"][:4].copy()
    wave, wst = eng.run_schedule_coherences(p, s)
    rev, rst = eng.run_schedule_coherences(p[:, ::-1].copy(), s[::-1].copy())
    assert np.all(wst == 0)
    for i in range(4):
        alone, ast = eng.run_schedule_coherences(p[:, i:i + 1].copy(), s[i:i + 1].copy())
        np.testing.assert_array_equal(alone[:, 0], wave[:, i], err_msg=f"point {i} alone / in its wave")
        np.testing.assert_array_equal(rev[:, 3 - i], wave[:, i], err_msg=f"point {i} reversed wave")
        assert ast[0] == wst[i] == rst[3 - i]


# ---- 6. launch shapes
@pytest.fixture(scope="module")
def shapes(eng):
    rng = np.random.default_rng(606)
    n, ns = 149, 7
    p = SP.random_params(rng, n)
    s = PS.assemble(rng.uniform(0.05, 1.0, (n, ns)), rng.uniform(0.0, 1.2, (n, ns)),
                    rng.uniform(-3, 3, (n, ns)), rng.uniform(-0.5, 0.5, (n, ns)))
    return p, s, eng.run_schedule_coherences(p, s)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 37, 149])
def test_launch_shapes(eng, shapes, n):
    p, s, (full, fst) = shapes
    assert np.all(fst == 0)
    coh, st = eng.run_schedule_coherences(p[:, :n].copy(), s[:n].copy())
    np.testing.assert_array_equal(coh, full[:, :n], err_msg=f"n = {n}")
    np.testing.assert_array_equal(st, fst[:n])


def _device(eng, p, s):
    db = E.ScheduleCoherenceDeviceBatch(eng, p, s)
    try:
        assert db.launch(timed=True) > 0.0
        return db.fetch()
    finally:
        db.free()


def test_shared_and_device_resident(eng, shapes):
    p, s, (full, fst) = shapes
    per, pst = eng.run_schedule_coherences(p, np.repeat(s[:1], p.shape[1], axis=0))
    sh, sst = eng.run_schedule_coherences(p, s[0])
    assert np.all(pst == 0)
    np.testing.assert_array_equal(sh, per, err_msg="shared table")
    np.testing.assert_array_equal(sst, pst)
    dcoh, dst = _device(eng, p, s)
    np.testing.assert_array_equal(dcoh, full, err_msg="device-resident, per-point")
    np.testing.assert_array_equal(dst, fst)
    dcoh, dst = _device(eng, p, s[0])
    np.testing.assert_array_equal(dcoh, sh, err_msg="device-resident, shared")
    np.testing.assert_array_equal(dst, sst)


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
    base, bst = eng.run_schedule_coherences(p0, s0)
    assert np.all(bst == 0)
    for rows in ([4], [5], [6], [7], [4, 5, 6, 7]):
        p, s = p0.copy(), s0.copy()
        for i in rows:
            _spoil(p, s, i, kind)
        coh, st = eng.run_schedule_coherences(p, s)
        good = [i for i in range(12) if i not in rows]
        np.testing.assert_array_equal(st[rows], BAD)
        np.testing.assert_array_equal(st, eng.run_schedule(p, s, states=False).status,
                                      err_msg=f"{kind} at {rows}: status of the state kernel")
        np.testing.assert_array_equal(coh[:, good], base[:, good], err_msg=f"{kind} at {rows}: neighbours")
        for i in rows:
            np.testing.assert_array_equal(coh[:, i], IDENTITY, err_msg=f"{kind}: row {i}")


def test_nan_in_the_last_segment(eng):
    """n_seg = 17: the NaN sits alone in the partial second chunk, where every lane past it reads
    it again.  Its row is refused; the neighbours are the oracle's, as in test_chunk_edges."""
    p, s, good = SP.nan_last_segment()
    coh, st = eng.run_schedule_coherences(p, s)
    np.testing.assert_array_equal(st, np.where(np.arange(5) == SP.NAN_ROW, BAD, 0))
    err = float(np.abs(coh[:, good] - _golden_rows("chunk17")[:, good]).max())
    print(f"NaN in the last segment: neighbours max|d coh| = {err:.3e}")
    assert err < TOL
    np.testing.assert_array_equal(coh[:, SP.NAN_ROW], IDENTITY)


# ---- 8. step cap
@pytest.mark.parametrize("row", [0, 2, 4])
def test_step_cap(eng, row):
    b = SC.batch("aba")
    p, s = b["params"], b["sched"].copy()
    base, bst = eng.run_schedule_coherences(p, s)
    s[row, N.SC["X"], 3] = SC.capped_segment(p, row, s[row, N.SC["AMP"], 3], s[row, N.SC["DELTA"], 3])
    assert SC.build_argument(p, row, s[row, N.SC["AMP"], 3], s[row, N.SC["DELTA"], 3], s[row, N.SC["X"], 3]) > SC.X_CAP
    coh, st = eng.run_schedule_coherences(p, s)
    good = [i for i in range(5) if i != row]
    assert st[row] == CAP and np.all(st[good] == 0) and np.all(bst == 0)
    assert np.all(np.isfinite(coh))
    np.testing.assert_array_equal(coh[:, row], IDENTITY)
    np.testing.assert_array_equal(coh[:, good], base[:, good])


# ---- 9. the product
def test_calibration_file_against_smooth_jp(eng, tmp_path):
    """calibrate_cz on the table from_smooth_jp builds of the smooth-JP defaults writes the
    process fidelities that the same call with SmoothJPSimulationInputs writes."""
    warnings.simplefilter("ignore")
    kw = dict(temperature=np.linspace(1e-6, 5e-6, 5))
    d = PR.SMOOTH_JP_DEFAULTS
    sdom = PH.derive_batch(CF.SmoothJPSimulationInputs(), include_noise=True, **kw).cols["smooth_delta_over_omega"]
    tab = PS.from_smooth_jp(d["A"], d["omega_mod_ratio"], d["phi_offset"], d["omega_tau"], sdom, 300)
    docs = []
    for inputs, sub in ((CF.SmoothJPSimulationInputs(), "ref"), (CF.PulseScheduleInputs.from_table(tab), "tab")):
        paths = CAL.calibrate_cz(inputs, str(tmp_path / sub), **kw)
        assert len(paths) == 1
        with open(paths[0]) as f:
            docs.append(json.load(f))
    ref, got = docs
    assert got["metadata"]["process_map"] is True and len(got["points"]) == len(ref["points"]) == 5
    worst = 0.0
    for a, b in zip(got["points"], ref["points"]):
        # no kernel failure; the warning bits (GAUGE_UNSTABLE on these noisy points) are the batch's
        assert a["status"] & N.STATUS_FAIL_MASK == 0 and b["status"] & N.STATUS_FAIL_MASK == 0
        for k in ("process_infidelity", "avg_gate_infidelity"):
            worst = max(worst, abs(a["error_rates"][k] - b["error_rates"][k]))
    print(f"calibration files: max difference of the process / average gate fidelities {worst:.3e}")
    assert worst < 1e-9


def test_kraus_operators_rebuild_the_map(eng):
    b = SC.batch("random")
    pm = NM.schedule_process_maps(b["params"], b["sched"], engine=eng, with_kraus=True)
    K = pm.kraus_ops                                         # (n, 16, 4, 4): K_k[c, a]
    S = np.einsum("nkca,nkdb->ncdab", K, np.conj(K)).reshape(-1, 16, 16)
    err = float(np.abs(S - pm.S).max())
    print(f"Kraus reconstruction: max|dS| = {err:.3e}, ranks {pm.kraus_rank}")
    assert err < 1e-9 and np.all(pm.kraus_rank > 1)
