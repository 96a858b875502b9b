"""The kernels that produce every process fidelity, at their edges: coherence_prop_kernel and
coherence4_prop_kernel (ryd_coh_prop.inc, ryd_coh4_prop.inc: the default path) along every
branch of cp_sector / c4_sector -- builds without squarings and the identity build, the two
quad banks at equal depth, a wave that mixes identical-atom and unequal rows, rows that rebuild
on different segments, |xi| != 1, refused rows at every row position, ragged launches, the
device-resident entry point -- and the per-lane coherence_cheb_kernel / coherence4_cheb_kernel
(RYD_COH_PROP=0) on the same inputs.

References: the expm oracle on the full 81 x 81 (dim 3) or 256 x 256 (dim 4) Liouvillian,
TOL = 1e-10 absolute on every coherence row (the project's tolerance), and the same point run
alone, in another order or beside other rows ("same bits" is assert_array_equal).  Inputs
come from coh_points.py (checked on the CPU by test_coh_points_cpu.py); every oracle row is
computed once per module.  Each comparison prints its measured maximum per point before it
asserts.
"""
import numpy as np
import pytest

import coh_points as CP
import dim4_points as D4
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from process_map_util import PATHS, coh_path

pytestmark = pytest.mark.gpu

TOL = 1e-10
K0, K1, K2, K3 = (N.C[k] for k in ("K0", "K1", "K2", "K3"))
dims = pytest.mark.parametrize("dim", CP.DIMS)
paths = pytest.mark.parametrize("path", PATHS, ids=["prop", "per_lane"])


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


@pytest.fixture(scope="module")
def oracle():
    """oracle(key, p, protocol, dim, n_steps=None, cols=None) -> (NCOH, n) rows, computed once
    per (key, dim, n_steps) and read-only."""
    cache = {}

    def get(key, p, protocol, dim, n_steps=None, cols=None):
        k = (key, dim, n_steps)
        if k not in cache:
            cache[k] = CP.oracle_batch(p, protocol, dim, n_steps, cols)
            cache[k].setflags(write=False)
        return cache[k]
    return get


def _run(eng, p, protocol, dim, path=None, n_steps=None):
    with coh_path(path):
        coh, st = eng.run_coherences(p, protocol, n_steps=n_steps, dim=dim)
    assert coh.shape == (N.NCOH, p.shape[1])
    return coh, st


def _vs_oracle(coh, st, ref, what, cols=None, rows=slice(None)):
    """Columns ``cols`` (all) of a run against the oracle's, rows ``rows``, within TOL."""
    cols = list(range(coh.shape[1]) if cols is None else cols)
    err = np.abs(coh[rows][:, cols] - ref[rows][:, cols]).max(axis=0)
    print(f"{what}: max|d coh| against the oracle per point " + " ".join(f"{e:.2e}" for e in err)
          + f" -> {err.max():.3e}")
    assert np.all(st[cols] == 0), f"{what}: status {st[cols]}"
    np.testing.assert_allclose(coh[rows][:, cols], ref[rows][:, cols], atol=TOL, rtol=0, err_msg=what)


def _alone(eng, p, protocol, dim, c, n_steps=None):
    return _run(eng, p[:, c:c + 1].copy(), protocol, dim, None, n_steps)


# ---- a. the ladders ---------------------------------------------------------------------------

def _ladders(dim):
    parts = [D4.tau_ladder4(), D4.x_ladder4()]
    assert [q.shape[1] for q in parts] == [33, 48]
    return CP.for_dim(np.concatenate(parts, axis=1), dim)


@dims
@paths
def test_ladders_match_oracle(eng, oracle, dim, path):
    """Depths 5-8, every series degree without squarings, and the identity build.  The last
    point (x below X_SKIP on both bounds) returns exactly the unit rows."""
    p = _ladders(dim)
    ref = oracle("ladders", p, "lp_square", dim)
    coh, st = _run(eng, p, "lp_square", dim, path)
    _vs_oracle(coh, st, ref, f"dim {dim} {path}: tau ladder", range(33))
    _vs_oracle(coh, st, ref, f"dim {dim} {path}: x ladder", range(33, 81))
    for bound in CP.BOUNDS:
        x = (bound(p, "lp_square") * p[N.P["TAU"]])
        assert x[-1] < D4.X_SKIP < x[-2]
    np.testing.assert_array_equal(coh[:, -1], CP.identity_rows())


@dims
def test_ladder_points_alone(eng, dim):
    """Every ladder point alone (n = 1) has the bits it has in the ladder."""
    p = _ladders(dim)
    coh, st = _run(eng, p, "lp_square", dim)
    assert np.all(st == 0)
    for c in range(p.shape[1]):
        c1, s1 = _alone(eng, p, "lp_square", dim, c)
        assert s1[0] == 0
        np.testing.assert_array_equal(c1[:, 0], coh[:, c], err_msg=f"ladder point {c}")
    np.testing.assert_array_equal(_alone(eng, p, "lp_square", dim, 80)[0][:, 0], CP.identity_rows())


# ---- b. four kinds of row in one wave --------------------------------------------------------------

@dims
def test_four_kinds_of_row_in_one_wave(eng, oracle, dim):
    """An identity-build row, an s = 0 row with a 14-term series, a row 14 squarings deep and a
    NaN row in all 24 orders: a row that sits a series or a squaring out keeps its bits."""
    rows, batch, order = CP.four_kinds()
    rows, batch = CP.for_dim(rows, dim), CP.for_dim(batch, dim)
    coh, st = _run(eng, batch, "lp_square", dim)
    ref = oracle("four_kinds", rows, "lp_square", dim, cols=range(3))
    alone = [_alone(eng, rows, "lp_square", dim, k) for k in range(3)]
    for k in range(3):
        assert alone[k][1][0] == 0
        print(f"dim {dim} four kinds, row kind {k} alone: max|d coh| against the oracle = "
              f"{np.abs(alone[k][0][:, 0] - ref[:, k]).max():.3e}")
        np.testing.assert_allclose(alone[k][0][:, 0], ref[:, k], atol=TOL, rtol=0)
    np.testing.assert_array_equal(alone[0][0][:, 0], CP.identity_rows())
    for w, o in enumerate(order):
        for r, k in enumerate(o):
            c = 4 * w + r
            if k == 3:
                assert st[c] & N.STATUS_BAD_INPUT, f"order {o}: the NaN row is not flagged"
            else:
                assert st[c] == 0, f"order {o} row {r}: status {st[c]}"
                np.testing.assert_array_equal(coh[:, c], alone[k][0][:, 0], err_msg=f"order {o}, row {r} (kind {k})")


# ---- c. the two quad banks at equal depth ------------------------------------------------------------

@dims
@paths
def test_equal_bank_depths(eng, oracle, dim, path):
    p = CP.for_dim(CP.equal_bank_points(), dim)
    ref = oracle("equal_bank", p, "lp_square", dim)
    coh, st = _run(eng, p, "lp_square", dim, path)
    print(f"dim {dim}: (main, V-free) bank depths {[CP.bank_depths(p, i) for i in range(3)]}")
    _vs_oracle(coh, st, ref, f"dim {dim} {path}: equal banks, K2", rows=slice(K2, K2 + 2))
    _vs_oracle(coh, st, ref, f"dim {dim} {path}: equal banks, K3", rows=slice(K3, K3 + 2))
    _vs_oracle(coh, st, ref, f"dim {dim} {path}: equal banks, all rows")
    if path is None:
        for c in range(3):
            np.testing.assert_array_equal(_alone(eng, p, "lp_square", dim, c)[0][:, 0], coh[:, c])


# ---- d. a wave that mixes identical-atom and unequal rows -----------------------------------------------

@dims
@paths
def test_mixed_wave_matches_oracle(eng, oracle, dim, path):
    p = CP.mixed_wave(dim)
    coh, st = _run(eng, p, "lp_square", dim, path)
    _vs_oracle(coh, st, oracle("mixed_wave", p, "lp_square", dim), f"dim {dim} {path}: mixed wave")


@dims
def test_mixed_wave_rows_keep_their_bits(eng, dim):
    """Identical rows build the K = 1 sector with their wave and must not write it: their K1
    rows are their K0 rows (the mirror), alone and in any order."""
    p = CP.mixed_wave(dim)
    coh, st = _run(eng, p, "lp_square", dim)
    assert np.all(st == 0)
    for c in range(8):
        c1, s1 = _alone(eng, p, "lp_square", dim, c)
        assert s1[0] == 0
        np.testing.assert_array_equal(c1[:, 0], coh[:, c], err_msg=f"column {c} alone")
    for c in CP.MIXED_IDENTICAL:
        np.testing.assert_array_equal(coh[K1:K1 + 8, c], coh[K0:K0 + 8, c], err_msg=f"column {c}: K1 is not K0")
        np.testing.assert_array_equal(CP.swapped_rows(coh[:, c])[:K3], coh[:K3, c])
    for c in (1, 3, 4, 6):
        assert np.abs(coh[K1:K1 + 8, c] - coh[K0:K0 + 8, c]).max() > 1e-9     # built, not mirrored
    rev, sr = _run(eng, p[:, ::-1].copy(), "lp_square", dim)
    assert np.all(sr == 0)
    np.testing.assert_array_equal(rev[:, ::-1], coh)


# ---- e. rows that rebuild on different segments -----------------------------------------------------------

def _schedules(dim):
    p = CP.for_dim(CP.schedule_points(), dim)
    return p, np.concatenate([p, p[:, ::-1]], axis=1), np.r_[0:12, 11:-1:-1]


@dims
def test_rows_rebuild_on_different_segments(eng, oracle, dim):
    p, both, at = _schedules(dim)
    ref = oracle("schedules", p, "bangbang", dim)
    coh, st = _run(eng, both, "bangbang", dim)
    print(f"dim {dim} schedules: builds required {[len(D4.bb_builds(p, c)) for c in range(12)]}")
    _vs_oracle(coh, st, ref[:, at], f"dim {dim} prop: schedules, both orders")
    for c in range(12):
        c1, s1 = _alone(eng, p, "bangbang", dim, c)
        assert s1[0] == 0
        for col in (c, 23 - c):
            np.testing.assert_array_equal(coh[:, col], c1[:, 0], err_msg=f"schedule point {c} in column {col}")


@dims
def test_schedules_on_the_per_lane_path(eng, oracle, dim):
    p, both, at = _schedules(dim)
    ref = oracle("schedules", p, "bangbang", dim)
    coh, st = _run(eng, both, "bangbang", dim, "0")
    keep = [c for c in range(24) if at[c] not in CP.SCHEDULE_LONG]
    _vs_oracle(coh, st, ref[:, at], f"dim {dim} per-lane: schedules without the long segment", keep)


@dims
def test_per_lane_path_on_one_long_dissipative_segment(eng, oracle, dim):
    p, _, _ = _schedules(dim)
    ref = oracle("schedules", p, "bangbang", dim)
    q = p[:, list(CP.SCHEDULE_LONG)].copy()
    coh, st = _run(eng, q, "bangbang", dim, "0")
    _vs_oracle(coh, st, ref[:, list(CP.SCHEDULE_LONG)], f"dim {dim} per-lane: one long dissipative segment")


# ---- f. non-unit xi and smooth-JP step counts ---------------------------------------------------------------

@dims
@paths
def test_non_unit_xi(eng, oracle, dim, path):
    """|xi| = 1.01 and 0.5: pulse 2 has its own key and is built; the other columns keep the
    bits they have without the perturbation."""
    p, q, special = CP.nonunit_xi()
    p, q = CP.for_dim(p, dim), CP.for_dim(q, dim)
    base, sb = _run(eng, p, "lp_square", dim, path)
    coh, st = _run(eng, q, "lp_square", dim, path)
    assert np.all(sb == 0)
    _vs_oracle(coh, st, oracle("nonunit_xi", q, "lp_square", dim), f"dim {dim} {path}: non-unit xi")
    others = [c for c in range(8) if c not in (1, 4)]
    np.testing.assert_array_equal(coh[:, others], base[:, others])
    for c in (1, 4):
        assert np.abs(coh[:, c] - base[:, c]).max() > 1e-6


@dims
@paths
@pytest.mark.parametrize("n_steps", CP.JP_STEPS)
def test_smooth_jp_step_counts(eng, oracle, dim, path, n_steps):
    p = CP.for_dim(CP.jp_points(), dim)
    batches = [("unequal", p)]
    if n_steps == 30:
        batches.append(("identical", D4.sym(p.copy())))
    for name, b in batches:
        assert E.symmetric_atoms(b) == (name == "identical")
        coh, st = _run(eng, b, "smooth_jp", dim, path, n_steps)
        _vs_oracle(coh, st, oracle("jp_" + name, b, "smooth_jp", dim, n_steps),
                   f"dim {dim} {path}: smooth JP, n_steps = {n_steps}, {name} atoms")


# ---- g. refused rows ---------------------------------------------------------------------------------------

def _check_refused(coh, st, clean, marks, what):
    bad = {c: (name, bit) for c, name, bit in marks}
    for c, (name, bit) in bad.items():
        if bit == N.STATUS_STEP_CAP:
            assert st[c] & N.STATUS_FAIL_MASK == N.STATUS_STEP_CAP, f"{what}: {name} in column {c}: status {st[c]}"
        else:
            assert st[c] & bit, f"{what}: {name} in column {c}: status {st[c]}"
    good = [c for c in range(coh.shape[1]) if c not in bad]
    assert np.all(st[good] == 0), f"{what}: status {st[good]} beside refused rows"
    np.testing.assert_array_equal(coh[:, good], clean[:, good], err_msg=f"{what}: beside refused rows")


@dims
@paths
@pytest.mark.parametrize("protocol", ["lp_square", "bangbang"])
def test_refused_rows_flag_their_point_only(eng, dim, path, protocol):
    """Each refused input at each of the four row positions of a wave: it is flagged, and its
    three neighbours have status 0 and the bits of the batch without it."""
    ns = 8 if protocol == "bangbang" else None
    clean_p, edited_p, marks = CP.refused_batch(protocol, dim)
    clean, s0 = _run(eng, clean_p, protocol, dim, path, ns)
    assert np.all(s0 == 0)
    coh, st = _run(eng, edited_p, protocol, dim, path, ns)
    print(f"dim {dim} {path} {protocol}: statuses of the refused rows "
          + " ".join(f"{name}@{c % 4}:{st[c]}" for c, name, _ in marks))
    _check_refused(coh, st, clean, marks, f"dim {dim} {path} {protocol}")
    # valid wave / wholly invalid wave / valid wave
    five = CP.for_dim(CP.five_valid(protocol), dim)
    w = np.concatenate([five[:, :4], five[:, :4], five[:, [4, 0, 1, 2]]], axis=1)
    edits = CP.invalid_columns(protocol, dim)
    names = ["nan", "omega_zero", "negative_rate", "nan_rates_too"]
    v = w.copy()
    for r, name in enumerate(names):
        edits[name][0](v, 4 + r)
    clean, s0 = _run(eng, w, protocol, dim, path, ns)
    assert np.all(s0 == 0)
    coh, st = _run(eng, v, protocol, dim, path, ns)
    _check_refused(coh, st, clean, [(4 + r, name, N.STATUS_BAD_INPUT) for r, name in enumerate(names)],
                   f"dim {dim} {path} {protocol}: an invalid wave between valid ones")


# ---- h. launch shape ------------------------------------------------------------------------------------------

@dims
def test_launch_shapes(eng, dim):
    """37 points are 10 blocks, the last with one live row: a grid that is no multiple of 8.
    Every prefix of 1 ... 8 points, the reversed batch, and a 38-block launch whose blocks the
    kernel permutes return the same bits per point."""
    p = CP.for_dim(CP.launch_points("lp_square"), dim)
    coh, st = _run(eng, p, "lp_square", dim)
    assert np.all(st == 0) and np.all(np.isfinite(coh))
    for n in range(1, 9):
        c, s = _run(eng, p[:, :n].copy(), "lp_square", dim)
        assert np.all(s == 0)
        np.testing.assert_array_equal(c, coh[:, :n], err_msg=f"prefix of {n} points")
    rev, sr = _run(eng, p[:, ::-1].copy(), "lp_square", dim)
    assert np.all(sr == 0)
    np.testing.assert_array_equal(rev[:, ::-1], coh)
    # xcd_block permutes the blocks of whole 32-block groups only, so 10 blocks keep their
    # order.  149 points are 38 blocks: one permuted group, a tail of 6 in order, one live row
    # in the last -- the smallest launch on that path.  Column c holds point c mod 37.
    src = np.arange(149) % 37
    big, sb = _run(eng, p[:, src].copy(), "lp_square", dim)
    assert np.all(sb == 0)
    np.testing.assert_array_equal(big, coh[:, src])


# ---- i. the device-resident path -------------------------------------------------------------------------------

@dims
@pytest.mark.parametrize("protocol", ["lp_square", "bangbang"])
def test_device_resident_batch(eng, dim, protocol):
    """CoherenceDeviceBatch (ryd_run_coherences_device, the path the bench times) returns
    run_coherences' rows and status bit for bit."""
    p = CP.for_dim(CP.launch_points(protocol), dim)
    coh, st = _run(eng, p, protocol, dim)
    assert np.all(st == 0)
    db = E.CoherenceDeviceBatch(eng, p, protocol, dim=dim)
    try:
        db.launch()
        c1, s1 = db.fetch()
        ms = db.launch(timed=True)
        c2, s2 = db.fetch()
    finally:
        db.free()
    assert ms > 0.0
    for c, s in ((c1, s1), (c2, s2)):
        np.testing.assert_array_equal(c, coh)
        np.testing.assert_array_equal(s, st)
