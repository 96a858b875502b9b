"""The inputs of test_gpu_coh_build.py, checked before they reach a GPU (no GPU here): the
depths and series degrees the ladders walk on both of the coherence kernels' bounds, the bank
depths, build counts and atom classes of the new batches, the statuses the refused rows must
get by the kernels' own rules, and the oracle itself where the GPU tests lean on it: dim 3
against dim 4 at GMJ = 0, the atom-swap row mapping, and the identity map's rows."""
import numpy as np
import pytest

import coh_points as CP
import dim4_points as D4
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from process_map4_util import process_map_dim, spec4_from_params
from process_map_util import rows_from_map


def _depths_degrees(p, bound):
    x = bound(p, "lp_square") * p[N.P["TAU"]]
    dk = [D4.depth_terms4(v) for v in x]
    return x, [d[0] for d in dk], [d[2] for d in dk]


def test_ladders_walk_both_bounds():
    """tau ladder: depths 6, 7, 8 on the main bound and 5, 6, 7 on the V-free one.  x ladder:
    series degrees 1-13 and the identity on the main bound, 1-11 and the identity on the V-free
    one, no squarings below X_BASE, and the last point alone the identity on both."""
    p = D4.tau_ladder4()
    for bound, want in zip(CP.BOUNDS, ({6, 7, 8}, {5, 6, 7})):
        x, s, _ = _depths_degrees(p, bound)
        print(f"tau ladder, {bound.__name__}: x {x.min():.1f} ... {x.max():.1f}, depths {sorted(set(s))}")
        assert set(s) == want
        assert min(D4.depth_margin(v) for v in x) >= D4.DEPTH_MARGIN
    p = D4.x_ladder4()
    assert p.shape[1] == 48
    for bound, top in zip(CP.BOUNDS, (13, 11)):
        x, s, kt = _depths_degrees(p, bound)
        print(f"x ladder, {bound.__name__}: x {x.max():.3g} ... {x.min():.3g}, degrees {sorted(set(kt))}")
        assert set(kt) == set(range(1, top + 1)) | {-1}
        assert kt[-1] == -1 and all(k >= 1 for k in kt[:-1])
        assert set(s) <= {0, 1} and all(d == 0 for d, v in zip(s, x) if v <= D4.X_BASE)
    # the V-free bank keeps its distance from every depth and term boundary
    x = CP.omega_vfree(p, "lp_square") * p[N.P["TAU"]]
    m = min(min(D4.depth_margin(v), D4.term_margin(v)) for v in x)
    print(f"x ladder on the V-free bound: least margin {m:.2e}")
    assert m >= 3e-2
    for q in (D4.tau_ladder4(), D4.x_ladder4()):
        assert E.symmetric_atoms(q) and E.symmetric_atoms(CP.twin3(q))
        assert not CP.twin3(q)[list(CP.GMJ)].any() and q[list(CP.GMJ)].all()


def test_twin_ladders_keep_their_ends():
    """The dim-3 twins (GMJ = 0: a smaller bound) still change depth along the tau ladder, run
    every series degree the dim-4 x ladder runs on the main bound, and end in the identity."""
    t = CP.twin3(D4.tau_ladder4())
    for bound in CP.BOUNDS:
        _, s, _ = _depths_degrees(t, bound)
        assert len(set(s)) >= 2
    t = CP.twin3(D4.x_ladder4())
    for bound, top in zip(CP.BOUNDS, (13, 11)):
        _, _, kt = _depths_degrees(t, bound)
        print(f"x ladder twin, {bound.__name__}: degrees {sorted(set(kt))}")
        assert set(range(1, top + 1)) <= set(kt) and kt[-1] == -1 and all(k >= 1 for k in kt[:-1])


def test_equal_bank_points():
    p = CP.equal_bank_points()
    assert p[N.P["V"], 0] == 0.0
    np.testing.assert_allclose(p[N.P["V"]] / p[N.P["OMEGA"]], [0.0, 0.3, 1000.0], rtol=1e-15)
    d = [CP.bank_depths(p, i) for i in range(3)]
    print(f"equal_bank_points: (main, V-free) depths {d}")
    assert d[0][0] == d[0][1]
    assert CP.lp_build_x(p, 0, CP.omega_main) == CP.lp_build_x(p, 0, CP.omega_vfree)
    assert 0 <= d[1][0] - d[1][1] <= 1
    assert d[2][0] - d[2][1] >= 5
    for dim in CP.DIMS:
        assert not E.symmetric_atoms(CP.for_dim(p, dim))


@pytest.mark.parametrize("dim", CP.DIMS)
def test_mixed_wave(dim):
    p = CP.mixed_wave(dim)
    assert p.shape[1] == 8 and not E.symmetric_atoms(p)
    rates = D4.RATES4 if dim == 4 else D4.RATES
    for c in range(8):
        differ = [k for k in D4.RATES4 if p[N.P[k + "_A"], c] != p[N.P[k + "_B"], c]]
        if c in CP.MIXED_IDENTICAL:
            assert differ == [] and E.symmetric_atoms(p[:, c:c + 1])
        elif c == 6:
            assert differ == ["GMJ" if dim == 4 else "GPHI"]
        else:
            assert differ == list(rates)
    if dim == 3:
        assert not p[list(CP.GMJ)].any()
    assert sorted(set(range(8)) - set(CP.MIXED_IDENTICAL)) == [1, 3, 4, 6]


def test_schedule_points():
    p = CP.schedule_points()
    assert p.shape[1] == 12
    assert E.symmetric_atoms(p[:, :6]) and E.symmetric_atoms(CP.twin3(p[:, :6]))
    for dim in CP.DIMS:
        q = CP.for_dim(p, dim)
        for c in range(6, 12):
            for k in (D4.RATES4 if dim == 4 else D4.RATES):
                assert q[N.P[k + "_A"], c] != q[N.P[k + "_B"], c]
        builds = [D4.bb_builds(q, c) for c in range(12)]
        assert tuple(len(b) for b in builds) == CP.SCHEDULE_BUILDS
        for c, b in enumerate(builds):
            assert min(D4.depth_margin(v) for v in b) >= D4.DEPTH_MARGIN, (dim, c)
            assert min(D4.term_margin(v) for v in b) >= D4.DEPTH_MARGIN, (dim, c)
    np.testing.assert_array_equal(p[N.P["NSEG"]], [5, 5, 5, 1, 8, 2] * 2)
    dts = [dt for _, dt in D4.bb_segments(p, 4)]
    assert len(dts) == 8 and len(set(dts)) == 8 and min(dts) > 0
    for c in CP.SCHEDULE_LONG:
        assert D4.bb_builds(p, c)[0] > 1e4            # the one long segment


def test_nonunit_xi():
    p, q, special = CP.nonunit_xi()
    assert special == (1, 4, 6)
    assert [len(D4.lp_builds(q, c)) for c in special] == [2, 2, 1]
    assert len(D4.lp_builds(p, 6)) == 1
    np.testing.assert_allclose(np.hypot(q[N.P["XI_RE"]], q[N.P["XI_IM"]])[list(special)], [1.01, 0.5, 1.0], rtol=1e-15)
    for c in (1, 4):                                  # phases off the axes
        assert min(abs(q[N.P["XI_RE"], c]), abs(q[N.P["XI_IM"], c])) > 0.1
    others = [c for c in range(8) if c not in (1, 4)]
    np.testing.assert_array_equal(p[:, others], q[:, others])
    np.testing.assert_array_equal(CP.nonunit_xi()[1], q)           # fixed seed


def test_launch_and_valid_points():
    for protocol in ("lp_square", "bangbang"):
        p = CP.launch_points(protocol)
        assert p.shape[1] == 37 and (37 + 3) // 4 == 10 and 37 % 4 == 1
        assert not E.symmetric_atoms(p) and E.symmetric_atoms(p[:, 0:1]) and not E.symmetric_atoms(p[:, 1:2])
        f = CP.five_valid(protocol)
        assert E.symmetric_atoms(f[:, [0, 2]]) and not E.symmetric_atoms(f[:, [1]])
    x = D4.omega4(CP.five_valid("lp_square"), "lp_square") * CP.five_valid("lp_square")[N.P["TAU"]]
    assert len({D4.depth_terms4(v)[0] for v in x}) >= 3           # mixed depth


def _point_valid(p, c, protocol, dim, n_steps):
    """point_valid and gmj_valid of ryd_engine.hip, restated."""
    g = lambda k: p[N.P[k], c]
    ok = g("OMEGA") > 0 and all(np.isfinite(g(k)) for k in ("OMEGA", "V", "DELTA", "DELTA1"))
    for k in D4.RATES:
        for a in "AB":
            ok = ok and g(f"{k}_{a}") >= 0 and np.isfinite(g(f"{k}_{a}"))
    if protocol == "bangbang":
        nseg = g("NSEG")
        ok = ok and np.isfinite(nseg) and 1 <= int(nseg) <= 8 and int(nseg) <= n_steps
    else:
        ok = ok and g("TAU") > 0 and np.isfinite(g("TAU"))
    if dim == 4:
        ok = ok and all(g(k) >= 0 and np.isfinite(g(k)) for k in ("GMJ_A", "GMJ_B"))
    return bool(ok)


@pytest.mark.parametrize("dim", CP.DIMS)
@pytest.mark.parametrize("protocol", ["lp_square", "bangbang"])
def test_refused_batch(protocol, dim):
    clean, edited, marks = CP.refused_batch(protocol, dim)
    names = {m[1] for m in marks}
    want = {"nan", "nan_rates_too", "omega_zero", "negative_rate"}
    want |= {"nseg_0", "nseg_9"} if protocol == "bangbang" else {"tau_inf", "cap"}
    want |= {"gmj_nan"} if dim == 4 else set()
    assert names == want and len(marks) == 4 * len(want) and clean.shape[1] == 4 * len(marks) <= 112
    at = {m[0]: m for m in marks}
    assert sorted(c % 4 for c in at) == sorted(list(range(4)) * len(want))    # every row position
    for c in range(clean.shape[1]):
        assert _point_valid(clean, c, protocol, dim, 8)
        if c not in at:
            np.testing.assert_array_equal(clean[:, c], edited[:, c])
            continue
        _, name, bit = at[c]
        if name == "cap":
            assert bit == N.STATUS_STEP_CAP and _point_valid(edited, c, protocol, dim, 8)
            x = (CP.omega_main(edited, protocol) * edited[N.P["TAU"]])[c]
            assert x > 1.4 * D4.X_CAP
        else:
            assert bit == N.STATUS_BAD_INPUT and not _point_valid(edited, c, protocol, dim, 8)
        if name == "nan":
            assert all(edited[N.P[k + a], c] == 0.0 for k in D4.RATES4 for a in ("_A", "_B"))
            assert np.isnan(np.delete(edited[:, c], [N.P[k + a] for k in D4.RATES4 for a in ("_A", "_B")])).all()


def test_four_kinds_of_row():
    rows, batch, order = CP.four_kinds()
    assert batch.shape[1] == 96 and len(set(order)) == 24
    (s0, _, k0, id0), (s1, _, k1, id1), (s2, _, _, id2) = (
        D4.depth_terms4(CP.lp_build_x(rows, i, CP.omega_main)[0]) for i in range(3))
    assert id0 and k0 == -1 and s0 == 0
    assert (s1, k1, id1) == (0, 13, False)
    assert s2 >= 13 and not id2
    for i in (0, 1):                                               # no squarings on the V-free bank either
        assert D4.depth_terms4(CP.lp_build_x(rows, i, CP.omega_vfree)[0])[0] == 0
    assert D4.depth_terms4(CP.lp_build_x(rows, 0, CP.omega_vfree)[0])[3]
    assert np.isnan(rows[:, 3]).all()
    for w, o in enumerate(order):
        np.testing.assert_array_equal(batch[:, 4 * w:4 * w + 4], rows[:, list(o)])


# ---- the oracle itself ------------------------------------------------------------------------

def test_oracle_dimensions_agree_at_zero_mj():
    """On strong points with GMJ = 0 the 81 x 81 and the 256 x 256 oracle give the same rows."""
    worst = 0.0
    for protocol, p, ns in (("lp_square", CP.twin3(CP.equal_bank_points()), None),
                            ("lp_square", CP.mixed_wave(3), None),
                            ("lp_square", CP.twin3(CP.nonunit_xi()[1][:, [1, 4, 6]]), None),
                            ("bangbang", CP.twin3(CP.schedule_points()), None),
                            ("smooth_jp", CP.twin3(CP.jp_points()), 3)):
        for i in range(p.shape[1]):
            if protocol == "bangbang" and i in (1, 3, 7, 9):      # bb_schedule_points' nominal points
                continue
            r3 = CP.oracle_rows(p, i, protocol, 3, ns)
            r4 = CP.oracle_rows(p, i, protocol, 4, ns)
            worst = max(worst, float(np.abs(r3 - r4).max()))
            assert np.abs(r3).max() > 1e-2
    print(f"oracle dim 3 / dim 4 at GMJ = 0: max|d rows| = {worst:.2e}")
    assert worst < 1e-13


def test_oracle_atom_swap_row_mapping():
    """The atom-swapped point's K1 rows are the point's K0 rows (and back), K2 stays, K3 is
    conjugated: CP.swapped_rows, pinned against rows_from_map on a strong unequal point."""
    p = D4.random_points4(np.random.default_rng(20261109), 1, "lp_square", "strong")
    assert not E.symmetric_atoms(p)
    rows = CP.oracle_rows(p, 0, "lp_square", 4)
    mirror = CP.oracle_rows(D4.swap_atoms(p), 0, "lp_square", 4)
    err = float(np.abs(mirror - CP.swapped_rows(rows)).max())
    print(f"oracle atom swap: max|d rows| = {err:.2e}")
    assert err < 1e-13
    k0, k1 = N.C["K0"], N.C["K1"]
    np.testing.assert_allclose(mirror[k1:k1 + 8], rows[k0:k0 + 8], atol=1e-13, rtol=0)
    assert np.abs(rows[k1:k1 + 8] - rows[k0:k0 + 8]).max() > 1e-6      # the atoms do differ
    # identical atoms: the mapping is the identity on K0 / K1 and K3 is real
    q = D4.sym(p.copy())
    same = CP.oracle_rows(q, 0, "lp_square", 4)
    np.testing.assert_allclose(CP.swapped_rows(same), same, atol=1e-13, rtol=0)


def test_oracle_identity_rows():
    """The identity end of the x ladder: the oracle's rows are those of the identity map."""
    want = CP.identity_rows()
    assert want.sum() == 6.0 and set(want) == {0.0, 1.0}
    for j in (N.C["K0"], N.C["K0"] + 6, N.C["K1"], N.C["K1"] + 6, N.C["K2"], N.C["K3"]):
        assert want[j] == 1.0
    p = D4.x_ladder4()
    for dim in CP.DIMS:
        q = CP.for_dim(p, dim)
        got = CP.oracle_rows(q, q.shape[1] - 1, "lp_square", dim)
        assert np.abs(got - want).max() <= 1e-15
    S = process_map_dim(spec4_from_params(p, p.shape[1] - 1, "lp_square"))
    np.testing.assert_allclose(rows_from_map(S)[1][:, 0], want, atol=1e-15, rtol=0)
