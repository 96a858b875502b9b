"""The inputs of test_gpu_dim4_build.py, checked before they reach a GPU (no GPU here): the
identical-atom flag of every batch, the ladders' distance from the depth boundaries and the
depths, series lengths and build counts they are meant to reach, and the oracle alone on one
strong unequal-atom point (trace, positivity, and the atom-swap mirror the GPU test uses)."""
import numpy as np
import pytest

import dim4_points as D4
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from process_map4_util import spec4_from_params


@pytest.mark.parametrize("protocol", ["lp_square", "smooth_jp", "bangbang"])
def test_identical_atom_flag(protocol):
    rng = np.random.default_rng(1)
    for kind in ("nominal", "strong", ["nominal", "strong"] * 3):
        p = D4.random_points4(rng, 6, protocol, kind)
        assert not E.symmetric_atoms(p)
        for k in D4.RATES4:                                   # every rate column differs
            assert np.all(p[N.P[k + "_A"]] != p[N.P[k + "_B"]])
        q = D4.sym(p.copy())
        assert E.symmetric_atoms(q)
        q[N.P["GMJ_B"], 3] *= 3.0                             # the mJ rate alone
        assert all(np.array_equal(q[N.P[k + "_A"]], q[N.P[k + "_B"]]) for k in D4.RATES)
        assert not E.symmetric_atoms(q)
        assert E.symmetric_atoms(D4.swap_atoms(D4.swap_atoms(p))) == E.symmetric_atoms(p)
        np.testing.assert_array_equal(D4.swap_atoms(D4.swap_atoms(p)), p)
    for p in (D4.tau_ladder4(), D4.x_ladder4(), D4.bb_schedule_points()):
        assert E.symmetric_atoms(p)


def test_point_classes():
    rng = np.random.default_rng(2)
    p = D4.random_points4(rng, 200, "lp_square", ["nominal", "strong"] * 100)
    Om, r = p[N.P["OMEGA"]], p[N.P["V"]] / p[N.P["OMEGA"]]
    nom, strong = slice(0, None, 2), slice(1, None, 2)
    assert r[nom].min() >= 10 and r[nom].max() <= 1000
    assert r[strong].min() >= 10 ** -0.5 and r[strong].max() <= 10 ** 1.5
    assert np.all(p[N.P["DELTA1"], strong] <= 0.3 * Om[strong])
    for k, hi in D4.STRONG_RATES:
        for a in "AB":
            g = p[N.P[f"{k}_{a}"]]
            assert np.all(g >= 0) and np.all(g[strong] <= hi * Om[strong])
    assert np.all(p[N.P["GMJ_A"], nom] <= 2e5) and np.all(p[N.P["GMJ_B"], nom] <= 2e5)
    # bang-bang keeps per-point switching times and the zero-length segment
    b = D4.random_points4(rng, 5, "bangbang", "strong")
    sw = b[N.P["SWT0"]:N.P["SWT0"] + 4]
    assert np.all(sw[1] == sw[0]) and np.unique(sw[0]).size == 5
    assert all(len(D4.bb_builds(D4.sym(b), i)) == 4 for i in range(5))


def test_depth_terms_restated():
    assert D4.depth_terms4(0.5) == (0, 0.5, 13, False)
    assert D4.depth_terms4(0.5000001)[0] == 1 and D4.depth_terms4(1.0)[0] == 1
    assert D4.depth_terms4(1.0000001)[0] == 2
    s, xs, kt, ident = D4.depth_terms4(3e6)
    assert 0.25 < xs <= 0.5 and xs * 2 ** s == 3e6 and kt in (11, 12, 13) and not ident
    assert D4.depth_terms4(1e-20) == (0, 1e-20, -1, True)
    assert D4.depth_terms4(1.1e-20)[2:] == (1, False)
    assert D4.depth_margin(0.5 * 2 ** 7 * (1 + 3e-7)) < D4.DEPTH_MARGIN < D4.depth_margin(0.5 * 2 ** 7 * (1 - 3e-6))
    with pytest.raises(AssertionError):
        D4.assert_depth_margin([0.3, 2.0 * (1 + 1e-7)], "a boundary")
    # the bound: rsum counts the mJ rate twice per atom
    p = D4.lp_strong_base()
    q = p.copy()
    q[N.P["GMJ_A"]] += 1000.0
    assert D4.omega4(q, "lp_square")[0] - D4.omega4(p, "lp_square")[0] == pytest.approx(2000.0, abs=1e-6)


def test_ladders_reach_what_they_claim():
    p = D4.tau_ladder4()
    assert p.shape[1] == 33
    x = D4.omega4(p, "lp_square") * p[N.P["TAU"]]
    s = np.array([D4.depth_terms4(v)[0] for v in x])
    assert np.all(np.diff(s) >= 0) and np.unique(s).size == 3 and s[-1] == s[0] + 2
    assert min(D4.depth_margin(v) for v in x) >= D4.DEPTH_MARGIN
    assert all(len(D4.lp_builds(p, i)) == 1 for i in (0, 32))
    p = D4.x_ladder4()
    x = D4.omega4(p, "lp_square") * p[N.P["TAU"]]
    assert min(D4.depth_margin(v) for v in x) >= D4.DEPTH_MARGIN
    kt = [D4.depth_terms4(v)[2] for v in x]
    assert set(range(1, 14)) <= set(kt) and kt[-1] == -1 and D4.depth_terms4(x[-1])[3]
    assert all(k >= 1 for k in kt[:-1])
    # each threshold is straddled: the two points around it differ by one term
    for t in D4.TH_BELOW:
        near = [k for v, k in zip(x, kt) if abs(v / (2 * t) - 1) < 1e-8]
        assert len(near) == 2 and near[0] == near[1] + 1
    p = D4.bb_schedule_points()
    builds = [D4.bb_builds(p, i) for i in range(4)]
    assert [len(b) for b in builds] == [1, 5, 4, 1]
    dts = [[dt for _, dt in D4.bb_segments(p, i)] for i in range(4)]
    assert len(set(dts[0])) == 1 and len(set(w for w, _ in D4.bb_segments(p, 0))) == 1
    assert len(set(dts[1])) == 5 and min(dts[1]) > 0
    assert dts[2][0] == 0.0 and len(set(dts[2])) == 5
    assert len(dts[3]) == 1
    for b in builds:
        assert min(D4.depth_margin(v) for v in b) >= D4.DEPTH_MARGIN


def test_oracle_alone_on_a_strong_unequal_point():
    """Trace, positivity and the atom-swap mirror of the oracle itself: exchanging the A and B
    columns gives rho with the atoms swapped and inputs 01 <-> 10 exchanged.  Every coordinate
    class of a strong point is large against 1e-10."""
    p = D4.random_points4(np.random.default_rng(20261022), 1, "lp_square", "strong")
    assert not E.symmetric_atoms(p)
    rho = D4.run_segments(spec4_from_params(p, 0, "lp_square"))
    assert rho.shape == (4, 16, 16)
    np.testing.assert_allclose(np.einsum("kaa->k", rho), 1.0, atol=1e-12)
    np.testing.assert_allclose(rho, np.conj(np.swapaxes(rho, -1, -2)), atol=1e-13)
    assert np.linalg.eigvalsh(rho).min() > -1e-12
    rminus = [i for i in range(16) if 3 in divmod(i, 4)]
    big = max(np.abs(rho[:, rminus, :]).max(), np.abs(rho[:, :, rminus]).max())
    print(f"largest |rho| entry touching |r->: {big:.2e}")
    assert big > 1e-2
    mirror = D4.run_segments(spec4_from_params(D4.swap_atoms(p), 0, "lp_square"))
    err = np.abs(mirror - D4.swap_rho(rho)).max()
    print(f"oracle mirror: max|d rho| = {err:.2e}")
    assert err < 1e-12
    assert np.abs(mirror - rho).max() > 1e-6                  # the atoms do differ
