"""hilbert_space_dim = 4 with GMJ_A = GMJ_B = 0 is the dim-3 model: |r-> is never reached.
The per-lane Chebyshev kernels (states and coherences) run one body for both dimensions, and
the coherence propagator kernels repeat one control flow, so each is held here from both
sides: the same points through dim 3 and dim 4 agree to the project's 1e-10.  (The oracle's 81 x 81 and 256 x 256
maps on these parameter columns agree to 1e-13.)"""
import numpy as np
import pytest

import coh_points as CP
import dim4_points as D4
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from process_map_util import PATHS, coh_path
from test_gpu_parity import _random_points

pytestmark = pytest.mark.gpu
TOL = 1e-10
CASES = [("lp_square", None), ("smooth_jp", 30), ("bangbang", None)]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _points(protocol, identical):
    p = _random_points(np.random.default_rng(99), 5, protocol)
    assert not p[N.P["GMJ_A"]].any() and not p[N.P["GMJ_B"]].any()
    if identical:
        for k in ("G1", "G0", "GPHI", "GSC"):
            p[N.P[k + "_B"]] = p[N.P[k + "_A"]]
    assert E.symmetric_atoms(p) == identical
    return p


@pytest.mark.parametrize("identical", [False, True], ids=["unequal", "identical"])
@pytest.mark.parametrize("protocol,n_steps", CASES)
def test_coherence_rows_agree_across_dimensions(eng, protocol, n_steps, identical):
    p = _points(protocol, identical)
    for path in PATHS:
        with coh_path(path):
            c3, s3 = eng.run_coherences(p, protocol, n_steps=n_steps, dim=3)
            c4, s4 = eng.run_coherences(p, protocol, n_steps=n_steps, dim=4)
        assert np.all(s3 == 0) and np.all(s4 == 0)
        assert c3.shape == c4.shape == (N.NCOH, 5)
        print(f"{protocol} RYD_COH_PROP={path}: max|coh4 - coh3| per point = "
              f"{np.abs(c4 - c3).max(axis=0)}")
        np.testing.assert_allclose(c4, c3, atol=TOL, rtol=0, err_msg=f"{protocol}/{path}")


def _strong_points(protocol, identical):
    """Five "strong" points (V / Omega 0.3 ... 30, rates that are percents of Omega: every
    sector coordinate is large against TOL) with the GMJ columns zeroed."""
    seed = 20261110 + [c[0] for c in CASES].index(protocol)
    p = CP.twin3(D4.random_points4(np.random.default_rng(seed), 5, protocol, "strong"))
    if identical:
        p = D4.sym(p)
    assert E.symmetric_atoms(p) == identical
    return p


@pytest.mark.parametrize("identical", [False, True], ids=["unequal", "identical"])
@pytest.mark.parametrize("protocol,n_steps", CASES)
def test_strong_coherence_rows_agree_across_dimensions(eng, protocol, n_steps, identical):
    p = _strong_points(protocol, identical)
    for path in PATHS:
        with coh_path(path):
            c3, s3 = eng.run_coherences(p, protocol, n_steps=n_steps, dim=3)
            c4, s4 = eng.run_coherences(p, protocol, n_steps=n_steps, dim=4)
        assert np.all(s3 == 0) and np.all(s4 == 0)
        print(f"strong {protocol} RYD_COH_PROP={path}: max|coh4 - coh3| per point = "
              f"{np.abs(c4 - c3).max(axis=0)}")
        np.testing.assert_allclose(c4, c3, atol=TOL, rtol=0, err_msg=f"{protocol}/{path}")


def test_x_ladder_twin_agrees_across_dimensions(eng):
    """The x ladder's dim-3 twin: every series degree without squarings and the identity build,
    through both dimensions' kernels on the same columns."""
    p = CP.twin3(D4.x_ladder4())
    for path in PATHS:
        with coh_path(path):
            c3, s3 = eng.run_coherences(p, "lp_square", dim=3)
            c4, s4 = eng.run_coherences(p, "lp_square", dim=4)
        assert np.all(s3 == 0) and np.all(s4 == 0)
        print(f"x ladder twin RYD_COH_PROP={path}: max|coh4 - coh3| = {np.abs(c4 - c3).max():.3e}")
        np.testing.assert_allclose(c4, c3, atol=TOL, rtol=0, err_msg=f"x ladder twin/{path}")
        np.testing.assert_array_equal(c3[:, -1], CP.identity_rows())
        np.testing.assert_array_equal(c4[:, -1], CP.identity_rows())


@pytest.mark.parametrize("identical", [False, True], ids=["unequal", "identical"])
@pytest.mark.parametrize("protocol,n_steps", CASES)
def test_state_rows_agree_across_dimensions(eng, protocol, n_steps, identical):
    """lindblad4_cheb_kernel against lindblad_cheb_kernel: row 6a + b of the 36-row state is
    row 5a + b of the 25-row one for a, b < 5; the e-- rows stay empty."""
    p = _points(protocol, identical)
    r3 = eng.run(p, protocol, "lindblad", n_steps=n_steps, method="cheb_vector", dim=3)
    r4 = eng.run(p, protocol, "lindblad", n_steps=n_steps, method="cheb_vector", dim=4)
    assert np.all(r3.status == 0) and np.all(r4.status == 0)
    s3 = r3.state.reshape(5, 5, -1)
    s4 = r4.state.reshape(6, 6, -1)
    assert s3.shape[2] == s4.shape[2] == 20
    d = np.abs(s4[:5, :5] - s3).max()
    minus = max(np.abs(s4[5]).max(), np.abs(s4[:, 5]).max())
    print(f"{protocol}: max|state4 - state3| = {d:.3e}, max |e-- rows| = {minus:.3e}")
    np.testing.assert_allclose(s4[:5, :5], s3, atol=TOL, rtol=0)
    assert minus <= TOL
