"""tests/sched_ket_points.py checks itself on the CPU: its analytic phase Jacobian against
central differences of its own chain, the gauge sum, and
``pulse_schedules.gate_fidelity_and_gradient`` against central differences of
``noise_models.gate_fidelity`` -- on the first four points of the batch "random", segments 0, 5
and 19.

Bounds.  Central differences at h = 1e-6 carry the difference quotient's rounding eps / h ~
1e-10 per unit of the differenced quantity and a truncation h^2 f''' / 6 ~ 1e-12; the bound
1e-7 leaves room for both (measured: 3.9e-9 on the overlaps, 8.9e-10 on the fidelities; one
run on one machine, not a tolerance).  sum_s da/dphi_s is zero in exact arithmetic -- a global
phase of the drive changes nothing -- and is a sum of 20 terms of size <= 2 rounded at 1e-16:
1e-12.
"""
import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import pulse_schedules as PS
from tests import sched_ket_points as KP
from tests import sched_points as SP

H = 1e-6
SEGS = (0, 5, 19)
NPT = 4


@pytest.fixture(scope="module")
def base():
    b = SP.batch("random")
    p, s = b["params"][:, :NPT], b["sched"][:NPT]
    return p, s, KP.chain(p, s)


@pytest.fixture(scope="module")
def shifted(base):
    """The chains with segment s's phase moved by +-H, for the three segments."""
    p, s, _ = base
    out = {}
    for seg in SEGS:
        for sign in (+1, -1):
            t = s.copy()
            t[:, N.SC["PHASE"], seg] += sign * H
            out[seg, sign] = KP.chain(p, t)
    return out


def test_jacobian_against_central_differences(base, shifted):
    _, _, ref = base
    worst = 0.0
    for seg in SEGS:
        for c, key in enumerate(("a01", "a11")):
            fd = (shifted[seg, +1][key] - shifted[seg, -1][key]) / (2 * H)
            worst = max(worst, float(np.abs(fd - ref["J"][:, c, seg]).max()))
    print(f"analytic Jacobian against central differences: {worst:.2e}")
    assert worst <= 1e-7


def test_gauge_sum_is_zero(base):
    _, _, ref = base
    worst = float(np.abs(ref["J"].sum(axis=2)).max())
    print(f"sum over segments of the Jacobian: {worst:.2e}")
    assert worst <= 1e-12


def test_zero_length_segment_has_an_exact_zero_column(base):
    _, s, ref = base
    zero = s[:, N.SC["X"], :] == 0.0
    assert zero.sum(axis=1).tolist() == [1] * NPT
    for c in range(2):
        assert np.all(ref["J"][:, c, :][zero] == 0.0)
    # and a segment of positive length does move the overlaps
    assert np.all(np.abs(ref["J"][:, 1, :][~zero]).reshape(NPT, -1).max(axis=1) > 1e-3)


@pytest.mark.parametrize("which, idx", [("process", 0), ("avg_gate", 1)])
def test_fidelity_gradient_against_central_differences(base, shifted, which, idx):
    _, _, ref = base
    F, dF = PS.gate_fidelity_and_gradient(ref["a01"], ref["a11"], ref["J"], which)
    np.testing.assert_allclose(F, NM.gate_fidelity(NM.ket_maps(ref["kets"]))[idx], rtol=0, atol=1e-14)
    assert dF.shape == (NPT, ref["J"].shape[2])
    worst = 0.0
    for seg in SEGS:
        fp = NM.gate_fidelity(NM.ket_maps(shifted[seg, +1]["kets"]))[idx]
        fm = NM.gate_fidelity(NM.ket_maps(shifted[seg, -1]["kets"]))[idx]
        worst = max(worst, float(np.abs((fp - fm) / (2 * H) - dF[:, seg]).max()))
    print(f"{which} fidelity gradient against central differences: {worst:.2e}")
    assert worst <= 1e-7


def test_fidelity_gradient_refuses_bad_arguments(base):
    _, _, ref = base
    with pytest.raises(ValueError):
        PS.gate_fidelity_and_gradient(ref["a01"], ref["a11"], ref["J"], "other")
    with pytest.raises(ValueError):
        PS.gate_fidelity_and_gradient(ref["a01"], ref["a11"][:2], ref["J"])
