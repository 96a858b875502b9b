"""The oracle maps behind tests/test_gpu_schedule_coherences.py, recomputed here on the CPU:
every batch's map (tests/sched_coh_points.py: expm of the full Liouvillian per segment, the 16
qubit matrix units chained through) equals the recorded tests/golden/sched_maps.npz, its
diagonal block is the recorded state chain of tests/golden/sched_oracle.npz (an independent
composition: evolve_state on density matrices), and its Choi matrix is positive."""
import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from oracle import lindblad_oracle as O
from tests import sched_coh_points as SC
from tests import sched_points as SP


def test_batches_are_what_the_issue_asks():
    for name in SP.NAMES:                            # taken unchanged
        assert SC.batch(name) is SP.batch(name)
    a = SC.batch("aba")["sched"]
    assert SC.batch("aba")["params"].shape == (N.NPARAM, 5) and a.shape == (5, 4, 6)
    amp = a[:, N.SC["AMP"]]
    for i in range(5):
        A, B = amp[i, 0], amp[i, 1]
        assert A != B and list(amp[i]) == [A, B, A, B, A, A]
    assert np.all(np.ptp(a[:, N.SC["X"]], axis=1) == 0) and np.all(np.ptp(a[:, N.SC["DELTA"]], axis=1) == 0)
    assert np.all(np.ptp(a[:, N.SC["PHASE"]], axis=1) > 0)
    s = SC.batch("step16")["sched"]
    assert SC.batch("step16")["params"].shape == (N.NPARAM, 4) and s.shape == (4, 4, 33)
    amp = s[:, N.SC["AMP"]]
    assert np.all(amp[:, :16] == amp[:, :1]) and np.all(amp[:, 16:] == amp[:, 16:17]) and np.all(amp[:, 15] != amp[:, 16])
    assert np.all(np.ptp(s[:, N.SC["X"]], axis=1) == 0) and np.all(np.ptp(s[:, N.SC["DELTA"]], axis=1) == 0)
    for name in SC.NAMES:
        p = SC.batch(name)["params"]
        for k in ("G1", "G0", "GPHI", "GSC"):
            np.testing.assert_array_equal(p[N.P[k + "_A"]], p[N.P[k + "_B"]])
        assert SC.golden(name).shape == (p.shape[1], 16, 16)


@pytest.mark.parametrize("name", SC.NAMES)
def test_recorded_maps(name):
    """What the GPU tests read: finite, the diagonal block equal to the recorded state chains
    (<= 1e-13; the batches of this module have none), Choi matrix positive (>= -1e-12)."""
    S = SC.golden(name)
    assert np.all(np.isfinite(S))
    if name in SP.NAMES:
        rho = SP.golden(name)[:, :, O.QUBIT_INDEX][:, :, :, O.QUBIT_INDEX]
        err = float(np.abs(SC.diagonal_block(S) - rho).max())
        print(f"{name}: diagonal block against the recorded chains {err:.2e}")
        assert err <= 1e-13
    J = np.stack([O.choi_matrix(s) for s in S])
    assert float(np.abs(J - J.conj().transpose(0, 2, 1)).max()) < 1e-13
    w = float(np.linalg.eigvalsh(J).min())
    print(f"{name}: smallest Choi eigenvalue {w:.2e}")
    assert w >= -1e-12


@pytest.mark.slow
@pytest.mark.parametrize("name", SC.NAMES)
def test_oracle_maps(name):
    b = SC.batch(name)
    S = SC.oracle_maps(b["params"], b["sched"])
    drift = float(np.abs(S - SC.golden(name)).max())
    print(f"{name}: against the recorded maps {drift:.2e}")
    # the recorded map is this map (another LAPACK build may round differently)
    assert drift < 1e-12


def test_capped_segment_is_beyond_the_cap():
    """The x the step-cap test gives one segment: 3e6 on the main bound, and the (-1,+1)
    bank's bound (V left out) stays below it for these points, so the cap comes from V."""
    p = SC.batch("aba")["params"]
    for i in range(p.shape[1]):
        x = SC.capped_segment(p, i)
        assert abs(SC.build_argument(p, i, 1.0, 0.0, x) - 3e6) < 1.0 and 3e6 > SC.X_CAP
        assert SC.build_argument(p, i, 1.0, 0.0, x, with_v=False) < SC.X_CAP
