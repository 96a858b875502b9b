"""The static plan of the sym16 LP-square kernel's CU-balanced launch form
(`ryd_sym16_balance_plan`, the host side of the role table the kernel itself evaluates): for
every batch size and every groups-per-workgroup setting, each four-point group is run exactly
once -- by one whole-job wave, or by one producer and one consumer wave of the same
workgroup -- and nothing is planned past the batch.  No GPU.
"""
import numpy as np
import pytest

from noisyquantumsimulator_amd import engine as E

CUS = 256
WHOLE, PRODUCER, CONSUMER = 0, 1, 2


def _check(n, gpc_override):
    pl = E.sym16_balance_plan(n, CUS, gpc_override)
    G = (n + 3) // 4
    assert pl["groups"] == G
    assert 1 <= pl["waves"] <= 16
    if gpc_override:
        assert pl["gpc"] == gpc_override
    else:
        assert pl["gpc"] == max(1, -(-G // CUS))
    assert pl["workgroups"] == -(-G // pl["gpc"])
    role, job, present = pl["role"], pl["job"], pl["present"]
    assert role.shape == job.shape == present.shape == (pl["workgroups"], pl["waves"])
    # nothing present at or beyond G; what is absent lies at or beyond G
    assert np.all(job[present] < G) and np.all(job[~present] >= G) and np.all(job >= 0)
    cover = {r: np.bincount(job[present & (role == r)], minlength=G) for r in (WHOLE, PRODUCER, CONSUMER)}
    # every group once: a whole job, or one producer plus one consumer
    assert np.all(cover[WHOLE] + cover[PRODUCER] == 1)
    np.testing.assert_array_equal(cover[PRODUCER], cover[CONSUMER])
    # the two halves of a split job sit in the same workgroup and are absent together
    # (the role of a wave index is the same in every workgroup: compare column blocks)
    np.testing.assert_array_equal(role, np.broadcast_to(role[0], role.shape))
    pc, cc = role[0] == PRODUCER, role[0] == CONSUMER
    assert pc.sum() == cc.sum()
    np.testing.assert_array_equal(job[:, pc], job[:, cc])
    np.testing.assert_array_equal(present[:, pc], present[:, cc])
    if pc.any():
        assert np.all(np.diff(job[:, pc], axis=1) > 0)       # distinct jobs
    # a split happens for 1 or 2 left-over jobs only
    rem = pl["gpc"] % 4
    assert (role == PRODUCER).sum() == (pl["workgroups"] * rem if rem in (1, 2) else 0)


@pytest.mark.parametrize("gpc", [0, 1, 2, 5, 6, 9, 10, 13, 14])
def test_plan_covers_every_group_once(gpc):
    for n in range(1, 5001):
        _check(n, gpc)


def test_plan_rejects_bad_arguments():
    for n, cus, gpc in ((0, CUS, 0), (10, 0, 0), (10, CUS, 17), (10, CUS, -1)):
        with pytest.raises(ValueError):
            E.sym16_balance_plan(n, cus, gpc)


def test_auto_rule_on_the_flagship_size():
    """The C2 bench line's 10,000 points: 2500 groups on 256 CUs, 10 per workgroup, 8 whole
    jobs and 2 split ones -- 12 waves, three per SIMD."""
    pl = E.sym16_balance_plan(10000, CUS)
    assert (pl["gpc"], pl["waves"], pl["workgroups"]) == (10, 12, 250)
    assert pl["role"][0].tolist() == [0] * 8 + [1, 1, 2, 2]
    # strided over the batch: workgroup 3 (the fourth of its XCD's first line group: logical
    # position 12) takes groups 12, 262, 512, ...; its two split jobs are the last two
    assert pl["job"][3].tolist() == [12 + 250 * k for k in range(10)] + [12 + 250 * 8, 12 + 250 * 9]
