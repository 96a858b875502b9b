"""The entry of the balanced sym16 LP-square kernel (ryd_sym16_body.inc, ryd_sym16_bal.hip): no
workgroup barrier -- a consumer clears its own handoff flag before its first poll, the producer
only sets it -- and the arguments packed, reordered and preloaded into SGPRs.  Neither changes
an arithmetic instruction, so every comparison is bit for bit -- state, the whole summary with
its NaNs, status -- against the one-wave kernel (RYD_S16_BALANCE=0), through
engine.DeviceBatch, with RYD_S16_BALANCE=2 and RYD_S16_BALANCE_GPC forcing the form.

The lane-masked squarings (RYD_S16_MASK_IDLE, on in the product build) are a compile-time flag
of the balanced form's first build with no run-time switch: every case here, the depth cases
among them, runs them against the one-wave kernel, which has no masked form.
"""
import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from test_gpu_parity import _random_points
from test_gpu_sym16_balance import _same_bits
from test_gpu_sym16_build import _sym
from test_gpu_sym16_edges import PATTERN, _no_pattern, _prefill
from test_gpu_sym16_start import _launch, _run

pytestmark = pytest.mark.gpu

GPCS = (5, 6, 9, 10, 13)


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


@pytest.fixture(scope="module")
def rand164():
    return _sym(_random_points(np.random.default_rng(20261021), 164, "lp_square"))


@pytest.fixture(scope="module")
def onewave(eng, rand164):
    """The one-wave kernel's result for the first n points of the random batch, once per n."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = _run(eng, rand164[:, :n].copy(), BALANCE=0)
            assert np.all(cache[n].status == 0)
        return cache[n]
    return get


@pytest.mark.parametrize("gpc", GPCS)
def test_roles_and_sizes(eng, rand164, onewave, gpc):
    """g groups per workgroup: 5, 9 and 13 split one job, 6 and 10 two.  n = 4 g: a lone workgroup,
    every job present; 4 g + 1: two workgroups with the jobs strided over them, one job of a
    single live row, and every split job past the batch (its producer and its consumer leave by
    the same test); 8 g - 3: a ragged tail, the second workgroup's last split job holds one point."""
    for n in (4 * gpc, 4 * gpc + 1, 8 * gpc - 3):
        what = f"gpc={gpc} n={n}"
        _same_bits(_run(eng, rand164[:, :n].copy(), BALANCE=2, BALANCE_GPC=gpc), onewave(n), what)
        _same_bits(_run(eng, rand164[:, :n].copy(), BALANCE=2, BALANCE_GPC=gpc, BALANCE_NOHANDOFF=1), onewave(n),
                   what + ", fallback")


# squaring depths per wave (four rows each); None: the row is made invalid.  The build leaves
# RYD_LP_UNSQUARED = 2 levels to the states, so depths 2 .. 5 are 0 .. 3 squarings in the build
# (the handoff comes after min(2, squarings)) and 14, 16 are 12 and 14.
DEPTHS = ((0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (4, 4, 4, 4), (5, 5, 5, 5), (14, 14, 14, 14),
          (3, 5, 3, 5), (16, None, 2, 14), (2, 14, 14, 2))


@pytest.fixture(scope="module")
def ladder(eng, rand164, onewave):
    """Points whose durations are scaled by powers of two (the series argument with them, exactly)
    to the depths of DEPTHS, and the one-wave kernel's result for them."""
    n = 4 * len(DEPTHS)
    p = rand164[:, :n].copy()
    have = onewave(n).col("NSQUARE").astype(int)
    want = np.array([d for w in DEPTHS for d in w], dtype=object)
    bad = np.array([d is None for d in want])
    tgt = np.where(bad, 0, want).astype(int)
    p[N.P["TAU"]] *= np.exp2((tgt - have).astype(float))
    p[N.P["TAU"], bad] = -1.0
    ref = _run(eng, p, BALANCE=0)
    assert np.all(((ref.status & N.STATUS_BAD_INPUT) != 0) == bad) and np.all(ref.status[~bad] == 0)
    np.testing.assert_array_equal(ref.col("NSQUARE").astype(int)[~bad], tgt[~bad], err_msg="depths not as built")
    return p, ref


@pytest.mark.parametrize("gpc", (1, 2, 5, 6, 10))
def test_squaring_depths(eng, ladder, gpc):
    """Builds of 0, 1, 2, 3, 12 and 14 squarings, a wave that mixes two depths across its rows
    and one with an invalid row, as whole jobs and as split ones (gpc = 1, 2: every job is
    split; 5, 6: the last one or two of a workgroup), handed over and in the fallback."""
    p, ref = ladder
    for noh in (None, 1):
        for p64 in (None, 1):
            _same_bits(_run(eng, p, BALANCE=2, BALANCE_GPC=gpc, BALANCE_NOHANDOFF=noh, PARAM64=p64), ref,
                       f"gpc={gpc} NOHANDOFF={noh} PARAM64={p64}")


@pytest.mark.parametrize("gpc", (5, 6, 10))
def test_handoff_alternating_back_to_back(eng, rand164, gpc):
    """Three launches on one stream with no synchronisation between them, alternately with the
    handoff and with RYD_S16_BALANCE_NOHANDOFF=1, each with parameters of its own into
    outputs prefilled with a pattern.  Without a barrier a launch finds the flags its
    predecessor left set (or, after a fallback launch, set by producers nobody waited for): a
    consumer must act on its own workgroup's producer of this launch alone."""
    n = 8 * gpc - 3
    ps = [rand164[:, k:k + n].copy() for k in (0, 17, 41)]
    refs = [_run(eng, p, BALANCE=0) for p in ps]
    dbs = [E.DeviceBatch(eng, p, "lp_square", "lindblad") for p in ps]
    try:
        for first in (None, 1):
            for db in dbs:
                _prefill(db, PATTERN)
            for k, db in enumerate(dbs):
                noh = first if k % 2 == 0 else (1 if first is None else None)
                _launch(db, BALANCE=2, BALANCE_GPC=gpc, BALANCE_NOHANDOFF=noh)
            dbs[-1].synchronize()
            for k, (db, ref) in enumerate(zip(dbs, refs)):
                r = db.fetch()
                what = f"gpc={gpc} launch {k} of three back to back, the first with NOHANDOFF={first}"
                _no_pattern(r, what)
                _same_bits(r, ref, what)
    finally:
        for db in dbs:
            db.free()
