"""The CU-balanced launch form of the sym16 LP-square kernel (ryd_sym16.inc: one workgroup
per CU, left-over jobs split in time between a producer and a consumer wave through LDS)
against the one-wave kernel: the same per-point instructions, so every comparison is bit
for bit -- state, the whole summary (NaNs included) and status -- between RYD_S16_BALANCE=2
and RYD_S16_BALANCE=0 in one process, one launch each through engine.DeviceBatch.

Shapes: the smallest at which the form can go wrong -- every role mix of the role table
(gpc = 1, 2, 5, 6, 9, 10, 14), partial workgroups, absent jobs, a last group with one live
row, split jobs holding every series length, depth 0 to 14, identity columns, invalid rows and
a non-unit xi (the consumer's rebuild), and the consumer's fallback (NOHANDOFF).
"""
import contextlib
import os
import warnings

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import sweeps as SW
from test_gpu_parity import _random_points
from test_gpu_sym16_build import OWN, RATES, _c2_corners, _sym, _tau_ladder, _x_ladder

pytestmark = pytest.mark.gpu

KEYS = ("RYD_S16_BALANCE", "RYD_S16_BALANCE_GPC", "RYD_S16_BALANCE_NOHANDOFF")


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in KEYS}
    for k in KEYS:
        os.environ.pop(k, None)
    for k, v in kw.items():
        if v is not None:
            os.environ["RYD_S16_" + k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _run(eng, p, balance=None, gpc=None, nohandoff=None):
    """One launch of the batch (the switches are read per launch)."""
    assert E.symmetric_atoms(p)
    db = E.DeviceBatch(eng, p, "lp_square", "lindblad")
    try:
        with _env(BALANCE=balance, BALANCE_GPC=gpc, BALANCE_NOHANDOFF=nohandoff):
            db.launch()
            db.synchronize()
        return db.fetch()
    finally:
        db.free()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(ra, rb, what):
    np.testing.assert_array_equal(np.isnan(ra.summary), np.isnan(rb.summary), err_msg=f"{what}: summary NaNs")
    np.testing.assert_array_equal(_bits(ra.summary), _bits(rb.summary), err_msg=f"{what}: summary")
    np.testing.assert_array_equal(_bits(ra.state), _bits(rb.state), err_msg=f"{what}: state")
    np.testing.assert_array_equal(ra.status, rb.status, err_msg=f"{what}: status")


def _same_points(ra, ia, rb, ib, what, rows):
    sa = _bits(ra.state).reshape(25, ra.n, 4)[:, ia]
    sb = _bits(rb.state).reshape(25, rb.n, 4)[:, ib]
    np.testing.assert_array_equal(sa, sb, err_msg=f"{what}: state")
    np.testing.assert_array_equal(_bits(ra.summary)[rows][:, ia], _bits(rb.summary)[rows][:, ib],
                                  err_msg=f"{what}: summary")
    np.testing.assert_array_equal(ra.status[ia], rb.status[ib], err_msg=f"{what}: status")


def _split_points(n, gpc):
    """Point indices of the jobs that the plan splits between two waves."""
    pl = E.sym16_balance_plan(n, 256, gpc)
    j = np.unique(pl["job"][pl["present"] & (pl["role"] == 2)])
    idx = (4 * j[:, None] + np.arange(4)).ravel()
    return idx[idx < n]


@pytest.fixture(scope="module")
def ladder(eng):
    """The 117-point ladder batch (tau ladder, x ladder, C2 corners) and its one-wave result."""
    p = np.concatenate([_tau_ladder("lp_square"), _x_ladder(), _c2_corners()], axis=1)
    assert p.shape[1] == 117
    ref = _run(eng, p, balance=0)
    assert np.all(ref.status == 0)
    return dict(p=p, ref=ref)


@pytest.fixture(scope="module")
def rand60():
    return _sym(_random_points(np.random.default_rng(20261020), 60, "lp_square"))


def test_switch_reaches_the_balanced_launch(eng, rand60):
    """The forced form really takes the other launch path: a groups-per-workgroup value it
    cannot plan fails there, and is not even read with the form switched off."""
    p = rand60[:, :8].copy()
    with pytest.raises(N.EngineError):
        _run(eng, p, balance=2, gpc=17)
    assert np.all(_run(eng, p, balance=0, gpc=17).status == 0)


@pytest.mark.parametrize("gpc", [10, 6])
def test_ladder_batch(eng, ladder, gpc):
    p, ref = ladder["p"], ladder["ref"]
    r = _run(eng, p, balance=2, gpc=gpc)
    _same_bits(r, ref, f"ladder gpc={gpc}")
    sp = _split_points(117, gpc)
    print(f"gpc={gpc}: split points NSQUARE {sorted(set(ref.col('NSQUARE')[sp].astype(int)))} "
          f"series {sorted(set((ref.col('NMV_USEFUL')[sp] / 15 - 1).astype(int)))}")
    assert sp.size > 0


def test_ladder_batch_every_job_split(eng, ladder):
    """gpc = 2 splits every job, so by construction the handoff carries every case of the
    ladders: depths 0 to 14, every series length from 13 down to 1, and the identity columns
    of a point below X_SKIP."""
    p, ref = ladder["p"], ladder["ref"]
    sp = _split_points(117, 2)
    np.testing.assert_array_equal(sp, np.arange(117))
    nsq = ref.col("NSQUARE").astype(int)
    kt = (ref.col("NMV_USEFUL") / 15 - 1).astype(int)
    assert nsq.min() == 0 and nsq.max() == 14
    assert set(range(-1, 14)) - {0} <= set(kt)
    _same_bits(_run(eng, p, balance=2, gpc=2), ref, "ladder gpc=2")
    _same_bits(_run(eng, p, balance=2, gpc=2, nohandoff=1), ref, "ladder gpc=2, fallback")


def test_ladder_batch_reversed(eng, ladder):
    """Reversed, other points fall into the split jobs; every point keeps the bits it has in
    the forward batch (NMV_EXEC describes the wave, not the point)."""
    p, ref = ladder["p"], ladder["ref"]
    q = p[:, ::-1].copy()
    r = _run(eng, q, balance=2, gpc=10)
    _same_bits(r, _run(eng, q, balance=0), "reversed ladder")
    fwd = _run(eng, p, balance=2, gpc=10)
    _same_points(r, np.arange(117)[::-1], fwd, np.arange(117), "reversed against forward", OWN)
    # between them the split jobs of the three ladder runs hold the shallowest and the deepest
    # builds, the identity (a point below X_SKIP) and every series length
    sp = np.unique(np.r_[_split_points(117, 10), _split_points(117, 6), 116 - _split_points(117, 10)])
    nsq = ref.col("NSQUARE")[sp]
    kt = (ref.col("NMV_USEFUL")[sp] / 15 - 1).astype(int)
    print(f"split points {sp.size}: NSQUARE {sorted(set(nsq.astype(int)))} series {sorted(set(kt))}")
    assert nsq.min() == 0 and nsq.max() == 14 and -1 in kt


@pytest.mark.parametrize("n", [40, 37, 33, 32, 4])
def test_batch_ends_at_gpc10(eng, rand60, n):
    """n = 40: a full workgroup; 37: the split job 9 with one live row; 33: job 8 with one
    live row, job 9 absent; 32: no split job present; 4: one whole job."""
    p = rand60[:, :n].copy()
    _same_bits(_run(eng, p, balance=2, gpc=10), _run(eng, p, balance=0), f"n={n}")


@pytest.mark.parametrize("gpc", [1, 2, 5, 9, 14])
def test_role_mixes(eng, rand60, gpc):
    """gpc = 1, 5: one left-over job; 2: only split jobs; 9: one behind eight whole jobs;
    14: 16 waves per workgroup."""
    ref = _run(eng, rand60, balance=0)
    assert np.all(ref.status == 0)
    _same_bits(_run(eng, rand60, balance=2, gpc=gpc), ref, f"gpc={gpc}")


def test_many_workgroups_with_a_partial_one(eng):
    p = _sym(_random_points(np.random.default_rng(301), 301, "lp_square"))
    pl = E.sym16_balance_plan(301, 256, 2)
    # 76 groups, the last with one live row: 38 workgroups of two split jobs, the last one partial
    assert pl["workgroups"] == 38 and pl["groups"] == 76 and pl["present"].all()
    _same_bits(_run(eng, p, balance=2, gpc=2), _run(eng, p, balance=0), "n=301 gpc=2")


def _invalidate(p, i):
    p[:, i] = np.nan
    for k in RATES + ("GMJ",):
        p[N.P[k + "_A"], i] = p[N.P[k + "_B"], i] = 0.0


def test_invalid_rows_in_split_jobs(eng, rand60):
    """Split job 8 (points 32-35) with a NaN row, an Omega = 0 row and a negative-rate row;
    split job 9 (points 36-39) all invalid: flags on those rows only, the other points' bits
    as in the clean batch."""
    clean = rand60[:, :40].copy()
    p = clean.copy()
    _invalidate(p, 32)
    p[N.P["OMEGA"], 33] = 0.0
    p[N.P["G1_A"], 34] = p[N.P["G1_B"], 34] = -1.0
    for i in range(36, 40):
        _invalidate(p, i)
    np.testing.assert_array_equal(_split_points(40, 10), np.arange(32, 40))
    r = _run(eng, p, balance=2, gpc=10)
    _same_bits(r, _run(eng, p, balance=0), "invalid rows")
    bad = np.zeros(40, bool)
    bad[[32, 33, 34, 36, 37, 38, 39]] = True
    assert np.all(r.status[bad] & N.STATUS_BAD_INPUT) and np.all(r.status[~bad] == 0)
    good = np.flatnonzero(~bad)
    _same_points(r, good, _run(eng, clean, balance=2, gpc=10), good, "beside invalid rows", OWN)


def test_non_unit_xi_in_a_split_and_a_whole_job(eng, rand60):
    """|xi| = 1.01 and 0.5 in the split job 8 (the consumer rebuilds, with the one-wave code)
    and in the whole job 1 of the same launch."""
    p = rand60[:, :40].copy()
    for i, f in ((32, 1.01), (33, 0.5), (4, 1.01), (5, 0.5)):
        p[N.P["XI_RE"], i] *= f
        p[N.P["XI_IM"], i] *= f
    r = _run(eng, p, balance=2, gpc=10)
    ref = _run(eng, p, balance=0)
    assert np.all(ref.status == 0)
    # the rebuild ran: the waves of jobs 1 and 8 executed the series twice
    base = _run(eng, rand60[:, :40].copy(), balance=0)
    for j in (1, 8):
        np.testing.assert_array_equal(ref.col("NMV_EXEC")[4 * j:4 * j + 4], 2 * base.col("NMV_EXEC")[4 * j:4 * j + 4])
    _same_bits(r, ref, "non-unit xi")


def test_consumer_fallback(eng, rand60, ladder):
    """RYD_S16_BALANCE_NOHANDOFF=1: every consumer computes the producer's part itself."""
    p = rand60[:, :40].copy()
    _same_bits(_run(eng, p, balance=2, gpc=10, nohandoff=1), _run(eng, p, balance=0), "n=40 fallback")
    for gpc in (10, 6):
        _same_bits(_run(eng, ladder["p"], balance=2, gpc=gpc, nohandoff=1), ladder["ref"], f"ladder fallback gpc={gpc}")


def test_auto_mode(eng):
    """The automatic rule keeps the one-wave kernel for the small batches above and picks the
    balanced form for the C2 bench batch; there one launch of each gives the same bits.  What
    the launch itself chose, on the device's own CU count, shows in the one switch that only a
    balanced launch reads: an impossible groups-per-workgroup value fails there alone."""
    cus = 256                                   # MI355X (the kernel's own one-round test assumes it too)
    for n in (4, 32, 33, 37, 40, 60, 117, 301):
        assert not E.sym16_balance_plan(n, cus)["auto"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = E.pack_params(SW.c2_rank_shard(0, 1))
    assert p.shape[1] == 10000 and E.symmetric_atoms(p)
    pl = E.sym16_balance_plan(10000, cus)
    print(f"C2 on {cus} CUs: gpc {pl['gpc']}, {pl['workgroups']} workgroups of {pl['waves']} waves, auto {pl['auto']}")
    assert pl["auto"]
    _same_bits(_run(eng, p), _run(eng, p, balance=0), "C2 batch, auto")
    with pytest.raises(N.EngineError):          # auto took the balanced launch for C2 ...
        _run(eng, p, gpc=17)
    q = p[:, :117].copy()                       # ... and the one-wave kernel for a small batch
    assert np.all(_run(eng, q, gpc=17).status == 0)
