"""The start-up of the balanced sym16 LP-square kernel (ryd_sym16.inc, ryd_sym16_body.inc): its
first parameter load as one instruction per wave with 32-bit lane offsets and DPP row
broadcasts (or, by RYD_S16_PARAM64=1, column by column at 64-bit addresses), and its
branch-free validity test; around them the role mixes, the handoff flags across launches, the
launch switches and the leading dimensions.  None of it changes an arithmetic instruction, so
every comparison is bit for bit -- state, the whole summary with its NaNs, status -- against
the one-wave kernel (RYD_S16_BALANCE=0), through engine.DeviceBatch, with RYD_S16_BALANCE=2
and RYD_S16_BALANCE_GPC forcing the form.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from test_gpu_parity import _random_points
from test_gpu_sym16_balance import _same_bits
from test_gpu_sym16_build import RATES, _sym
from test_gpu_sym16_edges import GPCS, PATTERN, _no_pattern, _prefill

pytestmark = pytest.mark.gpu

KEYS = ("RYD_S16_BALANCE", "RYD_S16_BALANCE_GPC", "RYD_S16_BALANCE_NOHANDOFF", "RYD_S16_WT", "RYD_S16_STORE64",
        "RYD_S16_PARAM64")
# the 15 parameter columns LP square loads, in the kernel's order
COLUMNS = ("OMEGA", "DELTA", "V", "DELTA1") + tuple(k + s for k in RATES for s in ("_A", "_B")) + \
    ("TAU", "XI_RE", "XI_IM")
SIGNED = tuple(k + s for k in RATES for s in ("_A", "_B")) + ("TAU", "OMEGA")   # negative is invalid


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


@pytest.fixture(scope="module")
def rand164():
    return _sym(_random_points(np.random.default_rng(20261020), 164, "lp_square"))


def _launch(db, **kw):
    with _env(**kw):
        db.launch()


def _run(eng, p, upload=None, n_steps=None, **kw):
    """One launch of the batch p; `upload`: other parameters of the same shape put in its
    place on the device first (the descriptor stays the one built from p)."""
    db = E.DeviceBatch(eng, p, "lp_square", "lindblad", n_steps=n_steps)
    try:
        if upload is not None:
            assert upload.shape == p.shape
            N.check(eng.lib.ryd_memcpy_h2d(eng.handle, db.slot, db.d_params, upload.ctypes.data, upload.nbytes))
        _launch(db, **kw)
        db.synchronize()
        return db.fetch()
    finally:
        db.free()


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
def test_role_mixes(eng, rand164, onewave, gpc):
    """gpc = 1: a split job and no whole one; 2: two split jobs; 5, 6, 9, 10: whole jobs beside
    one or two split ones.  n = 4 gpc + 1: gpc - 1 jobs are absent, and their producers and
    consumers leave before the load; n = 1: a wave of one live row, its lanes clamped to it."""
    for n in (1, 37, 149, 4 * gpc + 1):
        _same_bits(_run(eng, rand164[:, :n].copy(), BALANCE=2, BALANCE_GPC=gpc), onewave(n), f"gpc={gpc} n={n}")


def test_stale_flags(eng, rand164, onewave):
    """What the kernel's workgroup barrier is for.  Launches back to back leave their flags in the
    LDS of the CUs they ran on: gpc = 6 publishes both slots, gpc = 5 the first only, and the
    next launch's consumers must not take a flag of an earlier launch for their producer's.
    The same after a launch of another kernel that uses LDS (the coherence kernel)."""
    n = 149
    p = rand164[:, :n].copy()
    ref = onewave(n)
    coh = E.CoherenceDeviceBatch(eng, p, "lp_square")
    db = E.DeviceBatch(eng, p, "lp_square", "lindblad")
    try:
        for other in (False, True):
            for seq in ((6, 5, 6), (6, 5, 6, 5)):
                for rep in range(3):
                    _prefill(db, PATTERN)
                    if other:
                        coh.launch()
                    for gpc in seq:
                        _launch(db, BALANCE=2, BALANCE_GPC=gpc)
                    db.synchronize()
                    r = db.fetch()
                    what = f"launches gpc={seq} back to back, round {rep}, coherence kernel first: {other}"
                    _no_pattern(r, what)
                    _same_bits(r, ref, what)
    finally:
        db.free()
        coh.free()


@pytest.mark.parametrize("gpc", (10, 6, 2))
def test_fallback_and_store_flavours(eng, rand164, onewave, gpc):
    p = rand164[:, :149].copy()
    ref = onewave(149)
    _same_bits(_run(eng, p, BALANCE=2, BALANCE_GPC=gpc, BALANCE_NOHANDOFF=1), ref, f"gpc={gpc}: a consumer that never polls")
    for s64 in (None, 1):
        _same_bits(_run(eng, p, BALANCE=2, BALANCE_GPC=gpc, STORE64=s64), ref, f"gpc={gpc} STORE64={s64}")
        _same_bits(_run(eng, p, BALANCE=2, BALANCE_GPC=gpc, STORE64=s64, BALANCE_NOHANDOFF=1), ref,
                   f"gpc={gpc} STORE64={s64}, fallback")


def _run_ld(eng, p, pad, n, ldp, lds, ldm, **kw):
    """The first n points of p launched with the leading dimensions given: the parameter block
    holds ldp columns (p, then `pad`), the outputs come back without their padding."""
    big = np.ascontiguousarray(np.concatenate([p[:, :n], pad], axis=1)[:, :ldp])
    assert big.shape[1] == ldp >= n and 4 * ldp >= lds >= 4 * n and ldp >= ldm >= n and E.symmetric_atoms(big)
    db = E.DeviceBatch(eng, big, "lp_square", "lindblad")
    try:
        _prefill(db, PATTERN)
        with _env(**kw):
            N.check(eng.lib.ryd_run_batch_device(eng.handle, db.slot, ctypes.byref(db.desc), db.d_params, n, ldp,
                                                 db.d_state, lds, db.d_summary, ldm, db.d_status, None, None))
        db.synchronize()
        full = db.fetch()                       # the buffers as DeviceBatch laid them out: read them as ours
    finally:
        db.free()
    state = np.ascontiguousarray(full.state).ravel()[:25 * lds].reshape(25, lds)
    summ = np.ascontiguousarray(full.summary).ravel()[:N.NSUMMARY * ldm].reshape(N.NSUMMARY, ldm)
    word = np.uint64(int.from_bytes(bytes([PATTERN] * 8), "little"))
    # nothing written beyond column n of any row: the padding keeps the prefill
    assert np.all(state[:, 4 * n:].view(np.uint64) == word), "state padding written"
    assert np.all(summ[:, n:].view(np.uint64) == word), "summary padding written"
    assert np.all(full.status[n:].view(np.uint8) == PATTERN), "status padding written"
    return E.EngineResult("lindblad", n, state[:, :4 * n].copy(), summ[:, :n].copy(), full.status[:n].copy(), 0.0,
                          0.0, 0.0, 0.0, 0.0, 3)


@pytest.mark.parametrize("gpc", (10, 5))
def test_leading_dimensions(eng, rand164, onewave, gpc):
    """ld_params, ld_state and ld_summary larger than n and all different: each reaches its
    own use, in both forms of the parameter load and both address forms of the stores."""
    n = 41
    pad = rand164[:, ::-1][:, :19].copy()
    ref = onewave(n)
    for ldp, lds, ldm in ((n + 19, 4 * n + 8, n + 5), (n + 7, 4 * n + 28, n + 3)):
        for kw in ({}, {"PARAM64": 1}, {"STORE64": 1}, {"PARAM64": 1, "STORE64": 1}):
            r = _run_ld(eng, rand164, pad, n, ldp, lds, ldm, BALANCE=2, BALANCE_GPC=gpc, **kw)
            _same_bits(r, ref, f"gpc={gpc} ld_params={ldp} ld_state={lds} ld_summary={ldm} {kw}")


def test_packed_switches(eng, rand164, onewave):
    """n_steps is ignored by LP square; every RYD_S16_WT value with every other switch set or
    clear, and a bad one still fails."""
    p = rand164[:, :37].copy()
    ref = onewave(37)
    for ns in (1, 7, 300):
        _same_bits(_run(eng, p, n_steps=ns, BALANCE=2, BALANCE_GPC=10), ref, f"n_steps={ns}")
    for wt in (0, 1, 3):
        for noh in (None, 1):
            for s64 in (None, 1):
                for p64 in (None, 1):
                    r = _run(eng, p, BALANCE=2, BALANCE_GPC=6, WT=wt, BALANCE_NOHANDOFF=noh, STORE64=s64, PARAM64=p64)
                    _same_bits(r, ref, f"WT={wt} NOHANDOFF={noh} STORE64={s64} PARAM64={p64}")
    for bad in ("2", "x", "", "11", "-1"):
        with pytest.raises(N.EngineError):
            _run(eng, p, BALANCE=2, BALANCE_GPC=6, WT=bad)
    _same_bits(_run(eng, p, BALANCE=2, BALANCE_GPC=6), ref, "after the refusals")


@pytest.mark.parametrize("n", (149, 160))
def test_column_offsets_32_and_64_bit(eng, rand164, onewave, n):
    """The batch is far below the 31-bit limit, so the one-instruction load with 32-bit lane
    offsets is taken; RYD_S16_PARAM64=1 forces the column-by-column 64-bit form.  The same
    addresses, the same bits."""
    p = rand164[:, :n].copy()
    for gpc in (10, 6, 1):
        a = _run(eng, p, BALANCE=2, BALANCE_GPC=gpc)
        b = _run(eng, p, BALANCE=2, BALANCE_GPC=gpc, PARAM64=1)
        _same_bits(a, b, f"n={n} gpc={gpc}: row load against 64-bit column loads")
        _same_bits(a, onewave(n), f"n={n} gpc={gpc}: row load against one-wave")


def _poisoned(rand164):
    """One point of each wave invalid in one column: NaN and infinity in each of the 15
    columns, a negative value where the column is a rate, the duration or the Rabi frequency;
    the last wave carries a non-unit xi row instead.  Returns the batch and its cases."""
    cases = [(c, v) for c in COLUMNS for v in (np.nan, np.inf)] + [(c, None) for c in SIGNED]
    n = 4 * (len(cases) + 1)
    assert n <= 164
    p = rand164[:, :n].copy()
    where = []
    for w, (c, v) in enumerate(cases):
        i = 4 * w + w % 4
        p[N.P[c], i] = -abs(p[N.P[c], i]) - 1.0 if v is None else v
        where.append((i, c, v))
    p[N.P["XI_RE"], n - 3] *= 1.01
    p[N.P["XI_IM"], n - 3] *= 1.01
    return p, where


def test_validation(eng, rand164):
    """The branch-free validity test gives point_valid's answer: status and every bit as the
    one-wave kernel, for whole jobs (gpc = 10, jobs 0-7), split jobs (gpc = 2: every job), the
    fallback and both forms of the parameter load."""
    p, where = _poisoned(rand164)
    clean = rand164[:, :p.shape[1]].copy()
    ref = _run(eng, clean, upload=p, BALANCE=0)
    for i, c, v in where:
        if c not in ("XI_RE", "XI_IM"):         # xi is not part of validity: its rows turn out non-finite
            assert ref.status[i] & N.STATUS_BAD_INPUT, f"point {i}: {c} = {v} not refused"
    bad = np.zeros(p.shape[1], bool)
    bad[[i for i, _, _ in where]] = True
    assert np.all(ref.status[~bad] == 0)
    for kw in ({"BALANCE_GPC": 10}, {"BALANCE_GPC": 2}, {"BALANCE_GPC": 2, "BALANCE_NOHANDOFF": 1},
               {"BALANCE_GPC": 6, "PARAM64": 1}, {"BALANCE_GPC": 5, "STORE64": 1}):
        _same_bits(_run(eng, clean, upload=p, BALANCE=2, **kw), ref, f"poisoned columns {kw}")
