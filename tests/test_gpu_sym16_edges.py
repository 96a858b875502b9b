"""The edges of the balanced sym16 LP-square launch (ryd_sym16_body.inc, ryd_sym16.inc): the
output stores in their write-through flavours (RYD_S16_WT=1: the state rows; 3: summary and
status too) against the plain one (RYD_S16_WT=0).  The flavour changes neither a value nor an
address, so every comparison is bit for bit -- state, the whole summary (NaNs included) and
status -- through engine.DeviceBatch, against the other flavour and against the one-wave
kernel (RYD_S16_BALANCE=0).

Shapes: every role mix of the role table (gpc = 1, 2, 5, 6, 9, 10) at n = 1, 37 and 149, and
at n = 4 gpc + 1: two workgroups that share gpc + 1 groups, the last of one live row, so
gpc - 1 jobs are absent (their waves leave right after the workgroup barrier).
"""
import contextlib
import os

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from test_gpu_parity import _random_points
from test_gpu_sym16_balance import _invalidate, _same_bits
from test_gpu_sym16_build import _sym

pytestmark = pytest.mark.gpu

KEYS = ("RYD_S16_BALANCE", "RYD_S16_BALANCE_GPC", "RYD_S16_BALANCE_NOHANDOFF", "RYD_S16_WT", "RYD_S16_STORE64")
GPCS = (1, 2, 5, 6, 9, 10)
PATTERN = 0xA5


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
def rand149():
    return _sym(_random_points(np.random.default_rng(20261020), 149, "lp_square"))


def _launch(db, **kw):
    with _env(**kw):
        db.launch()


def _prefill(db, byte):
    """Every output byte of the batch set to `byte` (ryd_memcpy_h2d)."""
    lib, h, s = db.eng.lib, db.eng.handle, db.slot
    for ptr, nbytes in ((db.d_state, 8 * db.width * 4 * db.n), (db.d_summary, 8 * N.NSUMMARY * db.n),
                        (db.d_status, 4 * db.n)):
        buf = np.full(nbytes, byte, dtype=np.uint8)
        N.check(lib.ryd_memcpy_h2d(h, s, ptr, buf.ctypes.data, nbytes))


def _run(eng, p, prefill=None, protocol="lp_square", n_steps=None, **kw):
    db = E.DeviceBatch(eng, p, protocol, "lindblad", n_steps=n_steps)
    try:
        if prefill is not None:
            _prefill(db, prefill)
        _launch(db, **kw)
        db.synchronize()
        return db.fetch()
    finally:
        db.free()


@pytest.fixture(scope="module")
def onewave(eng, rand149):
    """The one-wave kernel's result for the first n points of the random batch, once per n."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = _run(eng, rand149[:, :n].copy(), BALANCE=0)
            assert np.all(cache[n].status == 0)
        return cache[n]
    return get


@pytest.mark.parametrize("gpc", GPCS)
def test_forms_agree(eng, rand149, onewave, gpc):
    tail = 4 * gpc + 1
    pl = E.sym16_balance_plan(tail, 256, gpc)
    assert pl["workgroups"] == 2 and pl["groups"] == gpc + 1            # the last group: one live row
    assert gpc == 1 or not pl["present"].all()                          # gpc - 1 of the 2 gpc jobs are absent
    if gpc > 1:
        assert not E.sym16_balance_plan(1, 256, gpc)["present"].all()  # n = 1: absent jobs in the only workgroup
    for n in (1, 37, 149, tail):
        p = rand149[:, :n].copy()
        plain = _run(eng, p, BALANCE=2, BALANCE_GPC=gpc, WT=0)
        _same_bits(plain, onewave(n), f"gpc={gpc} n={n}: plain against one-wave")
        for w in (1, 3):
            wt = _run(eng, p, BALANCE=2, BALANCE_GPC=gpc, WT=w)
            _same_bits(wt, plain, f"gpc={gpc} n={n}: WT={w} against plain")
            _same_bits(wt, onewave(n), f"gpc={gpc} n={n}: WT={w} against one-wave")


@pytest.mark.parametrize("gpc", (10, 6))
def test_invalid_rows_non_unit_xi_and_64_bit_addresses(eng, rand149, gpc):
    bad = rand149[:, :41].copy()
    _invalidate(bad, 3)
    bad[N.P["OMEGA"], 33] = 0.0
    for i in range(36, 40):
        _invalidate(bad, i)
    xi = rand149[:, :41].copy()
    for i, f in ((32, 1.01), (5, 0.5), (40, 1.01)):
        xi[N.P["XI_RE"], i] *= f
        xi[N.P["XI_IM"], i] *= f
    for what, p in (("invalid rows", bad), ("non-unit xi", xi)):
        ref = _run(eng, p, BALANCE=0)
        for wt in (0, 1, 3):
            _same_bits(_run(eng, p, BALANCE=2, BALANCE_GPC=gpc, WT=wt), ref, f"{what} gpc={gpc} WT={wt}")
    assert np.all(_run(eng, bad, BALANCE=0).status[[3, 33, 36, 37, 38, 39]] & N.STATUS_BAD_INPUT)
    ref = _run(eng, xi, BALANCE=0, STORE64=1)
    for wt in (0, 1, 3):
        _same_bits(_run(eng, xi, BALANCE=2, BALANCE_GPC=gpc, WT=wt, STORE64=1), ref, f"64-bit addresses WT={wt}")


def _no_pattern(r, what):
    word = np.uint64(int.from_bytes(bytes([PATTERN] * 8), "little"))
    assert not np.any(np.ascontiguousarray(r.state).view(np.uint64) == word), f"{what}: state keeps the prefill"
    assert not np.any(np.ascontiguousarray(r.summary).view(np.uint64) == word), f"{what}: summary keeps the prefill"
    assert not np.any(r.status == np.uint32(word & np.uint64(0xFFFFFFFF))), f"{what}: status keeps the prefill"


@pytest.mark.parametrize("n,gpc", [(149, 10), (37, 6), (41, 10)])
def test_nothing_stale_nothing_missed(eng, rand149, n, gpc):
    p = rand149[:, :n].copy()
    plain = _run(eng, p, prefill=PATTERN, BALANCE=2, BALANCE_GPC=gpc, WT=0)
    _no_pattern(plain, "plain")
    for w, store64 in ((1, None), (3, None), (1, 1), (3, 1)):
        wt = _run(eng, p, prefill=PATTERN, BALANCE=2, BALANCE_GPC=gpc, WT=w, STORE64=store64)
        _no_pattern(wt, f"WT={w} STORE64={store64}")
        _same_bits(wt, plain, f"n={n} gpc={gpc} WT={w} STORE64={store64}: prefilled write-through against plain")


def test_store_flavours_in_turn_on_one_buffer(eng, rand149):
    a, b = rand149[:, :149].copy(), rand149[:, ::-1][:, :149].copy()
    ref = _run(eng, a, BALANCE=0)
    db = E.DeviceBatch(eng, a, "lp_square", "lindblad")
    try:
        for wt in (0, 1, 0, 3, 0):
            _prefill(db, PATTERN)
            _launch(db, BALANCE=2, BALANCE_GPC=10, WT=wt)
            db.synchronize()
            r = db.fetch()
            _no_pattern(r, f"WT={wt}")
            _same_bits(r, ref, f"one buffer, WT={wt}")
        # back to back on the same buffers, no synchronize in between: other parameters first,
        # so the last launch has to overwrite what the first two left, whatever their flavour
        N.check(eng.lib.ryd_memcpy_h2d(eng.handle, db.slot, db.d_params, b.ctypes.data, b.nbytes))
        _launch(db, BALANCE=2, BALANCE_GPC=10, WT=1)
        _launch(db, BALANCE=2, BALANCE_GPC=10, WT=0)
        _launch(db, BALANCE=2, BALANCE_GPC=10, WT=3)
        N.check(eng.lib.ryd_memcpy_h2d(eng.handle, db.slot, db.d_params, a.ctypes.data, a.nbytes))
        for last in (1, 0, 3):
            _launch(db, BALANCE=2, BALANCE_GPC=10, WT=1)
            _launch(db, BALANCE=2, BALANCE_GPC=10, WT=0)
            _launch(db, BALANCE=2, BALANCE_GPC=10, WT=last)
            db.synchronize()
            _same_bits(db.fetch(), ref, f"launches back to back, the last WT={last}")
    finally:
        db.free()


def test_switch_handling(eng, rand149):
    p = rand149[:, :37].copy()
    ref = _run(eng, p, BALANCE=0)
    for bad in ("2", "x", "", "11", "-1"):                     # not a value: every sym16 launch refuses it
        with pytest.raises(N.EngineError):
            _run(eng, p, BALANCE=2, WT=bad)
        with pytest.raises(N.EngineError):
            _run(eng, p, BALANCE=0, WT=bad)
    for wt in (1, 3):                                          # a value the one-wave kernels cannot honour
        with pytest.raises(N.EngineError):
            _run(eng, p, BALANCE=0, WT=wt)
        with pytest.raises(N.EngineError):
            _run(eng, p, WT=wt)                                # automatic rule: one-wave at this size
    jp = _sym(_random_points(np.random.default_rng(5), 8, "smooth_jp"))
    with pytest.raises(N.EngineError):
        _run(eng, jp, protocol="smooth_jp", n_steps=20, WT=1)
    assert np.all(_run(eng, jp, protocol="smooth_jp", n_steps=20, WT=0).status == 0)
    # plain stores are every form's own; after the refusals the device still works
    _same_bits(_run(eng, p, BALANCE=0, WT=0), ref, "one-wave, WT=0")
    _same_bits(_run(eng, p, BALANCE=2, WT=3), ref, "balanced, state and summary write-through")
    _same_bits(_run(eng, p, BALANCE=2), ref, "balanced, automatic")
