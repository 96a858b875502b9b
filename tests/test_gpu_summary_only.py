"""Summary-only runs (a NULL state pointer: engine.DeviceBatch(states=False), Engine.run(
states=False)) against the full run of the same batch: the whole summary (NaNs included,
compared as bit patterns) and the status word, bit for bit.

Every device-form case launches three times on buffers prefilled with 0xA5: the storing kernel
(states=True), the summary-only launch (the store-free twin where the descriptor has one, a
scratch state buffer otherwise), and the summary-only launch under RYD_NOSTATE=0 (always the
storing kernel into a scratch buffer).  Shapes are the smallest at which a kernel's epilogue can
go wrong: single points, a last wave / block with one live row, more than one block, invalid
rows at every position of a wave.  The host form, the product path and two comparisons with
the oracle (so that not everything is compared with itself) follow.
"""
import contextlib
import os
import warnings

import numpy as np
import pytest

import dim4_points as D4
from conftest import states_from_fixture
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import simulation as SIM
from noisyquantumsimulator_amd import sweeps as SW
from oracle import lindblad_oracle as O
from test_gpu_ket_block import _grid
from test_gpu_parity import TOL, _oracle_point, _random_points, _run_cfg
from test_gpu_shaped16 import _batch as _shaped_batch
from test_gpu_sym16_balance import _invalidate
from test_gpu_sym16_build import _sym

pytestmark = pytest.mark.gpu

KEYS = ("RYD_NOSTATE", "RYD_SYM16", "RYD_KET_BLOCK", "RYD_S16_BALANCE", "RYD_S16_BALANCE_GPC", "RYD_S16_WT",
        "RYD_S16_STORE64", "RYD_S16_PARAM64")
GPCS = (1, 2, 5, 6, 9, 10)
PATTERN = 0xA5
WORD = np.uint64(int.from_bytes(bytes([PATTERN] * 8), "little"))


@contextlib.contextmanager
def _env(**kw):
    """The library's switches (read per launch) set for the block: NOSTATE=0 -> RYD_NOSTATE=0,
    S16_WT=3 -> RYD_S16_WT=3, ...; every other switch of KEYS unset."""
    old = {k: os.environ.get(k) for k in KEYS}
    for k in KEYS:
        os.environ.pop(k, None)
    for k, v in kw.items():
        assert "RYD_" + k in KEYS, k
        if v is not None:
            os.environ["RYD_" + k] = str(v)
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_summary(ra, rb, what):
    """Summary (as bit patterns, so NaNs compare too) and status; the state is not compared."""
    assert ra.summary.shape == rb.summary.shape and ra.status.shape == rb.status.shape, what
    np.testing.assert_array_equal(np.isnan(ra.summary), np.isnan(rb.summary), err_msg=f"{what}: summary NaNs")
    np.testing.assert_array_equal(_bits(ra.summary), _bits(rb.summary), err_msg=f"{what}: summary")
    np.testing.assert_array_equal(ra.status, rb.status, err_msg=f"{what}: status")


def _no_pattern(r, what):
    assert not np.any(_bits(r.summary) == WORD), f"{what}: summary keeps the prefill"
    assert not np.any(r.status == np.uint32(WORD & np.uint64(0xFFFFFFFF))), f"{what}: status keeps the prefill"


def _launch(eng, p, protocol, evolution, states, env, **desc):
    """One launch on buffers prefilled with PATTERN."""
    db = E.DeviceBatch(eng, p, protocol, evolution, states=states, **desc)
    try:
        lib, h, s = eng.lib, eng.handle, db.slot
        fills = [(db.d_summary, 8 * N.NSUMMARY * db.n), (db.d_status, 4 * db.n)]
        if states:
            fills.append((db.d_state, 8 * db.width * 4 * db.n))
        else:
            assert db.d_state is None
        for ptr, nbytes in fills:
            buf = np.full(nbytes, PATTERN, dtype=np.uint8)
            N.check(lib.ryd_memcpy_h2d(h, s, ptr, buf.ctypes.data, nbytes))
        with _env(**env):
            db.launch()
            db.synchronize()
        return db.fetch()
    finally:
        db.free()


def _check(eng, p, protocol, evolution, what, env=None, full=None, **desc):
    """Storing kernel, summary-only launch and summary-only under RYD_NOSTATE=0 of one batch.
    Returns the storing kernel's result (``full``: reuse one)."""
    env = dict(env or {})
    p = np.ascontiguousarray(p)
    if full is None:
        full = _launch(eng, p, protocol, evolution, True, env, **desc)
        assert full.state is not None
        _no_pattern(full, f"{what}: storing kernel")
    for label, e in (("summary-only", env), ("RYD_NOSTATE=0", dict(env, NOSTATE=0))):
        so = _launch(eng, p, protocol, evolution, False, e, **desc)
        assert so.state is None, what
        _no_pattern(so, f"{what}: {label}")
        _same_summary(so, full, f"{what}: {label} against the storing kernel")
    return full


# ---------------------------------------------------------------------------------------------
# sym16, the one-wave kernels
# ---------------------------------------------------------------------------------------------
SYM16 = [("lp_square", None), ("bangbang", None), ("smooth_jp", 1), ("smooth_jp", 3), ("smooth_jp", 30)]


@pytest.fixture(scope="module")
def sym149():
    return {proto: _sym(_random_points(np.random.default_rng(20261020), 149, proto))
            for proto in ("lp_square", "bangbang", "smooth_jp")}


@pytest.mark.parametrize("protocol,n_steps", SYM16)
def test_sym16_one_wave(eng, sym149, protocol, n_steps):
    """n = 37: one live row in the last wave; 149: the xcd_block permutation with a tail."""
    for n in (1, 2, 3, 4, 5, 37, 149):
        p = sym149[protocol][:, :n].copy()
        for s64 in (None, 1):
            r = _check(eng, p, protocol, "lindblad", f"{protocol} n_steps={n_steps} n={n} STORE64={s64}",
                       env=dict(S16_BALANCE=0, S16_STORE64=s64), n_steps=n_steps)
            assert np.all(r.status == 0)


@pytest.mark.parametrize("protocol,n_steps", [("lp_square", None), ("bangbang", 5), ("smooth_jp", 3)])
def test_sym16_invalid_rows(eng, sym149, protocol, n_steps):
    """An invalid row at each of the four positions of the middle wave, then that whole wave
    invalid between two valid ones."""
    clean = sym149[protocol][:, :12].copy()
    cases = [[4 + k] for k in range(4)] + [[4, 5, 6, 7]]
    for rows in cases:
        p = clean.copy()
        for i in rows:
            _invalidate(p, i)
        r = _check(eng, p, protocol, "lindblad", f"{protocol} invalid rows {rows}", env=dict(S16_BALANCE=0),
                   n_steps=n_steps)
        bad = np.zeros(12, bool)
        bad[rows] = True
        assert np.all(r.status[bad] & N.STATUS_BAD_INPUT) and np.all(r.status[~bad] == 0)


# ---------------------------------------------------------------------------------------------
# sym16, the balanced form (LP square)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gpc", GPCS)
def test_sym16_balanced(eng, sym149, gpc):
    """Both store flavours of the summary (RYD_S16_WT 0 and 3) and both parameter-load forms
    (RYD_S16_PARAM64 unset and 1) of the balanced launch, against its storing kernel."""
    for n in (1, 37, 149, 4 * gpc + 1):
        p = sym149["lp_square"][:, :n].copy()
        for wt in (0, 3):
            for p64 in (None, 1):
                r = _check(eng, p, "lp_square", "lindblad", f"gpc={gpc} n={n} WT={wt} PARAM64={p64}",
                           env=dict(S16_BALANCE=2, S16_BALANCE_GPC=gpc, S16_WT=wt, S16_PARAM64=p64))
                assert np.all(r.status == 0)


def test_sym16_balanced_switch_is_read(eng, sym149):
    """The summary-only launch takes the balanced path too: a groups-per-workgroup value that
    cannot be planned fails there, as it does for the storing launch."""
    p = sym149["lp_square"][:, :8].copy()
    with pytest.raises(N.EngineError):
        _launch(eng, p, "lp_square", "lindblad", False, dict(S16_BALANCE=2, S16_BALANCE_GPC=17))


# ---------------------------------------------------------------------------------------------
# shaped16, the dim-4 propagator kernel, the ket block kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["gaussian", "cosine", "blackman"])
def test_shaped16(eng, shape):
    """The shaped kernel has no store-free twin (it measured no faster): one wave, a full wave,
    a second wave with one live row, three waves, through the scratch-buffer path."""
    pall = E.pack_params(_shaped_batch(9, shape))
    assert E.symmetric_atoms(pall)
    for n_steps in (2, 3, 40):
        for n in (1, 4, 5, 9):
            r = _check(eng, pall[:, :n].copy(), "lp_shaped", "lindblad", f"{shape} n_steps={n_steps} n={n}",
                       n_steps=n_steps, shape=shape)
            assert np.all(r.status == 0)


@pytest.mark.parametrize("protocol", ["lp_square", "bangbang", "smooth_jp"])
def test_dim4_prop(eng, protocol):
    """As test_shaped16: lindblad4_prop_kernel into a scratch buffer, four points per block."""
    pall = D4.sym(D4.random_points4(np.random.default_rng(20261020), 9, protocol))
    for n in (1, 4, 5, 9):
        r = _check(eng, pall[:, :n].copy(), protocol, "lindblad", f"dim 4 {protocol} n={n}", dim=4,
                   n_steps=30 if protocol == "smooth_jp" else None)
        assert np.all(r.status == 0)


@pytest.mark.parametrize("dim", [3, 4])
@pytest.mark.parametrize("kind", ["lp_square", "cosine", "bangbang", "smooth_jp"])
def test_ket_block(eng, kind, dim):
    """One thread per point in blocks of 256: a full block, one short of it, one more."""
    b = _grid(kind, n=257, dim=dim)
    pall = E.pack_params(b)
    key = E.protocol_key(b)
    shape = b.pulse_shape.lower() if key == "lp_shaped" else "square"
    for n in (1, 255, 256, 257):
        r = _check(eng, pall[:, :n].copy(), key, "ket", f"ket dim {dim} {kind} n={n}", dim=dim, shape=shape)
        assert np.all(r.status == 0)


# ---------------------------------------------------------------------------------------------
# the scratch-buffer path: descriptors without a store-free kernel
# ---------------------------------------------------------------------------------------------
def _asym(protocol, n):
    p = _random_points(np.random.default_rng(20261020), n, protocol)
    assert not E.symmetric_atoms(p)
    return p


SCRATCH = [
    # (what, evolution, protocol, points, env, descriptor)
    ("unequal atoms, lindblad_prop_kernel", "lindblad", "lp_square", "asym", {}, {}),
    ("unequal atoms, lindblad_prop_kernel", "lindblad", "bangbang", "asym", {}, {}),
    ("unequal atoms, the jp split", "lindblad", "smooth_jp", "asym", {}, dict(n_steps=30)),
    ("cheb_vector", "lindblad", "lp_square", "sym", {}, dict(method="cheb_vector")),
    ("cheb_vector, kets", "ket", "smooth_jp", "sym", {}, dict(method="cheb_vector", n_steps=30)),
    ("cheb_squaring", "lindblad", "lp_square", "sym", {}, dict(method="cheb_squaring")),
    ("cheb_squaring, the jp split", "lindblad", "smooth_jp", "sym", {}, dict(method="cheb_squaring", n_steps=30)),
    ("dopri5", "lindblad", "lp_square", "sym", {}, dict(method="dopri5")),
    ("RYD_SYM16=0", "lindblad", "lp_square", "sym", dict(SYM16=0), {}),
    ("RYD_SYM16=0", "lindblad", "smooth_jp", "sym", dict(SYM16=0), dict(n_steps=30)),
    ("RYD_KET_BLOCK=0", "ket", "lp_square", "sym", dict(KET_BLOCK=0), {}),
    ("RYD_KET_BLOCK=0, dim 4", "ket", "bangbang", "sym", dict(KET_BLOCK=0), dict(dim=4)),
    ("dim 4, unequal atoms", "lindblad", "lp_square", "asym4", {}, dict(dim=4)),
    ("dim 4, unequal atoms", "lindblad", "smooth_jp", "asym4", {}, dict(dim=4, n_steps=30)),
]


@pytest.mark.parametrize("case", SCRATCH, ids=lambda c: f"{c[0]}-{c[2]}".replace(" ", "_"))
def test_scratch_buffer_path(eng, sym149, case):
    what, evolution, protocol, points, env, desc = case
    if points == "sym":
        pall = sym149[protocol][:, :11].copy()
    elif points == "asym":
        pall = _asym(protocol, 11)
    else:
        pall = D4.random_points4(np.random.default_rng(20261020), 11, protocol)
        assert not E.symmetric_atoms(pall)
    for n in (1, 11):
        r = _check(eng, pall[:, :n].copy(), protocol, evolution, f"{what} {protocol} n={n}", env=env, **desc)
        assert np.all(r.status == 0)


def test_scratch_buffer_path_reports_failures(eng, sym149):
    """Status bits come through the scratch-buffer path as through the storing launch."""
    p = sym149["lp_square"][:, :11].copy()
    _invalidate(p, 6)
    r = _check(eng, p, "lp_square", "lindblad", "invalid row, RYD_SYM16=0", env=dict(SYM16=0))
    assert r.status[6] & N.STATUS_BAD_INPUT and np.all(np.delete(r.status, 6) == 0)


# ---------------------------------------------------------------------------------------------
# the host form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0], [0, 0]], ids=["one-slot", "two-slot"])
def test_host_form(sym149, devices):
    e = E.Engine(devices)
    try:
        for protocol, evolution in (("lp_square", "lindblad"), ("lp_square", "ket"), ("smooth_jp", "lindblad")):
            p = sym149[protocol][:, :37].copy()
            kw = dict(n_steps=30) if protocol == "smooth_jp" else {}
            full = e.run(p, protocol, evolution, **kw)
            so = e.run(p, protocol, evolution, states=False, **kw)
            assert so.state is None and full.state is not None
            _same_summary(so, full, f"host form {protocol} {evolution} {devices}")
            assert so.matvec_useful == full.matvec_useful and so.matvec_exec == full.matvec_exec
            with pytest.raises(ValueError, match="summary-only"):
                so.rho() if evolution == "lindblad" else so.kets()
            with _env(NOSTATE=0):
                _same_summary(e.run(p, protocol, evolution, states=False, **kw), full, "host form, RYD_NOSTATE=0")
        empty = e.run(np.zeros((N.NPARAM, 0)), "lp_square", "lindblad", states=False)
        assert empty.state is None and empty.summary.shape == (N.NSUMMARY, 0) and empty.status.shape == (0,)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------
# against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", ["lp_square", "bangbang", "smooth_jp"])
def test_populations_match_oracle(eng, protocol):
    """Summary-only POP0 of 8 random identical-atom points within TOL of the oracle's
    populations <x|rho_x|x>."""
    n, n_steps = 8, 30
    p = _sym(_random_points(np.random.default_rng(20261021), n, protocol))
    r = eng.run(p, protocol, "lindblad", n_steps=n_steps if protocol == "smooth_jp" else None, states=False)
    assert r.state is None and np.all(r.status == 0)
    pops = r.populations()
    kets = O.initial_kets()
    for i in range(n):
        ref = _oracle_point(p, i, protocol, n_steps=n_steps)
        for k, lab in enumerate(O.LABELS):
            x = int(np.argmax(np.abs(kets[lab])))
            err = abs(pops[i, k] - np.real(ref[lab][x, x]))
            assert err < TOL, f"{protocol} point {i} input {lab}: {err:g}"


@pytest.mark.parametrize("name", ["lp_medium_nf", "smooth_medium_nf", "lp_high_nf", "lp_low_nf", "smooth_high_nf",
                                  "smooth_low_nf", "bangbang_medium_nf", "lp_gaussian_nf"])
def test_ket_fixtures_summary_only(eng, evolution_golden, monkeypatch, name):
    """The noise-free fixtures' AVG_F and PENALTY from a summary-only run, against the stored
    reference states' figures."""
    run = E.Engine.run
    monkeypatch.setattr(E.Engine, "run", lambda self, *a, **kw: run(self, *a, states=False, **kw))
    e = evolution_golden[name]
    _, r = _run_cfg(eng, e["config"])
    assert r.evolution == "ket" and r.state is None and r.status[0] == 0
    _, avg, info = O.cz_fidelity(states_from_fixture(e))
    assert abs(r.col("AVG_F")[0] - avg) < TOL
    assert abs(r.col("PENALTY")[0] - info["cz_phase_fidelity"]) < TOL


# ---------------------------------------------------------------------------------------------
# the product path
# ---------------------------------------------------------------------------------------------
FIELDS = ("avg_fidelity", "fidelities", "populations", "controlled_phase", "cz_phase_fidelity", "status")


def _product_call(include_noise, phase_penalty, return_states):
    si, n, kw = SW.omega_delta_call(n_omega=10, n_delta=5, include_noise=include_noise)
    assert n == 50
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return SIM.simulate_CZ_gate_batch(si, n, phase_penalty=phase_penalty, return_states=return_states, **kw)


@pytest.fixture()
def recorded(monkeypatch):
    seen = []
    run = E.Engine.run

    def wrapper(self, *a, **kw):
        seen.append((a[2] if len(a) > 2 else kw.get("evolution"), kw.get("states", True)))
        return run(self, *a, **kw)
    monkeypatch.setattr(E.Engine, "run", wrapper)
    return seen


@pytest.mark.parametrize("include_noise,evolution", [(False, "ket"), (True, "lindblad")],
                         ids=["noise-free", "noisy-no-penalty"])
def test_product_path_runs_summary_only(recorded, include_noise, evolution):
    so = _product_call(include_noise, "reference" if not include_noise else "none", False)
    first = list(recorded)
    full = _product_call(include_noise, "reference" if not include_noise else "none", True)
    second = recorded[len(first):]
    assert first and all(ev == evolution and st is False for ev, st in first), first
    assert second and all(ev == evolution and st is True for ev, st in second), second
    assert so.states is None and full.states is not None
    assert so.avg_fidelity.shape == (50,)
    for f in FIELDS:
        a, b = np.asarray(getattr(so, f)), np.asarray(getattr(full, f))
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f)
        if a.dtype == np.float64:
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f)
        else:
            np.testing.assert_array_equal(a, b, err_msg=f)


def test_product_path_keeps_state_for_the_reference_penalty(recorded):
    """Noisy points under phase_penalty="reference": the LAPACK epilogue reads rho."""
    _product_call(True, "reference", False)
    assert recorded and all(ev == "lindblad" and st is True for ev, st in recorded), recorded
