"""The two kernels that produce the hilbert_space_dim=4 Lindblad states, at their edges:
lindblad4_prop_kernel (ryd_dim4_prop.inc: identical atoms, the default) along every path of
its propagator build -- the memo of the last build, rows of a wave that rebuild on different
segments, skipped segments, a second build for |xi| != 1, every series length, the identity
build, X_CAP, invalid rows -- and lindblad4_cheb_kernel<P, SYM> (unequal atoms, shaped
pulses, method="cheb_vector", RYD_DIM4_PROP=0) on the full 36-coordinate state.

References: the expm oracle on the 256 x 256 Liouvillian (TOL = 1e-10 absolute on the full
16 x 16 rho of all four inputs, the project's dim-4 tolerance) and the other kernel (the same
1e-10 on the 36 x 4 state and the populations).  "Same bits" is assert_array_equal.  Points
and restated depths come from dim4_points.py; every oracle run is made once, in a fixture.
Each comparison prints its measured maximum before it asserts.
"""
import numpy as np
import pytest

import dim4_points as D4
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from oracle import lindblad_oracle as O
from process_map4_util import lp_shaped_segments, spec4_from_params

pytestmark = pytest.mark.gpu

TOL = 1e-10
QPOP = (0, 1, 4, 5)                   # |00>, |01>, |10>, |11> in the dim-4 two-atom basis
# protocol: (n_steps between the kernels, n_steps against the oracle)
STEPS = {"lp_square": (None, None), "bangbang": (None, None), "smooth_jp": (30, 8)}
PROTOCOLS = tuple(STEPS)
SHAPED_STEPS = 6


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _run(eng, p, protocol, method="chebyshev", n_steps=None, shape="square"):
    return eng.run(p, protocol, "lindblad", n_steps=n_steps, shape=shape, method=method, dim=4)


def _oracle(p, i, protocol, n_steps=None):
    return D4.run_segments(spec4_from_params(p, i, protocol, n_steps=n_steps or 300))


def _agree(ra, rb, what):
    """Two kernels on one batch: the 36 x 4 states and the populations within TOL."""
    ds = float(np.abs(ra.state - rb.state).max())
    dp = float(np.abs(ra.populations() - rb.populations()).max())
    print(f"{what}: max|dstate| = {ds:.3e}, max|dpop| = {dp:.3e}")
    assert np.all(ra.status == 0) and np.all(rb.status == 0)
    np.testing.assert_allclose(ra.state, rb.state, atol=TOL, rtol=0)
    np.testing.assert_allclose(ra.populations(), rb.populations(), atol=TOL, rtol=0)


def _vs_oracle(r, refs, what):
    """refs: {point index: rho (4, 16, 16)}; the full rho of all four inputs within TOL."""
    rho = r.rho()
    errs = {i: float(np.abs(rho[i] - ref).max()) for i, ref in refs.items()}
    print(f"{what}: max|drho| against the oracle " + ", ".join(f"[{i}] {e:.3e}" for i, e in errs.items()))
    for i, ref in refs.items():
        assert r.status[i] == 0
        np.testing.assert_allclose(rho[i], ref, atol=TOL, rtol=0, err_msg=f"{what}: point {i}")


def _same_point(ra, ia, rb, ib, what, summary=True):
    """Points ia of run ra and ib of run rb have the same bits: state, status, and (the prop
    kernel's summary columns all describe the point alone) the summary."""
    ia, ib = np.atleast_1d(ia), np.atleast_1d(ib)
    sa = ra.state.reshape(36, ra.n, 4)[:, ia]
    sb = rb.state.reshape(36, rb.n, 4)[:, ib]
    np.testing.assert_array_equal(sa, sb, err_msg=f"{what}: state")
    np.testing.assert_array_equal(ra.status[ia], rb.status[ib], err_msg=f"{what}: status")
    if summary:
        ma, mb = ra.summary[:, ia], rb.summary[:, ib]
        np.testing.assert_array_equal(np.isnan(ma), np.isnan(mb), err_msg=f"{what}: summary NaNs")
        keep = ~np.isnan(ma)
        np.testing.assert_array_equal(ma[keep], mb[keep], err_msg=f"{what}: summary")


def _pops_and_trace(r, what):
    """POP0..3 are rho's diagonal entries at the inputs' own basis states; |11>'s trace is 1."""
    rho = r.rho()
    for k, q in enumerate(QPOP):
        np.testing.assert_array_equal(r.populations()[:, k], rho[:, k, q, q].real, err_msg=f"{what}: POP{k}")
    dt = float(np.abs(r.col("TRACE11") - 1).max())
    print(f"{what}: max|TRACE11 - 1| = {dt:.3e}")
    assert dt < 1e-11


def _sum_depths(xs):
    return sum(D4.depth_terms4(x)[0] for x in xs)


def _sum_terms(xs):
    return sum(D4.depth_terms4(x)[2] + 1 for x in xs)


# ---- a. three evaluations agree ---------------------------------------------------------

def _ident_points(protocol):
    """13 identical-atom points (three waves and a ragged row), nominal and strong
    alternating, so every wave mixes the two classes and their squaring depths."""
    seed = 20261100 + PROTOCOLS.index(protocol)
    kinds = ["nominal", "strong"] * 6 + ["nominal"]
    return D4.sym(D4.random_points4(np.random.default_rng(seed), 13, protocol, kinds))


@pytest.fixture(scope="module", params=PROTOCOLS)
def ident(request):
    protocol = request.param
    p = _ident_points(protocol)
    assert E.symmetric_atoms(p)
    # a strong point inside a full wave, a nominal one, and the ragged row
    refs = {i: _oracle(p, i, protocol, STEPS[protocol][1]) for i in (1, 6, 12)}
    return protocol, p, refs


def test_three_evaluations_agree(eng, ident):
    protocol, p, refs = ident
    ns_k, ns_o = STEPS[protocol]
    rp = _run(eng, p, protocol, "chebyshev", ns_k)
    rv = _run(eng, p, protocol, "cheb_vector", ns_k)
    print(f"{protocol}: NSQUARE {rp.col('NSQUARE').astype(int).tolist()}, "
          f"NMV_USEFUL {rp.col('NMV_USEFUL').astype(int).tolist()}")
    assert np.all(rv.col("NSQUARE") == 0)
    if protocol != "smooth_jp":                 # a short smooth-JP step of a strong point needs none
        assert np.all(rp.col("NSQUARE") > 0)
    _agree(rp, rv, f"{protocol} prop / vector")
    if ns_o != ns_k:
        rp = _run(eng, p, protocol, "chebyshev", ns_o)
        rv = _run(eng, p, protocol, "cheb_vector", ns_o)
        _agree(rp, rv, f"{protocol} prop / vector, n_steps = {ns_o}")
    for r, name in ((rp, "prop"), (rv, "vector")):
        _vs_oracle(r, refs, f"{protocol} {name}")
        _pops_and_trace(r, f"{protocol} {name}")


# ---- b. RYD_DIM4_PROP=0 -------------------------------------------------------------------

def test_dim4_prop_switch(eng, monkeypatch):
    p = _ident_points("lp_square")
    monkeypatch.delenv("RYD_DIM4_PROP", raising=False)
    rv = _run(eng, p, "lp_square", "cheb_vector")
    rp = _run(eng, p, "lp_square", "chebyshev")
    assert np.all(rp.status == 0) and np.all(rp.col("NSQUARE") > 0)
    monkeypatch.setenv("RYD_DIM4_PROP", "0")
    r0 = _run(eng, p, "lp_square", "chebyshev")
    assert np.all(r0.col("NSQUARE") == 0)
    _same_point(r0, np.arange(13), rv, np.arange(13), "RYD_DIM4_PROP=0 against cheb_vector")
    monkeypatch.delenv("RYD_DIM4_PROP")
    r1 = _run(eng, p, "lp_square", "chebyshev")
    _same_point(r1, np.arange(13), rp, np.arange(13), "RYD_DIM4_PROP unset again")


# ---- c. unequal atoms against the oracle --------------------------------------------------

@pytest.fixture(scope="module", params=PROTOCOLS)
def unequal(request):
    protocol = request.param
    rng = np.random.default_rng(20261200 + PROTOCOLS.index(protocol))
    kinds = {"lp_square": ("nominal", "strong", "strong"), "bangbang": ("nominal", "strong"),
             "smooth_jp": ("strong", "nominal")}[protocol]
    p = D4.random_points4(rng, len(kinds), protocol, kinds)
    for k in D4.RATES4:
        assert np.all(p[N.P[k + "_A"]] != p[N.P[k + "_B"]])
    if protocol == "lp_square":                 # one further point differs in GMJ_B alone
        g = D4.sym(p[:, 1:2].copy())
        g[N.P["GMJ_B"]] *= 3.0
        p = np.concatenate([p, g], axis=1)
    assert not E.symmetric_atoms(p)
    ns = STEPS[protocol][1]
    return protocol, p, ns, {i: _oracle(p, i, protocol, ns) for i in range(p.shape[1])}


def test_unequal_atoms_match_oracle_and_mirror(eng, unequal):
    protocol, p, ns, refs = unequal
    r = _run(eng, p, protocol, "chebyshev", ns)
    assert np.all(r.status == 0) and np.all(r.col("NSQUARE") == 0)      # the per-lane sector kernel
    _vs_oracle(r, refs, f"{protocol} unequal atoms")
    _pops_and_trace(r, f"{protocol} unequal atoms")
    # atoms exchanged: the same states with the atoms swapped and inputs 01 <-> 10 exchanged
    m = _run(eng, D4.swap_atoms(p), protocol, "chebyshev", ns)
    assert np.all(m.status == 0)
    want = D4.swap_rho(r.rho())
    err = float(np.abs(m.rho() - want).max())
    print(f"{protocol} unequal atoms: mirror max|drho| = {err:.3e}")
    np.testing.assert_allclose(m.rho(), want, atol=TOL, rtol=0)
    _vs_oracle(m, {i: D4.swap_rho(ref) for i, ref in refs.items()}, f"{protocol} atoms exchanged")
    assert np.abs(m.rho() - r.rho()).max() > 1e-6                       # the atoms do differ


# ---- d. shaped LP -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shaped():
    """Two strong points under a cosine envelope of SHAPED_STEPS steps: identical atoms
    (lindblad4_cheb_kernel<LP_SHAPED, true>) and unequal atoms (<LP_SHAPED, false>)."""
    p = D4.random_points4(np.random.default_rng(20261300), 2, "lp_square", "strong")
    p[N.P["AREA_CORR"]] = 2.0
    p[:, 0:1] = D4.sym(p[:, 0:1].copy())
    refs = []
    for i in range(2):
        spec = spec4_from_params(p, i, "lp_shaped", pulse_shape="cosine")
        assert spec.area_correction == 2.0 and spec.pulse_shape == "cosine"
        refs.append(D4.run_segments(spec, lp_shaped_segments(spec, SHAPED_STEPS)))
    return p, refs


def test_shaped_lp_matches_oracle(eng, shaped):
    p, refs = shaped
    assert E.symmetric_atoms(p[:, :1]) and not E.symmetric_atoms(p[:, 1:])
    for i, what in enumerate(("identical atoms", "unequal atoms")):
        r = _run(eng, p[:, i:i + 1].copy(), "lp_shaped", n_steps=SHAPED_STEPS, shape="cosine")
        _vs_oracle(r, {0: refs[i]}, f"shaped LP, {what}")
        _pops_and_trace(r, f"shaped LP, {what}")
    both = _run(eng, p, "lp_shaped", n_steps=SHAPED_STEPS, shape="cosine")
    _vs_oracle(both, dict(enumerate(refs)), "shaped LP, one batch")


# ---- e. depth and series ladders ------------------------------------------------------------

@pytest.fixture(scope="module")
def ladders(eng):
    parts = [D4.tau_ladder4(), D4.x_ladder4()]
    p = np.concatenate(parts, axis=1)
    nt = parts[0].shape[1]
    refs = {i: _oracle(p, i, "lp_square") for i in (0, nt - 1)}
    return dict(p=p, tau=slice(0, nt), x=slice(nt, p.shape[1]), refs=refs,
                rp=_run(eng, p, "lp_square", "chebyshev"), rv=_run(eng, p, "lp_square", "cheb_vector"))


def test_tau_ladder_depths(ladders):
    p, rp, t = ladders["p"], ladders["rp"], ladders["tau"]
    assert E.symmetric_atoms(p)
    _agree(rp, ladders["rv"], "LP ladders prop / vector")
    x = (D4.omega4(p, "lp_square") * p[N.P["TAU"]])[t]
    s = np.array([D4.depth_terms4(v)[0] for v in x])
    nsq = rp.col("NSQUARE")[t]
    print(f"tau ladder: NSQUARE {nsq.astype(int).tolist()}")
    assert np.all(np.diff(nsq) >= 0) and np.unique(nsq).size == 3
    np.testing.assert_array_equal(nsq, s)
    _vs_oracle(rp, ladders["refs"], "tau ladder ends, prop")
    _vs_oracle(ladders["rv"], ladders["refs"], "tau ladder ends, vector")


def test_x_ladder_series_lengths_and_identity(ladders):
    p, rp, xl = ladders["p"], ladders["rp"], ladders["x"]
    x = (D4.omega4(p, "lp_square") * p[N.P["TAU"]])[xl]
    dk = [D4.depth_terms4(v) for v in x]
    kt = np.array([d[2] for d in dk])
    use = rp.col("NMV_USEFUL")[xl]
    print(f"x ladder: NMV_USEFUL {use.astype(int).tolist()}")
    np.testing.assert_array_equal(use, kt + 1)                          # xi = i: one build
    np.testing.assert_array_equal(rp.col("NSQUARE")[xl], [d[0] for d in dk])
    assert set(range(1, 14)) <= set((use - 1).astype(int))
    # the last point is the identity build: the four basis inputs come back exactly
    assert dk[-1][3] and x[-1] < D4.X_SKIP and use[-1] == 0
    want = np.zeros((36, 4))
    for k in range(4):
        want[6 * (k >> 1) + (k & 1), k] = 1.0
    last = rp.n - 1
    np.testing.assert_array_equal(rp.state.reshape(36, rp.n, 4)[:, last], want)
    assert rp.status[last] == 0
    np.testing.assert_array_equal(ladders["rv"].state.reshape(36, rp.n, 4)[:, last], want)


# ---- f. rows that rebuild on different segments ------------------------------------------------

@pytest.fixture(scope="module")
def schedules():
    p4 = D4.bb_schedule_points()
    return p4, {i: _oracle(p4, i, "bangbang") for i in range(4)}


def test_rows_rebuild_on_different_segments(eng, schedules):
    p4, refs = schedules
    p = np.concatenate([p4, p4[:, ::-1]], axis=1)             # the second wave: the same points reversed
    at = np.array([0, 1, 2, 3, 3, 2, 1, 0])                   # column -> point
    assert E.symmetric_atoms(p)
    r = _run(eng, p, "bangbang")
    builds = [D4.bb_builds(p4, i) for i in range(4)]
    assert len(set(len(b) for b in builds)) >= 3
    nsq, use = r.col("NSQUARE"), r.col("NMV_USEFUL")
    print(f"bang-bang schedules: builds required {[len(b) for b in builds]}, "
          f"NSQUARE {nsq.astype(int).tolist()}, NMV_USEFUL {use.astype(int).tolist()}")
    for i in range(4):
        one = _run(eng, p4[:, i:i + 1].copy(), "bangbang")
        for c in (i, 7 - i):
            _same_point(r, c, one, 0, f"schedule point {i} in column {c} against alone")
    np.testing.assert_array_equal(nsq, [_sum_depths(builds[i]) for i in at])
    np.testing.assert_array_equal(use, [_sum_terms(builds[i]) for i in at])
    _vs_oracle(r, refs, "bang-bang schedules, prop")
    # the vector kernel on the three points made of short segments (point 3: the next test)
    rv = _run(eng, p4[:, :3].copy(), "bangbang", "cheb_vector")
    _agree(_run(eng, p4[:, :3].copy(), "bangbang"), rv, "bang-bang schedules 0-2 prop / vector")
    _vs_oracle(rv, {i: refs[i] for i in range(3)}, "bang-bang schedules 0-2, vector")


@pytest.mark.xfail(strict=True, reason=(
    "cheb_segment (shared with the dim-3 kernels) runs ONE Chebyshev series over a whole segment; on a "
    "single segment that is both long in V dt and dissipative its rounding error is amplified "
    "exponentially in the segment's length.  Schedule point 3 (NSEG = 1, V / Omega = 656, x = 14522, "
    "GSC dt = 0.7): max|drho| = 7.2e-10 against the oracle on input |11> (inputs 00 / 01 / 10 at "
    "1e-13; lindblad4_prop_kernel 1.5e-12).  Along the segment's length: 2.8e-13 at x = 7261, "
    "9.2e-12 at 10165, 1.5e-10 at 13070, 7.2e-10 at 14522, 7.7e-9 at 17426, 6.1e-7 at 21783; with "
    "every rate off 2.6e-14 at the same x; dim 3 (lindblad_cheb_kernel) at the same point without "
    "GMJ 1.8e-11, as dim 4 without GMJ.  DESIGN.md section 0, row f4."))
def test_vector_kernel_on_one_long_dissipative_segment(eng, schedules):
    p4, refs = schedules
    rv = _run(eng, p4[:, 3:4].copy(), "bangbang", "cheb_vector")
    _vs_oracle(rv, {0: refs[3]}, "bang-bang schedule point 3 (one long segment), vector")


# ---- g. non-unit xi -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nonunit():
    kinds = ["strong", "nominal"] * 4 + ["strong"]
    p = D4.sym(D4.random_points4(np.random.default_rng(20261400), 9, "lp_square", kinds))
    p[N.P["XI_RE"], 5], p[N.P["XI_IM"], 5] = 0.0, 1.0         # |Omega xi| = |Omega| exactly: one build
    assert len(D4.lp_builds(p, 5)) == 1
    q = p.copy()
    q[N.P["XI_RE"], 5] *= 1.01
    q[N.P["XI_IM"], 5] *= 1.01
    builds = D4.lp_builds(q, 5)
    assert len(builds) == 2
    D4.assert_depth_margin(builds, "non-unit xi")
    assert min(D4.term_margin(x) for x in builds) >= D4.DEPTH_MARGIN
    return p, q, builds, {5: _oracle(q, 5, "lp_square")}


def test_non_unit_xi_builds_twice(eng, nonunit):
    p, q, builds, refs = nonunit
    base = _run(eng, p, "lp_square")
    r = _run(eng, q, "lp_square")
    rv = _run(eng, q, "lp_square", "cheb_vector")
    print(f"non-unit xi: NSQUARE base {base.col('NSQUARE').astype(int).tolist()}, "
          f"perturbed {r.col('NSQUARE').astype(int).tolist()}")
    assert np.all(base.status == 0)
    assert base.col("NSQUARE")[5] == D4.depth_terms4(builds[0])[0] > 0
    assert r.col("NSQUARE")[5] == _sum_depths(builds) > base.col("NSQUARE")[5]
    assert r.col("NMV_USEFUL")[5] == _sum_terms(builds) > base.col("NMV_USEFUL")[5]
    _agree(r, rv, "non-unit xi prop / vector")
    _vs_oracle(r, refs, "non-unit xi, prop")
    _vs_oracle(rv, refs, "non-unit xi, vector")
    others = np.flatnonzero(np.arange(9) != 5)
    _same_point(r, others, base, others, "the unperturbed points")


# ---- h. neighbour independence -------------------------------------------------------------------

def _five():
    kinds = ["nominal", "strong", "nominal", "strong", "strong"]
    return D4.sym(D4.random_points4(np.random.default_rng(20261500), 5, "lp_square", kinds))


def test_rows_beside_invalid_rows(eng):
    """Five points of mixed depth, each at each of the four row positions of a wave beside
    three NaN rows, and a wholly invalid wave between two valid ones."""
    p = _five()
    a = _run(eng, p, "lp_square")
    assert np.all(a.status == 0) and np.unique(a.col("NSQUARE")).size >= 3
    for i in range(5):
        _same_point(a, i, _run(eng, p[:, i:i + 1].copy(), "lp_square"), 0, f"point {i} alone")
    # wave w = 4 i + pos holds point i at row `pos`; the NaN rows' rate columns stay equal
    # numbers, so the batch still counts as identical atoms
    q = np.full((N.NPARAM, 5 * 4 * 4), np.nan)
    for k in D4.RATES4:
        q[N.P[k + "_A"]] = q[N.P[k + "_B"]] = 0.0
    at = np.array([(4 * i + pos) * 4 + pos for i in range(5) for pos in range(4)])
    q[:, at] = np.repeat(p, 4, axis=1)
    assert E.symmetric_atoms(q)
    d = _run(eng, q, "lp_square")
    bad = np.ones(q.shape[1], bool)
    bad[at] = False
    assert np.all(d.status[bad] & N.STATUS_BAD_INPUT)
    _same_point(a, np.repeat(np.arange(5), 4), d, at, "beside NaN rows")
    # valid wave, invalid wave, valid wave
    w = np.concatenate([p[:, :4], p[:, :4], p[:, [4, 0, 1, 2]]], axis=1)
    w[N.P["OMEGA"], 4:8] = 0.0
    assert E.symmetric_atoms(w)
    for method in ("chebyshev", "cheb_vector"):
        c = _run(eng, w, "lp_square", method)
        assert np.all(c.status[4:8] & N.STATUS_BAD_INPUT)
        ok = np.r_[0:4, 8:12]
        ref = a if method == "chebyshev" else _run(eng, p, "lp_square", method)
        _same_point(c, ok, ref, [0, 1, 2, 3, 4, 0, 1, 2], f"{method}: beside an invalid wave",
                    summary=method == "chebyshev")


@pytest.mark.parametrize("method", ["chebyshev", "cheb_vector"])
def test_bad_mj_rate_and_step_cap_flag_their_point_only(eng, method):
    kinds = ["strong", "nominal"] * 4 + ["strong"]
    p = D4.sym(D4.random_points4(np.random.default_rng(20261600), 9, "lp_square", kinds))
    base = _run(eng, p, "lp_square", method)
    assert np.all(base.status == 0)
    prop = method == "chebyshev"
    # a negative mJ rate on both atoms (still "identical atoms")
    q = p.copy()
    q[N.P["GMJ_A"], 2] = q[N.P["GMJ_B"], 2] = -1.0
    assert E.symmetric_atoms(q)
    r = _run(eng, q, "lp_square", method)
    good = np.flatnonzero(np.arange(9) != 2)
    assert r.status[2] & N.STATUS_BAD_INPUT and np.all(r.status[good] == 0)
    _same_point(r, good, base, good, f"{method}: beside a bad mJ rate", summary=prop)
    # x = 3e6 > X_CAP
    q = p.copy()
    q[N.P["TAU"], 6] = 3e6 / D4.omega4(p, "lp_square")[6]
    assert (D4.omega4(q, "lp_square") * q[N.P["TAU"]])[6] > 1.4 * D4.X_CAP
    r = _run(eng, q, "lp_square", method)
    good = np.flatnonzero(np.arange(9) != 6)
    assert r.status[6] == N.STATUS_STEP_CAP and np.all(r.status[good] == 0)
    _same_point(r, good, base, good, f"{method}: beside a capped point", summary=prop)
