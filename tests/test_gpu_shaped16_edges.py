"""The dim-3 shaped-pulse kernels at their edges: lindblad_shaped16_kernel (ryd_shaped16.inc:
identical atoms, the default, and bench.py's `shaped` workload) along every path of its
schedule -- the frame change under a ballot where only some rows of a wave rotate, |xi| != 1,
xi = 0, a negative amplitude, zero rates, sub-step counts that differ inside a wave, the
identity build, X_CAP, invalid rows (non-finite ones included) inside a live wave, more blocks
than XCDs with a ragged last wave, its work counters -- and the per-lane
lindblad_cheb_kernel<LP_SHAPED, SYM> (RYD_SHAPED16=0, method="cheb_vector"; unequal atoms run
SYM = false) on the full 25-coordinate state.

References: the expm oracle on the 81 x 81 Liouvillian at the run's own step count (TOL =
1e-10 absolute on the full 9 x 9 rho of all four inputs, the project's Lindblad tolerance) and
the other kernel (the same 1e-10 on the 25 x 4 state and the populations).  "Same bits" is
assert_array_equal.  Points and restated counts come from shaped_points.py, which
test_shaped_points_cpu.py checks; every oracle run is made once, in a module fixture.  Each
comparison prints its measured maximum before it asserts, and every run is checked for the
consistency of its summary columns (_summary_consistent) on the points with status 0.

NMV_EXEC.  On shaped16 it equals NMV_USEFUL and is 0 on a point that does not propagate.  On
the per-lane kernel include/ryd_engine.h defines it as wave-uniform: cheb_segment adds the
wave's series length on every lane, idle ones included, so an invalid, capped or skipped
point beside working ones reports its wave's count.  There the tests assert NMV_USEFUL == 0
and that NMV_EXEC is the one value of the point's wave.
"""
import os

import numpy as np
import pytest

import shaped_points as SP
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E

pytestmark = pytest.mark.gpu

TOL = 1e-10
QPOP = (0, 1, 3, 4)                   # |00>, |01>, |10>, |11> in the dim-3 two-atom basis
OWN = [i for name, i in N.S.items() if name != "NMV_EXEC"]     # columns that describe the point alone
KERNELS = ("shaped16", "per-lane")
IDENTITY = np.zeros((25, 4))
for _k in range(4):
    IDENTITY[5 * (_k >> 1) + (_k & 1), _k] = 1.0                # input k stays e_{a1} (x) e_{a2}


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _refs(name):
    """A module fixture refs_<name>: {(point, oracle shape, n_steps): rho} of one of
    shaped_points.oracle_cases(), computed once."""
    return pytest.fixture(scope="module", name="refs_" + name.replace(" ", "_"))(lambda: SP.oracle_refs(name))


refs_three_evaluations = _refs("three evaluations")
refs_xi_ladder = _refs("xi ladder")
refs_substep_mix = _refs("substep mix")
refs_unequal_atoms = _refs("unequal atoms")
refs_invalid_rows = _refs("invalid rows")
refs_cap_and_skip = _refs("cap and skip")
refs_many_blocks = _refs("many blocks")


def _per_lane(monkeypatch, on):
    if on:
        monkeypatch.setenv("RYD_SHAPED16", "0")
    else:
        monkeypatch.delenv("RYD_SHAPED16", raising=False)


def _run(eng, p, n_steps, shape="cosine", method="chebyshev", path=None, symmetric=None, what=""):
    """One lp_shaped Lindblad batch.  The kernel family is asked of ryd_batch_path for the
    descriptor that is launched and compared with ``path`` (default: SHAPED16 for identical
    atoms under the auto method, else LINDBLAD_CHEB); ``symmetric`` overrides the identical-atom
    flag the engine derives from the rate columns (a NaN pair is equal bits, not equal
    numbers).  The summary of every point with status 0 is checked for consistency."""
    p = E.param_block(p)
    if symmetric is None:
        symmetric = E.symmetric_atoms(p)
    desc = E.make_desc("lp_shaped", "lindblad", n_steps, shape, symmetric, method)
    if path is None:
        path = "SHAPED16" if symmetric and method == "chebyshev" else "LINDBLAD_CHEB"
    assert E.batch_path(desc) == N.PATH[path], f"{what}: not the {path} kernel"
    r = eng._summary_run(eng.lib.ryd_run_batch, desc, p, "lindblad", 3, True)
    _summary_consistent(r, what or path)
    return r


def _summary_consistent(r, what):
    """On the points with status 0: POPk is rho_k's own diagonal entry bit for bit, TRACE11 is
    1, AVG_POP == AVG_F == the mean of the four populations, the ket columns are NaN."""
    ok = r.status == 0
    if not ok.any():
        return
    rho, pops = r.rho(), r.populations()
    for k, q in enumerate(QPOP):
        np.testing.assert_array_equal(pops[ok, k], rho[ok, k, q, q].real, err_msg=f"{what}: POP{k}")
    dt = float(np.abs(r.col("TRACE11")[ok] - 1).max())
    print(f"{what}: max|TRACE11 - 1| = {dt:.3e}")
    assert dt < 1e-11
    mean = 0.25 * (pops[:, 0] + pops[:, 1] + pops[:, 2] + pops[:, 3])
    np.testing.assert_array_equal(r.col("AVG_POP")[ok], mean[ok], err_msg=f"{what}: AVG_POP")
    np.testing.assert_array_equal(r.col("AVG_F")[ok], mean[ok], err_msg=f"{what}: AVG_F")
    for name, width in (("OV_RE0", 4), ("OV_IM0", 4), ("CTRL_PHASE", 1), ("PENALTY", 1)):
        assert np.isnan(r.summary[N.S[name]:N.S[name] + width][:, ok]).all(), f"{what}: {name}"
    assert np.all(r.col("NSQUARE") == 0)


def _agree(ra, rb, what):
    """Two kernels on one batch: the 25 x 4 states and the populations within TOL."""
    ds = float(np.abs(ra.state - rb.state).max())
    dp = float(np.abs(ra.populations() - rb.populations()).max())
    print(f"{what}: max|dstate| = {ds:.3e}, max|dpop| = {dp:.3e}")
    assert np.all(ra.status == 0) and np.all(rb.status == 0)
    np.testing.assert_allclose(ra.state, rb.state, atol=TOL, rtol=0)
    np.testing.assert_allclose(ra.populations(), rb.populations(), atol=TOL, rtol=0)


def _vs_oracle(r, refs, what):
    """refs: {point index: rho (4, 9, 9)}; the full rho of all four inputs within TOL."""
    rho = r.rho()
    errs = {i: float(np.abs(rho[i] - ref).max()) for i, ref in refs.items()}
    print(f"{what}: max|drho| against the oracle " + ", ".join(f"[{i}] {e:.3e}" for i, e in errs.items()))
    for i, ref in refs.items():
        assert r.status[i] == 0
        np.testing.assert_allclose(rho[i], ref, atol=TOL, rtol=0, err_msg=f"{what}: point {i}")


def _pick(refs, shape, n_steps):
    """{point: rho} of one (shape, n_steps) from a fixture keyed (point, oracle shape, n_steps)."""
    s = shape if shape == "cosine" else "gaussian"
    out = {i: rho for (i, sh, ns), rho in refs.items() if sh == s and ns == n_steps}
    assert out
    return out


def _same_point(ra, ia, rb, ib, what, cols=None):
    """Points ia of run ra and ib of run rb have the same bits: state, status and the summary
    columns ``cols`` (all of them unless given), NaN positions compared as positions."""
    ia, ib = np.atleast_1d(ia), np.atleast_1d(ib)
    sa = ra.state.reshape(25, ra.n, 4)[:, ia]
    sb = rb.state.reshape(25, rb.n, 4)[:, ib]
    np.testing.assert_array_equal(sa, sb, err_msg=f"{what}: state")
    np.testing.assert_array_equal(ra.status[ia], rb.status[ib], err_msg=f"{what}: status")
    cols = list(range(N.NSUMMARY)) if cols is None else cols
    ma, mb = ra.summary[cols][:, ia], rb.summary[cols][:, ib]
    np.testing.assert_array_equal(np.isnan(ma), np.isnan(mb), err_msg=f"{what}: summary NaNs")
    keep = ~np.isnan(ma)
    np.testing.assert_array_equal(ma[keep], mb[keep], err_msg=f"{what}: summary")


def _holds_its_inputs(r, rows, what):
    """The rows kept their inputs: rho_x == |x><x| bit for bit, POP0..3 == 1, TRACE11 == 1,
    NMV_USEFUL == 0."""
    st = r.state.reshape(25, r.n, 4)
    for i in rows:
        np.testing.assert_array_equal(st[:, i], IDENTITY, err_msg=f"{what}: state of row {i}")
    np.testing.assert_array_equal(r.populations()[rows], 1.0, err_msg=f"{what}: POP")
    np.testing.assert_array_equal(r.col("TRACE11")[rows], 1.0, err_msg=f"{what}: TRACE11")
    np.testing.assert_array_equal(r.col("NMV_USEFUL")[rows], 0.0, err_msg=f"{what}: NMV_USEFUL")


def _idle_work_count(r, rows, kernel, what):
    """NMV_EXEC of rows that do not propagate, in a batch that is one wave of the per-lane
    kernel (at most 16 points): 0 on shaped16; on the per-lane kernel the wave's one value
    (include/ryd_engine.h: wave-uniform)."""
    exe = r.col("NMV_EXEC")
    print(f"{what}: NMV_EXEC {exe.astype(int).tolist()}")
    if kernel == "shaped16":
        np.testing.assert_array_equal(exe[rows], 0.0, err_msg=f"{what}: NMV_EXEC")
        np.testing.assert_array_equal(exe, r.col("NMV_USEFUL"), err_msg=f"{what}: NMV_EXEC != NMV_USEFUL")
    else:
        assert r.n <= 16 and np.unique(exe).size == 1 and exe[0] >= r.col("NMV_USEFUL").max() > 0, what


# ---- a. three evaluations agree, every shape -------------------------------------------------

@pytest.mark.parametrize("n_steps", [2, 3, 12])
@pytest.mark.parametrize("shape", SP.SHAPES)
def test_three_evaluations_agree(eng, monkeypatch, refs_three_evaluations, shape, n_steps):
    p = SP.THREE_POINTS
    assert p.shape[1] == 13 and E.symmetric_atoms(p)
    what = f"{shape}, n_steps = {n_steps}"
    _per_lane(monkeypatch, False)
    r16 = _run(eng, p, n_steps, shape, what=f"{what}, shaped16")
    _per_lane(monkeypatch, True)
    rl = _run(eng, p, n_steps, shape, path="LINDBLAD_CHEB", what=f"{what}, per-lane")
    _agree(r16, rl, f"{what}: shaped16 / per-lane")
    np.testing.assert_array_equal(r16.col("NMV_USEFUL"), SP.work_counts(p, n_steps))
    np.testing.assert_array_equal(r16.col("NMV_EXEC"), r16.col("NMV_USEFUL"))
    refs = _pick(refs_three_evaluations, shape, n_steps)
    assert sorted(refs) == [0, 5, 12]
    _vs_oracle(r16, refs, f"{what}, shaped16")
    _vs_oracle(rl, refs, f"{what}, per-lane")


# ---- b. the xi ladder ------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_xi_ladder(eng, monkeypatch, refs_xi_ladder, kernel):
    p, ns = SP.xi_ladder(), SP.EDGE_STEPS
    _per_lane(monkeypatch, kernel == "per-lane")
    path = "SHAPED16" if kernel == "shaped16" else "LINDBLAD_CHEB"
    r = _run(eng, p, ns, path=path, what=f"xi ladder, {kernel}")
    assert np.all(r.status == 0)
    _vs_oracle(r, _pick(refs_xi_ladder, "cosine", ns), f"xi ladder, {kernel}")
    rho = r.rho()[SP.ZERO_RATE_ROW, 3]
    pur = abs(np.einsum("ab,ba->", rho, rho).real - 1)
    print(f"xi ladder, {kernel}: zero-rate point |tr rho_11^2 - 1| = {pur:.3e}")
    assert pur <= 1e-10
    if kernel == "shaped16":
        np.testing.assert_array_equal(r.col("NMV_USEFUL"), SP.work_counts(p, ns))
    # each point alone: a row whose frame does not change is not disturbed by rotating
    # neighbours, and the other way round
    for i in range(8):
        one = _run(eng, p[:, i:i + 1].copy(), ns, path=path, what=f"xi ladder point {i} alone, {kernel}")
        _same_point(r, i, one, 0, f"xi ladder point {i} in its wave against alone, {kernel}",
                    cols=None if kernel == "shaped16" else OWN)


# ---- c. sub-step counts that differ inside a wave -------------------------------------------------

@pytest.mark.parametrize("n_steps", [2, 3])
def test_substep_mix(eng, monkeypatch, refs_substep_mix, n_steps):
    _per_lane(monkeypatch, False)
    p, want = SP.substep_mix(n_steps)
    r = _run(eng, p, n_steps, what=f"substep mix, n_steps = {n_steps}")
    print(f"substep mix, n_steps = {n_steps}: nsub {want['nsub'].tolist()}, kt {want['kt'].tolist()}, "
          f"NMV_USEFUL {r.col('NMV_USEFUL').astype(int).tolist()}")
    assert np.all(r.status == 0) and np.unique(want["nsub"]).size >= 3
    np.testing.assert_array_equal(r.col("NMV_USEFUL"), want["nmv"])
    np.testing.assert_array_equal(r.col("NMV_EXEC"), want["nmv"])
    _vs_oracle(r, _pick(refs_substep_mix, "cosine", n_steps), f"substep mix, n_steps = {n_steps}")
    for i in range(4):
        one = _run(eng, p[:, i:i + 1].copy(), n_steps, what=f"substep mix point {i} alone")
        _same_point(r, i, one, 0, f"substep mix point {i} in its wave against alone")


# ---- d. unequal atoms: lindblad_cheb_kernel<LP_SHAPED, false> -------------------------------------

def test_unequal_atoms_match_oracle_and_mirror(eng, monkeypatch, refs_unequal_atoms):
    _per_lane(monkeypatch, False)
    p, ns = SP.unequal_points(), SP.EDGE_STEPS
    for k in SP.RATES:
        assert np.all(p[N.P[k + "_A"]] != p[N.P[k + "_B"]])
    assert not E.symmetric_atoms(p)
    refs = _pick(refs_unequal_atoms, "cosine", ns)
    r = _run(eng, p, ns, path="LINDBLAD_CHEB", what="unequal atoms")
    assert np.all(r.status == 0)
    _vs_oracle(r, refs, "unequal atoms")
    m = _run(eng, SP.swap_atoms(p), ns, path="LINDBLAD_CHEB", what="atoms exchanged")
    assert np.all(m.status == 0)
    want = SP.swap_rho(r.rho())
    err = float(np.abs(m.rho() - want).max())
    print(f"unequal atoms: mirror max|drho| = {err:.3e}")
    np.testing.assert_allclose(m.rho(), want, atol=TOL, rtol=0)
    _vs_oracle(m, {i: SP.swap_rho(ref) for i, ref in refs.items()}, "atoms exchanged")
    assert np.abs(m.rho() - r.rho()).max() > 1e-6                       # the atoms do differ
    # the same points with identical atoms: the per-lane kernel with SYM = true against shaped16
    q = SP.sym(p.copy())
    rv = _run(eng, q, ns, method="cheb_vector", path="LINDBLAD_CHEB", what="sym(), cheb_vector")
    _agree(_run(eng, q, ns, what="sym(), shaped16"), rv, "sym() of the unequal points: shaped16 / cheb_vector")


# ---- e. invalid rows inside live waves ------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kernel", KERNELS)
def test_invalid_rows(eng, monkeypatch, refs_invalid_rows, kernel, variant):
    """A BAD_INPUT row holds the untouched inputs and flags nothing else, whatever made it
    invalid -- a non-finite V, DELTA, DELTA1, OMEGA or rate included -- and the valid rows of
    its wave have the bits of a run without it.  (Before its rows were neutralised, shaped16
    returned NaN rows with BAD_INPUT | NONFINITE for the non-finite columns: 0 * inf and
    0 * NaN in the generator rows of an inactive point.)"""
    p, valid = SP.invalid_rows(variant)
    ns = SP.EDGE_STEPS
    bad, good = np.flatnonzero(~valid), np.flatnonzero(valid)
    _per_lane(monkeypatch, kernel == "per-lane")
    path = "SHAPED16" if kernel == "shaped16" else "LINDBLAD_CHEB"
    what = f"invalid rows ({', '.join(SP.INVALID_WAYS[variant])}), {kernel}"
    r = _run(eng, p, ns, path=path, symmetric=True, what=what)
    print(f"{what}: status {r.status.tolist()}, NaN state rows "
          f"{[int(i) for i in range(9) if np.isnan(r.state.reshape(25, 9, 4)[:, i]).any()]}")
    np.testing.assert_array_equal(r.status[bad], N.STATUS_BAD_INPUT)
    np.testing.assert_array_equal(r.status[good], 0)
    _holds_its_inputs(r, bad, what)
    _idle_work_count(r, bad, kernel, what)
    clean = _run(eng, p[:, good].copy(), ns, path=path, symmetric=True, what=f"{what}: the valid rows alone")
    _same_point(r, good, clean, np.arange(good.size), f"{what}: valid rows against a run without the invalid ones")
    refs = _pick(refs_invalid_rows, "cosine", ns)           # the valid rows are those of variant 0
    np.testing.assert_array_equal(p[:, good], SP.invalid_rows(0)[0][:, good])
    assert sorted(refs) == [0, 8]
    _vs_oracle(r, refs, what)


# ---- f. X_CAP and the identity build -------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_cap_and_skip(eng, monkeypatch, refs_cap_and_skip, kernel):
    ns = SP.EDGE_STEPS
    p = SP.cap_and_skip(ns)
    _per_lane(monkeypatch, kernel == "per-lane")
    path = "SHAPED16" if kernel == "shaped16" else "LINDBLAD_CHEB"
    what = f"cap and skip, {kernel}"
    r = _run(eng, p, ns, path=path, what=what)
    print(f"{what}: status {r.status.tolist()}")
    np.testing.assert_array_equal(r.status, [0, N.STATUS_STEP_CAP, 0, 0])
    idle = [SP.CAPPED_ROW, SP.SKIPPED_ROW]
    _holds_its_inputs(r, idle, what)
    _idle_work_count(r, idle, kernel, what)
    clean = _run(eng, p[:, [0, 3]].copy(), ns, path=path, what=f"{what}: the valid rows alone")
    _same_point(r, [0, 3], clean, [0, 1], f"{what}: valid rows against a run of the two alone")
    _vs_oracle(r, _pick(refs_cap_and_skip, "cosine", ns), what)


# ---- g. more blocks than XCDs, a ragged last wave ---------------------------------------------------

def test_many_blocks(eng, monkeypatch, refs_many_blocks):
    _per_lane(monkeypatch, False)
    p, ns = SP.many_blocks(), SP.BLOCKS_STEPS
    assert p.shape[1] == 37 and E.symmetric_atoms(p)
    r = _run(eng, p, ns, what="many blocks")
    assert np.all(r.status == 0)
    np.testing.assert_array_equal(r.col("NMV_USEFUL"), SP.work_counts(p, ns))
    back = _run(eng, p[:, ::-1].copy(), ns, what="many blocks, reversed")
    _same_point(r, np.arange(37), back, np.arange(37)[::-1], "many blocks against the reversed batch")
    for i in (0, 3, 4, 31, 35, 36):
        one = _run(eng, p[:, i:i + 1].copy(), ns, what=f"many blocks point {i} alone")
        _same_point(r, i, one, 0, f"many blocks point {i} against alone")
    _vs_oracle(r, _pick(refs_many_blocks, "cosine", ns), "many blocks")


# ---- the recorded states of the build before invalid rows were neutralised -------------------------

def test_recorded_states_of_the_earlier_build(eng, monkeypatch):
    """tests/golden/shaped16_edges_*.npy (tools/shaped16_edges_baseline.py save) hold the states
    of tests a and g from the build before sh_point_or_neutral.  The build that introduced it
    gave the same bits (tools/shaped16_edges_baseline.py check, profiles/shaped16_edges/);
    another compiler may contract differently, so the suite asks for TOL and prints whether the
    bits are still the same."""
    _per_lane(monkeypatch, False)
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    three = np.load(os.path.join(gold, "shaped16_edges_three_evaluations.npy"))
    blocks = np.load(os.path.join(gold, "shaped16_edges_many_blocks.npy"))
    assert three.shape == (4, 3, 25, 52) and blocks.shape == (25, 148)
    got = np.stack([np.stack([_run(eng, SP.THREE_POINTS, ns, shape, what=f"recorded, {shape}, {ns}").state
                              for ns in (2, 3, 12)]) for shape in SP.SHAPES])
    gotb = _run(eng, SP.many_blocks(), SP.BLOCKS_STEPS, what="recorded, many blocks").state
    for name, a, b in (("three evaluations", got, three), ("many blocks", gotb, blocks)):
        same = np.array_equal(a.view(np.uint64), b.view(np.uint64))
        print(f"recorded states, {name}: max|dstate| = {float(np.abs(a - b).max()):.3e}, same bits: {same}")
        np.testing.assert_allclose(a, b, atol=TOL, rtol=0)
