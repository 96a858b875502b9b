"""Inputs for the dim-3 shaped-pulse kernel tests (lindblad_shaped16_kernel and the per-lane
lindblad_cheb_kernel<LP_SHAPED, SYM>): random parameter points with an area correction, the
shaped16 kernel's spectral bound, sub-step count, series degree and work counters restated on
the host, the named edge batches that walk its code paths, and the expm oracle for a shaped
pulse of any step count.  No GPU is touched here; test_shaped_points_cpu.py checks these
inputs, test_gpu_shaped16_edges.py runs them.

Two classes of point, as in dim4_points.py.  "nominal" is test_gpu_parity._random_points:
V / Omega from 10 to 1000.  "strong" has V / Omega from 0.3 to 30, DELTA1 up to 0.3 Omega and
rates that are percents of Omega, so every one of the 25 sector coordinates of every input is
large against the 1e-10 absolute tolerance.
"""
import contextlib
import math

import numpy as np
import scipy.linalg as sla

import dim4_points as D4
from bench import _cheb_terms
from noisyquantumsimulator_amd import _native as N
from oracle import lindblad_oracle as O
from process_map4_util import lp_shaped_segments
from test_gpu_parity import _random_points

RATES = D4.RATES
RATE_COLS = tuple(f"{k}_{a}" for a in "AB" for k in RATES)
X_SKIP = D4.X_SKIP              # ryd_engine.hip: at or below this a point is the identity
X_CAP = D4.X_CAP                # ryd_engine.hip: above this a segment is refused (STEP_CAP)
SH_XSUB = 20.0                  # ryd_shaped16.inc: the largest series argument of one (sub-)step
STABLE_MARGIN = 1e-9            # relative distance every x keeps from a change of nsub or kt
STRONG_RATES = D4.STRONG_RATES[:4]
SHAPES = ("cosine", "gaussian", "blackman", "square")

sym = D4.sym                    # the GMJ columns it also copies are zero in dim 3
swap_atoms = D4.swap_atoms


def random_shaped_points(rng, n, kind="nominal"):
    """(NPARAM, n) dim-3 LP-shaped points, every rate column different between the two atoms,
    AREA_CORR from [1, 2.5] (_random_points leaves it 0: a pulse of zero amplitude).  ``kind``
    is "nominal", "strong", or a sequence of the two, one per point."""
    p = _random_points(rng, n, "lp_square")
    kinds = [kind] * n if isinstance(kind, str) else list(kind)
    assert len(kinds) == n and set(kinds) <= {"nominal", "strong"}
    strong = np.array([k == "strong" for k in kinds], bool)
    Om = p[N.P["OMEGA"]]
    ratio = 10 ** rng.uniform(-0.5, 1.5, n)
    d1 = rng.uniform(0, 0.3, n)
    frac = {(k, a): rng.uniform(0, hi, n) for k, hi in STRONG_RATES for a in "AB"}
    p[N.P["AREA_CORR"]] = rng.uniform(1.0, 2.5, n)
    p[N.P["V"], strong] = (ratio * Om)[strong]
    p[N.P["DELTA1"], strong] = (d1 * Om)[strong]
    for (k, a), f in frac.items():
        p[N.P[f"{k}_{a}"], strong] = (f * Om)[strong]
    return p


def swap_rho(rho):
    """rho (..., 4 inputs, 9, 9) of the atom-swapped problem: inputs 01 <-> 10 exchanged and
    both two-atom indices (3 a + b) -> (3 b + a)."""
    r = np.asarray(rho)[..., [0, 2, 1, 3], :, :]
    lead = r.shape[:-2]
    return r.reshape(lead + (3, 3, 3, 3)).swapaxes(-4, -3).swapaxes(-2, -1).reshape(lead + (9, 9))


def set_xi(p, i, xi):
    p[N.P["XI_RE"], i], p[N.P["XI_IM"], i] = complex(xi).real, complex(xi).imag


# ---- the oracle -------------------------------------------------------------------------

def one_thread():
    """A context in which the BLAS behind scipy and numpy runs one thread: on 81 x 81 matrices
    a threaded BLAS only thrashes (the suite's conftest limits the libraries loaded before it
    ran, which need not include scipy's)."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:                                   # pragma: no cover
        return contextlib.nullcontext()
    return threadpool_limits(1)


def c_ops3_from_params(p, i):
    """Per-atom dim-3 collapse operators from the packed rate columns of point i, as
    test_gpu_parity._oracle_point builds them."""
    I3 = np.eye(3)
    unit = lambda to, frm: np.outer(I3[to], I3[frm]).astype(complex)
    ops = []
    for atom in "AB":
        emb = (lambda o: np.kron(o, I3)) if atom == "A" else (lambda o: np.kron(I3, o))
        for key, op in (("G1", unit(1, 2)), ("G0", unit(0, 2)), ("GPHI", unit(2, 2)), ("GSC", unit(1, 1))):
            rate = p[N.P[f"{key}_{atom}"], i]
            if rate > 0:
                ops.append(np.sqrt(rate) * emb(op))
    return ops


def spec3_from_params(p, i, shape):
    g = lambda k: p[N.P[k], i]
    return O.PointSpec(protocol="lp_shaped", Omega=g("OMEGA"), V=g("V"), Delta=g("DELTA"), tau=g("TAU"),
                       xi=complex(g("XI_RE"), g("XI_IM")), delta_zeeman=g("DELTA1"), dim=3, pulse_shape=shape,
                       area_correction=g("AREA_CORR"), c_ops=c_ops3_from_params(p, i))


def run_segments3(spec, n_steps, split=1):
    """rho (4 inputs in O.LABELS order, 9, 9) after the shaped pulse pair of ``n_steps`` time
    steps per pulse (process_map4_util.lp_shaped_segments: the reference recipe, which
    O.segments fixes at 500): one expm of the 81 x 81 column-stacked Liouvillian per distinct
    segment, applied to the four basis inputs together.  ``split`` > 1 takes every segment as
    expm(L dt / split)^split instead: the same map by another evaluation."""
    kets = O.initial_kets(3)
    v = np.stack([O.vec(np.outer(kets[lab], kets[lab].conj())) for lab in O.LABELS], axis=1)
    props = {}
    with one_thread():
        for H, t, _ in lp_shaped_segments(spec, n_steps):
            key = H.tobytes()
            if key not in props:                    # a constant envelope repeats one segment
                P = sla.expm(O.liouvillian(H, spec.c_ops) * (float(t[-1] - t[0]) / split))
                props[key] = np.linalg.matrix_power(P, split)
            v = props[key] @ v
    return np.stack([O.unvec(v[:, k], 9) for k in range(4)])


def oracle(p, i, shape, n_steps, split=1):
    return run_segments3(spec3_from_params(p, i, shape), n_steps, split)


# ---- the shaped16 kernel's own numbers, restated ----------------------------------------

def omega_shaped(p, amplitude=True):
    """The one-per-point spectral bound of lindblad_shaped16_kernel: h_bounds' span at
    half-width 0.5 |OMEGA AREA_CORR| max(1, |xi|), plus the eight rate columns.  Without
    ``amplitude``: the span at half-width 0, below the bound of every segment of either
    kernel."""
    xabs = np.sqrt(p[N.P["XI_RE"]] ** 2 + p[N.P["XI_IM"]] ** 2)
    om = p[N.P["OMEGA"]] * p[N.P["AREA_CORR"]] * np.maximum(1.0, xabs)
    w = 0.5 * np.sqrt(om * om) if amplitude else 0.0 * om
    assert not np.any(p[N.P["GMJ_A"]]) and not np.any(p[N.P["GMJ_B"]])
    return D4.omega4(p, "lp_shaped", seg_w=w)


def x_shaped(p, n_steps):
    """The series argument x = omega TAU / n_steps of every segment of a point."""
    return omega_shaped(p) * p[N.P["TAU"]] / n_steps


def substeps_terms(x):
    """(nsub, kt) of an active point: ceil(x / SH_XSUB) equal sub-steps above SH_XSUB, and
    the series degree of one sub-step."""
    x = float(x)
    nsub = int(math.ceil(x / SH_XSUB)) if x > SH_XSUB else 1
    return nsub, _cheb_terms(x / nsub)


def stable(x):
    """nsub and kt are the same at x (1 +- STABLE_MARGIN): the device's cheb_terms loop and
    ceil cannot then disagree with the host's by rounding."""
    x = float(x)
    return substeps_terms(x * (1 - STABLE_MARGIN)) == substeps_terms(x) == substeps_terms(x * (1 + STABLE_MARGIN))


def active(x):
    """A valid point propagates when X_SKIP < x <= X_CAP."""
    return X_SKIP < float(x) <= X_CAP


def work_counts(p, n_steps, valid=None):
    """NMV_USEFUL = NMV_EXEC of every point on shaped16: 2 (n_steps - 1) nsub (kt + 1) series
    terms, 0 for a point that does not propagate (invalid, capped or skipped)."""
    x = x_shaped(p, n_steps)
    ok = np.ones(x.size, bool) if valid is None else np.asarray(valid, bool)
    out = np.zeros(x.size)
    for i in np.flatnonzero(ok):
        if active(x[i]):
            nsub, kt = substeps_terms(x[i])
            out[i] = 2 * (n_steps - 1) * nsub * (kt + 1)
    return out


def assert_stable(p, n_steps, what, valid=None):
    x = x_shaped(p, n_steps)
    ok = np.ones(x.size, bool) if valid is None else np.asarray(valid, bool)
    for i in np.flatnonzero(ok):
        if active(x[i]):
            assert stable(x[i]), f"{what}: point {i} at n_steps = {n_steps} has x = {x[i]!r} beside a change of nsub or kt"
        else:
            assert min(abs(x[i] / X_SKIP - 1), abs(x[i] / X_CAP - 1)) > STABLE_MARGIN, f"{what}: point {i}"


# ---- named edge batches -----------------------------------------------------------------

def ident_points(seed, n, first="nominal"):
    """n identical-atom points, the two classes alternating from ``first``."""
    other = "strong" if first == "nominal" else "nominal"
    kinds = [first if i % 2 == 0 else other for i in range(n)]
    return sym(random_shaped_points(np.random.default_rng(seed), n, kinds))


THREE_POINTS = ident_points(20261101, 13)          # test a: three waves and a ragged row
XI_LADDER = (np.exp(0.7j), 1.0, 0.6 * np.exp(2.1j), 1.7 * np.exp(-1j),
             -1.0, 0.0, np.exp(0.7j), np.exp(0.7j))
ZERO_RATE_ROW = 7


def xi_ladder(seed=20261102):
    """Two waves of four identical-atom strong points.  Wave 0: xi = e^{0.7i}, exactly 1 (a row
    whose frame never changes beside rows that rotate), 0.6 e^{2.1i} and 1.7 e^{-1i} (|xi| != 1:
    the amplitude scaling of pulse 2 and the max(1, |xi|) of the bound).  Wave 1: exactly -1,
    exactly 0 (no frame update, a free second pulse), e^{0.7i} with AREA_CORR = -1.3 (a
    negative amplitude: the frame already turns at the first segment) and e^{0.7i} with all
    eight rates zero (a unitary point)."""
    p = sym(random_shaped_points(np.random.default_rng(seed), 8, "strong"))
    for i, xi in enumerate(XI_LADDER):
        set_xi(p, i, xi)
    assert p[N.P["XI_RE"], 1] == 1.0 and p[N.P["XI_IM"], 1] == 0.0
    assert p[N.P["XI_RE"], 4] == -1.0 and p[N.P["XI_IM"], 4] == 0.0
    assert p[N.P["XI_RE"], 5] == 0.0 and p[N.P["XI_IM"], 5] == 0.0
    p[N.P["AREA_CORR"], 6] = -1.3
    for c in RATE_COLS:
        p[N.P[c], ZERO_RATE_ROW] = 0.0
    return p


SUBSTEP_RATIOS = (1.0, 30.0, 300.0, 1000.0)


def substep_mix(n_steps, seed=20261103):
    """One wave of identical-atom points with V / Omega = 1, 30, 300 and 1000, the rates those
    of strong points: at n_steps = 2 their segments take from 1 to about 100 sub-steps.
    Returns (points, expectations): x, nsub, kt and the work counter per point."""
    p = sym(random_shaped_points(np.random.default_rng(seed), 4, "strong"))
    p[N.P["V"]] = np.array(SUBSTEP_RATIOS) * p[N.P["OMEGA"]]
    x = x_shaped(p, n_steps)
    st = [substeps_terms(v) for v in x]
    return p, dict(x=x, nsub=np.array([s[0] for s in st]), kt=np.array([s[1] for s in st]),
                   nmv=work_counts(p, n_steps))


INVALID_ROWS = (1, 2, 5, 6)
INVALID_WAYS = (("OMEGA = 0", "TAU = -1", "a negative rate", "V = inf"),
                ("DELTA = NaN", "DELTA1 = -inf", "G0_A = G0_B = NaN", "OMEGA = NaN"))


def invalid_rows(variant, seed=20261104):
    """9 identical-atom strong points -- two full waves and a ragged row -- of which rows 1,
    2, 5 and 6 are invalid, in the four ways INVALID_WAYS[variant] names; the others are
    valid, their xi differ and row 4 has xi = 1 exactly, so both frame ballots fire in waves
    that hold invalid rows.  Returns (points, valid mask).  A NaN in G0_A and G0_B is the same
    column value on both atoms: the batch is one of identical atoms, though
    engine.symmetric_atoms (np.array_equal) does not say so."""
    p = sym(random_shaped_points(np.random.default_rng(seed), 9, "strong"))
    set_xi(p, 4, 1.0)
    r = INVALID_ROWS
    if variant == 0:
        p[N.P["OMEGA"], r[0]] = 0.0
        p[N.P["TAU"], r[1]] = -1.0
        p[N.P["GSC_A"], r[2]] = p[N.P["GSC_B"], r[2]] = -1.0
        p[N.P["V"], r[3]] = np.inf
    else:
        p[N.P["DELTA"], r[0]] = np.nan
        p[N.P["DELTA1"], r[1]] = -np.inf
        p[N.P["G0_A"], r[2]] = p[N.P["G0_B"], r[2]] = np.nan
        p[N.P["OMEGA"], r[3]] = np.nan
    valid = np.ones(9, bool)
    valid[list(r)] = False
    return p, valid


CAPPED_ROW, SKIPPED_ROW = 1, 2


def cap_and_skip(n_steps, seed=20261105):
    """One wave: a valid strong point, the same point with TAU such that the bound at zero
    amplitude -- below every segment's bound in either kernel -- gives x = 2 X_CAP (every
    segment is refused), the same point with TAU = 1e-30 (x <= X_SKIP: the identity, status
    0), and another valid strong point."""
    two = sym(random_shaped_points(np.random.default_rng(seed), 2, "strong"))
    p = two[:, [0, 0, 0, 1]].copy()
    p[N.P["TAU"], CAPPED_ROW] = 2.0 * X_CAP * n_steps / omega_shaped(p, amplitude=False)[CAPPED_ROW]
    p[N.P["TAU"], SKIPPED_ROW] = 1e-30
    return p


def many_blocks(seed=20261106):
    """37 identical-atom points, nominal and strong alternating: 10 blocks of one wave, more
    than the 8 XCDs that xcd_block deals blocks to, the last wave holding one live row."""
    return ident_points(seed, 37)


def unequal_points(seed=20261107):
    """5 strong points, every rate column different between the atoms."""
    return random_shaped_points(np.random.default_rng(seed), 5, "strong")


EDGE_STEPS = 6                   # n_steps of the xi ladder, the unequal atoms, the invalid rows, cap and skip
BLOCKS_STEPS = 4


def oracle_cases():
    """(name, points, point indices, shapes, step counts) of every oracle run
    test_gpu_shaped16_edges.py makes."""
    return [("three evaluations", THREE_POINTS, (0, 5, 12), SHAPES, (2, 3, 12)),
            ("xi ladder", xi_ladder(), tuple(range(8)), ("cosine",), (EDGE_STEPS,)),
            ("substep mix", substep_mix(2)[0], tuple(range(4)), ("cosine",), (2, 3)),
            ("unequal atoms", unequal_points(), tuple(range(5)), ("cosine",), (EDGE_STEPS,)),
            ("invalid rows", invalid_rows(0)[0], (0, 8), ("cosine",), (EDGE_STEPS,)),
            ("cap and skip", cap_and_skip(EDGE_STEPS), (0, 3), ("cosine",), (EDGE_STEPS,)),
            ("many blocks", many_blocks(), (0, 36), ("cosine",), (BLOCKS_STEPS,))]


def oracle_shapes(shapes):
    """The envelopes that differ for the oracle: gaussian, blackman and square all evaluate to
    the constant 1 (O.envelope), so the first of them stands for the three."""
    return [s for s in shapes if s == "cosine"] + [s for s in shapes if s != "cosine"][:1]


def oracle_refs(name):
    """{(point, oracle shape, n_steps): rho (4, 9, 9)} of one of oracle_cases()."""
    (p, idx, shapes, steps), = [c[1:] for c in oracle_cases() if c[0] == name]
    return {(i, s, ns): oracle(p, i, s, ns) for i in idx for s in oracle_shapes(shapes) for ns in steps}
