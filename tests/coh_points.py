"""Inputs for the coherence propagator kernel tests (coherence_prop_kernel, coherence4_prop_kernel
and their per-lane twins): the dim-3 twin of a dim-4 point, the two bounds the kernels scale
their builds by (the (0,-1), (-1,0), (-1,-1) sectors' and the (-1,+1) bank's, which leaves V
out), the batches that walk the kernels' branches, and the expm oracle's coherence rows.  No
GPU is touched here; test_coh_points_cpu.py checks these inputs, test_gpu_coh_build.py runs
them.  Points, ladders and the restated build come from dim4_points.py.
"""
import itertools

import numpy as np

import dim4_points as D4
from noisyquantumsimulator_amd import _native as N
from process_map4_util import process_map_dim, spec4_from_params
from process_map_util import rows_from_map, spec_from_params

DIMS = (3, 4)
GMJ = (N.P["GMJ_A"], N.P["GMJ_B"])
# B-atom rate factors of an "unequal" copy of an identical-atom point: every rate differs
UNEQUAL = (("G1", 1.37), ("G0", 0.61), ("GPHI", 1.21), ("GSC", 0.83), ("GMJ", 3.0))


def twin3(p):
    """The dim-3 twin: the same columns with GMJ_A = GMJ_B = 0."""
    q = p.copy()
    q[GMJ[0]] = q[GMJ[1]] = 0.0
    return q


def for_dim(p, dim):
    return p if dim == 4 else twin3(p)


def omega_main(p, protocol, **kw):
    """The bound of the (0,-1), (-1,0) and (-1,-1) sectors: the state kernel's."""
    return D4.omega4(p, protocol, **kw)


def omega_vfree(p, protocol, **kw):
    """The bound of the (-1,+1) bank: the same with the V column zeroed."""
    q = p.copy()
    q[N.P["V"]] = 0.0
    return D4.omega4(q, protocol, **kw)


BOUNDS = (omega_main, omega_vfree)


def unequal(p):
    """An identical-atom batch with every B rate scaled away from A's."""
    q = p.copy()
    for k, f in UNEQUAL:
        q[N.P[k + "_B"]] *= f
    return q


# ---- the oracle -------------------------------------------------------------------------

def identity_rows():
    """The rows of the identity map: 1.0 in the re slot of each input's own image."""
    return rows_from_map(np.eye(16, dtype=complex))[1][:, 0]


def oracle_rows(p, i, protocol, dim, n_steps=None, segs=None):
    """(NCOH,) expected coherence rows of point i of ``p`` (already for_dim): one expm of the
    full column-stacked Liouvillian (81 x 81 or 256 x 256) per segment."""
    mk = spec_from_params if dim == 3 else spec4_from_params
    spec = mk(p, i, protocol, n_steps=n_steps or 300)
    return rows_from_map(process_map_dim(spec, segs))[1][:, 0]


def oracle_batch(p, protocol, dim, n_steps=None, cols=None):
    """(NCOH, n) oracle rows of every column (or of ``cols``; the others are NaN)."""
    out = np.full((N.NCOH, p.shape[1]), np.nan)
    for i in (range(p.shape[1]) if cols is None else cols):
        out[:, i] = oracle_rows(p, i, protocol, dim, n_steps)
    return out


def swapped_rows(coh):
    """The rows of the atom-swapped point from the point's own: K0 <-> K1 row for row (the
    units (0,1), (2,3) of K0 are (0,2), (1,3) of K1 under 01 <-> 10), K2 (|00><11|) as it
    is, K3 (|01><10| -> |10><01|) conjugated."""
    out = np.array(coh, copy=True)
    k0, k1, k3 = N.C["K0"], N.C["K1"], N.C["K3"]
    out[k0:k0 + 8], out[k1:k1 + 8] = coh[k1:k1 + 8], coh[k0:k0 + 8]
    out[k3 + 1] = -coh[k3 + 1]
    return out


# ---- LP builds on both bounds -------------------------------------------------------------

def lp_build_x(p, i, bound):
    """The x of LP point i's builds on ``bound`` (D4.lp_builds for the main one)."""
    q = p[:, i:i + 1]
    Om, tau = q[N.P["OMEGA"]], q[N.P["TAU"]]
    w1 = 0.5 * np.sqrt(Om * Om)
    w2 = 0.5 * np.sqrt((Om * q[N.P["XI_RE"]]) ** 2 + (Om * q[N.P["XI_IM"]]) ** 2)
    xs = [float((bound(q, "lp_square", seg_w=w1) * tau)[0])]
    if w2[0] != w1[0]:
        xs.append(float((bound(q, "lp_square", seg_w=w2) * tau)[0]))
    return xs


def bank_depths(p, i):
    """(depth of the (-1,-1) bank, depth of the (-1,+1) bank) of LP point i's first build."""
    return tuple(D4.depth_terms4(lp_build_x(p, i, b)[0])[0] for b in BOUNDS)


def assert_margins(xs, what):
    D4.assert_depth_margin(xs, what)
    assert min(D4.term_margin(x) for x in xs) >= D4.DEPTH_MARGIN, what


def _strong(seed, n, protocol, kind="strong"):
    return D4.random_points4(np.random.default_rng(seed), n, protocol, kind)


# ---- the batches ------------------------------------------------------------------------

def equal_bank_points(seed=20261101):
    """Three unequal-atom strong LP points: V = 0 exactly (both banks have one bound),
    V / Omega = 0.3 (the banks equal or one level apart), V / Omega = 1000 (far apart)."""
    p = _strong(seed, 3, "lp_square")
    p[N.P["V"]] = np.array([0.0, 0.3, 1000.0]) * p[N.P["OMEGA"]]
    for i in range(3):
        for b in BOUNDS:
            assert_margins(lp_build_x(p, i, b), f"equal_bank_points {i}")
    return p


def mixed_wave(dim, seed=20261102):
    """Eight strong LP points, two waves: columns 0, 2, 5, 7 identical atoms, 1, 3, 4 unequal
    in every rate, 6 unequal in GMJ_B alone (dim 4) or in GPHI_B alone (its dim-3 twin)."""
    p = _strong(seed, 8, "lp_square")
    same = [0, 2, 5, 6, 7]
    p[:, same] = D4.sym(p[:, same].copy())
    if dim == 4:
        p[N.P["GMJ_B"], 6] *= 3.0
    else:
        p = twin3(p)
        p[N.P["GPHI_B"], 6] *= 3.0
    return p


MIXED_IDENTICAL = (0, 2, 5, 7)


def schedule_points(seed=20261103):
    """Twelve bang-bang points whose rows rebuild on different segments: D4.bb_schedule_points
    (1, 5, 4 and 1 builds), an NSEG = 8 point with eight distinct durations and an NSEG = 2
    point (both strong), each once with identical atoms (columns 0-5) and once unequal (6-11)."""
    more = D4.sym(_strong(seed, 2, "bangbang"))
    ot = more[N.P["OMEGA_TAU"], 0]
    rng = np.random.default_rng(seed + 1)
    more[N.P["NSEG"]] = [8, 2]
    more[N.P["SWT0"]:N.P["SWT0"] + 7, 0] = np.array([0.07, 0.19, 0.28, 0.43, 0.55, 0.72, 0.86]) * ot
    more[N.P["PHI0"]:N.P["PHI0"] + 8, 0] = rng.uniform(-np.pi, np.pi, 8)
    more[N.P["SWT0"]:N.P["SWT0"] + 7, 1] = 0.0
    more[N.P["SWT0"], 1] = 0.41 * more[N.P["OMEGA_TAU"], 1]
    same = np.concatenate([D4.bb_schedule_points(), more], axis=1)
    p = np.concatenate([same, unequal(same)], axis=1)
    for q in (p, twin3(p)):
        for c in range(p.shape[1]):
            assert_margins(D4.bb_builds(q, c), f"schedule point {c}")
    return p


SCHEDULE_BUILDS = (1, 5, 4, 1, 8, 2) * 2
SCHEDULE_LONG = (3, 9)        # D4.bb_schedule_points point 3 (one long dissipative segment), both copies


def nonunit_xi(seed=20261104):
    """(base, perturbed, special): eight LP points, strong and nominal alternating, identical
    atoms on the even columns.  In ``perturbed`` column 1 has xi scaled by 1.01 and column 4 by
    0.5 (phases off the axes: two builds each); column 6 has xi = i in both (one build)."""
    p = _strong(seed, 8, "lp_square", ["strong", "nominal"] * 4)
    even = [0, 2, 4, 6]
    p[:, even] = D4.sym(p[:, even].copy())
    for c, ph in ((1, 0.7), (4, 2.3)):
        p[N.P["XI_RE"], c], p[N.P["XI_IM"], c] = np.cos(ph), np.sin(ph)
    p[N.P["XI_RE"], 6], p[N.P["XI_IM"], 6] = 0.0, 1.0
    q = p.copy()
    for c, f in ((1, 1.01), (4, 0.5)):
        q[N.P["XI_RE"], c] *= f
        q[N.P["XI_IM"], c] *= f
    for c in (1, 4, 6):
        for b in BOUNDS:
            assert_margins(lp_build_x(q, c, b), f"nonunit_xi column {c}")
    return p, q, (1, 4, 6)


JP_STEPS = (1, 2, 3, 30)


def jp_points(seed=20261105):
    """Three strong unequal-atom smooth-JP points, run at every n_steps of JP_STEPS."""
    return _strong(seed, 3, "smooth_jp")


def launch_points(protocol, seed=20261106):
    """37 points, strong and nominal alternating: 10 blocks, the last with one live row.
    Every third column has identical atoms."""
    p = _strong(seed + (protocol != "lp_square"), 37, protocol, (["strong", "nominal"] * 19)[:37])
    same = list(range(0, 37, 3))
    p[:, same] = D4.sym(p[:, same].copy())
    return p


def five_valid(protocol, seed=20261107):
    """Five valid points of mixed depth; columns 0 and 2 have identical atoms."""
    p = _strong(seed + (protocol != "lp_square"), 5, protocol, ["nominal", "strong", "nominal", "strong", "strong"])
    p[:, [0, 2]] = D4.sym(p[:, [0, 2]].copy())
    return p


# ---- rows the kernels must refuse -------------------------------------------------------------

def _nan_column(p, c):
    p[:, c] = np.nan
    for k in D4.RATES4:                     # the rate columns stay equal numbers
        p[N.P[k + "_A"], c] = p[N.P[k + "_B"], c] = 0.0


def _set(name, value):
    def edit(p, c):
        p[N.P[name], c] = value
    return edit


def _cap(p, c):
    p[N.P["TAU"], c] = 3e6 / D4.omega4(p[:, c:c + 1], "lp_square")[0]


def invalid_columns(protocol, dim):
    """{name: (edit(p, column), expected status bit)} for ``protocol`` ("lp_square" or
    "bangbang") and ``dim``.  Every edit but "cap" must give BAD_INPUT; "cap" (LP) sets
    x = 3e6 > X_CAP on the main bound and must give STEP_CAP alone."""
    bad = N.STATUS_BAD_INPUT

    def nan_rates_too(p, c):                # dim 3 has no GMJ columns to spoil: the entry point wants them 0
        p[:, c] = np.nan
        if dim == 3:
            p[list(GMJ), c] = 0.0
    out = {"nan": (_nan_column, bad), "nan_rates_too": (nan_rates_too, bad),
           "omega_zero": (_set("OMEGA", 0.0), bad), "negative_rate": (_set("G0_B", -1.0), bad)}
    if protocol == "bangbang":
        out["nseg_0"] = (_set("NSEG", 0.0), bad)
        out["nseg_9"] = (_set("NSEG", 9.0), bad)
    else:
        out["tau_inf"] = (_set("TAU", np.inf), bad)
        out["cap"] = (_cap, N.STATUS_STEP_CAP)
    if dim == 4:
        out["gmj_nan"] = (_set("GMJ_B", np.nan), bad)
    return out


def refused_batch(protocol, dim):
    """(clean, edited, [(column, name, bit)]): one wave per (edit, row position) -- wave w holds
    the valid points w, w + 1, w + 2, w + 3 (mod 5), and in ``edited`` the edit at row ``pos``."""
    five = for_dim(five_valid(protocol), dim)
    edits = invalid_columns(protocol, dim)
    waves = list(itertools.product(edits, range(4)))
    clean = np.concatenate([five[:, [(w + r) % 5 for r in range(4)]] for w in range(len(waves))], axis=1)
    edited, marks = clean.copy(), []
    for w, (name, pos) in enumerate(waves):
        edits[name][0](edited, 4 * w + pos)
        marks.append((4 * w + pos, name, edits[name][1]))
    return clean, edited, marks


# ---- four kinds of row in one wave ----------------------------------------------------------

def four_kinds():
    """(rows (NPARAM, 4), batch (NPARAM, 96), order): an identity-build row (the x ladder's
    last point), an s = 0 row with a full-length series (x = 0.45 on the main bound: degree
    13), the deepest nominal row (V / Omega = 1000) and a NaN row; ``batch`` holds the 24
    orders of the four, one wave each, and ``order[w]`` is wave w's permutation."""
    ident = D4.x_ladder4()[:, -1:]
    full = D4.lp_strong_base()
    full[N.P["TAU"]] = 0.45 / D4.omega4(full, "lp_square")
    deep = _strong(20261108, 1, "lp_square", "nominal")
    deep[N.P["V"]] = 1000.0 * deep[N.P["OMEGA"]]
    rows = np.concatenate([ident, full, deep, np.full((N.NPARAM, 1), np.nan)], axis=1)
    order = list(itertools.permutations(range(4)))
    return rows, np.concatenate([rows[:, list(o)] for o in order], axis=1), order
