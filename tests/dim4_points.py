"""Inputs for the dim-4 Lindblad kernel tests (lindblad4_prop_kernel, lindblad4_cheb_kernel):
random parameter points with the mJ columns, the kernels' spectral bound and squaring depth
restated on the host, the ladders and bang-bang schedules that walk their build paths, and
the expm oracle for an explicit segment list.  No GPU is touched here;
test_dim4_points_cpu.py checks these inputs, test_gpu_dim4_build.py runs them.

Two classes of point.  "nominal" is test_gpu_parity._random_points with mJ rates: V / Omega
from 10 to 1000, where the |11> triangle's r+- r+- coordinates stay small.  "strong" has
V / Omega from 0.3 to 30 and rates that are percents of Omega, so every one of the 36 sector
coordinates of every input is large against the 1e-10 absolute tolerance.
"""
import math

import numpy as np
import scipy.linalg as sla

from bench import _cheb_terms_small
from noisyquantumsimulator_amd import _native as N
from oracle import lindblad_oracle as O
from test_gpu_parity import _random_points

RATES = ("G1", "G0", "GPHI", "GSC")
RATES4 = RATES + ("GMJ",)
X_BASE = 0.5            # ryd_coh_prop.inc CP_XS: the series argument the squarings start from
X_SKIP = 1e-20          # ryd_engine.hip: at or below this a build is the identity
X_CAP = 2.0e6           # ryd_engine.hip: above this a segment is refused (STEP_CAP)
DEPTH_MARGIN = 1e-6     # relative distance every ladder keeps from a depth boundary
# upper limits of the "strong" rates, as fractions of Omega
STRONG_RATES = (("G1", 0.01), ("G0", 0.02), ("GPHI", 0.03), ("GSC", 0.02), ("GMJ", 0.05))
# bench._TH_SMALL below X_BASE / 2: the term-count thresholds a build without squarings can meet
TH_BELOW = (1e-17, 4.4721359549995795e-09, 3.914867641168864e-06, 0.00012446659545769568,
            0.0010371372893366482, 0.004394290351366487, 0.0125993232817844, 0.02822864716464555,
            0.05356271212458357, 0.09036001686117834, 0.1398168813097236, 0.20262580209060138)


def random_points4(rng, n, protocol, kind="nominal"):
    """(NPARAM, n) dim-4 points, every rate column different between the two atoms.  ``kind``
    is "nominal", "strong", or a sequence of the two, one per point."""
    p = _random_points(rng, n, protocol)
    kinds = [kind] * n if isinstance(kind, str) else list(kind)
    assert len(kinds) == n and set(kinds) <= {"nominal", "strong"}
    strong = np.array([k == "strong" for k in kinds])
    Om = p[N.P["OMEGA"]]
    gmj = rng.uniform(0, 2e5, (2, n))
    ratio = 10 ** rng.uniform(-0.5, 1.5, n)
    d1 = rng.uniform(0, 0.3, n)
    frac = {(k, a): rng.uniform(0, hi, n) for k, hi in STRONG_RATES for a in "AB"}
    p[N.P["GMJ_A"]], p[N.P["GMJ_B"]] = gmj
    p[N.P["V"], strong] = (ratio * Om)[strong]
    p[N.P["DELTA1"], strong] = (d1 * Om)[strong]
    for (k, a), f in frac.items():
        p[N.P[f"{k}_{a}"], strong] = (f * Om)[strong]
    return p


def sym(p):
    """Identical atoms: the A columns copied to B, GMJ included."""
    for k in RATES4:
        p[N.P[k + "_B"]] = p[N.P[k + "_A"]]
    return p


def swap_atoms(p):
    """The same points with atoms A and B exchanged."""
    q = p.copy()
    for k in RATES4:
        q[N.P[k + "_A"]], q[N.P[k + "_B"]] = p[N.P[k + "_B"]], p[N.P[k + "_A"]]
    return q


def swap_rho(rho):
    """rho (..., 4 inputs, 16, 16) of the atom-swapped problem: inputs 01 <-> 10 exchanged and
    both two-atom indices (4 a + b) -> (4 b + a)."""
    r = np.asarray(rho)[..., [0, 2, 1, 3], :, :]
    lead = r.shape[:-2]
    return r.reshape(lead + (4, 4, 4, 4)).swapaxes(-4, -3).swapaxes(-2, -1).reshape(lead + (16, 16))


# ---- the kernels' spectral bound and build, restated ----------------------------------

def omega4(p, protocol, seg_w=None, seg_dl=None):
    """The dim-4 kernels' bound per point: h_bounds' Gershgorin span over the energies
    {0, delta1, -Delta} with half-width ``seg_w`` = |Omega_seg| / 2 per excitable atom, plus
    rsum = the four rate columns of both atoms + 2 (GMJ_A + GMJ_B).  ``seg_w`` defaults to
    |OMEGA| / 2, ``seg_dl`` to the DELTA column (0 for bang-bang, which has no detuning)."""
    Om, V, d1 = p[N.P["OMEGA"]], p[N.P["V"]], p[N.P["DELTA1"]]
    w = 0.5 * np.abs(Om) if seg_w is None else seg_w
    if seg_dl is None:
        seg_dl = p[N.P["DELTA"]] if protocol != "bangbang" else 0.0 * Om
    e = [np.zeros_like(Om), d1, -seg_dl]
    emin, emax = np.full_like(Om, np.inf), np.full_like(Om, -np.inf)
    for a1 in range(3):
        for a2 in range(a1, 3):
            en = e[a1] + e[a2] + (V if a1 == a2 == 2 else 0.0)
            r = w * ((a1 > 0) + (a2 > 0))
            emin, emax = np.minimum(emin, en - r), np.maximum(emax, en + r)
    rsum = 2.0 * (np.abs(p[N.P["GMJ_A"]]) + np.abs(p[N.P["GMJ_B"]]))
    rsum = rsum + sum(np.abs(p[N.P[k + "_A"]]) + np.abs(p[N.P[k + "_B"]]) for k in RATES)
    return emax - emin + rsum


def depth_terms4(x):
    """(s, xs, kt, identity) of one build at argument x = omega dt: s = ceil(log2(x / X_BASE))
    squarings above X_BASE, the series argument xs = x / 2^s, its degree kt (the series has
    kt + 1 terms), and whether the build is the identity (xs <= X_SKIP: kt = -1)."""
    x = float(x)
    s = int(math.ceil(math.log2(x / X_BASE))) if x > X_BASE else 0
    xs = math.ldexp(x, -s)
    if not xs > X_SKIP:
        return s, xs, -1, True
    return s, xs, _cheb_terms_small(xs), False


def depth_margin(x):
    """Relative distance of x from the nearest depth boundary X_BASE 2^k, k >= 0."""
    x = float(x)
    if not x > 0:
        return 1.0
    k = max(0, int(round(math.log2(x / X_BASE))))
    return abs(x / math.ldexp(X_BASE, k) - 1.0)


def assert_depth_margin(x, what):
    m = min(depth_margin(v) for v in np.atleast_1d(x))
    assert m >= DEPTH_MARGIN, f"{what}: an x lies {m:.1e} (relative) from a depth boundary"


def term_margin(x):
    """Relative distance of the series argument of a build at x from the nearest term-count
    threshold (1.0 for the identity build)."""
    _, xs, _, ident = depth_terms4(x)
    return 1.0 if ident else min(abs(xs / (2 * t) - 1.0) for t in TH_BELOW)


# ---- LP ladders -------------------------------------------------------------------------

def lp_strong_base(seed=20261020):
    """One identical-atom strong LP point with xi = i: the base of both ladders.  The build
    key is the rounded |Omega xi| = sqrt((Omega xi_re)^2 + (Omega xi_im)^2), which for a
    general xi on the unit circle differs from |Omega| by an ulp in about one point of five
    (a second, harmless build); with xi = i it is |Omega| exactly, so the ladders can assert
    the counters of a single build.  General phases are the business of the other tests."""
    p = sym(random_points4(np.random.default_rng(seed), 1, "lp_square", "strong"))
    p[N.P["XI_RE"]], p[N.P["XI_IM"]] = 0.0, 1.0
    assert len(lp_builds(p, 0)) == 1
    return p


def tau_ladder4(n=33):
    """One strong point, the pulse duration scaled geometrically over a factor of 4: the
    depth changes twice along the ladder."""
    f = np.geomspace(1.0, 4.0, n)
    p = np.repeat(lp_strong_base(), n, axis=1)
    p[N.P["TAU"]] *= f
    assert_depth_margin(omega4(p, "lp_square") * p[N.P["TAU"]], "tau ladder")
    return p


def x_ladder4():
    """48 LP points whose x = omega tau falls from about 1 to below X_SKIP: both sides (a
    relative 1e-9) of each of the 12 term-count thresholds below X_BASE / 2, and a geometric
    fill down to 5e-21, the identity."""
    th = np.array(TH_BELOW)
    x = np.concatenate([2 * th * (1 + 1e-9), 2 * th * (1 - 1e-9), np.geomspace(0.97, 5e-21, 24)])
    x = np.sort(x)[::-1]
    assert x.size == 48 and x[0] > X_BASE and x[-1] < X_SKIP
    assert_depth_margin(x, "x ladder")
    p = np.repeat(lp_strong_base(), x.size, axis=1)
    p[N.P["TAU"]] = x / omega4(p, "lp_square")
    return p


def lp_builds(p, i):
    """The x of every propagator build that LP point i requires: pulse 1, and pulse 2 when
    |Omega xi| or the duration differs from pulse 1's (the laser phase alone needs none)."""
    q = p[:, i:i + 1]
    Om, tau = q[N.P["OMEGA"]], q[N.P["TAU"]]
    w1 = 0.5 * np.sqrt(Om * Om)
    w2 = 0.5 * np.sqrt((Om * q[N.P["XI_RE"]]) ** 2 + (Om * q[N.P["XI_IM"]]) ** 2)
    xs = [float((omega4(q, "lp_square", seg_w=w1) * tau)[0])]
    if w2[0] != w1[0]:
        xs.append(float((omega4(q, "lp_square", seg_w=w2) * tau)[0]))
    return xs


# ---- bang-bang schedules ----------------------------------------------------------------

def _trim(x, bits):
    """x rounded to ``bits`` significant bits."""
    m, e = math.frexp(x)
    return math.ldexp(round(m * 2 ** bits), e - bits)


def bb_segments(p, i):
    """[(w, dt)] of bang-bang point i's NSEG segments, in the kernels' arithmetic: the bounds
    are switching times / Omega, dt their difference (below 1e-18: a skipped segment, 0), and
    w = |Omega e^{i phi}| / 2 from the segment's rounded (Omega cos phi, Omega sin phi)."""
    Om, nseg = p[N.P["OMEGA"], i], int(p[N.P["NSEG"], i])
    b = [0.0] + [p[N.P["SWT0"] + k, i] / Om for k in range(nseg - 1)] + [p[N.P["OMEGA_TAU"], i] / Om]
    out = []
    for s in range(nseg):
        dt = b[s + 1] - b[s]
        ph = p[N.P["PHI0"] + s, i]
        out.append((0.5 * math.sqrt((Om * math.cos(ph)) ** 2 + (Om * math.sin(ph)) ** 2),
                    0.0 if dt < 1e-18 else dt))
    return out


def bb_builds(p, i):
    """The x of every build that bang-bang point i's own schedule requires: a segment of
    positive length whose (|Omega|, dt) differs from the previous such segment's."""
    q = p[:, i:i + 1]
    xs, last = [], None
    for w, dt in bb_segments(p, i):
        if dt > 0.0 and (w, dt) != last:
            xs.append(float(omega4(q, "bangbang", seg_w=np.array([w]))[0] * dt))
            last = (w, dt)
    return xs


def bb_schedule_points(seed=20261021):
    """Four identical-atom bang-bang points whose rows rebuild on different segments:
      0 (strong)   five equal durations, phases +-0.9: one build serves all five segments;
      1 (nominal)  five distinct durations: five builds;
      2 (strong)   a first segment of zero length, then four distinct durations: four builds;
      3 (nominal)  NSEG = 1: one build, and four segments that do not exist.
    Point 0's Omega is trimmed to 20 significant bits and its switching times are k d Omega
    with a 20-bit d, so the products, the quotients k d and their differences d are exact in
    double precision and the five durations are the same number; cos(-x) = cos(x) and
    sin(-x) = -sin(x) make the five |Omega e^{i phi}| the same number too."""
    rng = np.random.default_rng(seed)
    p = sym(random_points4(rng, 4, "bangbang", ("strong", "nominal", "strong", "nominal")))
    ot = p[N.P["OMEGA_TAU"], 0]
    sw = slice(N.P["SWT0"], N.P["SWT0"] + 4)
    ph = slice(N.P["PHI0"], N.P["PHI0"] + 5)
    Om0 = _trim(p[N.P["OMEGA"], 0], 20)
    d = _trim(ot / (5 * Om0), 20)
    p[N.P["OMEGA"], 0] = Om0
    p[sw, 0] = [k * d * Om0 for k in range(1, 5)]
    p[N.P["OMEGA_TAU"], 0] = 5 * d * Om0
    p[ph, 0] = [0.9, -0.9, 0.9, -0.9, 0.9]
    p[sw, 1] = np.array([0.13, 0.37, 0.52, 0.81]) * ot
    p[sw, 2] = np.array([0.0, 0.21, 0.48, 0.83]) * ot
    p[N.P["NSEG"], 3] = 1
    for i in range(4):
        assert_depth_margin(bb_builds(p, i), f"bang-bang schedule point {i}")
        assert min(term_margin(v) for v in bb_builds(p, i)) >= DEPTH_MARGIN
    return p


# ---- the oracle -------------------------------------------------------------------------

def run_segments(spec, segs=None):
    """rho (4 inputs in O.LABELS order, D, D) after the piecewise-constant schedule ``segs``
    (O.segments(spec) unless given; lp_shaped_segments for a shaped pulse with few steps):
    one expm of the full column-stacked Liouvillian per segment, applied to the four basis
    inputs together -- O.run_point's propagators, each computed once."""
    D = spec.dim ** 2
    if segs is None:
        segs = O.segments(spec)
    kets = O.initial_kets(spec.dim)
    v = np.stack([O.vec(np.outer(kets[lab], kets[lab].conj())) for lab in O.LABELS], axis=1)
    for H, t, _ in segs:
        v = sla.expm(O.liouvillian(H, spec.c_ops) * float(t[-1] - t[0])) @ v
    return np.stack([O.unvec(v[:, k], D) for k in range(4)])
