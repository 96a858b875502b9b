"""The control-Jacobian oracle (tests/sched_ket_ctl_points.py) against finite differences of the
ket chain it extends, and the four-field fidelity gradient against finite differences of
``noise_models.gate_fidelity``.  No device.

Finite-difference bounds.  Fields are in the table's units, where |H| / Omega <= W with
W = 2.2 max(1, V / Omega) (the widest diagonal is V + 2 |Delta|; V / Omega <= 1000 in these
batches).  An overlap of the chain (|a| <= 1) carries rounding d of about 9 eps per 9 x 9
matrix-vector product, d = 20 x 1e-15 = 2e-14 for at most 20 segments; it does not cancel between
neighbouring tables.  A central difference errs by at most h^2 W^3 / 6 + d / h, the second-order
one-sided one at x = 0, (-3 f(0) + 4 f(h) - f(2 h)) / (2 h), by h^2 W^3 / 3 + 4 d / h.  The step
h = 5e-5 / W nearly minimises the latter: 8.4e-10 W + 1.6e-9 W.  So the bound is 2.5e-9 W for
each point, at most 5.5e-6, for derivatives of size 0.1 .. 10.
"""
import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import pulse_schedules as PS
from tests import sched_ket_ctl_points as CP
from tests import sched_ket_points as KP

SC = N.SC
FD_STEP, FD_TOL = 5e-5, 2.5e-9                     # both in units of 1 / W and W: see above


def _width(p, i):
    return 2.2 * max(1.0, p[N.P["V"], i] / p[N.P["OMEGA"], i])


def _overlaps(p, tab):
    r = KP.chain(p, tab[None])
    return np.array([r["a01"][0], r["a11"][0]])


def test_hamiltonian_is_linear_in_the_table():
    b = CP.batch("zero_x")
    p, s = b["params"], b["sched"]
    for i in range(p.shape[1]):
        Om, V, d1 = p[N.P["OMEGA"], i], p[N.P["V"], i], p[N.P["DELTA1"], i]
        for x, a, ph, d in s[i].T[:4]:
            H0, Ha, Hd = CP.hamiltonian_parts(p, i, ph)
            H = CP.O.two_atom_hamiltonian(a * Om * np.exp(1j * ph), d * Om, V, 3, delta_zeeman=d1)
            assert np.abs(H - (H0 + a * Ha + d * Hd)).max() <= 1e-15 * np.abs(H).max()


def test_new_batches_hold_what_they_claim():
    b = CP.batch("degenerate")
    p, s = b["params"], b["sched"]
    assert s.shape == (5, 4, 17) and p.shape[1] == 5
    Om, d1 = p[N.P["OMEGA"]], p[N.P["DELTA1"]]
    for seg in (1, 5):                              # a = 0 and d1 + Delta = 0 = 2 d1 - (d1 - Delta)
        assert np.all(s[:, SC["AMP"], seg] == 0.0)
        np.testing.assert_allclose(d1 + s[:, SC["DELTA"], seg] * Om, 0.0, atol=1e-9 * Om.max())
    assert np.all(s[:, SC["AMP"], 8] == 1e-9)
    arg = 0.5 * s[:, SC["AMP"], 10:14] * s[:, SC["X"], 10:14]      # gap dt / 2 of the 2 x 2 block
    assert np.all(arg[:, :2] < CP.SINC_SWITCH) and np.all(arg[:, 2:] > CP.SINC_SWITCH)
    np.testing.assert_allclose(arg / CP.SINC_SWITCH, [[0.5, 0.999, 1.001, 2.0]] * 5, rtol=1e-12)
    z = CP.batch("zero_x")["sched"]
    assert z.shape == (5, 4, 17)
    assert [np.flatnonzero(z[i, SC["X"]] == 0.0).tolist() for i in range(5)] == \
        [[0], [16], [6, 7], [15], [0, 6, 7, 15, 16]]
    ph = z[:, SC["PHASE"]]
    assert np.all(ph[:, 1:] != ph[:, :-1])          # every zero segment has a phase of its own
    PS.validate_schedule(s, 5)
    PS.validate_schedule(z, 5)


def test_reference_extends_the_phase_oracle():
    for name in CP.NEW:
        ref, b = CP.reference(name), CP.batch(name)
        old = KP.chain(b["params"], b["sched"])
        np.testing.assert_array_equal(ref["C"][:, SC["PHASE"]], old["J"])
        np.testing.assert_array_equal(ref["kets"], old["kets"])
        zero = b["sched"][:, SC["X"]] == 0.0
        for f in ("AMP", "PHASE", "DELTA"):
            assert np.all(ref["C"][:, SC[f]][np.broadcast_to(zero[:, None], (5, 2, 17))] == 0.0)
        if name == "zero_x":                        # the one-sided duration derivative is not zero
            assert np.all(np.abs(ref["C"][:, SC["X"]]).max(axis=1)[zero] > 1e-3)


@pytest.mark.parametrize("name", CP.NEW + ("random",))
def test_reference_against_differences_of_the_chain(name):
    b, ref = CP.batch(name), CP.reference(name)
    p, s = b["params"], b["sched"]
    n, ns = p.shape[1], s.shape[-1]
    rng = np.random.default_rng(1)
    worst = 0.0
    for i in range(min(n, 5)):
        pi = p[:, i:i + 1]
        h = FD_STEP / _width(p, i)
        zeros = np.flatnonzero(s[i, SC["X"]] == 0.0).tolist()
        special = [sg for sg in (1, 8, 10, 11, 12, 13) if sg < ns] if name == "degenerate" else []
        segs = sorted(set(zeros) | set(rng.choice(ns, 4, replace=False).tolist()) | set(special))
        for sg in segs:
            for f in ("X", "AMP", "DELTA"):
                t = s[i].copy()
                v0 = t[SC[f], sg]
                want = ref["C"][i, SC[f], :, sg]
                if f != "X" and s[i, SC["X"], sg] == 0.0:
                    assert np.all(want == 0.0)        # a zero-duration segment: zeros by definition
                    continue
                if f == "X" and v0 == 0.0:            # at the bound x = 0: second-order one-sided
                    f0 = _overlaps(pi, t)
                    t[SC[f], sg] = h
                    f1 = _overlaps(pi, t)
                    t[SC[f], sg] = 2 * h
                    f2 = _overlaps(pi, t)
                    fd = (-3 * f0 + 4 * f1 - f2) / (2 * h)
                else:                                 # (the oracle's H is linear in a, also through a = 0)
                    t[SC[f], sg] = v0 + h
                    fp = _overlaps(pi, t)
                    t[SC[f], sg] = v0 - h
                    fm = _overlaps(pi, t)
                    fd = (fp - fm) / (2 * h)
                worst = max(worst, float(np.abs(fd - want).max()) / (FD_TOL * _width(p, i)))
    print(f"{name}: oracle against differences of the chain, max error / bound = {worst:.3e}")
    assert worst < 1.0


@pytest.mark.parametrize("which", ("avg_gate", "process"))
def test_fidelity_gradient_in_four_fields(which):
    """dF of ``gate_fidelity_and_gradient`` from the oracle's (n, 4, 2, n_seg) Jacobian against
    central differences of ``noise_models.gate_fidelity`` on the chain's kets.  F is a quadratic
    form of the overlaps with |dF/da| <= 1, so the bound of the module docstring carries over."""
    b, ref = CP.batch("degenerate"), CP.reference("degenerate")
    p, s = b["params"], b["sched"]
    F, dF = PS.gate_fidelity_and_gradient(ref["a01"], ref["a11"], ref["C"], which)
    assert F.shape == (5,) and dF.shape == (5, 4, 17)
    Fp, dFp = PS.gate_fidelity_and_gradient(ref["a01"], ref["a11"], ref["C"][:, SC["PHASE"]], which)
    np.testing.assert_array_equal(F, Fp)
    np.testing.assert_array_equal(dF[:, SC["PHASE"]], dFp)
    k = 0 if which == "process" else 1
    np.testing.assert_allclose(F, NM.gate_fidelity(NM.ket_maps(ref["kets"]))[k], atol=1e-13, rtol=0)
    worst = 0.0
    for i in range(5):
        pi = p[:, i:i + 1]
        h = FD_STEP / _width(p, i)
        for f in ("X", "AMP", "PHASE", "DELTA"):
            for sg in (0, 3, 9, 12, 16):
                t = s[i].copy()
                v0 = t[SC[f], sg]
                t[SC[f], sg] = v0 + h
                fp = NM.gate_fidelity(NM.ket_maps(KP.chain(pi, t[None])["kets"]))[k][0]
                t[SC[f], sg] = v0 - h
                fm = NM.gate_fidelity(NM.ket_maps(KP.chain(pi, t[None])["kets"]))[k][0]
                worst = max(worst, abs((fp - fm) / (2 * h) - dF[i, SC[f], sg]) / (FD_TOL * _width(p, i)))
    print(f"{which}: four-field gradient against differences, max error / bound = {worst:.3e}")
    assert worst < 1.0
