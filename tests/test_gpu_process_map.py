"""Process maps on the GPU (ryd_run_coherences + the diagonal sector) against the
oracle's full-Liouvillian definition.  Tolerance 1e-10 on every
map element, as the state parity tests.  The oracle comparisons run on both coherence
paths: coherence_prop_kernel (the default) and coherence_cheb_kernel (RYD_COH_PROP=0)."""
import warnings

import numpy as np
import pytest

import oracle_evaluator as OE
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import configurations as CF
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import physics as PH
from oracle import lindblad_oracle as O
from process_map4_util import lp_shaped_segments, process_map_dim
from process_map_util import PATHS, coh_path, spec_from_params
from test_gpu_parity import _random_points

pytestmark = pytest.mark.gpu
TOL = 1e-10
QI = O.QUBIT_INDEX


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


def _both_paths_match_oracle(eng, p, protocol, n_steps, what):
    """Every point's map against the oracle's (computed once) on both coherence paths."""
    n = p.shape[1]
    ref = [O.process_map(spec_from_params(p, i, protocol, n_steps=n_steps or 300)) for i in range(n)]
    for path in PATHS:
        with coh_path(path):
            pm = NM.gate_process_maps(p, protocol, n_steps=n_steps, engine=eng, with_kraus=True)
        assert np.all(pm.status == 0)
        for i in range(n):
            print(f"{protocol} {what} RYD_COH_PROP={path} point {i}: max|dS| = {np.abs(pm.S[i] - ref[i]).max():.3e}")
        for i in range(n):
            np.testing.assert_allclose(pm.S[i], ref[i], atol=TOL, rtol=0, err_msg=f"{protocol}/{path}/{i}")
        assert np.all(pm.kraus_rank > 1)                  # noisy: not a unitary channel


@pytest.mark.parametrize("protocol,n_steps", [("lp_square", None), ("smooth_jp", 30), ("bangbang", None)])
def test_process_map_matches_oracle(eng, protocol, n_steps):
    rng = np.random.default_rng(99)
    p = _random_points(rng, 5, protocol)                 # asymmetric atoms, random rates
    _both_paths_match_oracle(eng, p, protocol, n_steps, "unequal atoms")


@pytest.mark.parametrize("protocol,n_steps", [("lp_square", None), ("smooth_jp", 30), ("bangbang", None)])
def test_process_map_identical_atoms_matches_oracle(eng, protocol, n_steps):
    """B rates = A rates: coherence_prop_kernel mirrors the (-1, 0) sector from (0, -1) instead
    of building it -- the path of every reference configuration and of the bench."""
    rng = np.random.default_rng(101)
    p = _random_points(rng, 5, protocol)
    for k in ("G1", "G0", "GPHI", "GSC"):
        p[N.P[k + "_B"]] = p[N.P[k + "_A"]]
    assert E.symmetric_atoms(p)
    _both_paths_match_oracle(eng, p, protocol, n_steps, "identical atoms")


def test_shaped_lp_process_map_matches_oracle(eng):
    """A cosine envelope: a new amplitude every segment, so coherence_cheb_kernel whatever
    RYD_COH_PROP says.  3 derived points (temperatures and laser power spread as in the dim-4
    twin of this test), 2 x 11 segments."""
    n = 3
    exc = CF.TwoPhotonExcitationConfig(
        laser_1=CF.LaserParameters(power=50e-6, waist=50e-6, polarization="pi", polarization_purity=0.95),
        laser_2=CF.LaserParameters(power=0.3, waist=50e-6, polarization="sigma+", polarization_purity=0.95))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b = PH.derive_batch(CF.LPSimulationInputs(excitation=exc, pulse_shape="cosine"), n, hilbert_space_dim=3,
                            species="Rb87", n_rydberg=70, tweezer_power=0.020, tweezer_waist=0.8e-6,
                            spacing_factor=2.8, B_field=1e-4, NA=0.5, temperature=np.linspace(1e-6, 3e-5, n),
                            overrides=dict(laser_2_power=np.geomspace(0.03, 3.0, n)))
    assert E.protocol_key(b) == "lp_shaped"
    pm = NM.gate_process_maps(E.pack_params(b), "lp_shaped", n_steps=12, shape="cosine", engine=eng)
    assert np.all(pm.status == 0)
    for i in range(n):
        spec = OE.point_spec(b, i)
        assert spec.protocol == "lp_shaped" and spec.pulse_shape == "cosine" and spec.dim == 3
        ref = process_map_dim(spec, lp_shaped_segments(spec, 12))
        print(f"shaped point {i}: max|dS| = {np.abs(pm.S[i] - ref).max():.3e}")
        np.testing.assert_allclose(pm.S[i], ref, atol=TOL, rtol=0)


def test_noise_free_map_is_the_ket_unitary(eng):
    """Zero rates: the coherence kernels and the ket kernel are independent routes to
    the same qubit-block unitary, S = U_q (x) conj(U_q)."""
    rng = np.random.default_rng(5)
    p = _random_points(rng, 40, "lp_square")
    for k in ("G1", "G0", "GPHI", "GSC"):
        p[N.P[k + "_A"]] = p[N.P[k + "_B"]] = 0.0
    pm = NM.gate_process_maps(p, "lp_square", engine=eng, with_kraus=True)
    psi = eng.run(p, "lp_square", "ket").kets()           # (n, 4 inputs, 9)
    Uq = psi[:, :, QI].transpose(0, 2, 1)                 # U_q[c, a] = <c|psi_a>
    S_ket = np.einsum("nca,ndb->ncdab", Uq, np.conj(Uq)).reshape(-1, 16, 16)
    np.testing.assert_allclose(pm.S, S_ket, atol=TOL, rtol=0)
    assert np.all(pm.kraus_rank == 1)


def test_large_batch_channel_properties(eng):
    rng = np.random.default_rng(8)
    n = 2000
    p = _random_points(rng, n, "lp_square")
    pm = NM.gate_process_maps(p, "lp_square", engine=eng)
    assert np.all(pm.status == 0)
    w = np.linalg.eigvalsh(pm.choi)
    assert w.min() > -1e-10                               # completely positive
    # trace non-increasing: Tr_out J <= I_in
    T = np.einsum("nacbc->nab", pm.choi.reshape(n, 4, 4, 4, 4))
    assert np.linalg.eigvalsh(np.eye(4) - T).min() > -1e-10
    assert np.all((pm.process_fidelity <= 1 + 1e-12) & (pm.leakage >= -1e-12))
    np.testing.assert_allclose(pm.pauli_probs.sum(axis=1), 1 - pm.leakage, atol=1e-11)
    for i in (0, n - 1):
        ref = O.process_map(spec_from_params(p, i, "lp_square"))
        np.testing.assert_allclose(pm.S[i], ref, atol=TOL, rtol=0)


def test_coherence_rows_are_independent_of_their_wave(eng):
    """4 points per wave, each row (and each quad bank) with its own squaring depth: a
    ragged batch gives every point the bits it gets alone."""
    rng = np.random.default_rng(17)
    p = _random_points(rng, 7, "lp_square")
    coh, st = eng.run_coherences(p, "lp_square")
    assert np.all(st == 0)
    for i in (0, 3, 6):
        c1, s1 = eng.run_coherences(p[:, i:i + 1].copy(), "lp_square")
        np.testing.assert_array_equal(c1[:, 0], coh[:, i])
