"""Process maps for hilbert_space_dim=4 on the GPU (coherence4_prop_kernel and
coherence4_cheb_kernel + the 36-dim diagonal sector) against the oracle's full 256 x 256
Liouvillian.  Tolerance 1e-10 on every map element, 1e-9 on fidelities.  Shapes are tiny
and chosen for the kernel's layout: 4 points per wave, per-row squaring depths, a ragged
last wave, the bank-masked quads, the identical-atom mirror."""
import json
import warnings

import numpy as np
import pytest

import oracle_evaluator as OE
from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import calibration as CAL
from noisyquantumsimulator_amd import configurations as CF
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import physics as PH
from noisyquantumsimulator_amd import simulation as SIM
from process_map4_util import lp_shaped_segments, process_map_dim, spec4_from_params
from process_map_util import PATHS, coh_path as _coh_path

pytestmark = pytest.mark.gpu
TOL = 1e-10
FTOL = 1e-9
KW = dict(species="Rb87", n_rydberg=70, tweezer_power=0.020, tweezer_waist=0.8e-6, temperature=2e-6,
          spacing_factor=2.8, B_field=1e-4, NA=0.5)
SI = {"lp_square": CF.LPSimulationInputs, "smooth_jp": CF.SmoothJPSimulationInputs,
      "bangbang": CF.JPSimulationInputs}


def _exc(purity=0.95):
    return CF.TwoPhotonExcitationConfig(
        laser_1=CF.LaserParameters(power=50e-6, waist=50e-6, polarization="pi", polarization_purity=purity),
        laser_2=CF.LaserParameters(power=0.3, waist=50e-6, polarization="sigma+", polarization_purity=purity))


def _batch(si, n, **kw):
    """n derived dim-4 points: temperatures 1e-6 ... 3e-5 and laser_2_power over a decade
    (different squaring depths within one wave)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PH.derive_batch(si, n, hilbert_space_dim=4,
                               **dict(KW, temperature=np.linspace(1e-6, 3e-5, n)),
                               overrides=dict(laser_2_power=np.geomspace(0.03, 3.0, n)), **kw)


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


@pytest.fixture(scope="module")
def lp5():
    """The 5-point LP batch (one full wave and one ragged row) and its oracle maps."""
    b = _batch(CF.LPSimulationInputs(excitation=_exc()), 5)
    ref = [process_map_dim(OE.point_spec(b, i)) for i in range(5)]
    return b, E.pack_params(b), ref


@pytest.mark.parametrize("protocol,n,n_steps", [("lp_square", 5, None), ("smooth_jp", 3, 12), ("bangbang", 5, None)])
def test_dim4_process_map_matches_oracle(eng, lp5, protocol, n, n_steps):
    if protocol == "lp_square":
        b, p, ref = lp5
    else:
        b = _batch(SI[protocol](excitation=_exc()), n)
        p = E.pack_params(b)
        ref = [process_map_dim(OE.point_spec(b, i, n_steps=n_steps or 300)) for i in range(n)]
    assert np.all(b["mJ_leakage_rate"] > 0)
    assert E.protocol_key(b) == protocol
    for path in PATHS:
        with _coh_path(path):
            pm = NM.gate_process_maps(p, protocol, n_steps=n_steps, engine=eng, dim=4)
        assert np.all(pm.status == 0)
        for i in range(n):
            err = np.abs(pm.S[i] - ref[i]).max()
            print(f"{protocol} RYD_COH_PROP={path} point {i}: max|dS| = {err:.3e}")
            np.testing.assert_allclose(pm.S[i], ref[i], atol=TOL, rtol=0, err_msg=f"{protocol}/{path}/{i}")


def test_dim4_unequal_atoms(eng, lp5):
    """GMJ_B x 3 and G1_B x 1.37: the (-1,0) sector is built, not mirrored.  The last point
    differs in GMJ alone: identical atoms means the four rate columns AND the mJ rate."""
    _, p5, _ = lp5
    p = np.concatenate([p5, p5[:, :1]], axis=1)
    p[N.P["GMJ_B"]] *= 3.0
    p[N.P["G1_B"], :5] *= 1.37
    assert all(p[N.P[k + "_A"], 5] == p[N.P[k + "_B"], 5] for k in ("G1", "G0", "GPHI", "GSC"))
    ref = [process_map_dim(spec4_from_params(p, i, "lp_square")) for i in range(6)]
    for path in PATHS:
        with _coh_path(path):
            pm = NM.gate_process_maps(p, "lp_square", engine=eng, dim=4)
        assert np.all(pm.status == 0)
        for i in range(6):
            err = np.abs(pm.S[i] - ref[i]).max()
            print(f"unequal RYD_COH_PROP={path} point {i}: max|dS| = {err:.3e}")
            np.testing.assert_allclose(pm.S[i], ref[i], atol=TOL, rtol=0, err_msg=f"{path}/{i}")


def test_dim4_shaped_lp(eng):
    """A cosine envelope: a new amplitude every segment, so the per-lane Chebyshev kernel."""
    b = _batch(CF.LPSimulationInputs(excitation=_exc(), pulse_shape="cosine"), 2)
    assert E.protocol_key(b) == "lp_shaped" and np.all(b["mJ_leakage_rate"] > 0)
    p = E.pack_params(b)
    pm = NM.gate_process_maps(p, "lp_shaped", n_steps=12, shape="cosine", engine=eng, dim=4)
    assert np.all(pm.status == 0)
    for i in range(2):
        spec = OE.point_spec(b, i)
        assert spec.protocol == "lp_shaped" and spec.pulse_shape == "cosine"
        ref = process_map_dim(spec, lp_shaped_segments(spec, 12))
        print(f"shaped point {i}: max|dS| = {np.abs(pm.S[i] - ref).max():.3e}")
        np.testing.assert_allclose(pm.S[i], ref, atol=TOL, rtol=0)


def test_dim4_noise_free_map_is_the_ket_unitary(eng):
    """Zero rates (GMJ too): the coherence kernels and the ket kernel are independent routes
    to S = U_q (x) conj(U_q).  Two batches of 8 (two full waves): the decade of laser power
    for the map, and nominal power for the Kraus rank -- noise_models.kraus counts Choi
    eigenvalues above 1e-12 of the largest (4e-12 absolute), 25 times below the map
    tolerance, and a propagator built by s squarings carries ~2^s eps:
    2e-12 at the s = 14 of the weakest laser, 2e-13 at nominal power."""
    si = CF.LPSimulationInputs(excitation=_exc())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nominal = PH.derive_batch(si, 8, hilbert_space_dim=4, **dict(KW, temperature=np.linspace(1e-6, 3e-5, 8)))
    for b, rank in ((_batch(si, 8), False), (nominal, True)):
        p = E.pack_params(b)
        for k in ("G1", "G0", "GPHI", "GSC", "GMJ"):
            p[N.P[k + "_A"]] = p[N.P[k + "_B"]] = 0.0
        pm = NM.gate_process_maps(p, "lp_square", engine=eng, with_kraus=True, dim=4)
        assert np.all(pm.status == 0)
        S_ket = NM.ket_maps(eng.run(p, "lp_square", "ket", dim=4).kets(), 4)
        np.testing.assert_allclose(pm.S, S_ket, atol=TOL, rtol=0)
        if rank:
            assert np.all(pm.kraus_rank == 1)


def test_dim4_coherence_rows_are_independent_of_their_wave(eng):
    p = E.pack_params(_batch(CF.LPSimulationInputs(excitation=_exc()), 7))
    coh, st = eng.run_coherences(p, "lp_square", dim=4)
    assert np.all(st == 0)
    for i in (0, 3, 6):
        c1, s1 = eng.run_coherences(p[:, i:i + 1].copy(), "lp_square", dim=4)
        assert s1[0] == 0
        np.testing.assert_array_equal(c1[:, 0], coh[:, i])


def test_dim4_channel_properties(eng):
    n = 500
    rng = np.random.default_rng(8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b = PH.derive_batch(CF.LPSimulationInputs(excitation=_exc()), n, hilbert_space_dim=4,
                            **dict(KW, temperature=rng.uniform(1e-6, 3e-5, n)))
    pm = NM.gate_process_maps(E.pack_params(b), "lp_square", engine=eng, dim=4)
    assert np.all(pm.status == 0)
    assert np.linalg.eigvalsh(pm.choi).min() > -1e-10                 # completely positive
    T = np.einsum("nacbc->nab", pm.choi.reshape(n, 4, 4, 4, 4))       # Tr_out J <= I_in
    assert np.linalg.eigvalsh(np.eye(4) - T).min() > -1e-10
    assert np.all(pm.process_fidelity <= 1 + 1e-12) and np.all(pm.leakage >= -1e-12)


def test_dim4_bad_mj_rate_flags_its_point_only(eng):
    p = E.pack_params(_batch(CF.LPSimulationInputs(excitation=_exc()), 6))
    for path in PATHS:
        with _coh_path(path):
            clean, st0 = eng.run_coherences(p, "lp_square", dim=4)
            q = p.copy()
            q[N.P["GMJ_A"], 2] = -1.0
            coh, st = eng.run_coherences(q, "lp_square", dim=4)
        assert np.all(st0 == 0)
        good = np.arange(6) != 2
        assert st[2] & N.STATUS_BAD_INPUT and np.all(st[good] == 0)
        np.testing.assert_array_equal(coh[:, good], clean[:, good])


@pytest.fixture(scope="module")
def drop_in():
    """simulate_CZ_gate in dim 4 and dim 3 with process_fidelity=True, and the oracle's figure."""
    kw = dict(KW, temperature=2e-5)
    si = CF.LPSimulationInputs(excitation=_exc())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r4 = SIM.simulate_CZ_gate(si, hilbert_space_dim=4, process_fidelity=True, **kw)
        r3 = SIM.simulate_CZ_gate(si, hilbert_space_dim=3, process_fidelity=True, **kw)
        b = PH.derive_batch(si, hilbert_space_dim=4, **kw)
    fpro, favg = NM.gate_fidelity(process_map_dim(OE.point_spec(b, 0))[None])
    return r4, r3, float(fpro[0]), float(favg[0])


def test_simulate_cz_gate_dim4_process_fidelity(drop_in):
    r4, r3, fpro, favg = drop_in
    assert r4.process_fidelity is not None and np.isfinite(r4.process_fidelity)
    print(f"dim 4 F_pro = {r4.process_fidelity:.10f} (oracle {fpro:.10f}), dim 3 {r3.process_fidelity:.10f}")
    assert abs(r4.process_fidelity - fpro) < FTOL
    assert abs(r4.avg_gate_fidelity - favg) < FTOL
    assert abs(r4.process_fidelity - r3.process_fidelity) > 1e-4      # the mJ channel is not dropped
    n = 6
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        br = SIM.simulate_CZ_gate_batch(CF.LPSimulationInputs(excitation=_exc()), n, hilbert_space_dim=4,
                                        process_fidelity=True,
                                        **dict(KW, temperature=np.linspace(1e-6, 3e-5, n)))
    assert np.all(br.is_mixed)                                         # every point is noisy
    assert np.all(np.isfinite(br.process_fidelity)) and np.all(np.isfinite(br.avg_gate_fidelity))
    assert np.all(br.status & N.STATUS_FAIL_MASK == 0)


def test_calibrate_cz_dim4_uses_the_dim4_map(tmp_path):
    si = CF.LPSimulationInputs(excitation=_exc())
    T = np.array([1e-5, 2e-5])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        paths = CAL.calibrate_cz(si, str(tmp_path), hilbert_space_dim=4, temperature=T,
                                 **{k: v for k, v in KW.items() if k not in ("temperature", "species", "n_rydberg")})
        br = SIM.simulate_CZ_gate_batch(si, 2, hilbert_space_dim=4, process_fidelity=True,
                                        **dict(KW, temperature=T))
    assert len(paths) == 1
    with open(paths[0]) as f:
        doc = json.load(f)
    for i, rec in enumerate(doc["points"]):
        assert abs(rec["error_rates"]["process_infidelity"] - (1 - br.process_fidelity[i])) < FTOL
