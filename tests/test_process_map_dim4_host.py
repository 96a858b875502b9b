"""Host side of the dim-4 process maps on CPU: the test helpers are pinned to the oracle
(its dim-3 process map, its dim-4 collapse-operator list, its shaped-pulse segments), and
noise_models.assemble_maps reads the 36-row dim-4 states."""
import warnings

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import configurations as CF
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import noise_models as NM
from noisyquantumsimulator_amd import physics as PH
from oracle import lindblad_oracle as O
from process_map4_util import lp_shaped_segments, process_map_dim, rows4_from_map, spec4_from_params
from process_map_util import spec_from_params
from test_process_map_host import _random_params

KW = dict(species="Rb87", n_rydberg=70, tweezer_power=0.020, tweezer_waist=0.8e-6, temperature=2e-5,
          spacing_factor=2.8, B_field=1e-4, NA=0.5)


def _exc(purity=0.95):
    return CF.TwoPhotonExcitationConfig(
        laser_1=CF.LaserParameters(power=50e-6, waist=50e-6, polarization="pi", polarization_purity=purity),
        laser_2=CF.LaserParameters(power=0.3, waist=50e-6, polarization="sigma+", polarization_purity=purity))


@pytest.fixture(scope="module")
def derived4():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b = PH.derive_batch(CF.LPSimulationInputs(excitation=_exc()), hilbert_space_dim=4, **KW)
    return b, E.pack_params(b)


def test_process_map_dim_is_the_oracles_on_dim3():
    spec = spec_from_params(_random_params(4), 0, "lp_square")
    np.testing.assert_allclose(process_map_dim(spec), O.process_map(spec), atol=1e-14, rtol=0)


def test_spec4_liouvillian_is_the_oracle_c_op_lists(derived4):
    b, p = derived4
    assert b["mJ_leakage_rate"][0] > 0 and p[N.P["GMJ_A"], 0] > 0
    spec = spec4_from_params(p, 0, "lp_square")
    H = O.segments(spec)[1][0]
    ref_ops = O.collapse_operators({k: b.cols[k][0] for k in O.RATE_KEYS}, 4)
    L, Lref = O.liouvillian(H, spec.c_ops), O.liouvillian(H, ref_ops)
    Ld, Lrd = L - O.liouvillian(H, []), Lref - O.liouvillian(H, [])     # the dissipators alone
    assert np.abs(Ld - Lrd).max() <= 1e-12 * np.abs(Lrd).max()
    assert np.abs(L - Lref).max() <= 1e-12 * np.abs(Lref).max()


def test_lp_shaped_segments_restate_the_oracle(derived4):
    _, p = derived4
    spec = spec4_from_params(p, 0, "lp_shaped", pulse_shape="cosine")
    spec.area_correction = 1.7
    ref, got = O.segments(spec), lp_shaped_segments(spec, 500)
    assert len(ref) == len(got) == 998
    for k in (0, 1, 250, 498, 499, 700, 997):
        np.testing.assert_array_equal(got[k][0], ref[k][0])
        np.testing.assert_array_equal(got[k][1], ref[k][1])


def test_assemble_maps_reads_dim4_rows(derived4):
    _, p = derived4
    S = process_map_dim(spec4_from_params(p, 0, "lp_square"))
    state, coh = rows4_from_map(S)
    assert state.shape == (36, 4)
    got = NM.assemble_maps(state, coh, dim=4)[0]
    # the whole map, to the oracle's own rounding (its adjoint elements and its structural
    # zeros come out of a 256 x 256 expm independently: ~1e-14); then exactly, element by
    # element, on the support the rows carry, with the adjoints as their conjugates
    np.testing.assert_allclose(got, S, atol=1e-12, rtol=0)
    rows = ((N.C["K0"], ((0, 1), (2, 3))), (N.C["K1"], ((0, 2), (1, 3))))
    for _, units in rows:
        for a, b in units:
            for c, d in units:
                assert got[4 * c + d, 4 * a + b] == S[4 * c + d, 4 * a + b]
                assert got[4 * d + c, 4 * b + a] == np.conj(S[4 * c + d, 4 * a + b])
    assert got[3, 3] == S[3, 3] and got[12, 12] == np.conj(S[3, 3])
    assert got[6, 6] == S[6, 6] and got[9, 9] == np.conj(S[6, 6])
    for x in range(4):
        for y in range(4):
            assert got[5 * y, 5 * x] == S[5 * y, 5 * x].real
    with pytest.raises(ValueError):
        NM.assemble_maps(state, coh, dim=5)


def test_dim3_entry_points_refuse_mj_rates(derived4):
    """A params block with GMJ columns is a dim-4 block: the dim-3 coherence entry points
    refuse it before any GPU call (they would drop the mJ channel silently)."""
    _, p = derived4
    with pytest.raises(ValueError, match="GMJ"):
        E.check_coherence_dim(p, 3)
    E.check_coherence_dim(p, 4)
    with pytest.raises(ValueError):
        E.check_coherence_dim(p, 5)
