"""Summary-only runs, the parts that need no GPU: the rule that decides whether an engine pass
of simulate_CZ_gate_batch brings the state rows back, the EngineResult of a summary-only run,
and the ABI version (the nullable state pointer is an additive change)."""
import itertools

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from noisyquantumsimulator_amd import simulation as SIM


def test_needs_state_truth_table():
    """State is needed iff the caller asked for it, the process fidelity is built from it, or
    the points are Lindblad points whose reference phase penalty reads rho."""
    for evol, pen, ret, pro in itertools.product(("ket", "lindblad"), ("reference", "none"),
                                                 (False, True), (False, True)):
        want = ret or pro or (evol == "lindblad" and pen == "reference")
        got = SIM.needs_state(evol, pen, ret, pro)
        assert got is want, (evol, pen, ret, pro)
    # the cases the bulk callers hit
    assert SIM.needs_state("ket", "reference", False, False) is False        # noise-free optimiser candidates
    assert SIM.needs_state("lindblad", "none", False, False) is False        # phase_penalty="none" sweeps
    assert SIM.needs_state("lindblad", "reference", False, False) is True    # the LAPACK epilogue reads rho


@pytest.mark.parametrize("evolution,call", [("lindblad", "rho"), ("ket", "kets")])
def test_summary_only_result_has_no_state(evolution, call):
    r = E.EngineResult(evolution, 2, None, np.zeros((N.NSUMMARY, 2)), np.zeros(2, np.uint32), 0.0, 0.0, 0.0,
                       0.0, 0.0)
    assert r.state is None
    with pytest.raises(ValueError, match="summary-only"):
        getattr(r, call)()
    assert r.populations().shape == (2, 4)                                   # the summary still serves


def test_abi_version_unchanged():
    assert N.RYD_ABI_VERSION == 5
