"""Which kernel family a batch descriptor runs (`ryd_batch_path`, the selection function the
launch itself calls), pinned for every descriptor and every selection switch.  The expectation
is written out here from the "Selection order" table of DESIGN.md and the rules of the
library's descriptor validation; the library is asked once per (switch setting, descriptor).
Host code only: no GPU.
"""
import itertools
import os

import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E

PATH = N.PATH
NOSTATE = PATH["NOSTATE"]
ERR_UNSUPPORTED = -3
# switch -> the family it turns off
SWITCHES = {"RYD_SYM16": "SYM16", "RYD_SHAPED16": "SHAPED16", "RYD_DIM4_PROP": "DIM4_PROP",
            "RYD_KET_BLOCK": "KET_BLOCK", "RYD_JP_SPLIT": "JP_SPLIT"}
ALL_VARS = tuple(SWITCHES) + ("RYD_NOSTATE",)
SETTINGS = (None,) + ALL_VARS                      # nothing set, then each variable alone at 0
FEW = ("lp_square", "bangbang", "smooth_jp")       # gates that are a product of few propagators
N_STEPS = {"lp_square": 0, "lp_shaped": 500, "bangbang": 4, "smooth_jp": 300}
DESCS = tuple(itertools.product((3, 4), N.EVOL, N.METHOD, N.PROTO, (0, 1), (0, 1)))


def expected(dim, evolution, method, protocol, symmetric, has_state, off):
    """The table, first match wins; `off`: the one variable set to 0, or None."""
    if dim == 4 and method not in ("chebyshev", "cheb_vector"):
        return ERR_UNSUPPORTED
    if method in ("dopri5", "cheb_squaring") and evolution != "lindblad":
        return ERR_UNSUPPORTED
    lind, auto, few = evolution == "lindblad", method == "chebyshev", protocol in FEW
    prop = dim == 3 and lind and (method == "cheb_squaring" or (auto and few))
    if method == "dopri5":
        path = "DOPRI5"
    elif dim == 4 and lind and auto and symmetric and few and off != "RYD_DIM4_PROP":
        path = "DIM4_PROP"
    elif dim == 3 and lind and auto and symmetric and protocol == "lp_shaped" and off != "RYD_SHAPED16":
        path = "SHAPED16"
    elif dim == 3 and lind and auto and symmetric and few and off != "RYD_SYM16":
        path = "SYM16"
    elif prop and protocol == "smooth_jp" and off != "RYD_JP_SPLIT":
        path = "JP_SPLIT"
    elif prop:
        path = "LINDBLAD_PROP"
    elif lind:
        path = "LINDBLAD_CHEB"
    elif auto and off != "RYD_KET_BLOCK":
        path = "KET_BLOCK"
    else:
        path = "KET_CHEB"
    twin = not has_state and path in ("SYM16", "KET_BLOCK") and off != "RYD_NOSTATE"
    return PATH[path] | (NOSTATE if twin else 0)


def ask(desc_key):
    dim, evolution, method, protocol, symmetric, has_state = desc_key
    d = E.make_desc(protocol, evolution, n_steps=N_STEPS[protocol], shape="gaussian", symmetric=bool(symmetric),
                    method=method, dim=dim, rtol=1e-10, atol=1e-12, max_steps=1000)
    return N.load().ryd_batch_path(d, has_state)


@pytest.fixture(scope="module")
def answers():
    """{setting: {descriptor: ryd_batch_path}} with every selection variable out of the
    environment but the one of the setting; the environment is put back afterwards."""
    saved = {v: os.environ.pop(v, None) for v in ALL_VARS}
    out = {}
    try:
        for off in SETTINGS:
            if off:
                os.environ[off] = "0"
            try:
                out[off] = {k: ask(k) for k in DESCS}
            finally:
                if off:
                    del os.environ[off]
    finally:
        for v, val in saved.items():
            if val is not None:
                os.environ[v] = val
    return out


@pytest.mark.parametrize("off", SETTINGS)
def test_every_descriptor_takes_the_path_of_the_table(answers, off):
    assert len(DESCS) == 256
    wrong = {k: (answers[off][k], expected(*k, off)) for k in DESCS if answers[off][k] != expected(*k, off)}
    assert not wrong


def test_rejected_descriptors_set_the_error_text(answers):
    assert answers[None][(4, "lindblad", "dopri5", "lp_square", 1, 1)] == ERR_UNSUPPORTED
    ask((3, "ket", "cheb_squaring", "lp_square", 1, 1))
    assert N.load().ryd_last_error() == b"squaring method is Lindblad-only"
    with pytest.raises(N.EngineError):
        E.batch_path(E.make_desc("lp_square", "ket", method="dopri5"))
    assert E.batch_path(E.make_desc("lp_square", "lindblad", method="dopri5"), states=False) == PATH["DOPRI5"]


@pytest.mark.parametrize("switch", SWITCHES)
def test_a_switch_moves_its_own_family_and_nothing_else(answers, switch):
    base, got = answers[None], answers[switch]
    family = PATH[SWITCHES[switch]]
    moved = [k for k in DESCS if got[k] != base[k]]
    assert moved                                                       # it selects something
    assert all(base[k] & ~NOSTATE == family for k in moved)           # only out of its family
    assert all(got[k] != base[k] for k in DESCS if base[k] >= 0 and base[k] & ~NOSTATE == family)
    assert not any(v >= 0 and v & ~NOSTATE == family for v in got.values())


def test_the_nostate_bit(answers):
    twins = {PATH["SYM16"], PATH["KET_BLOCK"]}
    for off, table in answers.items():
        for k, v in table.items():
            if v < 0 or not v & NOSTATE:
                continue
            assert v & ~NOSTATE in twins and k[-1] == 0 and off != "RYD_NOSTATE"
    # and it does appear: on both families, and under every selection switch but the family's own
    assert {v & ~NOSTATE for v in answers[None].values() if v >= 0 and v & NOSTATE} == twins
    moved = [k for k in DESCS if answers["RYD_NOSTATE"][k] != answers[None][k]]
    assert moved and all(answers[None][k] == answers["RYD_NOSTATE"][k] | NOSTATE for k in moved)
