"""The sym16 kernel's serial stretches (ryd_sym16.inc: segment 1 of LP square without a
second parameter load, the output stores as a wave-uniform base plus a 32-bit lane offset
or per lane in 64 bits, the shared segment loop and epilogue of bang-bang and smooth JP):
small batches of every size up to three waves, a wave that mixes every kind of row, both
store forms, padded output buffers.

Points are identical-atom variants of test_gpu_parity._random_points (B rates = A rates),
as in test_gpu_sym16_build.py, whose 1e-11 against the per-input vector kernel
(`method="cheb_vector"`) is the tolerance here too.  The reference runs are made once per
module and shared.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from noisyquantumsimulator_amd import _native as N
from noisyquantumsimulator_amd import engine as E
from test_gpu_parity import _random_points
from test_gpu_sym16_build import ATOL, OWN, _omega, _same_point, _sym

pytestmark = pytest.mark.gpu

NPTS = 9
SIZES = (1, 2, 3, 4, 5, 7, 9)
SENTINEL = -1.2345678901234567e77
PHYS = [i for i in range(N.NSUMMARY) if i not in (N.S["NMV_USEFUL"], N.S["NMV_EXEC"], N.S["NSQUARE"])]


@pytest.fixture(scope="module")
def eng():
    return E.Engine()


@pytest.fixture(scope="module")
def pts():
    p = _sym(_random_points(np.random.default_rng(20261020), NPTS, "lp_square"))
    assert E.symmetric_atoms(p)
    return p


def _run(eng, p, protocol="lp_square", method="chebyshev", n_steps=None):
    return eng.run(np.ascontiguousarray(p), protocol, "lindblad", n_steps=n_steps, method=method)


@pytest.fixture(scope="module")
def alone(eng, pts):
    """Every point run as a batch of one."""
    return [_run(eng, pts[:, i:i + 1]) for i in range(NPTS)]


@pytest.fixture(scope="module")
def batches(eng, pts):
    """The first n points as one batch, for every size: sym16 kernel and vector kernel."""
    return {n: (_run(eng, pts[:, :n]), _run(eng, pts[:, :n], method="cheb_vector")) for n in SIZES}


def test_batch_sizes(eng, pts, alone, batches):
    for n, (r16, rv) in batches.items():
        ds = float(np.abs(r16.state - rv.state).max())
        dm = float(np.nanmax(np.abs(r16.summary[PHYS] - rv.summary[PHYS])))
        print(f"n = {n}: max|dstate| = {ds:.3e}, max|dsummary| = {dm:.3e}")
        assert np.all(r16.status == 0)
        np.testing.assert_array_equal(r16.status, rv.status)
        np.testing.assert_allclose(r16.state, rv.state, atol=ATOL, rtol=0)
        # the summary's physical rows (the work counters describe the method); a row the
        # Lindblad evolution does not compute is NaN in both
        np.testing.assert_allclose(r16.summary[PHYS], rv.summary[PHYS], atol=ATOL, rtol=0, equal_nan=True)
        for i in range(n):
            _same_point(r16, [i], alone[i], [0], f"n = {n}, point {i} against its own run", OWN)
    # every point at every position of a wave: `shift` copies of point 0 in front
    for shift in range(4):
        q = np.concatenate([np.repeat(pts[:, :1], shift, axis=1), pts], axis=1)
        r = _run(eng, q)
        for i in range(NPTS):
            _same_point(r, [shift + i], alone[i], [0], f"point {i} at wave position {(i + shift) % 4}", OWN)


def test_mixed_wave(eng, pts):
    """One wave: a unit-xi point, |xi| = 0.7, an invalid row (NaN Omega), x below X_SKIP."""
    q = pts[:, :4].copy()
    q[N.P["XI_RE"], 1] *= 0.7
    q[N.P["XI_IM"], 1] *= 0.7
    q[N.P["OMEGA"], 2] = np.nan
    q[N.P["TAU"], 3] = 1e-21 / _omega(q[:, 3:4], "lp_square")[0]
    assert E.symmetric_atoms(q)
    assert abs(np.hypot(q[N.P["XI_RE"], 0], q[N.P["XI_IM"], 0]) - 1.0) <= 1e-15
    assert abs(np.hypot(q[N.P["XI_RE"], 1], q[N.P["XI_IM"], 1]) - 0.7) <= 1e-15
    r = _run(eng, q)
    single = [_run(eng, q[:, i:i + 1]) for i in range(4)]
    for i in range(4):
        _same_point(r, [i], single[i], [0], f"row {i} against its own run", OWN)
        for name in ("NSQUARE", "NMV_USEFUL"):
            assert r.col(name)[i] == single[i].col(name)[0], (name, i)
    print("status", r.status, "NSQUARE", r.col("NSQUARE"), "NMV_USEFUL", r.col("NMV_USEFUL"))
    np.testing.assert_array_equal(r.status & N.STATUS_BAD_INPUT != 0, [False, False, True, False])
    np.testing.assert_array_equal(r.status[[0, 1, 3]], 0)
    # the non-unit point built a second propagator, the skipped one none
    assert r.col("NSQUARE")[1] > r.col("NSQUARE")[0] > 0
    assert r.col("NMV_USEFUL")[3] == 0 and r.col("NSQUARE")[3] == 0
    rv = _run(eng, q[:, [0, 1, 3]], method="cheb_vector")
    np.testing.assert_allclose(r.state.reshape(25, 4, 4)[:, [0, 1, 3]], rv.state.reshape(25, 3, 4), atol=ATOL, rtol=0)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from noisyquantumsimulator_amd import engine as E
p = np.load(sys.argv[3])
r = E.Engine().run(p, "lp_square", "lindblad", method="chebyshev")
np.savez(sys.argv[4], state=r.state, summary=r.summary, status=r.status)
"""


def test_store_forms(batches, pts, tmp_path):
    """RYD_S16_STORE64=1 in a fresh process: per-lane 64-bit store addresses, the same bytes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    np.save(tmp_path / "p.npy", np.ascontiguousarray(pts[:, :7]))
    env = dict(os.environ, RYD_S16_STORE64="1")
    subprocess.run([sys.executable, "-c", _CHILD, root, os.path.join(root, "tests"), str(tmp_path / "p.npy"),
                    str(tmp_path / "out.npz")], check=True, env=env, timeout=120)
    got, ref = np.load(tmp_path / "out.npz"), batches[7][0]
    assert got["state"].tobytes() == ref.state.tobytes()
    assert got["summary"].tobytes() == ref.summary.tobytes()
    assert got["status"].tobytes() == ref.status.tobytes()


def test_output_padding(eng, pts, batches):
    """ld_state and ld_summary larger than needed, buffers pre-filled with a sentinel: nothing
    outside the n points' columns is written, everything inside equals the tight layout."""
    n, lib, h = 7, eng.lib, eng.handle
    ref = batches[n][0]
    p = np.ascontiguousarray(pts[:, :n])
    lds, ldm, nst = 4 * n + 13, n + 6, n + 5
    state = np.full((25, lds), SENTINEL)
    summ = np.full((N.NSUMMARY, ldm), SENTINEL)
    status = np.full(nst, 0xA5A5A5A5, dtype=np.uint32)
    desc = E.make_desc("lp_square", "lindblad", 0, "square", True, "chebyshev")
    bufs = []
    try:
        for a in (p, state, summ, status):
            d = ctypes.c_void_p()
            N.check(lib.ryd_malloc(h, 0, a.nbytes, ctypes.byref(d)))
            bufs.append(d)
            N.check(lib.ryd_memcpy_h2d(h, 0, d, a.ctypes.data, a.nbytes))
        N.check(lib.ryd_run_batch_device(h, 0, ctypes.byref(desc), bufs[0], n, n, bufs[1], lds, bufs[2], ldm,
                                         bufs[3], None, None))
        N.check(lib.ryd_synchronize(h))
        for a, d in zip((state, summ, status), bufs[1:]):
            N.check(lib.ryd_memcpy_d2h(h, 0, a.ctypes.data, d, a.nbytes))
    finally:
        for d in bufs:
            lib.ryd_free(h, 0, d)
    assert state[:, :4 * n].tobytes() == ref.state.tobytes()
    assert summ[:, :n].tobytes() == ref.summary.tobytes()
    np.testing.assert_array_equal(status[:n], ref.status)
    assert np.all(state[:, 4 * n:] == SENTINEL) and np.all(summ[:, n:] == SENTINEL)
    assert np.all(status[n:] == 0xA5A5A5A5)


@pytest.mark.parametrize("protocol,n_steps", [("bangbang", None), ("smooth_jp", 20)])
def test_other_protocols_share_the_tail(eng, protocol, n_steps):
    p = _sym(_random_points(np.random.default_rng(20261021), 5, protocol))
    assert E.symmetric_atoms(p)
    r16 = _run(eng, p, protocol, n_steps=n_steps)
    rv = _run(eng, p, protocol, method="cheb_vector", n_steps=n_steps)
    print(f"{protocol}: max|dstate| = {float(np.abs(r16.state - rv.state).max()):.3e}")
    assert np.all(r16.status == 0) and np.all(rv.status == 0)
    np.testing.assert_allclose(r16.state, rv.state, atol=ATOL, rtol=0)
    np.testing.assert_allclose(r16.populations(), rv.populations(), atol=ATOL, rtol=0)
