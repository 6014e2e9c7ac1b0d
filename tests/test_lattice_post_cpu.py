"""The float64 posterior reference (tests/lattice_post_ref.py) that the GPU tests of lasr_align_post_* / lasr_lattice_post take their
expected values from: occupancies against enumeration of every path, a closed form on the all-zero lattice, finite differences of
lattice_ref.forward, the two sum invariants, -inf entries, an impossible lattice and U = 0.  Also: the new calls are bound and exposed."""
import inspect
from math import comb

import numpy as np
import pytest

import lattice_post_ref as P
import lattice_ref as R
from libreasr_amd import _native as N


def rand(T, U, seed, scale=8.0):
    rng = np.random.default_rng(seed)
    return -rng.random((T, U + 1)).astype(np.float32) * scale, -rng.random((T, U + 1)).astype(np.float32) * scale


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_align_post_pcm", "lasr_align_post_feats", "lasr_lattice_post"} <= names
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    assert callable(getattr(Engine, "lattice_post", None))
    assert "posteriors" in inspect.signature(Engine.align_pcm).parameters
    assert "posteriors" in inspect.signature(Engine.align_feats).parameters
    assert "posteriors" in inspect.signature(LibreASR.align).parameters
    import __graft_entry__ as graft
    graft.build()
    lib = N.lib()
    for meth in ("lasr_align_post_pcm", "lasr_align_post_feats", "lasr_lattice_post"):
        assert hasattr(lib, meth)
    assert lib.lasr_lattice_post(None, None, None, None, None, 1, *[None] * 8) == N.LASR_EINVAL      # no context: an error code


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("U", [0, 1, 2, 3])
def test_occupancies_against_every_path(T, U):
    for rep in range(5):
        b, e = rand(T, U, 1000 * T + 10 * U + rep)
        ll, ob, oe = P.brute(b, e, U)
        r = P.posteriors(b, e, U)
        assert abs(r["loglik"] - ll) < 1e-12 and abs(r["loglik_bwd"] - ll) < 1e-12
        assert np.abs(r["occ_b"] - ob).max() < 1e-12
        assert np.abs(r["occ_e"] - oe).max() < 1e-12
        ts = np.arange(T, dtype=np.float64)
        for u in range(U):
            p = oe[:, u]
            m = float(np.sum(ts * p))
            assert abs(r["tok_mean"][u] - m) < 1e-12
            assert abs(r["tok_var"][u] - float(np.sum((ts - m) ** 2 * p))) < 1e-12
            assert r["tok_peak"][u] == r["occ_e"][r["tok_peak_frame"][u], u] == r["occ_e"][:, u].max()
            assert np.all(r["occ_e"][:r["tok_peak_frame"][u], u] < r["tok_peak"][u])          # the FIRST of the largest


def test_closed_form_on_the_all_zero_lattice():
    """every path scores 0, so an occupancy is a count of paths: (paths into the cell) x (paths out of the edge's head) / all paths"""
    T, U = 6, 4
    z = np.zeros((T, U + 1), np.float32)
    r = P.posteriors(z, z, U)
    n_paths = comb(T - 1 + U, U)
    assert abs(r["loglik"] - np.log(n_paths)) < 1e-12
    for t in range(T):
        for u in range(U + 1):
            if u < U:
                assert abs(r["occ_e"][t, u] - comb(t + u, u) * comb(T - 1 - t + U - u - 1, U - u - 1) / n_paths) < 1e-12
            if t < T - 1:
                assert abs(r["occ_b"][t, u] - comb(t + u, u) * comb(T - 2 - t + U - u, U - u) / n_paths) < 1e-12
    assert r["occ_b"][T - 1, U] == 1.0 and np.all(r["occ_b"][T - 1, :U] == 0) and np.all(r["occ_e"][:, U] == 0)


@pytest.mark.parametrize("T,U", [(3, 2), (5, 3), (7, 1), (2, 4)])
def test_occupancies_are_the_gradient_of_loglik(T, U):
    """central finite differences of lattice_ref.forward, h = 1e-6 (float64 inputs, so that the step is exact to rounding)"""
    b, e = rand(T, U, 77 * T + U, scale=3.0)
    b, e = b.astype(np.float64), e.astype(np.float64)
    r = P.posteriors(b, e, U)
    h = 1e-6
    for t in range(T):
        for u in range(U + 1):
            bp, bm = b.copy(), b.copy()
            bp[t, u] += h
            bm[t, u] -= h
            g = (R.forward(bp, e, U) - R.forward(bm, e, U)) / (2 * h)
            assert abs(g - r["occ_b"][t, u]) < 1e-6, (t, u, g, r["occ_b"][t, u])
            if u < U:
                ep, em = e.copy(), e.copy()
                ep[t, u] += h
                em[t, u] -= h
                g = (R.forward(b, ep, U) - R.forward(b, em, U)) / (2 * h)
                assert abs(g - r["occ_e"][t, u]) < 1e-6, (t, u, g, r["occ_e"][t, u])


@pytest.mark.parametrize("T,U", [(1, 0), (1, 3), (5, 0), (9, 7), (30, 12), (12, 30)])
def test_sum_invariants_and_backward_loglik(T, U):
    b, e = rand(T, U, 5 * T + U)
    r = P.posteriors(b, e, U)
    assert abs(r["loglik"] - R.forward(b, e, U)) < 1e-9 and abs(r["loglik_bwd"] - R.forward(b, e, U)) < 1e-9
    assert np.abs(r["occ_b"].sum(axis=1) - 1).max() < 1e-10          # one blank per frame
    if U:
        assert np.abs(r["occ_e"][:, :U].sum(axis=0) - 1).max() < 1e-10   # every label exactly once
        assert np.all((0 <= r["tok_mean"]) & (r["tok_mean"] <= T - 1 + 1e-9)) and np.all(r["tok_var"] >= 0)
        assert np.all(np.diff(r["tok_mean"]) >= -1e-12)              # labels are emitted in order


def test_minus_inf_entries():
    b, e = P.minus_inf_lattice()
    r = P.posteriors(b, e, 3)
    for k in ("occ_b", "occ_e", "tok_mean", "tok_var", "tok_peak"):
        assert np.all(np.isfinite(r[k])), k
    assert np.isfinite(r["loglik"]) and abs(r["loglik_bwd"] - r["loglik"]) < 1e-9
    assert r["occ_e"][0, 0] == 0 and r["occ_b"][2, 1] == 0
    ll, ob, oe = P.brute(b, e, 3)
    assert abs(ll - r["loglik"]) < 1e-12 and np.abs(ob - r["occ_b"]).max() < 1e-12 and np.abs(oe - r["occ_e"]).max() < 1e-12
    assert np.abs(r["occ_b"].sum(axis=1) - 1).max() < 1e-10 and np.abs(r["occ_e"][:, :3].sum(axis=0) - 1).max() < 1e-10


def test_impossible_lattice():
    b, e = P.impossible_lattice()
    r = P.posteriors(b, e, 2)
    assert r["loglik"] == -np.inf and r["loglik_bwd"] == -np.inf
    assert np.all(r["occ_b"] == 0) and np.all(r["occ_e"] == 0)
    assert list(r["tok_mean"]) == [-1, -1] and list(r["tok_var"]) == [0, 0]
    assert list(r["tok_peak_frame"]) == [-1, -1] and list(r["tok_peak"]) == [0, 0]


def test_no_labels():
    b, e = rand(5, 0, 7)
    r = P.posteriors(b, e, 0)
    want = float(np.asarray(b, np.float64).sum())
    assert r["loglik"] == pytest.approx(want, abs=1e-12) and r["loglik_bwd"] == pytest.approx(want, abs=1e-12)
    assert np.allclose(r["occ_b"], 1.0, rtol=0, atol=1e-12) and np.all(r["occ_e"] == 0)
    assert r["tok_mean"].size == 0 and r["tok_peak_frame"].size == 0
