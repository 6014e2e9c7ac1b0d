"""Banded lattice posteriors without a GPU: the float64 reference of tests/lattice_band_post_ref.py against lattice_post_ref on the
spread lattice (the same operations in the same order: occupancies and loglik differ by exactly 0), against the enumeration of every
path, its sum invariants, the no-path convention, and the new names of the library and of the Python surface."""
import warnings

import numpy as np
import pytest

import lattice_band_post_ref as Q
import lattice_band_ref as B
import lattice_post_ref as P
from libreasr_amd import _native as N

SPREAD_SHAPES = [(1, 0, 1), (1, 3, 2), (5, 0, 4), (2, 1, 1), (3, 2, 2), (9, 7, 3), (12, 20, 5), (64, 63, 8), (70, 130, 17), (300, 5, 3),
                 (40, 200, 90), (25, 30, 31)]       # (T, U, band), every one with T (U + 1) <= 20 000


def rand64(rng, T, U):
    return (-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32), -(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32))


def check_no_path(r, T, w, U):
    assert r["loglik"] == -np.inf
    assert np.all(r["occ_b"] == 0) and np.all(r["occ_e"] == 0) and r["occ_b"].shape == (T, w)
    assert list(r["tok_mean"]) == [-1.0] * U and list(r["tok_var"]) == [0.0] * U
    assert list(r["tok_peak_frame"]) == [-1] * U and list(r["tok_peak"]) == [0.0] * U
    for k in ("occ_b", "occ_e", "tok_mean", "tok_var", "tok_peak"):
        assert not np.any(np.isnan(r[k])), k


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_align_band_post_pcm", "lasr_align_band_post_feats", "lasr_lattice_band_post"} <= names
    import inspect
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    assert list(inspect.signature(Engine.lattice_band_post).parameters) == ["self", "blank", "emit", "lo", "U"]
    for meth in ("align_band_post_pcm", "align_band_post_feats"):
        ps = inspect.signature(getattr(Engine, meth)).parameters
        assert list(ps)[1] == "slots" and list(ps)[3:] == ["token_lists", "band", "max_passes", "windows", "lattice", "viterbi"], meth
        assert ps["band"].default is inspect.Parameter.empty and ps["max_passes"].default == 1 and ps["windows"].default is None
        assert ps["lattice"].default is False and ps["viterbi"].default is True
    ps = inspect.signature(LibreASR.align_band).parameters
    assert list(ps) == ["self", "audio", "transcript", "band", "max_passes", "posteriors"]
    assert ps["band"].default == 64 and ps["max_passes"].default == 4 and ps["posteriors"].default is True
    import __graft_entry__ as graft
    graft.build()
    lib = N.lib()
    assert lib.lasr_lattice_band_post(None, None, None, None, None, None, None, 1, *([None] * 8)) == N.LASR_EINVAL   # no context: an error code
    assert lib.lasr_align_band_post_feats(None, None, 0, None, None, None, None, 4, 1, *([None] * 16)) == N.LASR_EINVAL
    assert lib.lasr_align_band_post_pcm(None, None, 0, None, None, None, None, 4, 1, *([None] * 16)) == N.LASR_EINVAL


@pytest.mark.parametrize("windows", ["linear", "random"])
def test_equals_full_reference_on_the_spread_lattice(windows):
    rng = np.random.default_rng(5757)
    worst = dict(bwd=0.0, sums=0.0, mean=0.0, var=0.0)
    for T, U, band in SPREAD_SHAPES:
        assert T * (U + 1) <= 20000
        b, e = rand64(rng, T, U)
        w = B.width(T, U, band)
        lo = B.linear(T, U, band) if windows == "linear" else Q.random_windows(rng, T, U, w)
        assert B.valid(T, U, w, lo)
        bb, eb = B.cut(b, lo, w), B.cut(e, lo, w)
        got = Q.posteriors(bb, eb, lo, U)
        ref = P.posteriors(B.spread(bb, lo, U), B.spread(eb, lo, U), U)
        assert got["loglik"] == ref["loglik"] == B.forward(bb, eb, lo, U), (T, U, band)
        if ref["loglik"] == -np.inf:
            check_no_path(got, T, w, U)
            continue
        assert got["loglik_bwd"] == ref["loglik_bwd"]
        assert np.array_equal(got["occ_b"], B.cut(ref["occ_b"], lo, w)) and np.array_equal(got["occ_e"], B.cut(ref["occ_e"], lo, w))
        # nothing of the full lattice's occupancy lies outside the band
        inside = B.spread(np.ones((T, w)), lo, U, fill=0.0) > 0
        assert np.all(ref["occ_b"][~inside] == 0) and np.all(ref["occ_e"][~inside] == 0)
        assert [int(t) for t in got["tok_peak_frame"]] == [int(t) for t in ref["tok_peak_frame"]]
        assert np.array_equal(got["tok_peak"], ref["tok_peak"])
        if U:                                             # (the full reference sums pairwise, this one in frame order)
            worst["mean"] = max(worst["mean"], float(np.abs(got["tok_mean"] - ref["tok_mean"]).max()) / T)
            worst["var"] = max(worst["var"], float(np.abs(got["tok_var"] - ref["tok_var"]).max()) / T ** 2)
        worst["bwd"] = max(worst["bwd"], abs(got["loglik_bwd"] - got["loglik"]))
        worst["sums"] = max(worst["sums"], Q.sum_invariants(got["occ_b"], got["occ_e"], lo, U))
    print(f"{windows} windows: {worst}")
    assert worst["mean"] <= 1e-12 and worst["var"] <= 1e-12
    assert worst["sums"] <= 1e-10 and worst["bwd"] <= 1e-9


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_against_enumeration(T):
    rng = np.random.default_rng(570 + T)
    seen_none = 0
    for U in range(4):
        for band in range(1, U + 2):
            w = B.width(T, U, band)
            for _ in range(6):
                b, e = rand64(rng, T, U)
                lo = Q.random_windows(rng, T, U, w)
                assert B.valid(T, U, w, lo)
                bb, eb = B.cut(b, lo, w), B.cut(e, lo, w)
                got = Q.posteriors(bb, eb, lo, U)
                with np.errstate(all="ignore"):           # (enumeration of a lattice without a path divides -inf by -inf)
                    ll, ob, oe = P.brute(B.spread(bb, lo, U), B.spread(eb, lo, U), U)
                if ll == -np.inf:
                    seen_none += 1
                    check_no_path(got, T, w, U)
                    continue
                assert abs(got["loglik"] - ll) <= 1e-12 and abs(got["loglik_bwd"] - ll) <= 1e-12
                assert np.abs(got["occ_b"] - B.cut(ob, lo, w)).max() <= 1e-12 and np.abs(got["occ_e"] - B.cut(oe, lo, w)).max() <= 1e-12
                assert abs(B.cut(ob, lo, w).sum() - ob.sum()) <= 1e-12 and abs(B.cut(oe, lo, w).sum() - oe.sum()) <= 1e-12
                assert Q.sum_invariants(got["occ_b"], got["occ_e"], lo, U) <= 1e-10
    assert T < 3 or seen_none > 0                         # random windows of three frames or more do disconnect


def test_disconnected_windows():
    rng = np.random.default_rng(34)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # no warning raised on the way to the sentinel values
        b, e = rand64(rng, 3, 4)                          # column 2 belongs to no frame
        lo = [0, 0, 3]
        assert B.valid(3, 4, 2, lo)
        check_no_path(Q.posteriors(B.cut(b, lo, 2), B.cut(e, lo, 2), lo, 4), 3, 2, 4)
        b, e = rand64(rng, 2, 1)                          # the only valid windows of (2, 1, 1) leave no path
        lo = [0, 1]
        assert B.valid(2, 1, 1, lo) and B.linear(2, 1, 1) == lo
        r = Q.posteriors(B.cut(b, lo, 1), B.cut(e, lo, 1), lo, 1)
        check_no_path(r, 2, 1, 1)
        assert r["loglik_bwd"] == -np.inf


def test_no_labels_and_single_frame():
    rng = np.random.default_rng(10)
    b, e = rand64(rng, 5, 0)                              # U = 0: w = 1, the path is five blanks
    r = Q.posteriors(b, e, [0] * 5, 0)
    assert r["loglik"] == float(np.asarray(b, np.float64).sum()) and np.all(r["occ_b"] == 1) and np.all(r["occ_e"] == 0)
    assert r["tok_mean"].shape == (0,)
    b, e = rand64(rng, 1, 3)                              # T = 1: w = U + 1, three emissions and the final blank
    assert B.width(1, 3, 2) == 4
    r = Q.posteriors(b, e, [0], 3)
    assert r["loglik"] == float(e[0, :3].astype(np.float64).sum() + b[0, 3])
    assert r["occ_e"].tolist() == [[1, 1, 1, 0]] and r["occ_b"].tolist() == [[0, 0, 0, 1]]
    assert r["tok_mean"].tolist() == [0, 0, 0] and r["tok_var"].tolist() == [0, 0, 0] and r["tok_peak_frame"].tolist() == [0, 0, 0]


def test_minus_inf_inside_the_band():
    rng = np.random.default_rng(77)
    T, U, band = 9, 7, 3
    b, e = rand64(rng, T, U)
    lo = B.linear(T, U, band)
    bb, eb = B.cut(b, lo, band).copy(), B.cut(e, lo, band).copy()
    eb[0, 0] = -np.inf                                    # label 1 cannot be emitted on frame 0
    bb[4, 1] = -np.inf
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = Q.posteriors(bb, eb, lo, U)
    ref = P.posteriors(B.spread(bb, lo, U), B.spread(eb, lo, U), U)
    assert np.isfinite(got["loglik"]) and got["loglik"] == ref["loglik"]
    assert got["occ_e"][0, 0] == 0 and got["occ_b"][4, 1] == 0
    assert np.array_equal(got["occ_b"], B.cut(ref["occ_b"], lo, band)) and np.array_equal(got["occ_e"], B.cut(ref["occ_e"], lo, band))
    assert Q.sum_invariants(got["occ_b"], got["occ_e"], lo, U) <= 1e-10
    for k in got:
        assert not np.any(np.isnan(got[k])), k
