"""The banded lattice without a GPU: the float64 reference of tests/lattice_band_ref.py against tests/lattice_ref.py and against the
enumeration of every in-band path; lasr_band_windows through the library against the Python arithmetic (the planted-path fixture,
random inputs, the argument checks); the same header stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/c/band_windows_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lattice_band_ref as B
import lattice_ref as R
from libreasr_amd import _native as N


def _lib():
    import __graft_entry__ as graft
    graft.build()
    return N.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def native_windows(T, U, band, frames=None, lo=None):
    """-> (rc, lo_out [T] (guard word behind it checked), touch)"""
    out = np.full(T + 1, -7, np.int32)
    touch = C.c_int(-7)
    fr = None if frames is None else np.array(list(frames) + [0], np.int32)       # (never null: U = 0 still recentres)
    cur = None if lo is None else np.array(lo, np.int32)
    rc = _lib().lasr_band_windows(T, U, band, _p(fr), _p(cur), _p(out), C.byref(touch))
    assert out[T] == -7
    return rc, out[:T].tolist(), touch.value


def random_lattice(rng, T, U):
    return (-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32), -(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32))


def random_windows(rng, T, U, w):
    """valid windows: sorted random starts with both ends pinned"""
    if T == 1:
        return [0]
    lo = sorted(int(v) for v in rng.integers(0, U + 2 - w, T))
    lo[0], lo[-1] = 0, U + 1 - w
    return lo


def random_path(rng, T, U):
    return sorted(int(v) for v in rng.integers(0, T, U))


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_band_windows", "lasr_align_band_pcm", "lasr_align_band_feats", "lasr_lattice_band_dp"} <= names
    import inspect
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    for meth in ("band_windows", "lattice_band_dp"):
        assert callable(getattr(Engine, meth, None)), meth
    for meth in ("align_pcm", "align_feats"):
        ps = inspect.signature(getattr(Engine, meth)).parameters
        assert ps["band"].default is None and ps["max_passes"].default == 1 and ps["windows"].default is None
    ps = inspect.signature(LibreASR.align).parameters
    assert ps["band"].default is None and ps["max_passes"].default == 4
    lib = _lib()
    assert lib.lasr_lattice_band_dp(None, None, None, None, None, None, None, 1, None, None, None) == N.LASR_EINVAL   # no context: an error code
    assert lib.lasr_align_band_feats(None, None, 0, None, None, None, None, 4, 1, *([None] * 10)) == N.LASR_EINVAL
    lo, touch = Engine.band_windows(5, 8, 3)                           # host only: no engine needed
    assert lo.tolist() == B.linear(5, 8, 3) and touch == 0


# ------------------------------------------------------------------------------- the reference itself
def test_full_width_band_is_the_full_lattice():
    rng = np.random.default_rng(56)
    for T, U in [(1, 0), (1, 3), (5, 0), (2, 1), (3, 2), (9, 7), (12, 20)]:
        b, e = random_lattice(rng, T, U)
        lo = B.linear(T, U, U + 1)
        assert lo == [0] * T and B.width(T, U, U + 1) == U + 1 and B.width(T, U, U + 50) == U + 1
        assert B.forward(b, e, lo, U) == R.forward(b, e, U)
        assert B.viterbi(b, e, lo, U) == R.viterbi(b, e, U)


def in_band(T, U, w, lo, frames):
    c = B.counts(T, U, frames)
    return all(lo[t] <= c[t] and c[t + 1] < lo[t] + w for t in range(T))


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_reference_against_enumeration(T):
    rng = np.random.default_rng(100 + T)
    seen_cut = 0
    for U in range(4):
        for band in range(1, U + 2):
            w = B.width(T, U, band)
            for _ in range(6):
                b, e = random_lattice(rng, T, U)
                lo = random_windows(rng, T, U, w)
                assert B.valid(T, U, w, lo)
                scores = [R.path_score(b, e, list(fr)) for fr in R.all_paths(T, U) if in_band(T, U, w, lo, fr)]
                seen_cut += len(scores) < len(list(R.all_paths(T, U)))
                bb, eb = B.cut(b, lo, w), B.cut(e, lo, w)
                ll, (v, fr) = B.forward(bb, eb, lo, U), B.viterbi(bb, eb, lo, U)
                if not scores:
                    assert ll == -np.inf and v == -np.inf and fr == [-1] * U
                    continue
                assert abs(ll - float(np.logaddexp.reduce(scores))) <= 1e-12
                assert abs(v - max(scores)) <= 1e-12
                assert in_band(T, U, w, lo, fr) and abs(R.path_score(b, e, fr) - v) <= 1e-12
                assert ll <= R.forward(b, e, U) + 1e-12 and v <= R.viterbi(b, e, U)[0] + 1e-12
    assert T == 1 or seen_cut > 0                                       # some band really removed paths


def test_band_loglik_is_below_the_full_one():
    rng = np.random.default_rng(77)
    for T, U, band in [(20, 14, 4), (30, 9, 3), (7, 25, 6), (40, 40, 1)]:
        b, e = random_lattice(rng, T, U)
        w = B.width(T, U, band)
        for lo in (B.linear(T, U, band), random_windows(rng, T, U, w)):
            ll = B.forward(B.cut(b, lo, w), B.cut(e, lo, w), lo, U)
            assert ll <= R.forward(b, e, U) and not np.isnan(ll)
            assert B.viterbi(B.cut(b, lo, w), B.cut(e, lo, w), lo, U)[0] <= ll + 1e-12


def test_disconnected_windows():
    T, U, w = 3, 4, 2
    lo = [0, 0, 3]                                                      # column 2 belongs to no frame
    assert B.valid(T, U, w, lo)
    b, e = random_lattice(np.random.default_rng(3), T, U)
    with np.errstate(all="raise"):                                      # no inf - inf on the way
        ll = B.forward(B.cut(b, lo, w), B.cut(e, lo, w), lo, U)
        v, fr = B.viterbi(B.cut(b, lo, w), B.cut(e, lo, w), lo, U)
    assert ll == -np.inf and v == -np.inf and fr == [-1] * U
    out = B.pass_loop(b, e, U, w, 4, lo)
    assert len(out) == 1 and out[0][3] == 0                             # touch 0: the loop ends, the windows stay


# ------------------------------------------------------------------------------- lasr_band_windows
@pytest.mark.parametrize("T,U,band,seed", B.PLANTED)
def test_planted_path_fixture(T, U, band, seed):
    b, e, planted = B.planted(T, U, band, seed)
    assert np.all(b * 64 == np.round(b * 64)) and np.all(e * 64 == np.round(e * 64))
    v, fr = R.viterbi(b, e, U)
    assert fr == planted and v == -(T + U) / 64.0                       # the planted path is the full lattice's best
    w = B.width(T, U, band)
    assert not in_band(T, U, w, B.linear(T, U, band), planted)          # the linear windows do not contain it
    passes = B.pass_loop(b, e, U, band, B.PLANTED_MAX_PASSES)
    print(f"planted ({T}, {U}, {band}): {len(passes)} passes, scores {[p[1] for p in passes]}")
    assert len(passes) <= B.PLANTED_MAX_PASSES and passes[-1][3] == 0 and passes[-1][2] == planted
    rc, lo0, touch = native_windows(T, U, band)
    assert rc == N.LASR_OK and lo0 == passes[0][0] and touch == 0
    for lo, _, frames, touch in passes:                                 # every pass: the library's windows and touch are the reference's
        want, want_touch = B.recentre(T, U, band, frames, lo)
        rc, got, got_touch = native_windows(T, U, band, frames, lo)
        assert rc == N.LASR_OK and got == want and got_touch == want_touch == touch
    for (lo, _, frames, _), nxt in zip(passes, passes[1:]):
        assert native_windows(T, U, band, frames, lo)[1] == nxt[0]


def test_windows_random_inputs():
    rng = np.random.default_rng(21)
    n_touch = 0
    for _ in range(400):
        T, U, band = int(rng.integers(1, 50)), int(rng.integers(0, 40)), int(rng.integers(1, 14))
        w = B.width(T, U, band)
        rc, lo, touch = native_windows(T, U, band)
        assert rc == N.LASR_OK and lo == B.linear(T, U, band) and B.valid(T, U, w, lo) and touch == 0
        cur = random_windows(rng, T, U, w)
        fr = random_path(rng, T, U)
        rc, new, touch = native_windows(T, U, band, fr, cur)
        assert rc == N.LASR_OK and B.valid(T, U, w, new)
        assert (new, touch) == B.recentre(T, U, band, fr, cur)
        n_touch += touch
    assert 0 < n_touch < 400


def test_windows_argument_checks():
    fr, lo = [0, 1, 1], [0, 0, 1, 2]                                    # T = 4, U = 3, band = 2
    assert native_windows(4, 3, 2, fr, lo)[0] == N.LASR_OK
    assert native_windows(0, 3, 2, fr, lo)[0] == N.LASR_EINVAL
    lib = _lib()
    out, f, l = np.zeros(4, np.int32), np.array(fr, np.int32), np.array(lo, np.int32)
    assert lib.lasr_band_windows(4, -1, 2, _p(f), _p(l), _p(out), None) == N.LASR_EINVAL
    assert lib.lasr_band_windows(4, 3, 0, _p(f), _p(l), _p(out), None) == N.LASR_EINVAL
    assert lib.lasr_band_windows(4, 3, -2, None, None, _p(out), None) == N.LASR_EINVAL
    assert lib.lasr_band_windows(4, 3, 2, _p(f), _p(l), None, None) == N.LASR_EINVAL
    assert lib.lasr_band_windows(4, 3, 2, _p(f), None, _p(out), None) == N.LASR_EINVAL      # a path without the windows it was found in
    assert lib.lasr_band_windows(4, 3, 2, _p(f), _p(l), _p(out), None) == N.LASR_OK         # touch is optional
    for bad in ([2, 1, 1], [0, 1, 4], [-1, 1, 1]):                      # decreasing; outside [0, T)
        assert native_windows(4, 3, 2, bad, lo)[0] == N.LASR_EINVAL
    for bad in ([1, 1, 1, 2], [0, 1, 0, 2], [0, 1, 2, 1], [0, 1, 3, 2], [0, -1, 1, 2]):     # lo[0], order, lo[T-1], range
        assert native_windows(4, 3, 2, fr, bad)[0] == N.LASR_EINVAL


def test_band_windows_under_asan_ubsan(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the image"
    exe = str(tmp_path / "band_windows_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(root, "tests", "c", "band_windows_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "band_windows_check: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
