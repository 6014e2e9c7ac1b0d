"""The float64 lattice reference (tests/lattice_ref.py) that the GPU tests of lasr_align_* / lasr_lattice_dp take their expected values
from: both recursions against brute-force enumeration of every path, the tie rule, U = 0, and their relation to the numpy oracle's
greedy decode.  Also: the new calls are bound and exposed."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import lattice_ref as R
from libreasr_amd import _native as N
from oracle import rnnt_oracle as O
from test_alignment_cpu import oracle, utterances


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_align_pcm", "lasr_align_feats", "lasr_lattice_dp"} <= names
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    for meth in ("align_pcm", "align_feats", "lattice_dp"):
        assert callable(getattr(Engine, meth, None)), meth
    assert "lattice" in inspect.signature(Engine.align_pcm).parameters
    for meth in ("align", "score"):
        assert callable(getattr(LibreASR, meth, None)), meth
    import __graft_entry__ as graft
    graft.build()
    lib = N.lib()
    for meth in ("lasr_align_pcm", "lasr_align_feats", "lasr_lattice_dp"):
        assert hasattr(lib, meth)
    assert lib.lasr_lattice_dp(None, None, None, None, None, 1, None, None, None) == N.LASR_EINVAL      # no context: an error code


def test_lattice_tables_under_asan_ubsan(tmp_path):
    """Layout and table image of the full, banded and tree lattice (lasr_lattice_tables.hip.h, standard C++): every device view inside
    the image, none overlapping, aligned, reading back its input; offsets against formulas written out in the program."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the image"
    exe = str(tmp_path / "lattice_tables_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(root, "tests", "c", "lattice_tables_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lattice_tables_check: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def brute(b, e, U):
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    scores = [R.path_score(b, e, list(fr)) for fr in R.all_paths(b.shape[0], U)]
    return float(np.logaddexp.reduce(scores)), float(max(scores))


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("U", [0, 1, 2, 3])
def test_recursions_against_every_path(T, U):
    rng = np.random.default_rng(100 * T + U)
    for _ in range(5):
        b = -rng.random((T, U + 1)).astype(np.float32) * 8
        e = -rng.random((T, U + 1)).astype(np.float32) * 8
        ll, best = brute(b, e, U)
        assert abs(R.forward(b, e, U) - ll) < 1e-12
        v, frames = R.viterbi(b, e, U)
        assert abs(v - best) < 1e-12
        assert len(frames) == U and frames == sorted(frames) and all(0 <= f < T for f in frames)
        assert abs(R.path_score(b, e, frames) - v) < 1e-12
        assert v <= ll + 1e-12


def test_tie_takes_the_blank_predecessor():
    # every path of an all-equal lattice has the same score: going back from (T-1, U) the blank predecessor is taken while there is
    # one, so every label lands on frame 0
    T, U = 4, 3
    b = np.full((T, U + 1), -0.5, np.float32)
    e = np.full((T, U + 1), -0.5, np.float32)
    v, frames = R.viterbi(b, e, U)
    assert v == -0.5 * (T + U) and frames == [0, 0, 0]
    # a strictly better emission predecessor does win
    e2 = e.copy()
    e2[2, 1] = -0.25
    v2, frames2 = R.viterbi(b, e2, U)
    assert v2 == -0.5 * (T + U) + 0.25 and frames2[1] == 2


def test_no_labels():
    rng = np.random.default_rng(7)
    b = -rng.random((5, 1)).astype(np.float32)
    e = np.zeros((5, 1), np.float32)
    want = float(np.asarray(b, np.float64).sum())
    assert R.forward(b, e, 0) == pytest.approx(want, abs=1e-12)
    v, frames = R.viterbi(b, e, 0)
    assert v == pytest.approx(want, abs=1e-12) and frames == []


def test_lattice_against_the_greedy_oracle():
    """On the oracle's own greedy tokens: viterbi <= loglik; and where greedy hit no per-frame cap, its path is a lattice path, so
    the best path scores at least -neg_logp."""
    m = oracle("tiny")
    uncapped = 0
    for p in utterances():
        feats = O.features_offline(p)
        y, neg_logp, _, iters = m.decode_greedy(feats, max_iters=3)
        b, e = R.lattice(m, feats, y)
        assert b.shape == (feats.shape[0], len(y) + 1) and np.all(e[:, len(y)] == 0)
        ll = R.forward(b, e, len(y))
        v, frames = R.viterbi(b, e, len(y))
        assert v <= ll + 1e-9
        per = np.bincount(np.asarray(frames, np.int64), minlength=feats.shape[0])
        # a frame is capped when its 3rd evaluation was non-blank: greedy emitted 3 tokens on it
        emitted = _tokens_per_frame(m, feats, 3)
        if max(emitted, default=0) < 3:
            uncapped += 1
            assert v >= -neg_logp - 1e-4, (v, -neg_logp)
        assert per.sum() == len(y)
    assert uncapped >= 2           # T 25 / U 1 and T 6 / U 0


def _tokens_per_frame(m, feats, max_iters):
    from test_alignment_cpu import derive
    y, _, _, _, outs = m.decode_greedy(feats, max_iters=max_iters, return_logits=True)
    recs, _, _, _ = derive(outs, feats.shape[0], max_iters, m.blank)
    return list(np.bincount(np.asarray([f for f, _ in recs], np.int64), minlength=feats.shape[0]))


def test_long_uncapped_transcript():
    """U >= 5 without a capped frame: the transcript of decode_greedy(max_iters=16); no frame may have hit that cap."""
    m = oracle("tiny")
    feats = O.features_offline(utterances()[0])
    y, neg_logp, _, iters = m.decode_greedy(feats, max_iters=16)
    assert len(y) >= 5
    assert max(_tokens_per_frame(m, feats, 16)) < 16       # no frame hit the cap: greedy's path is a path of the lattice
    b, e = R.lattice(m, feats, y)
    ll = R.forward(b, e, len(y))
    v, frames = R.viterbi(b, e, len(y))
    assert v <= ll + 1e-9
    assert v >= -neg_logp - 1e-4, (v, -neg_logp)
