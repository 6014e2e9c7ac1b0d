"""Beam records without a GPU: the restatement of the spec that the GPU tests compare against, and the host's hypothesis tree.

  * tests/beam_records_ref.py:beam_frame_rec == oracle/rnnt_oracle.py:_beam_frame -- every hypothesis, `y` and `score` equal (==, not
    close: the same float operations in the same order) after every frame, offline and streamed, with and without an LM; and its
    records are well-formed (one per token, the frame it was emitted on, a log p that sums -- with the blanks' -- to the score).
  * libreasr_amd/csrc/lasr_beamhist.hip.h under AddressSanitizer + UndefinedBehaviorSanitizer (tests/c/beamhist_check.cpp): the only
    place where the tree's compaction runs (the engine's threshold of 2^18 nodes is out of reach of any GPU test).
  * the margin rule's cap: of the 24 (shape, width, stream) cases the GPU tests compare rank by rank, at most 3 may fall back."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import beam_records_ref as R
from oracle import rnnt_oracle as O


def _same(spec, mine):
    assert len(spec) == len(mine)
    for a, b in zip(spec, mine):
        assert a["y"] == b["y"] and a["score"] == b["score"], (a["y"], b["y"], a["score"], b["score"])
        assert len(b["r"]) == len(b["y"])
        fr = [f for f, _ in b["r"]]
        assert fr == sorted(fr)
        assert all(np.isfinite(lp) and lp <= 0 for _, lp in b["r"])


@pytest.mark.parametrize("name,W,lm", [("tiny", 2, None), ("tiny", 4, None), ("tiny", 8, None), ("tiny_lstm", 4, None),
                                       ("tiny", 2, "tiny_lm")])
def test_restatement_equals_the_spec_offline(name, W, lm):
    m = R.model(name, lm)[0]
    pcm = R.offline_pcm(name, R.LM_PCM_SEED if lm else 1234)
    for i, p in enumerate(pcm):
        feats = O.features_offline(p)
        enc, _ = m.encoder(feats[None])
        spec, mine = m.beam_init(), R.beam_init_rec(m)
        for t in range(enc.shape[1]):
            ms, mm = [], []
            spec = m._beam_frame(spec, enc[0, t], W, 3, ms)
            mine = R.beam_frame_rec(m, mine, enc[0, t], t, W, 3, mm)
            assert ms == mm
            _same(spec, mine)
            assert all(f <= t for h in mine for f, _ in h["r"])
            assert all(np.bincount([f for f, _ in h["r"]], minlength=1).max() <= 3 for h in mine)
        # the records' log p are the non-blank terms of the score: what is left are the blanks' (<= 0)
        for h in mine:
            assert h["score"] - sum(lp for _, lp in h["r"]) <= 1e-9
        # the cached reference of the GPU tests is this very computation
        assert [h[0] for h in R.offline_ref(name, W, lm, R.LM_PCM_SEED if lm else 1234)[i]["beam"]] == [h[0] for h in R.ranked(mine)]


def test_lm_case_has_a_repick_that_differs_from_the_joints_token():
    """What pins "the token is the fuser's re-pick, log p stays the joint's" on the GPU: in an utterance that the margin rule compares
    in full, a hypothesis holds a token that is NOT the joint's best non-blank one, while its record is that one's log p."""
    ref = R.offline_ref("tiny", 2, "tiny_lm", R.LM_PCM_SEED)
    full = [u for u in ref if u["margin"] >= R.MARGIN]
    assert sum(sum(u["repicked"]) for u in full) > 0, [(u["margin"], u["repicked"]) for u in ref]
    # and the re-pick changed what the beam holds: the same beam without the LM differs
    plain = R.offline_ref("tiny", 2, None, R.LM_PCM_SEED)
    assert any(u["beam"][0][0] != p["beam"][0][0] for u, p in zip(ref, plain))


@pytest.mark.parametrize("name,W", R.SHAPES)
def test_restatement_equals_the_spec_streamed(name, W):
    m = R.model(name)[0]
    ref = R.stream_ref(name, W)
    for i, chunks in enumerate(R.stream_inputs()):
        fe, dec = O.StreamFrontend(), O.StreamBeamDecoder(m, W)
        j = 0
        for ch in chunks:
            o = fe.push(ch)
            if o is None:
                continue
            dec.step(o)
            spec = sorted(range(len(dec.hyps)), key=lambda q: (-dec.hyps[q]["score"], q))
            got = ref[i]["steps"][j]
            assert len(got) == len(spec)
            for (y, fr, lp, sc), q in zip(got, spec):
                assert y == dec.hyps[q]["y"] and sc == dec.hyps[q]["score"]
                assert len(y) == len(fr) == len(lp) and all(0 <= f < ref[i]["T"][j] for f in fr)
            j += 1
        assert j == len(ref[i]["steps"]) == 21
        assert ref[i]["speech"] == 19           # the two last model steps see nothing but the log-mel floor


def test_margin_rule_lets_at_most_three_cases_fall_back():
    """A (shape, width, stream) case is compared in full if the oracle's smallest selection-boundary gap and its smallest gap
    between two kept hypotheses are both >= 1e-3.  Oracle-only, so it is counted here: the cap is a condition on the inputs."""
    fall = []
    for name, W in R.SHAPES:
        for i, u in enumerate(R.offline_ref(name, W)):
            if u["margin"] < R.MARGIN:
                fall.append(("offline", name, W, i, u["margin"]))
        for i, s in enumerate(R.stream_ref(name, W)):
            if R.full_upto(s) < s["speech"]:
                fall.append(("streamed", name, W, i, min(s["margin"][:s["speech"]])))
    print("cases below the margin:", fall)
    assert len(fall) <= 3, fall


def test_host_tree_under_asan_ubsan(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the image"
    exe = str(tmp_path / "beamhist_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(root, "tests", "c", "beamhist_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "beamhist_check: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
