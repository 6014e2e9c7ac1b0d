"""What the numpy oracle makes of a non-finite PCM sample (no GPU): the semantics the test_gpu_nonfinite_*.py files lean on.
Cases and references: tests/nonfinite_cases.py."""
import numpy as np
import pytest

import nonfinite_cases as NC
from oracle import rnnt_oracle as O

KINDS = list(NC.BAD)


def test_argmax_semantics():
    """numpy's (and torch's) argmax: NaN is the maximum, the first one wins; a row of -inf gives 0"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    assert int(np.argmax(np.full(64, nan, np.float32))) == 0
    assert int(np.argmax(np.full(64, -inf, np.float32))) == 0
    assert int(np.argmax(np.array([1.0, inf, nan, 5.0, nan], np.float32))) == 2
    assert int(np.argmax(np.array([nan, inf], np.float32))) == 0
    import torch
    assert int(torch.argmax(torch.tensor([1.0, float("inf"), float("nan"), 5.0, float("nan")]))) == 2
    assert int(torch.argmax(torch.full((64,), float("-inf")))) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_logmel_touched_frames(kind):
    """the frames the bad sample reaches are non-finite in all 128 bins, every other frame has the clean audio's bits.  For the
    huge value "reaches" means a non-zero window weight (the property it was chosen for); NaN and Inf poison through the zero
    padding of the window too"""
    clean = NC.clean_pcm()[NC.ROW]
    with np.errstate(all="ignore"):
        got, want = O.logmel(NC.poisoned(kind)), O.logmel(clean)
    touched = NC.touched_frames(kind, NC.POS, NC.N_SAMPLES)
    assert len(touched) == (3 if kind == "huge" else 7), touched
    mask = np.zeros(got.shape[0], bool)
    mask[touched] = True
    assert got.shape == want.shape == (1 + NC.N_SAMPLES // NC.HOP, 128)
    assert not np.isfinite(got[mask]).any()
    assert np.array_equal(NC.bits(got[~mask]), NC.bits(want[~mask]))
    assert np.isfinite(want).all()


def test_huge_value_window_weights():
    """the smallest non-zero Hann weight still overflows the square of the huge value in float32; weight 0 is exactly 0"""
    w = O.hann_periodic(NC.WIN)
    assert w[0] == 0 and (w[1:] > 0).all()
    assert 5e-5 < float(w[1:].min()) < 7e-5
    with np.errstate(all="ignore"):
        assert np.isinf(np.float32((float(w[1:].min()) * NC.HUGE) ** 2))


@pytest.mark.parametrize("kind", KINDS)
def test_stream_goes_quiet(kind):
    """StreamFrontend + stream_decoder: the steps before the first poisoned one are the clean stream's, that step holds a prefix
    of the clean step's tokens, every later step is empty (argmax 0 = blank 0 on NaN rows, forever: the state is carried)"""
    clean, bad, k = NC.stream_ref("tiny", None), NC.stream_ref("tiny", kind), NC.onset_step(kind)
    assert len(clean.steps) == len(bad.steps) == 14
    assert 0 < k < len(clean.steps) - 1
    assert bad.steps[:k] == clean.steps[:k]
    assert bad.steps[k] == clean.steps[k][:len(bad.steps[k])]
    assert all(s == [] for s in bad.steps[k + 1:])
    assert len(bad.tokens) < len(clean.tokens) and len(bad.tokens) > 0                  # a strict, non-empty prefix
    assert all(0 <= v < 64 for v in bad.tokens)


def test_stream_onsets_differ():
    """NaN reaches the stream one log-mel window earlier than the huge value (the zero padding of the Hann window): the two
    transcripts are cut at different tokens, so a front-end that drops the zero-weight samples is told apart"""
    assert NC.stream_ref("tiny", "nan").tokens != NC.stream_ref("tiny", "huge").tokens
    assert NC.stream_ref("tiny", "nan").steps == NC.stream_ref("tiny", "inf").steps == NC.stream_ref("tiny", "ninf").steps


@pytest.mark.parametrize("kind", KINDS)
def test_offline_goes_quiet(kind):
    clean, bad = NC.offline_ref("tiny", None), NC.offline_ref("tiny", kind)
    assert 0 < len(bad) < len(clean) and bad == clean[:len(bad)]


@pytest.mark.parametrize("kind", KINDS)
def test_nonzero_blank_emits_token_zero(kind):
    """blank = V - 1: argmax 0 of a NaN row is a token.  Behind the onset every frame emits token 0 max_iters times, exactly"""
    cap = 3
    mod = NC.nonzero_blank()
    assert mod.blank == mod.V - 1 != 0
    clean, bad, k = NC.stream_ref("nz", None, cap), NC.stream_ref("nz", kind, cap), NC.onset_step(kind)
    assert bad.steps[:k] == clean.steps[:k]
    for j in range(k + 1, len(bad.steps)):
        assert bad.steps[j] == [0] * (cap * bad.T[j]), (j, bad.steps[j])
    tail = bad.steps[k]
    n0 = 0
    while n0 < len(tail) and tail[len(tail) - 1 - n0] == 0:
        n0 += 1
    assert n0 >= cap and n0 % cap == 0                   # whole frames of token 0 close the onset step ...
    assert tail[:len(tail) - n0] == clean.steps[k][:len(tail) - n0]                    # ... behind a prefix of the clean step
    # offline: the encoder is NaN from the first poisoned frame to the end of the utterance
    off_c, off = NC.offline_ref("nz", None, cap), NC.offline_ref("nz", kind, cap)
    z = 0
    while z < len(off) and off[len(off) - 1 - z] == 0:
        z += 1
    assert z >= cap and z % cap == 0 and off[:len(off) - z] == off_c[:len(off) - z]
    assert all(0 <= v < mod.V for v in bad.tokens + off)
