"""Per-token alignment records, CPU side: the new calls are bound and exposed, and the helper that the GPU tests
(test_gpu_alignment.py) take their expected (frame, log p) from is pinned to the numpy oracle.

The oracle returns the logits of every joint evaluation (return_logits=True) but not where each one happened; `derive` replays
the greedy state machine of Transducer.decode_greedy / transcribe_stream over them (models.py:405-443, 530-571): a blank
decision, or the max_iters-th evaluation of a frame, moves on to the next frame."""
import inspect

import numpy as np
import pytest

from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O

F32 = np.float32
LENS = [48000, 32311, 9000]          # ragged: 3.0 s, 2.02 s (no multiple of hop or chunk), 0.56 s (too quiet a start to emit)


def derive(outs, T, max_iters, blank):
    """outs: logits [V] of every joint evaluation, in order; T frames.  -> (records, t_end, evals, logps): per emitted token
    (frame, log p), the frame cursor after the last evaluation, evaluations per frame, log p of EVERY decision.  log p = the
    log-softmax at the argmax in the oracle's own float32 arithmetic (OracleTransducer.joint_logp)."""
    t, it = 0, 0
    recs, evals, logps = [], [0] * T, []
    for z in outs:
        assert t < T, "more evaluations than the frames can hold"
        z = np.asarray(z, F32)
        m = z.max(-1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=F32))
        lp = (z - lse).astype(F32)
        a = int(lp.argmax())
        logps.append(float(lp[a]))
        it += 1
        evals[t] += 1
        if a != blank:
            recs.append((t, float(lp[a])))
        if a == blank or it >= max_iters:
            t, it = t + 1, 0
    return recs, t, evals, logps


def utterances():
    pcm = synth.synth_pcm(3, max(LENS), seed=1234)
    return [pcm[i][:n] for i, n in enumerate(LENS)]


_MODELS = {}


def oracle(name):
    if name not in _MODELS:
        cfg = synth.model_cfg(name)
        sd = synth.synth_state_dict(cfg, seed=0)
        _MODELS[name] = O.OracleTransducer(sd, cfg)
    return _MODELS[name]


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_set_alignments", "lasr_fetch_aligned", "lasr_fetch_many_aligned"} <= names
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    for meth in ("set_alignments", "fetch_aligned", "fetch_many_aligned"):
        assert callable(getattr(Engine, meth, None)), meth
    assert "return_alignment" in inspect.signature(LibreASR.transcribe).parameters
    assert "return_alignment" in inspect.signature(LibreASR.stream).parameters
    import __graft_entry__ as graft
    graft.build()
    lib = N.lib()
    for meth in ("lasr_set_alignments", "lasr_fetch_aligned", "lasr_fetch_many_aligned"):
        assert hasattr(lib, meth)
    assert lib.lasr_set_alignments(None, 1) == N.LASR_EINVAL          # no context: an error code, nothing dereferenced


@pytest.mark.parametrize("name", ["tiny", "tiny_lstm", "tiny_soft"])
def test_derive_is_pinned_to_the_offline_oracle(name):
    m = oracle(name)
    ntok, capped, multi = [], 0, 0
    for p in utterances():
        feats = O.features_offline(p)
        T = feats.shape[0]
        y, neg_logp, score, iters_all, outs = m.decode_greedy(feats, max_iters=3, return_logits=True)
        recs, t_end, evals, logps = derive(outs, T, 3, m.blank)
        assert t_end == T
        assert len(recs) == len(y)
        assert evals == list(iters_all)
        assert abs(-float(np.sum(np.asarray(logps, np.float64))) - neg_logp) < 1e-6
        frames = [f for f, _ in recs]
        assert frames == sorted(frames) and all(0 <= f < T for f in frames)
        per = np.bincount(np.asarray(frames, np.int64), minlength=T)
        assert per.max(initial=0) <= 3
        # the engine's alignment_score follows from the frames alone: iters = ntok + 1, or max_iters when the cap was hit
        it = np.where(per == 3, 3, per + 1)
        assert list(it) == list(iters_all)
        assert abs((it.sum() - (it == 1).sum()) / (it.sum() + 1e-4) - score) < 1e-12
        ntok.append(len(y))
        capped += int((per == 3).sum())
        multi += int((per > 1).sum())
    # what these inputs cover: bursts (several tokens on a frame), a row without tokens and, on tiny_lstm, the per-frame cap
    assert ntok[2] == 0 and ntok[0] >= 12
    assert multi >= 3
    if name == "tiny_lstm":
        assert capped >= 9


@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_derive_is_pinned_to_the_stream_oracle(name):
    m = oracle(name)
    pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
    fe, dec = O.StreamFrontend(), m.stream_decoder()
    n = 0
    for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=10):
        o = fe.push(ch)
        if o is None:
            continue
        y_seq, outs = dec.step(o, return_logits=True)
        recs, t_end, evals, _ = derive(outs, o.shape[0], 10, m.blank)
        assert t_end == o.shape[0]
        assert len(recs) == len(y_seq)
        assert all(1 <= e <= 10 for e in evals)
        n += len(recs)
    assert n == len(dec.y) and n >= 8
