"""Non-finite audio through the decode loops (needs an MI355X): one of four streams carries a NaN, an Inf or a huge finite sample
at sample 16000 of 2 s of audio.  The poisoned stream must decide as the oracle does (argmax of a NaN row = 0: quiet at blank 0,
token 0 up to the symbol cap at a nonzero blank), every id it hands out must lie in [0, V), its three neighbours must not
notice -- bit for bit against a run of the same engine shape in which that slot carries the clean audio -- and reset(slot, 15)
must give the slot back.  Every equality is exact.  Cases and oracle runs: tests/nonfinite_cases.py (pinned on the CPU by
test_nonfinite_cpu.py).

This file relies on both layers of the contract of DESIGN.md ("Non-finite input"): every selection kernel yields an index in
[0, V) and every gather indexed by a device-resident token clamps it.  Every wait is bounded: a decode loop that never finishes
fails the test instead of hanging it."""
import time

import numpy as np
import pytest

import nonfinite_cases as NC
from libreasr_amd import synth

pytestmark = pytest.mark.gpu

N_SLOTS = 4
BAD_SLOT = 1               # position of the poisoned stream among the four
KINDS3 = ["nan", "inf", "huge"]
V = 64
WAIT_S = 10.0


def make(sd, cfg, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    return Engine(sd, cfg, max_streams=16, **kw)


def audio(kind):
    """four utterances, stream BAD_SLOT = utterance NC.ROW, poisoned when kind is not None"""
    rows = [0, NC.ROW, 1, 2]
    assert rows[BAD_SLOT] == NC.ROW
    pcm = [NC.clean_pcm()[r] for r in rows]
    if kind is not None:
        pcm[BAD_SLOT] = NC.poisoned(kind)
    return pcm


def chunk_rows(pcm):
    ch = [NC.chunks(p) for p in pcm]
    assert len({len(c) for c in ch}) == 1
    return [np.stack([c[k] for c in ch]) for k in range(len(ch[0]))]


def fetch_step(eng, slots, mode):
    if mode == "aligned":
        out = []
        for s in slots:
            tok, fr, lp, neg_logp, align = eng.fetch_aligned(s)
            out.append((tok, fr.tobytes(), NC.bits(lp).tobytes(), neg_logp, align))
        return out
    if mode == "nbest":
        return [[(t, fr.tobytes(), NC.bits(lp).tobytes(), sc) for t, fr, lp, sc in eng.fetch_nbest(s)] for s in slots]
    return [(eng.fetch(s)[0],) for s in slots]


def run_sync(eng, slots, pcm, mode="aligned"):
    """-> per model step, per slot: what fetch_step hands out"""
    hist = []
    for ch in chunk_rows(pcm):
        eng.push(slots, ch)
        if eng.step(slots):
            hist.append(fetch_step(eng, slots, mode))
    return hist


def bounded_wait(eng, slots):
    """wait() for the oldest step once peek says it is decoded for every slot (the poll of test_gpu_parity.py, bounded)"""
    t0 = time.time()
    while True:
        if all(len(eng.peek(s)[0]) >= 1 for s in slots):
            break
        assert time.time() - t0 < WAIT_S, "the decode loop did not finish a submitted step"
    return eng.wait()


def run_pipelined(eng, slots, pcm, lookahead=2, mode="aligned"):
    hist = []
    for ch in chunk_rows(pcm):
        eng.push_submit(slots, ch)
        while eng.pending() > lookahead:
            if bounded_wait(eng, slots):
                hist.append(fetch_step(eng, slots, mode))
    while eng.pending():
        if bounded_wait(eng, slots):
            hist.append(fetch_step(eng, slots, mode))
    return hist


def tokens_of(hist, i):
    return [list(step[i][0]) for step in hist]


def check_neighbours(got, want):
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        for i in range(N_SLOTS):
            if i != BAD_SLOT:
                assert a[i] == b[i], (j, i)
    assert sum(len(step[i][0]) for step in want for i in range(N_SLOTS) if i != BAD_SLOT) > 0


def same_but_frames(again, want):
    """a single-slot run against slot BAD_SLOT of `want`: tokens, log p bits, log p sum and alignment score (the frames count from
    the slot's open and go on across a reset)"""
    assert len(again) == len(want)
    for j, (a, b) in enumerate(zip(again, want)):
        a, b = a[0], b[BAD_SLOT]
        assert (a[0], a[2], a[3], a[4]) == (b[0], b[2], b[3], b[4]), j


def in_range(hist, i, vocab=V):
    ids = [t for s in tokens_of(hist, i) for t in s]
    assert all(0 <= t < vocab for t in ids), ids
    return ids


_CLEAN = {}


def clean_hist(key, build, run):
    """the clean run of an engine shape, once per module: -> hist"""
    if key not in _CLEAN:
        eng = build()
        try:
            slots = [eng.open() for _ in range(N_SLOTS)]
            _CLEAN[key] = run(eng, slots, audio(None))
        finally:
            eng.close()
    return _CLEAN[key]


def tiny_engine(dtype="f32", **kw):
    sd, cfg, _ = NC.tiny()
    eng = make(sd, cfg, dtype=dtype, **kw)
    if kw.get("beam", 1) == 1:
        eng.set_alignments(True)
    else:
        eng.set_beam_records(True)
    return eng


# ------------------------------------------------------------------------------- greedy
@pytest.mark.parametrize("kind", KINDS3)
def test_sync_greedy(kind):
    want = clean_hist("sync f32", tiny_engine, run_sync)
    ref = NC.stream_ref("tiny", kind)
    eng = tiny_engine()
    try:
        slots = [eng.open() for _ in range(N_SLOTS)]
        got = run_sync(eng, slots, audio(kind))
        in_range(got, BAD_SLOT)
        assert tokens_of(got, BAD_SLOT) == ref.steps                 # step by step what the oracle's stream decoder emits
        assert tokens_of(want, BAD_SLOT) == NC.stream_ref("tiny", None).steps
        check_neighbours(got, want)
        # recovery: the clean utterance through the poisoned slot after reset(.., 15) decodes like a fresh engine's
        eng.reset(slots[BAD_SLOT], 15)
        again = run_sync(eng, [slots[BAD_SLOT]], [NC.clean_pcm()[NC.ROW]])
        assert [list(s[0][0]) for s in again] == tokens_of(want, BAD_SLOT)
        same_but_frames(again, want)
    finally:
        eng.close()


def test_pipelined_greedy():
    """push_submit / wait with two steps in flight; the clean run takes the same protocol"""
    want = clean_hist("pipelined f32", tiny_engine, run_pipelined)
    assert [[s[i][0] for i in range(N_SLOTS)] for s in want] == [[s[i][0] for i in range(N_SLOTS)] for s in clean_hist("sync f32", tiny_engine, run_sync)]
    eng = tiny_engine()
    try:
        slots = [eng.open() for _ in range(N_SLOTS)]
        got = run_pipelined(eng, slots, audio("nan"))
        in_range(got, BAD_SLOT)
        assert tokens_of(got, BAD_SLOT) == NC.stream_ref("tiny", "nan").steps
        check_neighbours(got, want)
        eng.reset(slots[BAD_SLOT], 15)
        again = run_pipelined(eng, [slots[BAD_SLOT]], [NC.clean_pcm()[NC.ROW]])
        assert [list(s[0][0]) for s in again] == tokens_of(want, BAD_SLOT)
        same_but_frames(again, want)
    finally:
        eng.close()


def test_sync_greedy_bf16():
    """bf16 operands: the engine's tokens follow the bf16 oracle only approximately on clean audio (test_gpu_bf16.py), so the
    poisoned stream is held against the same engine's clean run: the steps before the first poisoned one are equal, that step
    holds a prefix, every later step is empty.  The first poisoned step is the oracle's (the front-end is float32)"""
    build = lambda: tiny_engine("bf16")
    want = clean_hist("sync bf16", build, run_sync)
    k = NC.onset_step("nan")
    eng = build()
    try:
        slots = [eng.open() for _ in range(N_SLOTS)]
        got = run_sync(eng, slots, audio("nan"))
        in_range(got, BAD_SLOT)
        g, w = tokens_of(got, BAD_SLOT), tokens_of(want, BAD_SLOT)
        assert g[:k] == w[:k] and g[k] == w[k][:len(g[k])] and all(s == [] for s in g[k + 1:])
        check_neighbours(got, want)
        eng.reset(slots[BAD_SLOT], 15)
        again = run_sync(eng, [slots[BAD_SLOT]], [NC.clean_pcm()[NC.ROW]])
        assert [list(s[0][0]) for s in again] == tokens_of(want, BAD_SLOT)
        same_but_frames(again, want)
    finally:
        eng.close()


def test_nonzero_blank():
    """blank = V - 1: behind the poison the stream emits token 0 up to the cap on every frame, exactly as the oracle"""
    mod, cap = NC.nonzero_blank(), 3
    ref = NC.stream_ref("nz", "nan", cap)

    def build():
        eng = make(mod.sd, mod.cfg, max_iters_stream=cap, blank=mod.blank, bos=mod.bos)
        eng.set_alignments(True)
        return eng
    want = clean_hist("sync nz", build, run_sync)
    eng = build()
    try:
        slots = [eng.open() for _ in range(N_SLOTS)]
        got = run_sync(eng, slots, audio("nan"))
        in_range(got, BAD_SLOT, mod.V)
        assert tokens_of(got, BAD_SLOT) == ref.steps
        assert tokens_of(got, BAD_SLOT)[-1] == [0] * (cap * ref.T[-1])
        check_neighbours(got, want)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- LM shallow fusion
@pytest.mark.parametrize("int8", [False, True], ids=["fp32", "int8"])
def test_lm_attached(int8):
    """tiny_soft + tiny_lm.  (The LM's state has no debug read-out, so its staying finite is not asserted directly; it only ever
    sees token embeddings, and the recovery run below would show a NaN left in it.)"""
    cfg = synth.model_cfg("tiny_soft")
    sd = synth.synth_state_dict(cfg, seed=0)

    def build():
        eng = make(sd, cfg)
        eng.attach_lm(synth.synth_lm_state_dict("tiny_lm"), int8=int8)
        eng.set_alignments(True)
        return eng
    want = clean_hist(("lm", int8), build, run_sync)
    k = NC.onset_step("nan")
    eng = build()
    try:
        slots = [eng.open() for _ in range(N_SLOTS)]
        got = run_sync(eng, slots, audio("nan"))
        in_range(got, BAD_SLOT)
        g, w = tokens_of(got, BAD_SLOT), tokens_of(want, BAD_SLOT)
        assert g[:k] == w[:k] and g[k] == w[k][:len(g[k])] and all(s == [] for s in g[k + 1:])
        assert sum(len(s) for s in g) > 0
        check_neighbours(got, want)
        eng.reset(slots[BAD_SLOT], 15)
        again = run_sync(eng, [slots[BAD_SLOT]], [NC.clean_pcm()[NC.ROW]])
        assert [list(s[0][0]) for s in again] == tokens_of(want, BAD_SLOT)
        same_but_frames(again, want)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- beam search
def test_beam4():
    """every hypothesis of a poisoned beam stream dies on the first non-finite frame (its candidates' scores are NaN: none
    is selected); from that model step on fetch_nbest returns an empty list.  (The parents of a round reach the host only as
    indices into its W current paths: an index outside [0, W) would fail there, not return.)"""
    W = 4
    build = lambda: tiny_engine(beam=W)
    run = lambda eng, slots, pcm: run_sync(eng, slots, pcm, mode="nbest")
    want = clean_hist("beam4", build, run)
    k = NC.onset_step("nan")
    eng = build()
    try:
        slots = [eng.open() for _ in range(N_SLOTS)]
        got = run(eng, slots, audio("nan"))
        assert len(got) == len(want)
        for j, step in enumerate(got):
            hyps = step[BAD_SLOT]
            assert len(hyps) <= W
            assert all(0 <= t < V for h in hyps for t in h[0])
            if j < k:
                assert hyps == want[j][BAD_SLOT], j
            else:
                assert hyps == [], (j, hyps)
        assert any(len(h[0]) for h in got[k - 1][BAD_SLOT])
        for j, (a, b) in enumerate(zip(got, want)):                  # the neighbours' N-best lists, records and scores
            for i in range(N_SLOTS):
                if i != BAD_SLOT:
                    assert a[i] == b[i], (j, i)
        eng.reset(slots[BAD_SLOT], 15)
        again = run(eng, [slots[BAD_SLOT]], [NC.clean_pcm()[NC.ROW]])
        assert [[h[0] for h in s[0]] for s in again] == [[h[0] for h in s[BAD_SLOT]] for s in want]      # every hypothesis, token for token
    finally:
        eng.close()


# ------------------------------------------------------------------------------- offline
@pytest.mark.parametrize("kind", ["nan", "huge"])
def test_offline(kind):
    """transcribe_pcm over four utterances, one poisoned: the other three equal their solo transcripts, the poisoned one the oracle's"""
    eng = tiny_engine()
    try:
        slots = [eng.open() for _ in range(N_SLOTS)]
        clean = audio(None)
        solo = []
        for i in range(N_SLOTS):
            eng.transcribe_pcm([slots[i]], [clean[i]])
            solo.append(eng.fetch_aligned(slots[i]))
        assert solo[BAD_SLOT][0] == NC.offline_ref("tiny", None)
        eng.transcribe_pcm(slots, audio(kind))
        got = [eng.fetch_aligned(s) for s in slots]
        assert all(0 <= t < V for t in got[BAD_SLOT][0])
        assert got[BAD_SLOT][0] == NC.offline_ref("tiny", kind)
        for i in range(N_SLOTS):
            if i != BAD_SLOT:
                assert got[i][0] == solo[i][0] and len(solo[i][0]) > 0, i
                assert np.array_equal(got[i][1], solo[i][1]) and np.array_equal(NC.bits(got[i][2]), NC.bits(solo[i][2])), i
    finally:
        eng.close()
