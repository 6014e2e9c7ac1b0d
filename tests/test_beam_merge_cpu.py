"""Beam merging without a GPU: the restatement the GPU tests compare against (tests/beam_merge_ref.py), and the Python plumbing.

  1. with the merge step skipped, frame_merge == beam_records_ref.beam_frame_rec (y, records, score: ==) after every frame, offline
     and streamed;
  2. no collision: in every round, two survivors have equal identities iff they hold equal token lists;
  3. distinctness: at the end of every frame the live hypotheses are pairwise distinct;
  4. exact against enumeration on a two-symbol fake model where nothing is pruned: the merged score of the hypothesis with n tokens
     is the log-sum over all emit / blank sequences with n emissions (1e-12);
  5. upper bound: an uncapped hypothesis's merged score never exceeds the lattice's total for its tokens (1e-9);
  6. the margin rule's caps (how many cases the GPU test may compare by rank 0 + structure only);
  7. the facade's merge= and Engine.set_beam_merge against fakes."""
import itertools
import math

import numpy as np
import pytest

import beam_merge_ref as M
import beam_records_ref as R
import lattice_ref as L
from oracle import rnnt_oracle as O


def _same(rec, mine):
    mine = M.live(mine)
    assert len(rec) == len(mine)
    for a, b in zip(rec, mine):
        assert a["y"] == b["y"] and a["score"] == b["score"] and a["r"] == b["r"], (a["y"], b["y"], a["score"], b["score"])
        assert b["idt"] == M.ident_of(b["y"])


@pytest.mark.parametrize("name,W", M.SHAPES)
def test_without_the_merge_step_it_is_the_records_restatement_offline(name, W):
    m = R.model(name)[0]
    for p in R.offline_pcm(name):
        enc, _ = m.encoder(O.features_offline(p)[None])
        rec, mine = R.beam_init_rec(m), M.beam_init(m)
        for t in range(enc.shape[1]):
            mr, mm = [], []
            rec = R.beam_frame_rec(m, rec, enc[0, t], t, W, 3, mr)
            mine = M.frame_merge(m, mine, enc[0, t], t, W, 3, mm, merge=False)
            assert mr == mm
            _same(rec, mine)
            assert all(h is None for h in mine[len(rec):])          # without merging the dead slots are the tail


@pytest.mark.parametrize("name,W", M.SHAPES)
def test_without_the_merge_step_it_is_the_records_restatement_streamed(name, W):
    ref = R.stream_ref(name, W)
    got = M.stream_run(name, W, merge_at=lambda i, j: False)
    for a, b in zip(ref, got):
        assert a["steps"] == b["steps"] and a["T"] == b["T"] and a["margin"] == b["margin"] and a["speech"] == b["speech"]
        assert len(b["steps"]) == 21


def _watch(case):
    """on_round / on_frame hooks that check 2. and 3. and count"""
    seen = {"rounds": 0, "frames": 0, "dups": 0}

    def on_round(surv):
        seen["rounds"] += 1
        for a, b in itertools.combinations(surv, 2):
            assert (a["idt"] == b["idt"]) == (a["y"] == b["y"]), (case, a["y"], b["y"])
            seen["dups"] += a["y"] == b["y"]

    def on_frame(hyps):
        seen["frames"] += 1
        ys = [tuple(h["y"]) for h in M.live(hyps)]
        assert len(set(ys)) == len(ys), (case, ys)
    return seen, on_round, on_frame


@pytest.mark.parametrize("name,W", M.SHAPES)
def test_no_collision_and_distinct_at_every_frame_end(name, W):
    m = R.model(name)[0]
    merges = []
    for i, p in enumerate(R.offline_pcm(name)):
        enc, _ = m.encoder(O.features_offline(p)[None])
        seen, on_round, on_frame = _watch((name, W, "offline", i))
        hyps, stats = M.beam_init(m), {}
        for t in range(enc.shape[1]):
            hyps = M.frame_merge(m, hyps, enc[0, t], t, W, 3, None, True, on_round, stats)
            on_frame(hyps)
        assert seen["frames"] == enc.shape[1] and seen["rounds"] >= seen["frames"]
        merges.append(stats.get("merges", 0))
        # the cached reference of the GPU tests is this very computation
        assert M.offline_ref(name, W)[i]["beam"] == M.ranked(hyps)
    print(name, W, "merges per utterance:", merges)
    if name == "tiny":
        assert sum(merges) >= 1, merges                             # the inputs exercise the rule
    for i, chunks in enumerate(R.stream_inputs()):
        seen, on_round, on_frame = _watch((name, W, "streamed", i))
        fe, dec = O.StreamFrontend(), M.StreamBeamMerge(m, W)
        dec.on_round, dec.on_frame = on_round, on_frame
        for j, ch in enumerate(chunks):
            o = fe.push(ch)
            if o is not None:
                dec.step(o)
            if j == 12:
                dec.reset()                                         # identities restart: the checks hold across it
        assert seen["frames"] > 0


# ------------------------------------------------------------------------------- 4. exact, against enumeration
class TwoSymbols:
    """blank = 0 and one token.  joint_logp comes from a table indexed by (frame, len(y)); the 'encoder frame' is the frame's index,
    the 'predictor state' the number of tokens."""
    blank, lm, bos = 0, None, 1

    def __init__(self, T, seed):
        z = np.random.default_rng(seed).normal(size=(T, T + 1, 2)) * 1.5
        self.table = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)

    def beam_init(self):
        return [dict(score=0.0, y=[], h_pred=np.zeros((1, 1), np.int64), pstate=0)]

    def predictor(self, toks, pstate):
        return np.full((1, 1), pstate + len(toks), np.int64), pstate + len(toks)

    def joint_logp(self, h_pred, h_enc):
        return self.table[int(h_enc[0, 0]), int(h_pred[0, 0])][None], None


@pytest.mark.parametrize("T,seed", [(3, 0), (3, 1), (4, 2), (4, 3)])
def test_merged_score_equals_enumeration(T, seed):
    m = TwoSymbols(T, seed)
    hyps = M.beam_init(m)
    for t in range(T):
        hyps = M.frame_merge(m, hyps, np.array([t]), t, 8, 1)
    got = {len(h["y"]): h["score"] for h in M.live(hyps)}
    assert len(got) == len(M.live(hyps)) == T + 1                   # nothing pruned: one hypothesis per length
    # the machine's own path cost with max_iters = 1: per frame ONE decision, blank or the token (an emission at the cap pays no blank)
    want = {}
    for choice in itertools.product((0, 1), repeat=T):
        n, s = 0, 0.0
        for t, c in enumerate(choice):
            s += float(m.table[t, n, c])
            n += c
        want.setdefault(n, []).append(s)
    for n in range(T + 1):
        tot = max(want[n]) + math.log(sum(math.exp(s - max(want[n])) for s in want[n]))
        assert abs(got[n] - tot) <= 1e-12, (n, got[n], tot)


# ------------------------------------------------------------------------------- 5. upper bound
@pytest.mark.parametrize("name,W", M.SHAPES)
def test_uncapped_merged_score_is_below_the_lattice_total(name, W):
    m = R.model(name)[0]
    n = 0
    for i, p in enumerate(R.offline_pcm(name)):
        feats = O.features_offline(p)
        u = M.offline_ref(name, W, max_iters=10)[i]
        for (y, _, _, score), capped in zip(u["beam"], u["capped"]):
            if capped:
                continue
            b, e = L.lattice(m, feats, y)
            tot = L.forward(b, e, len(y))
            assert score <= tot + 1e-9, (name, W, i, y, score, tot)
            n += 1
    assert n > 0


# ------------------------------------------------------------------------------- 6. the margin rule's caps
def test_margin_rule_caps():
    off, stre = [], []
    for name, W in M.SHAPES:
        for i, u in enumerate(M.offline_ref(name, W)):
            if u["margin"] < M.MARGIN:
                off.append((name, W, i, u["margin"]))
        for i, s in enumerate(M.stream_ref(name, W)):
            if M.full_upto(s) < s["speech"]:
                stre.append((name, W, i, M.full_upto(s), min(s["margin"][:s["speech"]])))
    print("offline cases below the margin:", off)
    print("streamed cases below the margin (stream, first step below):", stre)
    assert len(off) <= 2, off
    assert len(stre) <= 2, stre


# ------------------------------------------------------------------------------- 7. facade and engine plumbing
class FakeEngine:
    def __init__(self, beam):
        self.beam, self.calls, self.slots = beam, [], set()

        class D:
            chunk, stride, hop, sample_rate = 1280, 8, 160, 16000
        self.desc = D()

    def open(self):
        self.slots.add(0)
        return 0

    def close_slot(self, s):
        self.slots.remove(s)

    def set_beam_merge(self, on=True):
        self.calls.append(("merge", on))

    def set_beam_records(self, on=True):
        self.calls.append(("records", on))

    def transcribe_pcm(self, slots, pcm):
        self.calls.append(("transcribe", len(slots)))

    def push(self, slots, pcm):
        pass

    def step(self, slots):
        return True

    def fetch(self, s):
        return [3, 4], 1.0, 0.0

    def fetch_nbest(self, s, k):
        return [([3, 4], np.array([0, 2]), np.array([-0.5, -0.25], np.float32), -1.5)][:k]


def _facade(eng):
    from libreasr_amd.api import LibreASR

    class Model:
        engine = eng
    return LibreASR(None, None, Model(), None, None)


PCM = np.zeros(16000, np.float32)


def test_facade_merge_argument():
    eng = FakeEngine(4)
    asr = _facade(eng)
    assert asr.transcribe(PCM, return_ids=True) == [3, 4]
    assert eng.calls == [("transcribe", 1)]                                       # merge=None leaves the switch alone
    eng.calls.clear()
    out = asr.transcribe(PCM, nbest=2, merge=True)
    assert eng.calls == [("merge", True), ("records", True), ("transcribe", 1)]
    assert out[0]["score"] == -1.5 and [t for t, _, _ in out[0]["tokens"]] == [3, 4]
    eng.calls.clear()
    assert asr.transcribe([PCM], return_ids=True, merge=False) == [[3, 4]]
    assert eng.calls == [("merge", False), ("transcribe", 1)]
    eng.calls.clear()
    assert list(asr.stream([PCM[:1280]], return_ids=True, merge=True)) == [[3, 4]]
    assert eng.calls == [("merge", True)]
    eng.calls.clear()
    assert list(asr.stream([PCM[:1280]], return_ids=True)) == [[3, 4]] and eng.calls == []
    assert not eng.slots


def test_facade_merge_needs_a_beam_engine():
    eng = FakeEngine(1)
    asr = _facade(eng)
    for merge in (True, False):
        with pytest.raises(ValueError):
            asr.transcribe(PCM, merge=merge)
        with pytest.raises(ValueError):
            next(asr.stream([PCM[:1280]], merge=merge))
    assert eng.calls == [] and not eng.slots
    assert asr.transcribe(PCM, return_ids=True) == [3, 4]                         # None: fine on a greedy engine


def test_engine_method_and_native_signature():
    from libreasr_amd import _native as N
    from libreasr_amd.engine import Engine
    sig = {n: (r, a) for n, r, a in N.SYMBOLS}
    assert sig["lasr_set_beam_merge"] == sig["lasr_set_beam_records"]

    class Lib:
        def __init__(self):
            self.calls = []

        def lasr_set_beam_merge(self, ctx, on):
            self.calls.append((ctx, on))
            return 0 if ctx == "ok" else N.LASR_ESTATE

        def lasr_last_error(self, ctx):
            return b"refused"

    e = Engine.__new__(Engine)
    e.lib, e.ctx = Lib(), "ok"
    e.set_beam_merge()
    e.set_beam_merge(False)
    e.set_beam_merge(on=True)
    assert e.lib.calls == [("ok", 1), ("ok", 0), ("ok", 1)]
    e.ctx = "busy"
    with pytest.raises(N.LasrError) as ei:
        e.set_beam_merge(True)
    assert "refused" in str(ei.value)
    e.ctx = None                                                                  # (nothing for __del__ to close)
