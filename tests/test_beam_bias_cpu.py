"""Contextual biasing in beam search, CPU side (no GPU): lasr_beam_bias_compile / lasr_bias_walk through the library against the
brute force of beam_bias_ref.py; the walk invariant; the restatement with zero gains pinned to beam_records_ref.beam_frame_rec; the
input conditions of the GPU tests (test_gpu_beam_bias.py) asserted on the restatement alone; the host logic of
LibreASR.set_beam_hotwords / Engine.set_beam_bias against stand-ins; and the header under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/c/beam_bias_check.cpp, a stand-alone program)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import beam_bias_ref as BB
import beam_merge_ref as BM
import beam_records_ref as R
from libreasr_amd import _native as N
from oracle import rnnt_oracle as O

VOCAB, BLANK = 64, 0


def lib():
    import __graft_entry__ as graft
    graft.build()
    return N.lib()


def compiled(phrases, weights, vocab=VOCAB, blank=BLANK):
    from libreasr_amd.engine import beam_bias_compile
    return beam_bias_compile(lib(), phrases, weights, vocab, blank)


def same(g, ref):
    """the library's graph against the brute-force one, array for array (gains and backs bit for bit)"""
    assert g.n_nodes == ref.n_nodes
    assert g.edge_off.tolist() == ref.off.tolist()
    assert g.edge_tok.tolist() == ref.tok.tolist()
    assert g.edge_next.tolist() == ref.nxt.tolist()
    assert g.edge_gain.tobytes() == ref.gain.tobytes()
    assert g.node_back.tobytes() == ref.back.tobytes()
    assert g.depth.tolist() == ref.depth.tolist()


def edge(ref, v, a):
    toks, nxts, gains = ref.edges(v)
    i = list(toks).index(a)
    return int(nxts[i]), float(gains[i])


# ------------------------------------------------------------------------------- (a) the compiler and the walk
a_, b_, c_, d_ = 5, 9, 7, 11
NAMED = {
    "one one-token phrase": ([[a_]], [1.5]),
    "shared prefix": ([[a_, b_, c_], [a_, b_, a_]], [1.0, 2.0]),
    "proper prefix, weight on the shorter": ([[a_, b_], [a_, b_, c_]], [3.0, 1.0]),
    "proper prefix, weight on the longer": ([[a_, b_], [a_, b_, c_]], [1.0, 3.0]),
    "same phrase twice": ([[a_, b_], [a_, b_]], [0.5, 2.5]),
    "failure transition to an inner node": ([[a_, a_, b_]], [2.0]),
    "one ends where another begins": ([[a_, b_], [b_, c_]], [1.0, 2.0]),
    "suffix phrase inside a longer one": ([[a_, b_, c_, d_], [b_, c_]], [1.0, 4.0]),
}


@pytest.mark.parametrize("case", sorted(NAMED))
def test_compile_named_cases(case):
    phrases, weights = NAMED[case]
    ref = BB.automaton(phrases, weights)
    same(compiled(phrases, weights), ref)
    idx = {p: i for i, p in enumerate(ref.paths)}
    assert ref.back[0] == 0 and np.all(ref.back <= 0)
    if case == "one one-token phrase":
        assert ref.term[1] and ref.back.tolist() == [0.0, 0.0]                 # a completed phrase is not revocable
        assert edge(ref, 1, a_) == (1, 1.5)                                      # a a: the second a starts (and completes) a new match
    if case == "failure transition to an inner node":
        aa = idx[(a_, a_)]
        assert ref.back[aa] == -4.0 and ref.back[idx[(a_,)]] == -2.0
        assert edge(ref, aa, a_) == (aa, 0.0)                                    # a a . a: 4 handed back, a a paid again
        assert edge(ref, idx[(a_, a_, b_)], a_) == (idx[(a_,)], 2.0)             # behind a completed phrase nothing is held
    if case == "one ends where another begins":
        assert edge(ref, idx[(a_, b_)], c_) == (idx[(b_, c_)], 4.0)              # b is credited in both (a stated limit)
    if case == "suffix phrase inside a longer one":
        abc = idx[(a_, b_, c_)]
        assert ref.back[abc] == -3.0                                             # a b c x: b c completed only as a suffix -- not credited
        assert not any(ref.edges(abc)[0] == a_ + 1)
        assert edge(ref, abc, b_) == (idx[(b_,)], 4.0 - 3.0)
    if case == "proper prefix, weight on the shorter":
        ab = idx[(a_, b_)]
        assert ref.term[ab] and ref.back[ab] == 0.0 and ref.back[idx[(a_, b_, c_)]] == 0.0
        assert edge(ref, ab, c_) == (idx[(a_, b_, c_)], 1.0)


def test_compile_random_sets():
    rng = np.random.default_rng(11)
    for _ in range(200):
        k = int(rng.integers(1, 7))
        phrases = [[int(t) for t in rng.integers(1, 5, int(rng.integers(1, 6)))] for _ in range(k)]
        weights = [float(w) for w in rng.integers(0, 9, k) * 0.25]
        same(compiled(phrases, weights, vocab=8), BB.automaton(phrases, weights, symbols=range(1, 8)))
    # weights that are no multiples of a power of two: the double sums in path order, rounded once
    for _ in range(20):
        k = int(rng.integers(1, 5))
        phrases = [[int(t) for t in rng.integers(1, 5, int(rng.integers(1, 6)))] for _ in range(k)]
        weights = [float(np.float32(w)) for w in rng.uniform(0.0, 3.0, k)]
        same(compiled(phrases, weights, vocab=8), BB.automaton(phrases, weights, symbols=range(1, 8)))


def raw_compile(tok, nt, w, k, vocab, blank, cap_n, cap_e, null=None):
    L = lib()
    tok, nt, w = np.asarray(tok, np.int32), np.asarray(nt, np.int32), np.asarray(w, np.float32)
    off, etok, enxt = (np.full(max(cap_n + 1, cap_e, 1), -3, np.int32) for _ in range(3))
    egain, back = np.full(max(cap_e, 1), -3, np.float32), np.full(max(cap_n, 1), -3, np.float32)
    nn, ne = C.c_int(-7), C.c_int(-7)
    ptr = lambda name, a: None if name == null else a.ctypes.data_as(C.c_void_p)
    rc = L.lasr_beam_bias_compile(ptr("tokens", tok), ptr("n_tokens", nt), ptr("weights", w), k, vocab, blank, cap_n, cap_e,
                                  ptr("edge_off", off), ptr("edge_tok", etok), ptr("edge_next", enxt), ptr("edge_gain", egain),
                                  ptr("node_back", back), None, None if null == "n_nodes" else C.byref(nn),
                                  None if null == "n_edges" else C.byref(ne))
    return rc, nn.value, ne.value, (off, etok, enxt, egain, back)


def test_compile_capacity_and_refusals():
    phrases, weights = NAMED["one ends where another begins"]
    ref = BB.automaton(phrases, weights)
    n, e = ref.n_nodes, len(ref.tok)
    tok, nt = sum(phrases, []), [len(p) for p in phrases]
    rc, nn, ne, out = raw_compile(tok, nt, weights, 2, VOCAB, BLANK, n, e)                 # exact capacity
    assert (rc, nn, ne) == (N.LASR_OK, n, e) and out[0][:n + 1].tolist() == ref.off.tolist()
    assert out[4][:n].tobytes() == ref.back.tobytes()
    for cap_n, cap_e in ((n - 1, e), (n, e - 1), (0, 0)):
        rc, nn, ne, out = raw_compile(tok, nt, weights, 2, VOCAB, BLANK, cap_n, cap_e)
        assert (rc, nn, ne) == (N.LASR_EFULL, n, e)                                          # the counts say what is needed
        assert all(np.all(a == -3) for a in out)                                             # nothing else is written
    bad = {
        "k < 1": dict(k=0),
        "empty phrase": dict(nt=[2, 0]),
        "id >= vocab": dict(tok=[a_, VOCAB, b_, c_]),
        "id < 0": dict(tok=[a_, -1, b_, c_]),
        "blank": dict(tok=[a_, BLANK, b_, c_]),
        "negative weight": dict(w=[1.0, -0.5]),
        "infinite weight": dict(w=[np.inf, 1.0]),
        "nan weight": dict(w=[1.0, np.nan]),
        "a gain beyond 1000": dict(w=[1000.5, 1.0]),
    }
    for what, kw in bad.items():
        args = dict(tok=tok, nt=nt, w=weights, k=2)
        args.update(kw)
        rc, nn, ne, out = raw_compile(args["tok"], args["nt"], args["w"], args["k"], VOCAB, BLANK, n, e)
        assert (rc, nn, ne) == (N.LASR_EINVAL, 0, 0), what
        assert all(np.all(a == -3) for a in out), what
    # the 1000 bound on what a failed match hands back: three held tokens of 400 each; two are fine
    rc, nn, ne, _ = raw_compile([1, 2, 3, 4], [4], [400.0], 1, VOCAB, BLANK, 16, 16)
    assert (rc, nn, ne) == (N.LASR_EINVAL, 0, 0)
    assert not BB.within_bound(BB.automaton([[1, 2, 3, 4]], [400.0]))
    rc, nn, ne, _ = raw_compile([1, 2, 3], [3], [400.0], 1, VOCAB, BLANK, 16, 16)
    assert rc == N.LASR_OK and BB.within_bound(BB.automaton([[1, 2, 3]], [400.0]))
    for null in ("tokens", "n_tokens", "weights", "edge_off", "edge_tok", "edge_next", "edge_gain", "node_back", "n_nodes", "n_edges"):
        rc, nn, ne, _ = raw_compile(tok, nt, weights, 2, VOCAB, BLANK, n, e, null=null)
        assert rc == N.LASR_EINVAL, null
        assert (null == "n_nodes" or nn == 0) and (null == "n_edges" or ne == 0), null
    # more than 65536 nodes: 257 x 256 distinct two-token phrases over a vocabulary of 512
    big = [[x, y] for x in range(1, 258) for y in range(1, 257)]
    rc, nn, ne, _ = raw_compile(sum(big, []), [2] * len(big), [1.0] * len(big), len(big), 512, BLANK, 8, 8)
    assert (rc, nn, ne) == (N.LASR_EINVAL, 0, 0)


def lib_walk(g, tokens, start=0, blank=BLANK):
    from libreasr_amd.engine import bias_walk
    return bias_walk(lib(), g, tokens, blank, start)


def test_walk_invariant_on_random_strings():
    """the summed gains of any token string from the root = the bonus of its completed matches + held(current node), with the
    bookkeeping of beam_bias_ref.bonus_sim (from the phrases alone) as the right-hand side; the library's walk, the restatement's
    walk and the brute-force graph agree token for token"""
    rng = np.random.default_rng(5)
    for _ in range(60):
        k = int(rng.integers(1, 6))
        phrases = [[int(t) for t in rng.integers(1, 5, int(rng.integers(1, 6)))] for _ in range(k)]
        weights = [float(w) for w in rng.integers(0, 9, k) * 0.25]             # multiples of 0.25: every sum is exact
        ref = BB.automaton(phrases, weights, symbols=range(1, 8))
        g = compiled(phrases, weights, vocab=8)
        for _ in range(8):
            toks = [int(t) for t in rng.integers(0, 8, int(rng.integers(0, 30)))]
            end, total, gains = lib_walk(g, toks)
            rend, rtotal, rgains = BB.walk(ref, toks, BLANK)
            assert (end, total) == (rend, rtotal) and gains.tobytes() == rgains.tobytes()
            done, pend, path = BB.bonus_sim(phrases, weights, [t for t in toks if t != BLANK])
            assert total == done + pend
            assert ref.paths[end] == path and float(-ref.back[end]) == pend
            # from a node in the middle: the walk is the graph's, whatever brought the row there
            cut = len(toks) // 2
            mid, t1, _ = lib_walk(g, toks[:cut])
            end2, t2, _ = lib_walk(g, toks[cut:], start=mid)
            assert end2 == end and t1 + t2 == total
    g = compiled([[a_, b_]], [1.0])
    for bad in (dict(start=g.n_nodes), dict(start=-1)):
        with pytest.raises(N.LasrError):
            lib_walk(g, [a_], **bad)
    with pytest.raises(N.LasrError):
        lib_walk(g, [a_, -1])
    assert lib_walk(g, [])[:2] == (0, 0.0)


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_beam_bias_compile", "lasr_set_beam_bias", "lasr_beam_bias_state", "lasr_bias_walk", "lasr_beam_bias_round"} <= names
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    for meth in ("beam_bias_compile", "set_beam_bias", "beam_bias_state", "bias_walk", "beam_bias_round"):
        assert callable(getattr(Engine, meth, None)), meth
    assert callable(getattr(LibreASR, "set_beam_hotwords", None))
    L = lib()
    assert L.lasr_set_beam_bias(None, 0, None, None, None, None, None) == N.LASR_EINVAL          # no context: an error code
    assert L.lasr_beam_bias_state(None, 0, None) == N.LASR_EINVAL
    assert L.lasr_beam_bias_round(None, None, 1, None, None, None, None, None, 3, None, None, None, None, None, None, None, None) == N.LASR_EINVAL


# ------------------------------------------------------------------------------- (b) zero gains: the restatement is the beam's
@pytest.mark.parametrize("name,W", BB.SHAPES)
def test_zero_gain_restatement_is_the_offline_beam(name, W):
    g, runs = BB.offline_ref(name, W, "zero")
    assert not g.gain.any() and not g.back.any()
    plain = R.offline_ref(name, W)
    none = BB.offline_run(name, W, None)
    for u, v, p in zip(runs, none, plain):
        assert u["beam"] == p["beam"] and v["beam"] == p["beam"]                # tokens, frames, log p and scores: ==
        assert all(b == 0.0 for b in u["bon"])
        assert u["margin"] <= p["margin"]                                       # (the W + 1 tokens per row can only add boundary candidates)


def test_zero_gain_restatement_is_the_stream_beam():
    _, runs = BB.stream_ref(zero=True)
    for s, p in zip(runs, R.stream_ref("tiny", 4)):
        assert s["steps"] == p["steps"] and s["T"] == p["T"] and s["speech"] == p["speech"]


# ------------------------------------------------------------------------------- (c) the GPU tests' input conditions
def test_offline_cases_meet_their_conditions():
    decides = 0
    for name, W in BB.SHAPES:
        g, on = BB.offline_ref(name, W)
        assert BB.within_bound(g)
        plain = R.offline_ref(name, W)
        assert len(on) == 3
        assert all(u["margin"] >= BB.MARGIN for u in on), (name, W, [u["margin"] for u in on])     # every utterance in full
        assert sum(u["beam"][0][0] != p["beam"][0][0] for u, p in zip(on, plain)) >= 2, (name, W)
        assert sum(u["stats"]["neg"] for u in on) >= 1, (name, W)                                    # a revocation was selected
        assert sum(u["stats"]["term"] for u in on) >= 1, (name, W)                                   # a phrase was completed
        for u in on:                                                                                 # bon is the walk's total
            for (toks, _, _, _), bon in zip(u["beam"], u["bon"]):
                assert BB.walk(g, toks, 0)[1] == pytest.approx(bon, abs=1e-9)
        _, keep = BB.offline_ref(name, W, "keep")
        decides += any(u["beam"][0][0] != q["beam"][0][0] for u, q in zip(on, keep))
    assert decides >= 1                    # the cancellation decides something: without it another hypothesis wins


def test_stream_case_meets_its_conditions():
    plain = R.stream_ref("tiny", 4)
    for reset_at in (None, BB.STREAM_RESET_AT):
        g, runs = BB.stream_ref(reset_at)
        assert sum(BB.full_upto(s) < s["speech"] for s in runs) <= 1
        if reset_at is not None:
            assert all(BB.full_upto(s) > reset_at for s in runs)                 # at least one step behind the reset is compared
    _, a = BB.stream_ref()
    assert any(s["steps"][BB.full_upto(s) - 1][0][0] != p["steps"][BB.full_upto(s) - 1][0][0] for s, p in zip(a, plain))
    assert sum(s["dec"].stats.get("neg", 0) for s in a) >= 1 and sum(s["dec"].stats.get("term", 0) for s in a) >= 1


def test_merge_restatement_with_bias_keeps_the_lowest_slots_node():
    """merging with a graph attached from the start: merged hypotheses hold equal tokens, hence equal nodes and equal bonuses"""
    g, _ = BB.offline_ref("tiny", 4)
    m = R.model("tiny")[0]
    enc, _ = m.encoder(O.features_offline(R.offline_pcm("tiny")[0])[None])
    hyps, stats = BB.beam_init(m), {}
    for t in range(enc.shape[1]):
        hyps = BB.frame_bias(m, hyps, enc[0, t], t, 4, 3, g, None, True, stats)
        live = BM.live(hyps)
        assert len({tuple(h["y"]) for h in live}) == len(live)                   # pairwise distinct after the merge
        for h in live:
            assert h["node"] == BB.walk(g, h["y"], 0)[0] and h["bon"] == pytest.approx(BB.walk(g, h["y"], 0)[1], abs=1e-9)
    assert stats.get("merges", 0) > 0


# ------------------------------------------------------------------------------- (d) host logic of the facade
class FakeEngine:
    """What LibreASR.set_beam_hotwords / transcribe(nbest=) use of an engine: the compiler and the walk go to the library (host
    only), everything else is recorded"""

    def __init__(self, beam=4, lm=False):
        self.beam, self.lm_cfg, self.calls, self.beam_bias = beam, ({"vocab": VOCAB} if lm else None), [], None

        class Desc:
            stride, hop, sample_rate = 8, 160, 16000
        self.desc = Desc()

    def beam_bias_compile(self, phrases, weights):
        self.calls.append(("compile", [list(p) for p in phrases], list(weights)))
        return compiled(phrases, weights)

    def set_beam_bias(self, graph):
        self.calls.append(("set", graph))
        self.beam_bias = graph

    def bias_walk(self, tokens, start=0, graph=None):
        return lib_walk(self.beam_bias if graph is None else graph, tokens, start)

    # transcribe(nbest=)
    def set_beam_records(self, on):
        pass

    def open(self):
        return 0

    def close_slot(self, s):
        pass

    def transcribe_pcm(self, slots, pcm):
        pass

    def fetch_nbest(self, slot, k):
        return [([a_, b_, c_], [0, 1, 2], [-0.5, -0.25, -1.0], 1.25), ([a_, c_], [0, 2], [-0.5, -2.0], -2.5)][:k]


class Lang:
    def numericalize(self, text):
        return [ord(ch) - ord("a") + 3 for ch in text]


def facade(eng, lang=None):
    from libreasr_amd.api import LibreASR

    class Model:
        engine = eng
    return LibreASR(None, lang, Model(), None, None)


def test_set_beam_hotwords_host_logic():
    eng = FakeEngine()
    asr = facade(eng, Lang())
    asr.set_beam_hotwords([[5, 9], "ab"], boost=[1.0, 0.5])
    assert eng.calls[0] == ("compile", [[5, 9], [3, 4]], [1.0, 0.5])
    assert eng.calls[1][0] == "set" and eng.calls[1][1].n_nodes == 5
    asr.set_beam_hotwords([[5, 9], [5]])                                          # the default boost, one float for every phrase
    assert eng.calls[2][2] == [1.0, 1.0]
    for clear in (None, []):
        asr.set_beam_hotwords(clear)
        assert eng.calls[-1] == ("set", None)
    n = len(eng.calls)
    for bad in (dict(phrases=[[5], []]), dict(phrases=[[5]], boost=[1.0, 2.0]), dict(phrases=[[5]], boost=-1.0),
                dict(phrases=[[5]], boost=float("nan")), dict(phrases=[[5]], boost=float("inf"))):
        with pytest.raises(ValueError):
            asr.set_beam_hotwords(**bad)
    with pytest.raises(TypeError):
        facade(eng, object()).set_beam_hotwords(["ab"])
    assert len(eng.calls) == n                                                     # nothing reached the engine
    for kw in (dict(beam=1), dict(lm=True)):
        e2 = FakeEngine(**kw)
        with pytest.raises(ValueError):
            facade(e2).set_beam_hotwords([[5]])
        assert e2.calls == []


def test_nbest_results_carry_the_bonus_when_hotwords_are_set():
    eng = FakeEngine()
    asr = facade(eng)
    asr._pcm = lambda x: x
    out = asr.transcribe(np.zeros(16000, np.float32), nbest=2)
    assert [sorted(h) for h in out] == [["score", "tokens"]] * 2                   # no graph: the results of before
    asr.set_beam_hotwords([[a_, b_, c_]], boost=0.75)
    out = asr.transcribe(np.zeros(16000, np.float32), nbest=2)
    assert [h["bonus"] for h in out] == [2.25, 0.0]                                # a b c completed; a c: 0.75 gained and handed back
    assert [h["score"] for h in out] == [1.25, -2.5]                               # the ranking score, untouched
    asr.set_beam_hotwords(None)
    assert "bonus" not in asr.transcribe(np.zeros(16000, np.float32), nbest=1)[0]


def test_engine_set_beam_bias_marshals_the_graph():
    from libreasr_amd.engine import BeamBiasGraph, Engine

    class Lib:
        def __init__(self):
            self.calls, self.rc = [], 0

        def lasr_set_beam_bias(self, ctx, n, off, tok, nxt, gain, back):
            self.calls.append((n, off, tok, nxt, gain, back))
            return self.rc

        def lasr_last_error(self, ctx):
            return b"refused"

    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.beam_bias = Lib(), None, None
    g = compiled([[5, 9, 7]], [1.0])
    assert isinstance(g, BeamBiasGraph) and g.n_nodes == 4 and g.n_edges == len(g.edge_tok) and g.node_back.size == 4
    eng.set_beam_bias(g)
    n, off, tok, nxt, gain, back = eng.lib.calls[0]
    assert n == 4 and off.value == g.edge_off.ctypes.data and gain.value == g.edge_gain.ctypes.data and back.value == g.node_back.ctypes.data
    assert eng.beam_bias is g
    eng.set_beam_bias(None)
    assert eng.lib.calls[1] == (0, None, None, None, None, None) and eng.beam_bias is None
    eng.lib.rc = N.LASR_ESTATE
    with pytest.raises(N.LasrError):
        eng.set_beam_bias(g)
    assert eng.beam_bias is None                                                   # a refusal changes nothing


# ------------------------------------------------------------------------------- the header under sanitizers
def test_beam_bias_header_under_asan_ubsan(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the image"
    exe = str(tmp_path / "beam_bias_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(root, "tests", "c", "beam_bias_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "beam_bias_check: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
