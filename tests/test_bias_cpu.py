"""Contextual biasing (hotwords), CPU side (no GPU): lasr_bias_compile through the library against the brute-force automaton of
bias_ref.py; the restatements of bias_ref.py pinned to the numpy oracle; the input conditions of the GPU tests
(test_gpu_bias.py) asserted on the restatement alone; the host logic of Engine.set_bias / LibreASR.set_hotwords against a fake
engine; and the compiler header under AddressSanitizer + UndefinedBehaviorSanitizer (tests/c/bias_check.cpp, a stand-alone
program)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bias_ref as B
from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O
from test_alignment_cpu import oracle, utterances

VOCAB, BLANK = 64, 0


def lib():
    import __graft_entry__ as graft
    graft.build()
    return N.lib()


def compiled(phrases, weights, vocab=VOCAB, blank=BLANK):
    from libreasr_amd.engine import bias_compile
    return bias_compile(lib(), phrases, weights, vocab, blank)


def same(g, ref):
    """the library's graph against the brute-force one, array for array"""
    assert g.n_nodes == ref.n_nodes
    assert g.edge_off.tolist() == ref.off.tolist()
    assert g.edge_tok.tolist() == ref.tok.tolist()
    assert g.edge_next.tolist() == ref.nxt.tolist()
    assert g.edge_bonus.tobytes() == ref.bonus.tobytes()
    assert g.depth.tolist() == ref.depth.tolist()


def delta(ref, v, a):
    toks, nxts, _ = ref.edges(v)
    hit = np.nonzero(toks == a)[0]
    return int(nxts[hit[0]]) if len(hit) else 0


# ------------------------------------------------------------------------------- (a) the compiler
a_, b_, c_ = 5, 9, 7
NAMED = {
    "one one-token phrase": ([[a_]], [1.5]),
    "shared prefix": ([[a_, b_, c_], [a_, b_, a_]], [1.0, 2.0]),
    "proper prefix, weight on the shorter": ([[a_, b_], [a_, b_, c_]], [3.0, 1.0]),
    "proper prefix, weight on the longer": ([[a_, b_], [a_, b_, c_]], [1.0, 3.0]),
    "same phrase twice": ([[a_, b_], [a_, b_]], [0.5, 2.5]),
    "failure transition to an inner node": ([[a_, a_, b_]], [2.0]),
    "one ends where another begins": ([[a_, b_], [b_, c_]], [1.0, 2.0]),
}


@pytest.mark.parametrize("case", sorted(NAMED))
def test_compile_named_cases(case):
    phrases, weights = NAMED[case]
    ref = B.automaton(phrases, weights)
    same(compiled(phrases, weights), ref)
    idx = {p: i for i, p in enumerate(ref.paths)}
    if case == "failure transition to an inner node":
        aa = idx[(a_, a_)]
        assert delta(ref, aa, a_) == aa                   # a a . a: the longest suffix that is a prefix is a a again
        assert delta(ref, idx[(a_, a_, b_)], a_) == idx[(a_,)]
    if case == "one ends where another begins":
        assert delta(ref, idx[(a_, b_)], c_) == idx[(b_, c_)]
        toks, _, bon = ref.edges(idx[(a_, b_)])
        assert bon[list(toks).index(c_)] == np.float32(2.0)
    if case == "proper prefix, weight on the shorter":
        assert ref.edges(0)[2].tolist() == [3.0] and ref.edges(idx[(a_, b_)])[2][list(ref.edges(idx[(a_, b_)])[0]).index(c_)] == 1.0
    if case == "proper prefix, weight on the longer":
        assert ref.edges(0)[2].tolist() == [3.0]
    if case == "same phrase twice":
        assert ref.n_nodes == 3 and ref.edges(0)[2].tolist() == [2.5]


def test_compile_random_sets():
    rng = np.random.default_rng(7)
    for _ in range(200):
        k = int(rng.integers(1, 7))
        phrases = [[int(t) for t in rng.integers(1, 5, int(rng.integers(1, 6)))] for _ in range(k)]
        weights = [float(w) for w in rng.integers(0, 9, k) * 0.25]
        same(compiled(phrases, weights, vocab=8), B.automaton(phrases, weights, symbols=range(1, 8)))


def raw_compile(tok, nt, w, k, vocab, blank, cap_n, cap_e, null=None):
    L = lib()
    tok, nt, w = np.asarray(tok, np.int32), np.asarray(nt, np.int32), np.asarray(w, np.float32)
    off, etok, enxt = (np.full(max(cap_n + 1, cap_e, 1), -3, np.int32) for _ in range(3))
    ebon = np.full(max(cap_e, 1), -3, np.float32)
    nn, ne = C.c_int(-7), C.c_int(-7)
    ptr = lambda name, a: None if name == null else a.ctypes.data_as(C.c_void_p)
    rc = L.lasr_bias_compile(ptr("tokens", tok), ptr("n_tokens", nt), ptr("weights", w), k, vocab, blank, cap_n, cap_e,
                             ptr("edge_off", off), ptr("edge_tok", etok), ptr("edge_next", enxt), ptr("edge_bonus", ebon), None,
                             None if null == "n_nodes" else C.byref(nn), None if null == "n_edges" else C.byref(ne))
    return rc, nn.value, ne.value, (off, etok, enxt, ebon)


def test_compile_capacity_and_refusals():
    phrases, weights = NAMED["one ends where another begins"]
    ref = B.automaton(phrases, weights)
    n, e = ref.n_nodes, len(ref.tok)
    tok, nt = sum(phrases, []), [len(p) for p in phrases]
    rc, nn, ne, out = raw_compile(tok, nt, weights, 2, VOCAB, BLANK, n, e)                 # exact capacity
    assert (rc, nn, ne) == (N.LASR_OK, n, e) and out[0][:n + 1].tolist() == ref.off.tolist()
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
    }
    for what, kw in bad.items():
        args = dict(tok=tok, nt=nt, w=weights, k=2)
        args.update(kw)
        rc, nn, ne, out = raw_compile(args["tok"], args["nt"], args["w"], args["k"], VOCAB, BLANK, n, e)
        assert (rc, nn, ne) == (N.LASR_EINVAL, 0, 0), what
        assert all(np.all(a == -3) for a in out), what
    for null in ("tokens", "n_tokens", "weights", "edge_off", "edge_tok", "edge_next", "edge_bonus", "n_nodes", "n_edges"):
        rc, nn, ne, _ = raw_compile(tok, nt, weights, 2, VOCAB, BLANK, n, e, null=null)
        assert rc == N.LASR_EINVAL, null
        assert (null == "n_nodes" or nn == 0) and (null == "n_edges" or ne == 0), null
    # more than 65536 nodes: 257 x 256 distinct two-token phrases over a vocabulary of 512
    big = [[x, y] for x in range(1, 258) for y in range(1, 257)]
    rc, nn, ne, _ = raw_compile(sum(big, []), [2] * len(big), [1.0] * len(big), len(big), 512, BLANK, 8, 8)
    assert (rc, nn, ne) == (N.LASR_EINVAL, 0, 0)
    # more than 2^22 edges: 4200 phrases that share no prefix and all start with a distinct token -- every node lists the 4200
    # first tokens, 1000 inner nodes more than suffice
    wide = [[t] for t in range(1, 4201)] + [[1, 1] + [2] * d for d in range(1, 1000)]
    rc, nn, ne, _ = raw_compile(sum(wide, []), [len(p) for p in wide], [1.0] * len(wide), len(wide), 4300, BLANK, 8, 8)
    assert (rc, nn, ne) == (N.LASR_EINVAL, 0, 0)


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_bias_compile", "lasr_set_bias", "lasr_bias_state", "lasr_bias_pick"} <= names
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    for meth in ("bias_compile", "set_bias", "bias_state", "bias_pick"):
        assert callable(getattr(Engine, meth, None)), meth
    assert callable(getattr(LibreASR, "set_hotwords", None))
    L = lib()
    assert L.lasr_set_bias(None, 0, None, None, None, None) == N.LASR_EINVAL          # no context: an error code
    assert L.lasr_bias_state(None, None, 0, None) == N.LASR_EINVAL
    assert L.lasr_bias_pick(None, None, None, 1, None, None, None) == N.LASR_EINVAL


# ------------------------------------------------------------------------------- (b) the restatement is the oracle's
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_zero_bonus_restatement_is_the_offline_oracle(name):
    m = oracle(name)
    phrases, weights = B.OFFLINE_CASES[name]
    zero = B.automaton(phrases, weights).zeroed()
    for p in utterances():
        feats = O.features_offline(p)
        want = m.decode_greedy(feats, max_iters=3)
        for g in (zero, B.automaton(phrases, [0.0] * len(phrases)), None):       # all-zero bonuses twice over; no graph at all
            got = B.decode_greedy(m, feats, g, 3)
            assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3]
            if g is not None:                              # the state walks the automaton and nothing else changes
                v = 0
                for (tok, _, _, node, _) in got[4]:
                    assert node == v
                    v = v if tok == m.blank else delta(g, v, tok)
                assert got[5] == v


def test_zero_bonus_restatement_is_the_stream_oracle():
    m = oracle("tiny")
    pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
    _, run = B.stream_ref(m, pcm, zero=True)
    fe, dec = O.StreamFrontend(), m.stream_decoder()
    want = []
    for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=10):
        o = fe.push(ch)
        if o is not None:
            want.append(dec.step(o))
    assert [s[0] for s in run["steps"]] == want and len(want) == 23
    assert B.stream_run(m, None, pcm)["steps"] == run["steps"]                   # frames and log p too


def test_pick_restatement_on_small_vectors():
    g = B.automaton([[a_, a_, b_], [c_]], [2.0, 0.0])
    z = np.full(16, -4.0, np.float32)
    z[BLANK] = 1.0
    assert B.pick(z, g, 0, BLANK)[:2] == (BLANK, 0)                              # -4 + 2 < 1
    z[a_] = -0.5
    assert B.pick(z, g, 0, BLANK)[:2] == (a_, 1)                                 # -0.5 + 2 > 1: a boosted token beats blank
    z[a_] = -1.0
    assert B.pick(z, g, 0, BLANK)[:2] == (BLANK, 0)                              # an exact tie: the lowest id wins
    z[3], z[BLANK] = 2.0, -9.0
    tok, nxt, margin = B.pick(z, g, 2, BLANK)                                    # an unlisted token: back to the root
    assert (tok, nxt) == (3, 0) and margin == pytest.approx(1.0)                 # 2.0 against -1 + 2
    assert abs(B.pick_logp(z, 3) - float(z[3] - np.log(np.exp(z.astype(np.float64)).sum()))) < 1e-12


# ------------------------------------------------------------------------------- (c) input conditions of the GPU tests
def test_offline_cases_meet_their_conditions():
    differ = beaten = capped = False
    deepest = 0
    for name in ("tiny", "tiny_lstm"):
        m = oracle(name)
        feats = [O.features_offline(p) for p in utterances()]
        g, runs = B.offline_ref(name, m, feats)
        same(compiled(*B.OFFLINE_CASES[name]), g)                                 # what the GPU test attaches is this automaton
        for f, (y, _, _, iters, dec, v, args) in zip(feats, runs):
            worst = min(d[4] for d in dec)
            print(f"{name}: {len(dec)} decisions, {len(y)} tokens, smallest margin {worst:.4f}, final node {v}")
            assert worst >= B.MARGIN                                              # every decision of every compared utterance
            differ |= y != m.decode_greedy(f, max_iters=3)[0]
            beaten |= any(d[0] != m.blank and a == m.blank for d, a in zip(dec, args))
            deepest = max([deepest, int(g.depth[v])] + [int(g.depth[d[3]]) for d in dec])
            capped |= any(i == 3 for i in iters)
    assert differ and beaten and deepest >= 3 and capped


def test_stream_case_meets_its_conditions():
    m = oracle("tiny")
    pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
    g, a = B.stream_ref(m, pcm)
    _, b = B.stream_ref(m, pcm, reset_at=B.STREAM_RESET_AT)
    plain = B.stream_run(m, None, pcm)
    same(compiled(*B.STREAM_CASE), g)
    assert a["speech"] == b["speech"] == 19 and len(a["steps"]) == 23
    worst = min(a["margins"][:19] + b["margins"][:19])
    print(f"stream: smallest margin over the compared steps {worst:.4f}")
    assert worst >= B.MARGIN
    assert [s[0] for s in a["steps"][:19]] != [s[0] for s in plain["steps"][:19]]          # biasing changes the transcript
    assert b["nodes"][B.STREAM_RESET_AT - 1] != 0                                           # the reset finds the row off the root
    assert sum(len(s[0]) for s in b["steps"][B.STREAM_RESET_AT:19]) > 0                     # tokens after the reset are compared
    assert max(int(g.depth[d[3]]) for d in a["decisions"]) >= 2


# ------------------------------------------------------------------------------- (d) host logic of the facade
class FakeEngine:
    """What LibreASR.set_hotwords uses of an engine: bias_compile goes to the library (host only), set_bias is recorded"""

    def __init__(self, beam=1, lm=False):
        self.beam, self.lm_cfg, self.calls = beam, ({"vocab": VOCAB} if lm else None), []

    def bias_compile(self, phrases, weights):
        self.calls.append(("compile", [list(p) for p in phrases], list(weights)))
        return compiled(phrases, weights)

    def set_bias(self, graph):
        self.calls.append(("set", graph))


class Lang:
    def numericalize(self, text):
        return [ord(ch) - ord("a") + 3 for ch in text]


def facade(eng, lang=None):
    from libreasr_amd.api import LibreASR

    class Model:
        engine = eng
    return LibreASR(None, lang, Model(), None, None)


def test_set_hotwords_host_logic():
    eng = FakeEngine()
    asr = facade(eng, Lang())
    asr.set_hotwords([[5, 9], "ab"], boost=[1.0, 0.5])
    assert eng.calls[0] == ("compile", [[5, 9], [3, 4]], [1.0, 0.5])
    assert eng.calls[1][0] == "set" and eng.calls[1][1].n_nodes == 5
    asr.set_hotwords([[5, 9], [5]], boost=1.25)                                   # one float serves every phrase
    assert eng.calls[2][2] == [1.25, 1.25]
    for clear in (None, []):
        asr.set_hotwords(clear)
        assert eng.calls[-1] == ("set", None)
    n = len(eng.calls)
    for bad in (dict(phrases=[[5], []]), dict(phrases=[[5]], boost=[1.0, 2.0]), dict(phrases=[[5]], boost=-1.0),
                dict(phrases=[[5]], boost=float("nan")), dict(phrases=[[5]], boost=float("inf"))):
        with pytest.raises(ValueError):
            asr.set_hotwords(**bad)
    with pytest.raises(TypeError):
        facade(eng, object()).set_hotwords(["ab"])                                 # text needs a language object that numericalizes
    assert len(eng.calls) == n                                                     # nothing reached the engine
    for kw in (dict(beam=4), dict(lm=True)):
        e2 = FakeEngine(**kw)
        with pytest.raises(ValueError):
            facade(e2).set_hotwords([[5]])
        assert e2.calls == []
        facade(e2).set_hotwords(None)                                              # clearing is always allowed
        assert e2.calls == [("set", None)]


def test_engine_set_bias_marshals_the_graph():
    """Engine.set_bias / bias_state against a recording stand-in for the library: the graph's arrays go through unchanged, None
    clears with n_nodes = 0, an error code raises"""
    from libreasr_amd.engine import BiasGraph, Engine

    class Lib:
        def __init__(self):
            self.calls, self.rc = [], 0

        def lasr_set_bias(self, ctx, n, off, tok, nxt, bon):
            self.calls.append((n, off, tok, nxt, bon))
            return self.rc

        def lasr_last_error(self, ctx):
            return b"refused"

    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx = Lib(), None
    g = compiled([[5, 9, 7]], [1.0])
    assert isinstance(g, BiasGraph) and g.n_nodes == 4 and g.n_edges == len(g.edge_tok)
    eng.set_bias(g)
    n, off, tok, nxt, bon = eng.lib.calls[0]
    assert n == 4 and off.value == g.edge_off.ctypes.data and bon.value == g.edge_bonus.ctypes.data
    eng.set_bias(None)
    assert eng.lib.calls[1] == (0, None, None, None, None)
    eng.lib.rc = N.LASR_ESTATE
    with pytest.raises(N.LasrError):
        eng.set_bias(g)


# ------------------------------------------------------------------------------- the compiler header under sanitizers
def test_bias_compiler_under_asan_ubsan(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the image"
    exe = str(tmp_path / "bias_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(root, "tests", "c", "bias_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bias_check: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
