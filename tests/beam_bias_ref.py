"""Contextual biasing in beam search (lasr_set_beam_bias), the spec of include/lasr.h restated in Python.

* `automaton`: the graph in beam form by BRUTE FORCE from its definition -- paths as tuples, delta by trying the suffixes of
  path(v) . a from the longest to the shortest (as bias_ref.automaton does), w / term / cum / held read off the paths.  Not the
  failure-link construction of lasr_bias.hip.h.
* `walk`: tokens through a graph; `bonus_sim`: the bookkeeping the gains stand for (a pending part that a failed match loses and a
  completed part that stays), from the phrases alone -- the walk invariant is checked against it.
* `frame_bias`: beam_merge_ref.frame_merge (slots keep their places; merge off by default) with the three changes of the biased
  round; every hypothesis carries `node` and `bon` (its summed gain since the last reset).  The margin bookkeeping takes W + 1
  tokens per row, so that the boundary candidate is always present; the selection itself sees W per row, as the spec says.
* `StreamBeamBias`: the stream wrapper with reset().

Shared by test_beam_bias_cpu.py (which pins all of this) and test_gpu_beam_bias.py (which takes its expected values from it)."""
import math

import numpy as np

import beam_merge_ref as BM
import beam_records_ref as R
import bias_ref as B
from oracle import rnnt_oracle as O

F32 = np.float32
MARGIN = R.MARGIN
SHAPES = R.SHAPES
GAIN_MAX = 1000.0


class Graph:
    """CSR edge lists in beam form: off [n + 1], tok / nxt / gain [E], back [n], depth [n]; paths: the trie prefix of every node;
    term [n]: a phrase ends exactly there"""

    def __init__(self, off, tok, nxt, gain, back, depth=None, paths=None, term=None):
        self.off = np.asarray(off, np.int32)
        self.tok = np.asarray(tok, np.int32)
        self.nxt = np.asarray(nxt, np.int32)
        self.gain = np.asarray(gain, F32)
        self.back = np.asarray(back, F32)
        self.depth = None if depth is None else np.asarray(depth, np.int32)
        self.paths, self.term = paths, term
        self.n_nodes = len(self.off) - 1
        self._rows = {}

    def edges(self, v):
        lo, hi = int(self.off[v]), int(self.off[v + 1])
        return self.tok[lo:hi], self.nxt[lo:hi], self.gain[lo:hi]

    def step(self, v, a, blank):
        """-> (next node, gain as float32) of token a at node v"""
        if a == blank:
            return v, F32(0.0)
        toks, nxts, gains = self.edges(v)
        hit = np.nonzero(toks == a)[0]
        if len(hit):
            return int(nxts[hit[0]]), gains[hit[0]]
        return 0, self.back[v]

    def row(self, v, V, blank):
        """g(v, .) over the vocabulary, float32 [V]"""
        if v not in self._rows:
            toks, _, gains = self.edges(v)
            x = np.full(V, self.back[v], F32)
            x[blank] = 0.0
            x[toks] = gains
            self._rows[v] = x
        return self._rows[v]

    def zeroed(self):
        return Graph(self.off, self.tok, self.nxt, np.zeros_like(self.gain), np.zeros_like(self.back), self.depth, self.paths, self.term)

    def no_revoke(self):
        """the same graph with every negative gain and every back set to 0: a bonus that is never handed back"""
        return Graph(self.off, self.tok, self.nxt, np.maximum(self.gain, F32(0.0)), np.zeros_like(self.back), self.depth, self.paths, self.term)


def automaton(phrases, weights, symbols=None):
    """the definition, by brute force (symbols: see bias_ref.automaton)"""
    phrases = [tuple(int(t) for t in p) for p in phrases]
    paths, index = B.trie(phrases)
    if symbols is None:
        symbols = sorted({t for p in phrases for t in p})
    whole = set(phrases)

    def w(path):
        return max(F32(wt) for p, wt in zip(phrases, weights) if p[:len(path)] == path)

    def cum(path):
        s = 0.0
        for k in range(1, len(path) + 1):
            s = s + float(w(path[:k]))
        return s

    def held(path):
        s = 0.0
        for k in range(1, len(path) + 1):
            s = 0.0 if path[:k] in whole else s + float(w(path[:k]))
        return s

    off, tok, nxt, gain, back = [0], [], [], [], []
    for p in paths:
        back.append(F32(-held(p)))
        for a in sorted(symbols):
            s = p + (a,)
            for k in range(len(s)):                       # the longest suffix first; the empty one is the root (not listed)
                if s[k:] in index:
                    tok.append(a)
                    nxt.append(index[s[k:]])
                    gain.append(w(s) if k == 0 else F32(cum(s[k:]) - held(p)))
                    break
        off.append(len(tok))
    return Graph(off, tok, nxt, gain, back, [len(p) for p in paths], paths, [p in whole for p in paths])


def within_bound(g):
    return bool(np.all(np.abs(g.gain) <= GAIN_MAX) and np.all(np.abs(g.back) <= GAIN_MAX))


def walk(g, tokens, blank, start=0):
    """-> (end node, the double sum of the f32 gains in order, the gains)"""
    v, total, gains = start, 0.0, []
    for a in tokens:
        v, x = g.step(v, int(a), blank)
        total += float(x)
        gains.append(x)
    return v, total, np.asarray(gains, F32)


def bonus_sim(phrases, weights, tokens):
    """What the gains account for, from the phrases alone: the current match is a trie path with a pending bonus (collected since
    the last completed phrase on it) and a completed bonus that stays.  A token that extends the match adds w to the pending part,
    and a completed phrase moves the pending part over.  A token that does not extend it loses the pending part; the longest
    suffix that is a trie prefix becomes the new match and is paid from its start.  -> (completed, pending, path)"""
    phrases = [tuple(int(t) for t in p) for p in phrases]
    prefixes = {p[:k] for p in phrases for k in range(len(p) + 1)}
    whole = set(phrases)

    def w(path):
        return float(max(F32(wt) for p, wt in zip(phrases, weights) if p[:len(path)] == path))

    done, pend, path = 0.0, 0.0, ()

    def extend(q):
        nonlocal done, pend
        pend += w(q)
        if q in whole:
            done, pend = done + pend, 0.0

    for a in tokens:
        s = path + (int(a),)
        if s in prefixes:
            extend(s)
            path = s
            continue
        pend = 0.0
        path = ()
        for k in range(1, len(s) + 1):
            if s[k:] in prefixes:
                path = s[k:]
                break
        for k in range(1, len(path) + 1):
            extend(path[:k])
    return done, pend, path


# ---------------------------------------------------------------------------- the biased round
def beam_init(m):
    h = BM.beam_init(m)
    h[0]["node"] = 0
    h[0]["bon"] = 0.0
    return h


def frame_bias(m, hyps, enc_t, t, W, max_iters, g, margins=None, merge=False, stats=None):
    """one encoder frame.  hyps: list of dict | None (slot order) -> list of W entries, dict | None.  g: Graph, or None for the
    round without a graph (the same code with every gain 0.0).  stats: counts of selected extensions -- "neg" with a negative gain,
    "term" into a node where a phrase ends, "ext" all of them -- and "frames" / "capped" (frames / frames that ended at the cap)."""
    A = [None if h is None else dict(h, inB=False) for h in hyps]
    capped = False
    for rnd in range(1, max_iters + 1):
        cands = []
        for b, h in enumerate(A):
            if h is None:
                continue
            if h["inB"]:
                cands.append((-h["score"], b, 0, -1, h, None, None, False))
                continue
            lp, _ = m.joint_logp(h["h_pred"], enc_t[None])
            lp = lp[0]
            gv = g.row(h["node"], len(lp), m.blank) if g is not None else np.zeros(len(lp), F32)
            s = (np.asarray(lp, F32) + gv).astype(F32)                       # (1) one f32 addition per token
            top = np.argsort(-s, kind="stable")[:W + 1]
            for i, v in enumerate(top):
                sc = (h["score"] + float(lp[v])) + float(gv[v])               # (2) in that order
                cands.append((-sc, b, 1, int(v), h, lp, gv, i >= W))
        cands.sort(key=lambda c: c[:4])
        offered = [c for c in cands if not c[7]]                              # the selection sees W per row
        sel = offered[:W]
        if margins is not None and len(cands) > len(sel) and len(sel) == W:
            rest = min(c[0] for c in cands if all(c is not s_ for s_ in sel))
            margins.append(rest - sel[-1][0])
        new = []
        for negs, b, kind, v, h, lp, gv, _ in sel:
            if kind == 0:
                new.append(h)
            elif v == m.blank:
                new.append(dict(h, score=-negs, inB=True))
            else:
                hp, ps = m.predictor([v], h["pstate"])
                nn = g.step(h["node"], v, m.blank)[0] if g is not None else 0      # (3) the parent's node, moved along delta
                if stats is not None:
                    stats["ext"] = stats.get("ext", 0) + 1
                    stats["neg"] = stats.get("neg", 0) + (1 if float(gv[v]) < 0 else 0)
                    stats["term"] = stats.get("term", 0) + (1 if g is not None and g.term is not None and g.term[nn] else 0)
                capped = capped or rnd == max_iters
                new.append(dict(score=-negs, y=h["y"] + [v], r=h["r"] + [(t, float(lp[v]))], h_pred=hp, pstate=ps,
                                inB=(rnd == max_iters), idt=BM.ident_append(h["idt"], v), capped=h["capped"] or rnd == max_iters,
                                node=nn, bon=h["bon"] + float(gv[v])))
        new += [None] * (W - len(new))
        if merge:                                           # ---- beam_merge_ref's merge step: the kept (lowest) slot's node stays
            for j in range(W):
                if new[j] is None:
                    continue
                acc, cap, second = new[j]["score"], new[j]["capped"], -math.inf
                for i in range(j + 1, W):
                    o = new[i]
                    if o is not None and o["idt"] == new[j]["idt"] and o["inB"] == new[j]["inB"]:
                        acc = BM.lae(acc, o["score"])
                        cap = cap or o["capped"]
                        second = max(second, o["score"])
                        new[i] = None
                        if stats is not None:
                            stats["merges"] = stats.get("merges", 0) + 1
                if second > -math.inf:
                    if margins is not None:
                        margins.append(new[j]["score"] - second)
                    new[j] = dict(new[j], score=acc, capped=cap)
        A = new
        if all(h["inB"] for h in BM.live(A)):
            break
    if stats is not None:
        stats["frames"] = stats.get("frames", 0) + 1
        stats["capped"] = stats.get("capped", 0) + (1 if capped else 0)
    keys = ("score", "y", "r", "h_pred", "pstate", "idt", "capped", "node", "bon")
    return [None if h is None else {k: h[k] for k in keys} for h in A]


def nodes_of(hyps):
    """lasr_beam_bias_state's row: the slots' nodes in slot order, -1 for a dead slot"""
    return [-1 if h is None else int(h["node"]) for h in hyps]


def bons_ranked(hyps):
    return [hyps[i]["bon"] for i in BM.order(hyps)]


class StreamBeamBias:
    """beam_merge_ref.StreamBeamMerge over frame_bias.  .g may be set between model steps (lasr_set_beam_bias in mid-stream: call
    .rebias(g), which also returns every slot to the root); .reset() restarts nodes and bonuses with the beam."""

    def __init__(self, m, W, g, max_iters=10, merge=False):
        self.m, self.W, self.g, self.max_iters, self.merge = m, W, g, max_iters, merge
        self.enc_state = None
        self.hyps = beam_init(m)
        self.t = 0
        self.prefix = ([], [], [], 0.0)
        self.step_margin = []
        self.stats = {}

    def step(self, chunk):
        enc, self.enc_state = self.m.encoder(chunk[None], self.enc_state)
        margins = []
        for k in range(enc.shape[1]):
            self.hyps = frame_bias(self.m, self.hyps, enc[0, k], self.t, self.W, self.max_iters, self.g, margins, self.merge, self.stats)
            self.t += 1
        margins.append(BM.hyp_gap(self.hyps))
        self.step_margin.append(min(margins))
        return self.beam()

    def beam(self):
        return BM.ranked(self.hyps, self.prefix)

    def nodes(self):
        return nodes_of(self.hyps)

    def rebias(self, g):
        self.g = g
        self.hyps = [None if h is None else dict(h, node=0) for h in self.hyps]

    def reset(self):
        self.prefix = self.beam()[0]
        self.enc_state = None
        self.hyps = beam_init(self.m)


# ---------------------------------------------------------------------------- the committed cases
# Found by tests/beam_bias_search.py; their conditions are asserted on the restatement alone in test_beam_bias_cpu.py.
# (name, W) -> (phrases, weights)
OFFLINE_CASES = {          # beam_bias_search.py offline NAME W: seeds 4, 3, 6 and 12 (smallest margins 0.0136, 0.0035, 0.0074, 0.0024;
                           # frames that end at the per-frame cap: 2.7 %, 19.8 %, 13.5 %, 40.5 %)
    ("tiny", 2): ([[25, 56, 3], [25, 56], [29, 25, 29], [25, 19], [25, 56, 44, 56]], [0.5, 1.25, 0.75, 2.0, 0.25]),
    ("tiny", 4): ([[25, 19], [25, 27], [25, 29], [25, 29, 33], [25, 19, 34, 28]], [1.0, 1.5, 1.25, 0.5, 1.5]),
    ("tiny_lstm", 4): ([[38, 4, 39], [33, 18, 44], [62, 33], [38, 4, 19, 15]], [1.25, 1.75, 1.5, 1.0]),
    ("tiny", 8): ([[25, 27], [25, 19], [25, 23], [25, 27, 38, 24]], [1.0, 0.5, 2.0, 1.5]),
}
# beam_bias_search.py stream tiny 4: seed 0 (no stream truncated by the margin rule, with and without the reset before step 7)
STREAM_CASE = ([[25, 23, 29], [22, 10], [25, 6, 44], [27, 4, 6, 17], [25, 23, 41, 36]], [1.25, 2.0, 0.75, 1.75, 1.5])
STREAM_RESET_AT = 7

_CACHE = {}


def offline_run(name, W, g, max_iters=3, merge=False, seed=1234):
    """per utterance: dict(beam = ranked whole beam, bon = per ranked hypothesis, nodes = slot order, T, margin, stats)"""
    m = R.model(name)[0]
    out = []
    for p in R.offline_pcm(name, seed):
        enc, _ = m.encoder(O.features_offline(p)[None])
        hyps, margins, stats = beam_init(m), [], {}
        for t in range(enc.shape[1]):
            hyps = frame_bias(m, hyps, enc[0, t], t, W, max_iters, g, margins, merge, stats)
        margins.append(BM.hyp_gap(hyps))
        out.append(dict(beam=BM.ranked(hyps), bon=bons_ranked(hyps), nodes=nodes_of(hyps), T=int(enc.shape[1]), margin=min(margins),
                        stats=stats))
    return out


def offline_ref(name, W, variant="on", merge=False):
    """the restatement run of OFFLINE_CASES[(name, W)] (computed once, shared by the CPU and the GPU tests) -> (graph, runs).
    variant: "on", "zero" (every gain 0) or "keep" (no revocation)"""
    key = ("offline", name, W, variant, merge)
    if key not in _CACHE:
        g = automaton(*OFFLINE_CASES[(name, W)])
        gg = {"on": g, "zero": g.zeroed(), "keep": g.no_revoke()}[variant]
        _CACHE[key] = (gg, offline_run(name, W, gg, merge=merge))
    return _CACHE[key]


def stream_run(name, W, g, reset_at=None, merge=False):
    """the streams of beam_records_ref.stream_inputs through StreamBeamBias; reset_at: reset() before that model step of every
    stream.  per stream: dict(steps, nodes = per step, T, margin, speech, dec)"""
    m = R.model(name)[0]
    out = []
    for chunks in R.stream_inputs():
        fe, dec = O.StreamFrontend(), StreamBeamBias(m, W, g, merge=merge)
        steps, nodes, T, speech = [], [], [], None
        for ch in chunks:
            o = fe.push(ch)
            if o is None:
                continue
            if reset_at is not None and len(steps) == reset_at:
                dec.reset()
            if speech is None and float(np.abs(np.asarray(o, np.float64) - R.SILENCE).max()) < 1e-4:
                speech = len(steps)
            steps.append(dec.step(o))
            nodes.append(dec.nodes())
            T.append(dec.t)
        out.append(dict(steps=steps, nodes=nodes, T=T, margin=list(dec.step_margin), speech=len(steps) if speech is None else speech,
                        dec=dec))
    return out


def stream_ref(reset_at=None, zero=False):
    """stream_run of STREAM_CASE on (`tiny`, 4), computed once per variant"""
    key = ("stream", reset_at, zero)
    if key not in _CACHE:
        g = automaton(*STREAM_CASE)
        _CACHE[key] = (g, stream_run("tiny", 4, g.zeroed() if zero else g, reset_at))
    return _CACHE[key]


full_upto = R.full_upto
