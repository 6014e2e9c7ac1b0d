"""Contextual biasing (hotwords), the spec restated in Python (include/lasr.h).  Three restatements:

* `automaton`: the phrase automaton built by BRUTE FORCE from its definition -- for every node and token the suffixes of
  path(v) . a are tried from the longest to the shortest against the set of trie prefixes.  Deliberately not the failure-link
  construction of lasr_bias.hip.h.
* `pick`: the biased decision on one float32 logits vector.
* `decode_greedy` / `StreamDecoder`: OracleTransducer.decode_greedy and _StreamDecoder.step with `pick` in place of argmax
  (the oracle is imported, not edited).  Each records (token, frame, lp, node, margin) per decision.

Shared by test_bias_cpu.py (which pins all of this) and test_gpu_bias.py (which takes its expected values from it)."""
import numpy as np

from oracle import rnnt_oracle as O

F32 = np.float32


class Graph:
    """CSR edge lists of the automaton: off [n + 1], tok / nxt / bonus [E], depth [n]; paths: the trie prefix of every node"""

    def __init__(self, off, tok, nxt, bonus, depth=None, paths=None):
        self.off = np.asarray(off, np.int32)
        self.tok = np.asarray(tok, np.int32)
        self.nxt = np.asarray(nxt, np.int32)
        self.bonus = np.asarray(bonus, F32)
        self.depth = None if depth is None else np.asarray(depth, np.int32)
        self.paths = paths
        self.n_nodes = len(self.off) - 1

    def edges(self, v):
        lo, hi = int(self.off[v]), int(self.off[v + 1])
        return self.tok[lo:hi], self.nxt[lo:hi], self.bonus[lo:hi]

    def zeroed(self):
        return Graph(self.off, self.tok, self.nxt, np.zeros_like(self.bonus), self.depth, self.paths)


def trie(phrases):
    """lasr_prefix_tree's nodes and order: depth ascending, then parent ascending, then first appearance.  -> list of paths"""
    paths, level = [()], [()]
    index = {(): 0}
    while level:
        nxt = []
        for p in level:                                   # parents ascending (a level is in node order)
            for ph in phrases:                            # first appearance = lowest phrase index
                ph = tuple(ph)
                if len(ph) > len(p) and ph[:len(p)] == p:
                    q = ph[:len(p) + 1]
                    if q not in index:
                        index[q] = len(paths)
                        paths.append(q)
                        nxt.append(q)
        level = nxt
    return paths, index


def automaton(phrases, weights, symbols=None):
    """the definition, by brute force.  symbols: the tokens to try per node (default: every token of a phrase; any other token
    cannot end a trie prefix, so its delta is 0 and it is not listed)"""
    phrases = [tuple(int(t) for t in p) for p in phrases]
    paths, index = trie(phrases)
    if symbols is None:
        symbols = sorted({t for p in phrases for t in p})

    def w(path):
        return max(F32(wt) for p, wt in zip(phrases, weights) if p[:len(path)] == path)

    off, tok, nxt, bonus = [0], [], [], []
    for p in paths:
        for a in sorted(symbols):
            s = p + (a,)
            for k in range(len(s)):                       # the longest suffix first; the empty one is the root (not listed)
                if s[k:] in index:
                    tok.append(a)
                    nxt.append(index[s[k:]])
                    bonus.append(w(s[k:]))
                    break
        off.append(len(tok))
    return Graph(off, tok, nxt, bonus, [len(p) for p in paths], paths)


def _before(x, xi, b, bi):
    """amax_before: larger value first, NaN largest (all NaN equal), smaller index among equals"""
    xn, bn = np.isnan(x), np.isnan(b)
    if xn or bn:
        return (xn and not bn) or (xn and bn and xi < bi)
    return x > b or (x == b and xi < bi)


def pick(z, g, v, blank):
    """the biased decision of a row in node v on logits z (float32).  -> (chosen, next node, margin): margin = the best minus the
    second-best biased score over the candidate set {arg} + edges + the second-best of z"""
    z = np.asarray(z, F32)
    arg = int(z.argmax())                                 # numpy's order is amax_before's: NaN largest, the first among equals
    toks, nxts, bon = g.edges(v)
    cand = {int(arg): z[arg]}
    for t, b in zip(toks, bon):
        cand[int(t)] = F32(z[t] + b)                      # one f32 addition, round to nearest (s(arg) >= z[arg] replaces it)
    if len(z) > 1:
        rest = np.delete(np.arange(len(z)), arg)
        j2 = int(rest[np.argmax(np.where(np.isnan(z[rest]), np.inf, z[rest]))])
        cand.setdefault(j2, z[j2])
    chosen = None
    for t in sorted(cand):
        if chosen is None or _before(cand[t], t, cand[chosen], chosen):
            chosen = t
    others = [float(cand[t]) for t in cand if t != chosen]
    margin = float(cand[chosen]) - max(others) if others else float("inf")
    if chosen == blank:
        return chosen, v, margin
    hit = np.nonzero(toks == chosen)[0]
    return chosen, (int(nxts[hit[0]]) if len(hit) else 0), margin


def pick_logp(z, chosen):
    """(z[chosen] - max z) - log sum exp(z - max z) in float64: what lasr_bias_pick's logp is held to"""
    z = np.asarray(z, np.float64)
    m = z.max()
    return float(z[chosen] - m - np.log(np.exp(z - m).sum()))


def decode_greedy(m, feats, g, max_iters=3):
    """OracleTransducer.decode_greedy with the biased decision (g None: the plain argmax through the same code).
    -> (tokens, neg_logp, align score, iters per frame, decisions, final node, args); decisions: (token, frame, lp, node,
    margin) of EVERY joint evaluation, node = the row's node before it, lp = the oracle's float32 log-softmax at the chosen
    token; args: the joint's own argmax at every decision (what the unbiased rule would have taken on the same logits)"""
    enc, _ = m.encoder(feats[None])
    enc = enc[0]
    h_pred, pstate = m.predictor([m.bos])
    y, log_p, iters_all, dec, v, args = [], 0.0, [], [], 0, []
    for t in range(enc.shape[0]):
        iters = 0
        while iters < max_iters:
            iters += 1
            lp, z = m.joint_logp(h_pred, enc[t][None])
            pred, nv, margin = _decide(z[0], g, v, m.blank)
            log_p += float(lp[0, pred])
            dec.append((pred, t, float(lp[0, pred]), v, margin))
            args.append(int(z[0].argmax()))
            v = nv
            if pred == m.blank:
                break
            y.append(pred)
            h_pred, pstate = m.predictor([pred], pstate)
        iters_all.append(iters)
    align = np.array(iters_all)
    s = align.sum()
    score = (s - int((align == 1).sum())) / (s + 1e-4)
    return y, -log_p, float(score), iters_all, dec, v, args


def _decide(z, g, v, blank):
    if g is None:
        a = int(np.asarray(z).argmax())
        top2 = np.partition(z, -2)[-2:]
        return a, 0, float(top2[1] - top2[0])
    return pick(z, g, v, blank)


class StreamDecoder:
    """_StreamDecoder.step with the biased decision; reset() also returns the row to the root (the predictor's reset rule)"""

    def __init__(self, m, g, max_iters=10):
        self.m, self.g, self.max_iters = m, g, max_iters
        self.y, self.decisions = [], []
        self.reset()

    def reset(self):
        self.enc_state = None
        self.h_pred, self.pstate = self.m.predictor([self.m.bos])
        self.node = 0

    def step(self, chunk):
        """-> (tokens, frames within the chunk, lps) of the step's emissions"""
        m = self.m
        enc, self.enc_state = m.encoder(chunk[None], self.enc_state)
        enc = enc[0]
        y_seq, frames, lps = [], [], []
        for t in range(enc.shape[0]):
            iters = 0
            while iters < self.max_iters:
                iters += 1
                lp, z = m.joint_logp(self.h_pred, enc[t][None])
                pred, nv, margin = _decide(z[0], self.g, self.node, m.blank)
                self.decisions.append((pred, t, float(lp[0, pred]), self.node, margin))
                self.node = nv
                if pred == m.blank:
                    break
                y_seq.append(pred)
                frames.append(t)
                lps.append(float(lp[0, pred]))
                self.h_pred, self.pstate = m.predictor([pred], self.pstate)
        self.y = self.y + y_seq
        return y_seq, frames, lps


SILENCE = float(np.log(np.float32(1e-6)))      # the log-mel floor: what every feature of a chunk of zeros is


def stream_run(m, g, pcm, reset_at=None, tail=10):
    """one stream through the oracle's streaming front-end and StreamDecoder (test_gpu_alignment.stream_ref's loop and its rule
    for .speech: the leading model steps with any feature above the floor).  reset_at: reset() before that model step.
    -> dict(steps=[(tokens, frames counted from the first step, lps)], nodes=[node after the step], margins=[smallest margin
    of the step's decisions], speech=int, decisions=[...])"""
    from libreasr_amd import synth
    fe, dec = O.StreamFrontend(), StreamDecoder(m, g)
    steps, nodes, margins, base, speech = [], [], [], 0, None
    for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=tail):
        o = fe.push(ch)
        if o is None:
            continue
        if reset_at is not None and len(steps) == reset_at:
            dec.reset()
        if speech is None and float(np.abs(np.asarray(o, np.float64) - SILENCE).max()) < 1e-4:
            speech = len(steps)
        n0 = len(dec.decisions)
        y, fr, lp = dec.step(o)
        steps.append((y, [base + f for f in fr], lp))
        nodes.append(dec.node)
        margins.append(min(d[4] for d in dec.decisions[n0:]))
        base += o.shape[0]
    return dict(steps=steps, nodes=nodes, margins=margins, speech=len(steps) if speech is None else speech, decisions=dec.decisions)


MARGIN = 1e-3          # every compared decision is at least this clear in the restatement: float32 rounding on the GPU decides none


# ---- the committed inputs of the GPU parity tests (found by tests/bias_search.py; their conditions are asserted on the
# restatement alone in test_bias_cpu.py).  name -> (phrases, weights)
OFFLINE_CASES = {          # bias_search.py offline NAME: seeds 11 and 30 (smallest margins 0.0396 and 0.0406)
    "tiny": ([[51, 33, 38], [46, 4, 32, 12]], [3.0, 6.0]),
    "tiny_lstm": ([[49, 29, 27], [42, 39, 17]], [6.0, 2.0]),
}
# bias_search.py stream tiny: seed 0 (smallest margin over the compared steps 0.0112, with and without the reset before step 7)
STREAM_CASE = ([[34, 19, 21, 5], [4, 13, 52], [58, 33, 40, 62], [41, 36, 37, 60]], [3.0, 6.0, 4.0, 2.0])
STREAM_RESET_AT = 7

_CACHE = {}


def offline_ref(name, m, feats_list):
    """per utterance the biased restatement run of OFFLINE_CASES[name] (computed once, shared by the CPU and the GPU tests):
    -> (graph, [decode_greedy's tuple per utterance])"""
    if ("offline", name) not in _CACHE:
        g = automaton(*OFFLINE_CASES[name])
        _CACHE[("offline", name)] = (g, [decode_greedy(m, f, g, 3) for f in feats_list])
    return _CACHE[("offline", name)]


def stream_ref(m, pcm, reset_at=None, zero=False):
    """stream_run of STREAM_CASE on `tiny` (computed once per variant).  zero: the same automaton with every bonus 0"""
    key = ("stream", reset_at, zero)
    if key not in _CACHE:
        g = automaton(*STREAM_CASE)
        _CACHE[key] = (g, stream_run(m, g.zeroed() if zero else g, pcm, reset_at))
    return _CACHE[key]
