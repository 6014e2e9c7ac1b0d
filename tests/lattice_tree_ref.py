"""Float64 reference of n-best rescoring over a prefix tree (lasr_prefix_tree / lasr_score_* / lasr_lattice_tree_dp): the trie the
library must build, and the two recursions of tests/lattice_ref.py run over a tree instead of a chain.

    b[t,v] = lp[t,v,blank], e[t,v] = lp[t,parent v,label v] (the emission that ENTERS v; e[t,0] = 0)
    alpha[0,0] = 0, alpha[t,v] = logaddexp(alpha[t-1,v] + b[t-1,v], alpha[t,parent v] + e[t,v]);  final[v] = alpha[T-1,v] + b[T-1,v]
"""
import numpy as np

NEG = -np.inf


def trie(cands):
    """-> (parent, label, depth, term): node 0 = the empty prefix; depth ascending, within a depth parent ascending, within a parent
    by first appearance (lowest candidate index)."""
    parent, label, depth, level = [-1], [-1], [0], {(): 0}
    for d in range(max((len(c) for c in cands), default=0)):
        keys = {}
        for c in cands:                                    # candidate order = first appearance
            if len(c) > d:
                keys.setdefault((level[tuple(c[:d])], int(c[d])), tuple(c[:d + 1]))
        nxt = {}
        for (p, y), pre in sorted(keys.items(), key=lambda kv: kv[0][0]):      # stable: parents ascending, appearance kept
            nxt[pre] = len(parent)
            parent.append(p), label.append(y), depth.append(d + 1)
        level.update(nxt)
    return parent, label, depth, [level[tuple(c)] for c in cands]


def path(parent, v):
    """root -> v"""
    out = []
    while v >= 0:
        out.append(v)
        v = parent[v]
    return out[::-1]


def tree_dp(b, e, parent, best=False):
    """-> final [N] float64: log P(prefix_v | x) per node (best=True: the best alignment's score; a tie takes the blank)"""
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    T, N = b.shape
    al = np.full((T, N), NEG)
    al[0, 0] = 0.0
    for t in range(T):
        for v in range(N):                                 # parent[v] < v: (t, parent v) is done
            if t == 0 and v == 0:
                continue
            x = al[t - 1, v] + b[t - 1, v] if t > 0 else NEG
            z = al[t, parent[v]] + e[t, v] if v > 0 else NEG
            al[t, v] = (z if z > x else x) if best else np.logaddexp(x, z)
    return al[T - 1] + b[T - 1]


def tree_lattice(m, feats, cands):
    """m: OracleTransducer, feats [T, F] -> (parent, label, depth, term, b, e) with b, e float32 [T, N] of the candidates' trie."""
    parent, label, depth, term = trie(cands)
    enc, _ = m.encoder(np.asarray(feats, np.float32)[None])
    enc = enc[0]
    T, N = enc.shape[0], len(parent)
    g, st = m.predictor([m.bos])
    states = [(g[0], st)]
    for v in range(1, N):
        g, st = m.predictor([int(label[v])], states[parent[v]][1])
        states.append((g[0], st))
    b, e = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    kids = [[] for _ in range(N)]
    for v in range(1, N):
        kids[parent[v]].append(v)
    for v in range(N):
        lp, _ = m.joint_logp(np.repeat(states[v][0][None], T, 0), enc)
        b[:, v] = lp[:, m.blank]
        for ch in kids[v]:
            e[:, ch] = lp[:, int(label[ch])]
    return parent, label, depth, term, b, e
