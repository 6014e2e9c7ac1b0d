"""Float64 reference of the teacher-forced RNN-T lattice (lasr_align_* / lasr_lattice_dp): the two log-softmax entries per cell
from the numpy oracle's encoder, predictor and joint, and the two recursions over them.

    b[t,u] = lp[t,u,blank], e[t,u] = lp[t,u,y_{u+1}],  lp[t,u,:] = log_softmax(joint(g_u, f_t))
    alpha[0,0] = 0, alpha[t,u] = logaddexp(alpha[t-1,u] + b[t-1,u], alpha[t,u-1] + e[t,u-1]);  loglik = alpha[T-1,U] + b[T-1,U]
    viterbi: the same with max; the emission predecessor (t, u-1) wins only if STRICTLY greater than the blank one (t-1, u).

`lattice` composes OracleTransducer.encoder / .predictor / .joint_logp, each pinned by the reference's goldens (test_oracle.py); the
composition itself (Transducer.forward, models.py:308-359, and loss.py:77-79) is not pinned by a golden of the reference's own."""
import itertools

import numpy as np

NEG = -np.inf


def lattice(m, feats, y):
    """m: OracleTransducer, feats [T, F], y: U non-blank ids -> (b, e) float32 [T, U + 1] (e[:, U] = 0)."""
    enc, _ = m.encoder(np.asarray(feats, np.float32)[None])
    enc = enc[0]
    T, U = enc.shape[0], len(y)
    g, st = m.predictor([m.bos])
    gs = [g[0]]
    for tok in y:
        g, st = m.predictor([int(tok)], st)
        gs.append(g[0])
    b = np.zeros((T, U + 1), np.float32)
    e = np.zeros((T, U + 1), np.float32)
    for u in range(U + 1):
        lp, _ = m.joint_logp(np.repeat(gs[u][None], T, 0), enc)
        b[:, u] = lp[:, m.blank]
        if u < U:
            e[:, u] = lp[:, int(y[u])]
    return b, e


def forward(b, e, U):
    """-> log P(y | x) in float64"""
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    T = b.shape[0]
    al = np.full((T, U + 1), NEG)
    al[0, 0] = 0.0
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            x = al[t - 1, u] + b[t - 1, u] if t > 0 else NEG
            z = al[t, u - 1] + e[t, u - 1] if u > 0 else NEG
            al[t, u] = np.logaddexp(x, z)
    return float(al[T - 1, U] + b[T - 1, U])


def viterbi(b, e, U):
    """-> (score incl. the final blank, frames [U]): frames[u-1] = the frame on which label u is emitted on the best path"""
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    T = b.shape[0]
    v = np.full((T, U + 1), NEG)
    em = np.zeros((T, U + 1), bool)
    v[0, 0] = 0.0
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            x = v[t - 1, u] + b[t - 1, u] if t > 0 else NEG
            z = v[t, u - 1] + e[t, u - 1] if u > 0 else NEG
            em[t, u] = z > x                       # a tie takes the blank predecessor
            v[t, u] = z if em[t, u] else x
    frames = [0] * U
    t, u = T - 1, U
    while u > 0:
        if em[t, u]:
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    return float(v[T - 1, U] + b[T - 1, U]), frames


def path_score(b, e, frames):
    """score of the path that emits label u on frames[u-1] (non-decreasing), final blank included"""
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    T, U = b.shape[0], len(frames)
    s, u = 0.0, 0
    for t in range(T):
        while u < U and frames[u] == t:
            s += e[t, u]
            u += 1
        s += b[t, u]
    assert u == U
    return float(s)


def all_paths(T, U):
    """every monotone assignment of U labels to T frames"""
    return itertools.combinations_with_replacement(range(T), U)
