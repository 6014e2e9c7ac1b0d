"""Float64 reference of the banded RNN-T lattice (lasr_band_windows / lasr_align_band_* / lasr_lattice_band_dp), written from the
definitions of include/lasr.h.

An utterance of T frames and U labels with the requested width `band` has the effective width w = U + 1 (T == 1) or
min(band, U + 1); frame t owns the columns [lo[t], lo[t] + w).  Band layout: row t of a [T, w] array holds u = lo[t] + k at k.
b and e are lattice_ref's terms on the window cells and count -inf outside, and the recursions are lattice_ref's on that lattice:

    alpha[0,0] = 0, alpha[t,u] = logaddexp(alpha[t-1,u] + b[t-1,u], alpha[t,u-1] + e[t,u-1])  (a predecessor outside its window: -inf)
    loglik = alpha[T-1,U] + b[T-1,U];  viterbi the same with max, the emission predecessor winning only if STRICTLY greater

No path through the windows: loglik = viterbi = -inf, frames all -1 (and touch 0, the windows stay)."""
import numpy as np

NEG = -np.inf


# ------------------------------------------------------------------------------- window arithmetic (integers only)
def width(T, U, band):
    return U + 1 if T == 1 else min(band, U + 1)


def valid(T, U, w, lo):
    lo = [int(v) for v in lo]
    return (len(lo) == T and lo[0] == 0 and lo[-1] == U + 1 - w and all(0 <= v <= U + 1 - w for v in lo)
            and all(lo[t] >= lo[t - 1] for t in range(1, T)))


def linear(T, U, band):
    w = width(T, U, band)
    return [0 if T == 1 else (t * (U + 1 - w)) // (T - 1) for t in range(T)]


def counts(T, U, frames):
    """c(t) = #{u : frames[u] < t} for t = 0..T (c(T) = U): the path occupies the columns c(t)..c(t+1) on frame t"""
    c = [sum(1 for f in frames if f < t) for t in range(T)]
    return c + [U]


def recentre(T, U, band, frames, lo):
    """-> (lo', touch) from a best path found inside the windows lo"""
    w = width(T, U, band)
    assert valid(T, U, w, lo) and len(frames) == U
    c = counts(T, U, frames)
    top = U + 1 - w
    new = [min(max((c[t] + c[t + 1]) // 2 - w // 2, 0), top) for t in range(T)]
    new[0], new[T - 1] = 0, top
    touch = int(any((lo[t] > 0 and c[t] == lo[t]) or (lo[t] + w < U + 1 and c[t + 1] == lo[t] + w - 1) for t in range(T)))
    return new, touch


# ------------------------------------------------------------------------------- band layout
def cut(x, lo, w):
    """a full [T, U + 1] array -> its band [T, w]"""
    x = np.asarray(x)
    return np.stack([x[t, lo[t]:lo[t] + w] for t in range(x.shape[0])])


def spread(xb, lo, U, fill=NEG):
    """a band [T, w] -> the full [T, U + 1] float64 array, `fill` outside the windows"""
    xb = np.asarray(xb, np.float64)
    T, w = xb.shape
    out = np.full((T, U + 1), fill)
    for t in range(T):
        out[t, lo[t]:lo[t] + w] = xb[t]
    return out


# ------------------------------------------------------------------------------- the recursions, on band arrays
def forward(bb, eb, lo, U):
    """bb / eb: [T, w] in band layout -> loglik of the banded lattice (float64)"""
    bb, eb = np.asarray(bb, np.float64), np.asarray(eb, np.float64)
    T, w = bb.shape
    al = np.full((T, w), NEG)
    for t in range(T):
        for k in range(w):
            u = lo[t] + k
            if t == 0 and u == 0:
                al[t, k] = 0.0
                continue
            x = z = NEG
            if t > 0 and 0 <= u - lo[t - 1] < w:
                x = al[t - 1, u - lo[t - 1]] + bb[t - 1, u - lo[t - 1]]
            if k > 0:
                z = al[t, k - 1] + eb[t, k - 1]
            al[t, k] = NEG if max(x, z) == NEG else np.logaddexp(x, z)
    return float(al[T - 1, w - 1] + bb[T - 1, w - 1])


def viterbi(bb, eb, lo, U):
    """-> (score incl. the final blank, frames [U]); no path: (-inf, [-1] * U)"""
    bb, eb = np.asarray(bb, np.float64), np.asarray(eb, np.float64)
    T, w = bb.shape
    v = np.full((T, w), NEG)
    em = np.zeros((T, w), bool)
    for t in range(T):
        for k in range(w):
            u = lo[t] + k
            if t == 0 and u == 0:
                v[t, k] = 0.0
                continue
            x = z = NEG
            if t > 0 and 0 <= u - lo[t - 1] < w:
                x = v[t - 1, u - lo[t - 1]] + bb[t - 1, u - lo[t - 1]]
            if k > 0:
                z = v[t, k - 1] + eb[t, k - 1]
            em[t, k] = z > x                       # a tie takes the blank predecessor
            v[t, k] = z if em[t, k] else x
    score = float(v[T - 1, w - 1] + bb[T - 1, w - 1])
    if score == NEG:
        return score, [-1] * U
    frames = [0] * U
    t, u = T - 1, U
    while u > 0:
        if t == 0 or em[t, u - lo[t]]:
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    return score, frames


def pass_loop(b, e, U, band, max_passes, lo=None):
    """the pass loop of lasr_align_band_* on a FULL lattice b / e [T, U + 1]: -> list of (lo, score, frames, touch) per pass run.
    Ends when the path does not touch, when no window changed, or at max_passes."""
    T = np.asarray(b).shape[0]
    w = width(T, U, band)
    lo = linear(T, U, band) if lo is None else [int(v) for v in lo]
    out = []
    while True:
        score, frames = viterbi(cut(b, lo, w), cut(e, lo, w), lo, U)
        if score == NEG:
            new, touch = list(lo), 0
        else:
            new, touch = recentre(T, U, band, frames, lo)
        out.append((list(lo), score, frames, touch))
        if not touch or new == lo or len(out) >= max_passes:
            return out
        lo = new


def band_lattice(m, feats, y, lo, w):
    """m: OracleTransducer, feats [T, F], y: U non-blank ids -> (b, e) float32 [T, w] in band layout: the oracle's encoder, predictor
    and joint composed over the window cells only (e at u == U is 0)."""
    enc, _ = m.encoder(np.asarray(feats, np.float32)[None])
    enc = enc[0]
    T, U = enc.shape[0], len(y)
    g, st = m.predictor([m.bos])
    gs = [g[0]]
    for tok in y:
        g, st = m.predictor([int(tok)], st)
        gs.append(g[0])
    b = np.zeros((T, w), np.float32)
    e = np.zeros((T, w), np.float32)
    for t in range(T):
        us = list(range(lo[t], lo[t] + w))
        lp, _ = m.joint_logp(np.stack([gs[u] for u in us]), np.repeat(enc[t][None], w, 0))
        b[t] = lp[:, m.blank]
        for k, u in enumerate(us):
            if u < U:
                e[t, k] = lp[k, int(y[u])]
    return b, e


# ------------------------------------------------------------------------------- the planted-path fixture
def planted(T, U, band, seed):
    """A full lattice of multiples of 1/64 whose best path is known: -1/64 on the cells of a planted path, random values in
    [-8, -1] everywhere else -- any other path has as many terms and at least one of them <= -1, so the planted one is the unique
    best.  The path runs along the diagonal plus a triangular bulge of `band` labels at mid-utterance (integer arithmetic), so the
    linear windows do not contain it.  -> (b, e float32 [T, U + 1], frames [U])"""
    rng = np.random.default_rng(seed)
    b = -(rng.integers(64, 513, (T, U + 1)) / 64.0).astype(np.float32)
    e = -(rng.integers(64, 513, (T, U + 1)) / 64.0).astype(np.float32)
    cc = [0]
    for t in range(1, T):
        cc.append(max(cc[-1], min(U, t * U // (T - 1) + band * min(t, T - 1 - t) * 2 // (T - 1))))
    cc.append(U)
    frames = [min(t for t in range(T) if cc[t + 1] > u) for u in range(U)]
    for t in range(T):
        for u in range(cc[t], cc[t + 1]):
            e[t, u] = -1.0 / 64
        b[t, cc[t + 1]] = -1.0 / 64
    return b, e, frames


PLANTED = [(96, 64, 12, 9664), (40, 12, 6, 4012)]       # (T, U, band, seed)
PLANTED_MAX_PASSES = 6
