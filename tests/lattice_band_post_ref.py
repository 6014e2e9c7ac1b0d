"""Float64 reference of the banded lattice's edge posteriors (lasr_align_band_post_* / lasr_lattice_band_post), written from the
definitions of include/lasr.h directly on band arrays.

Band layout as tests/lattice_band_ref.py: row t of a [T, w] array holds u = lo[t] + k at k; b and e count -inf outside the windows.

    alpha as lattice_band_ref.forward;  loglik = alpha[T-1,U] + b[T-1,U]
    beta[T-1,U] = b[T-1,U], beta[t,u] = logaddexp(beta[t+1,u] + b[t,u], beta[t,u+1] + e[t,u]) on window cells
        (t+1,u) is inside iff t < T-1 and u >= lo[t+1];  (t,u+1) is inside iff u + 1 < lo[t] + w;  a successor outside counts -inf
    occ_b[t,u] = exp(alpha[t,u] + b[t,u] + beta[t+1,u] - loglik) where (t+1,u) is inside, else 0;  occ_b[T-1,U] = 1
    occ_e[t,u] = exp(alpha[t,u] + e[t,u] + beta[t,u+1] - loglik) where (t,u+1) is inside, else 0
    label u = 1..U, p(t) = occ_e[t,u-1] on the frames whose window holds column u-1 (0 elsewhere): mean, var, peak_frame, peak as
    lattice_post_ref;  loglik = -inf: every occupancy 0, mean -1, var 0, peak_frame -1, peak 0.

The operations and their order are lattice_post_ref's on the spread lattice, so the two agree to the last bit (pinned in
test_lattice_band_post_cpu.py, with enumeration of every path on small lattices)."""
import numpy as np

from lattice_post_ref import _lae

NEG = -np.inf


def alpha_beta(bb, eb, lo, U):
    """bb / eb [T, w] in band layout -> (alpha [T, w], beta [T, w], loglik, loglik_bwd) in float64"""
    bb, eb = np.asarray(bb, np.float64), np.asarray(eb, np.float64)
    T, w = bb.shape
    lo = [int(v) for v in lo]
    al = np.full((T, w), NEG)
    be = np.full((T, w), NEG)
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
            al[t, k] = _lae(x, z)
    for t in range(T - 1, -1, -1):
        for k in range(w - 1, -1, -1):
            u = lo[t] + k
            if t == T - 1 and u == U:
                be[t, k] = bb[t, k]
                continue
            x = z = NEG
            if t < T - 1 and u >= lo[t + 1]:
                x = be[t + 1, u - lo[t + 1]] + bb[t, k]
            if k + 1 < w:
                z = be[t, k + 1] + eb[t, k]
            be[t, k] = _lae(x, z)
    return al, be, float(al[T - 1, w - 1] + bb[T - 1, w - 1]), float(be[0, 0])


def posteriors(bb, eb, lo, U):
    """-> dict(loglik, loglik_bwd, occ_b, occ_e [T, w] float64 in band layout, tok_mean, tok_var, tok_peak [U] float64,
    tok_peak_frame [U] int)"""
    bb, eb = np.asarray(bb, np.float64), np.asarray(eb, np.float64)
    T, w = bb.shape
    lo = [int(v) for v in lo]
    al, be, ll, llb = alpha_beta(bb, eb, lo, U)
    ob, oe = np.zeros((T, w)), np.zeros((T, w))
    mean, var, peak, pf = np.full(U, -1.0), np.zeros(U), np.zeros(U), np.full(U, -1, np.int64)
    if ll != NEG:
        for t in range(T):
            for k in range(w):
                u = lo[t] + k
                if t < T - 1:
                    if u >= lo[t + 1]:
                        ob[t, k] = np.exp(al[t, k] + bb[t, k] + be[t + 1, u - lo[t + 1]] - ll)
                elif u == U:
                    ob[t, k] = 1.0
                if k + 1 < w:
                    oe[t, k] = np.exp(al[t, k] + eb[t, k] + be[t, k + 1] - ll)
        for u in range(U):
            m, best, bt = 0.0, -1.0, -1
            ts = [t for t in range(T) if 0 <= u - lo[t] < w]          # a contiguous range of frames
            assert ts == list(range(ts[0], ts[-1] + 1))
            for t in ts:
                p = oe[t, u - lo[t]]
                m += t * p
                if p > best:
                    best, bt = p, t
            v = 0.0
            for t in ts:
                v += (t - m) ** 2 * oe[t, u - lo[t]]
            mean[u], var[u], peak[u], pf[u] = m, v, best, bt
    return dict(loglik=ll, loglik_bwd=llb, occ_b=ob, occ_e=oe, tok_mean=mean, tok_var=var, tok_peak=peak, tok_peak_frame=pf)


def sum_invariants(ob, oe, lo, U):
    """-> the largest of |sum_u occ_b[t,u] - 1| over t and |sum_t occ_e[t,u] - 1| over u < U, from band arrays (float64 sums)"""
    ob, oe = np.asarray(ob, np.float64), np.asarray(oe, np.float64)
    T, w = ob.shape
    worst = float(np.abs(ob.sum(axis=1) - 1).max())
    col = np.zeros(U + 1)
    for t in range(T):
        col[lo[t]:lo[t] + w] += oe[t]
    if U:
        worst = max(worst, float(np.abs(col[:U] - 1).max()))
    return worst


def random_windows(rng, T, U, w):
    """valid windows of width w drawn at random: lo[0] = 0, lo[T-1] = U + 1 - w, non-decreasing (T == 1 needs w = U + 1)"""
    top = U + 1 - w
    if T == 1:
        assert top == 0
        return [0]
    mid = sorted(int(v) for v in rng.integers(0, top + 1, T - 2))
    return [0] + mid + [top]
