"""Float64 reference of the lattice's edge posteriors (lasr_align_post_* / lasr_lattice_post): the forward-backward algorithm over
the b / e arrays of tests/lattice_ref.py, and per label the statistics of its emission frame.

    alpha as lattice_ref.forward;  loglik = alpha[T-1,U] + b[T-1,U]
    beta[T-1,U] = b[T-1,U], beta[t,u] = logaddexp(beta[t+1,u] + b[t,u], beta[t,u+1] + e[t,u])   (a missing successor counts -inf)
    occ_b[t,u] = exp(alpha[t,u] + b[t,u] + beta[t+1,u] - loglik) (t < T-1), occ_b[T-1,U] = 1, occ_b[T-1,u<U] = 0
    occ_e[t,u] = exp(alpha[t,u] + e[t,u] + beta[t,u+1] - loglik) (u < U),   occ_e[t,U] = 0
    label u = 1..U, p(t) = occ_e[t,u-1]: mean = sum t p, var = sum (t - mean)^2 p, peak_frame = the first t of the largest p, peak = that p
    loglik = -inf: every occupancy 0, mean -1, var 0, peak_frame -1, peak 0.

Pinned in test_lattice_post_cpu.py against enumeration of every path, a closed form and finite differences of lattice_ref.forward."""
import numpy as np

NEG = -np.inf


def _lae(x, z):
    m = max(x, z)
    if m == NEG:
        return NEG
    return m + np.log1p(np.exp(-abs(x - z)))


def alpha_beta(b, e, U):
    """-> (alpha [T, U + 1], beta [T, U + 1], loglik, loglik_bwd) in float64"""
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    T = b.shape[0]
    al = np.full((T, U + 1), NEG)
    be = np.full((T, U + 1), NEG)
    al[0, 0] = 0.0
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            x = al[t - 1, u] + b[t - 1, u] if t > 0 else NEG
            z = al[t, u - 1] + e[t, u - 1] if u > 0 else NEG
            al[t, u] = _lae(x, z)
    be[T - 1, U] = b[T - 1, U]
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            if t == T - 1 and u == U:
                continue
            x = be[t + 1, u] + b[t, u] if t < T - 1 else NEG
            z = be[t, u + 1] + e[t, u] if u < U else NEG
            be[t, u] = _lae(x, z)
    return al, be, float(al[T - 1, U] + b[T - 1, U]), float(be[0, 0])


def posteriors(b, e, U):
    """-> dict(loglik, loglik_bwd, occ_b, occ_e [T, U + 1] float64, tok_mean, tok_var, tok_peak [U] float64, tok_peak_frame [U] int)"""
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    T = b.shape[0]
    al, be, ll, llb = alpha_beta(b, e, U)
    ob, oe = np.zeros((T, U + 1)), np.zeros((T, U + 1))
    mean, var, peak, pf = np.full(U, -1.0), np.zeros(U), np.zeros(U), np.full(U, -1, np.int64)
    if ll != NEG:
        for t in range(T):
            for u in range(U + 1):
                if t < T - 1:
                    ob[t, u] = np.exp(al[t, u] + b[t, u] + be[t + 1, u] - ll)
                elif u == U:
                    ob[t, u] = 1.0
                if u < U:
                    oe[t, u] = np.exp(al[t, u] + e[t, u] + be[t, u + 1] - ll)
        ts = np.arange(T, dtype=np.float64)
        for u in range(U):
            p = oe[:, u]
            mean[u] = float(np.sum(ts * p))
            var[u] = float(np.sum((ts - mean[u]) ** 2 * p))
            pf[u] = int(np.argmax(p))                    # the first of the largest
            peak[u] = float(p[pf[u]])
    return dict(loglik=ll, loglik_bwd=llb, occ_b=ob, occ_e=oe, tok_mean=mean, tok_var=var, tok_peak=peak, tok_peak_frame=pf)


def minus_inf_lattice():
    """T = 5, U = 3, multiples of 1/64 with two impossible edges: e[0,0] and b[2,1]"""
    rng = np.random.default_rng(99)
    b = -(rng.integers(0, 513, (5, 4)) / 64.0).astype(np.float32)
    e = -(rng.integers(0, 513, (5, 4)) / 64.0).astype(np.float32)
    e[0, 0] = NEG
    b[2, 1] = NEG
    return b, e


def impossible_lattice():
    """T = 4, U = 2: label 2 can never be emitted, loglik = -inf"""
    rng = np.random.default_rng(5)
    b = -(rng.integers(0, 513, (4, 3)) / 64.0).astype(np.float32)
    e = -(rng.integers(0, 513, (4, 3)) / 64.0).astype(np.float32)
    e[:, 1] = NEG
    return b, e


def brute(b, e, U):
    """occupancies by enumeration of every path (lattice_ref.all_paths): -> (loglik, occ_b, occ_e)"""
    import lattice_ref as R
    b, e = np.asarray(b, np.float64), np.asarray(e, np.float64)
    T = b.shape[0]
    paths = [list(fr) for fr in R.all_paths(T, U)]
    sc = np.array([R.path_score(b, e, fr) for fr in paths])
    ll = float(np.logaddexp.reduce(sc))
    ob, oe = np.zeros((T, U + 1)), np.zeros((T, U + 1))
    for fr, s in zip(paths, sc):
        w = float(np.exp(s - ll))
        u = 0
        for t in range(T):
            while u < U and fr[u] == t:
                oe[t, u] += w
                u += 1
            ob[t, u] += w
    return ll, ob, oe
