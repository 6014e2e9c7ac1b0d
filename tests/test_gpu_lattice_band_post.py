"""Banded lattice posteriors on the GPU (lasr_align_band_post_pcm / lasr_align_band_post_feats / lasr_lattice_band_post):
the occupancy of every edge of the teacher-forced RNN-T lattice restricted to a band of w labels per frame, over the alignments that
stay inside the windows, and per label the statistics of its emission frame.

Expected values: tests/lattice_band_post_ref.py (float64, pinned in test_lattice_band_post_cpu.py).  Bounds: those of
test_gpu_lattice_post.py, which carry over because the banded reference's own invariants hold to 4e-11 at the largest shape here
(2200 x 2000, band 32): loglik 1e-8, occupancies (<= 1, rounded once to f32) 2e-7, tok_mean 1e-9 T, tok_var 1e-9 T^2, tok_peak 1e-9,
f32 sum invariants 1e-6; the peak's frame must be equal, given a margin > 1e-6 between a label's two largest posteriors.  Model
tests: |d log occ| <= 2 (T + U) 2e-3 on the cells with a reference occupancy >= 1e-3, as in test_gpu_lattice_post.py."""
import ctypes as C

import numpy as np
import pytest

import bf16_exact as X
import lattice_band_post_ref as Q
import lattice_band_ref as B
from libreasr_amd import _native as N
from test_alignment_cpu import utterances
from test_gpu_lattice import SLOTS, TERM_TOL, feats_all, make, oracle, transcripts
from test_gpu_lattice_band import align, band_reference

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0, 1), (1, 3, 2), (5, 0, 4), (64, 63, 8), (70, 130, 17), (300, 5, 3), (40, 600, 300), (600, 700, 32), (2200, 2000, 32)]
N_RANDOM = len(SHAPES)
I_TIE, I_INF, I_NONE, I_RANDWIN = N_RANDOM, N_RANDOM + 1, N_RANDOM + 2, N_RANDOM + 3
POST_KEYS = ("occ_blank", "occ_emit", "tok_mean", "tok_var", "tok_peak_frame", "tok_peak")
_CACHE = {}


def vp(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def rand64(rng, T, U):
    return (-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32), -(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32))


def batch():
    """(T, U, w, lo, band b, band e) of every lattice of (a) and their float64 posteriors, computed once: the shapes under linear
    windows, then all-tie, -inf entries inside the band, disconnected windows, and one lattice under random valid windows"""
    if "batch" not in _CACHE:
        rng = np.random.default_rng(5757)
        cases = []
        for T, U, band in SHAPES:
            b, e = rand64(rng, T, U)
            w, lo = B.width(T, U, band), B.linear(T, U, band)
            cases.append((T, U, w, lo, B.cut(b, lo, w), B.cut(e, lo, w)))
        lo = B.linear(9, 7, 3)
        cases.append((9, 7, 3, lo, np.full((9, 3), -0.5, np.float32), np.full((9, 3), -0.5, np.float32)))
        b, e = rand64(rng, 9, 7)
        bb, eb = B.cut(b, lo, 3).copy(), B.cut(e, lo, 3).copy()
        eb[0, 0] = -np.inf
        bb[4, 1] = -np.inf
        cases.append((9, 7, 3, lo, bb, eb))
        b, e = rand64(rng, 3, 4)
        cases.append((3, 4, 2, [0, 0, 3], B.cut(b, [0, 0, 3], 2), B.cut(e, [0, 0, 3], 2)))
        b, e = rand64(rng, 50, 60)
        lo = Q.random_windows(rng, 50, 60, 9)
        assert B.valid(50, 60, 9, lo) and lo != B.linear(50, 60, 9)
        cases.append((50, 60, 9, lo, B.cut(b, lo, 9), B.cut(e, lo, 9)))
        refs = [Q.posteriors(bb, eb, lo, U) for T, U, w, lo, bb, eb in cases]
        assert refs[I_NONE]["loglik"] == -np.inf and all(np.isfinite(r["loglik"]) for i, r in enumerate(refs) if i != I_NONE)
        _CACHE["batch"] = (cases, refs)
    return _CACHE["batch"]


def raw_post(eng, b, e, Ts, Us, Ws, los, full=True):
    """lasr_lattice_band_post on concatenated band lattices (numpy arrays or device tensors) -> the output arrays, in the order of the
    C arguments"""
    n, cells, su = len(Ts), int(sum(int(t) * int(w) for t, w in zip(Ts, Ws))), max(int(sum(Us)), 1)
    ll = np.zeros(n)
    outs = [np.zeros(n), np.zeros(cells, np.float32), np.zeros(cells, np.float32), np.zeros(su), np.zeros(su), np.zeros(su, np.int32),
            np.zeros(su)] if full else [None] * 7
    ptr = lambda x: C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else vp(x)
    arr = lambda xs: np.ascontiguousarray(np.asarray(xs, np.int32))
    eng._chk(eng.lib.lasr_lattice_band_post(eng.ctx, ptr(b), ptr(e), vp(arr(Ts)), vp(arr(Us)), vp(arr(Ws)), vp(arr(los)), n, vp(ll),
                                            *[vp(x) for x in outs]))
    return [ll] + outs


def kernel_run():
    """one engine, the batch of (a) through every way in: the Python wrapper, raw with host inputs, raw with device inputs, raw with only
    loglik asked for, the lattices of at most 256 columns on their own, and lasr_lattice_band_dp"""
    if "run" not in _CACHE:
        import torch
        cases, _ = batch()
        Ts, Us, Ws = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
        los = [v for c in cases for v in c[3]]
        cat_b, cat_e = np.concatenate([c[4].reshape(-1) for c in cases]), np.concatenate([c[5].reshape(-1) for c in cases])
        small = [i for i, c in enumerate(cases) if c[2] <= 256]
        assert len(small) < len(cases) and len({c[2] for c in cases}) > 3             # both kernel instances, mixed widths
        eng = make("tiny")
        try:
            got = eng.lattice_band_post([c[4] for c in cases], [c[5] for c in cases], [c[3] for c in cases], Us)
            host = raw_post(eng, cat_b, cat_e, Ts, Us, Ws, los)
            dev = raw_post(eng, torch.as_tensor(cat_b).to(eng.device), torch.as_tensor(cat_e).to(eng.device), Ts, Us, Ws, los)
            only = raw_post(eng, cat_b, cat_e, Ts, Us, Ws, los, full=False)
            got_small = eng.lattice_band_post([cases[i][4] for i in small], [cases[i][5] for i in small], [cases[i][3] for i in small],
                                              [cases[i][1] for i in small])
            dp = eng.lattice_band_dp([c[4] for c in cases], [c[5] for c in cases], [c[3] for c in cases], Us, viterbi=False)
        finally:
            eng.close()
        _CACHE["run"] = (got, host, dev, only, small, got_small, dp)
    return _CACHE["run"]


def structure(r, lo, U):
    """what holds in every finite result, in band layout: nothing leaves a window, the last frame ends the path"""
    ob, oe = r["occ_blank"], r["occ_emit"]
    T, w = ob.shape
    assert np.all(oe[:, w - 1] == 0)
    for t in range(T - 1):
        assert np.all(ob[t, :max(0, min(w, lo[t + 1] - lo[t]))] == 0), t          # (t + 1, u) lies below the next window
    assert np.all(ob[T - 1, :w - 1] == 0) and ob[T - 1, w - 1] == 1


def sum_invariants(r, lo, U, tol=1e-6):
    worst = Q.sum_invariants(r["occ_blank"], r["occ_emit"], [int(v) for v in lo], U)
    assert worst <= tol, worst
    structure(r, [int(v) for v in lo], U)
    return worst


def check_no_path(g, T, w, U):
    assert g["loglik"] == -np.inf
    assert g["occ_blank"].shape == (T, w) and np.all(g["occ_blank"] == 0) and np.all(g["occ_emit"] == 0)
    assert list(g["tok_mean"]) == [-1.0] * U and list(g["tok_var"]) == [0.0] * U
    assert list(g["tok_peak_frame"]) == [-1] * U and list(g["tok_peak"]) == [0.0] * U


# ------------------------------------------------------------------------------- (a) the kernels against float64
def test_kernels_against_float64():
    cases, refs = batch()
    got = kernel_run()[0]
    worst = dict(loglik=0.0, occ=0.0, mean=0.0, var=0.0, peak=0.0, sums=0.0)
    margin = np.inf
    for i, ((T, U, w, lo, bb, eb), g, ref) in enumerate(zip(cases, got, refs)):
        assert g["occ_blank"].shape == (T, w) and g["occ_emit"].shape == (T, w) and g["occ_blank"].dtype == np.float32
        for k in POST_KEYS:
            assert not np.any(np.isnan(g[k])), (i, k)
        if ref["loglik"] == -np.inf:                      # the disconnected windows: the -inf convention
            check_no_path(g, T, w, U)
            assert g["loglik_bwd"] == -np.inf
            continue
        d_ll = max(abs(g["loglik"] - ref["loglik"]), abs(g["loglik_bwd"] - ref["loglik_bwd"]))
        d_occ = max(float(np.abs(g["occ_blank"] - ref["occ_b"]).max()), float(np.abs(g["occ_emit"] - ref["occ_e"]).max()))
        d_mean = float(np.abs(g["tok_mean"] - ref["tok_mean"]).max()) if U else 0.0
        d_var = float(np.abs(g["tok_var"] - ref["tok_var"]).max()) if U else 0.0
        d_peak = float(np.abs(g["tok_peak"] - ref["tok_peak"]).max()) if U else 0.0
        s = sum_invariants(g, lo, U)
        print(f"band lattice {i} T {T} U {U} w {w}: dloglik {d_ll:.3g} docc {d_occ:.3g} dmean {d_mean:.3g} dvar {d_var:.3g} dpeak {d_peak:.3g} sums {s:.3g}")
        assert d_ll <= 1e-8, (i, d_ll)
        assert d_occ <= 2e-7, (i, d_occ)
        assert d_mean <= 1e-9 * max(1, T) and d_var <= 1e-9 * max(1, T) ** 2 and d_peak <= 1e-9, (i, d_mean, d_var, d_peak)
        worst = dict(loglik=max(worst["loglik"], d_ll), occ=max(worst["occ"], d_occ), mean=max(worst["mean"], d_mean / max(1, T)),
                     var=max(worst["var"], d_var / max(1, T) ** 2), peak=max(worst["peak"], d_peak), sums=max(worst["sums"], s))
        if i < N_RANDOM or i == I_RANDWIN:                # every label of the random lattices: the peak's frame, given a clear winner
            for u in range(U):
                p = np.sort(np.array([ref["occ_e"][t, u - lo[t]] for t in range(T) if 0 <= u - lo[t] < w]))[::-1]
                if p.size > 1:
                    margin = min(margin, float(p[0] - p[1]))
            assert margin > 1e-6, (i, margin)
            assert [int(t) for t in g["tok_peak_frame"]] == [int(t) for t in ref["tok_peak_frame"]], i
    print(f"maxima: {worst}; smallest margin between the two largest posteriors of a label: {margin:.3g}")
    g = got[I_INF]                                        # -inf entries: occupancy 0 on the impossible edges
    assert g["occ_emit"][0, 0] == 0 and g["occ_blank"][4, 1] == 0
    g = got[I_TIE]                                        # every in-band path ties: the first of equal posteriors is the peak
    ref = refs[I_TIE]
    assert [int(t) for t in g["tok_peak_frame"]] == [int(t) for t in ref["tok_peak_frame"]]


def test_device_inputs_null_outputs_and_the_small_instance():
    got, host, dev, only, small, got_small, _ = kernel_run()
    for h, d in zip(host, dev):
        assert h.tobytes() == d.tobytes()
    assert only[0].tobytes() == host[0].tobytes()         # every posterior output null: loglik alone
    assert [g["loglik"] for g in got] == list(host[0]) and [g["loglik_bwd"] for g in got] == list(host[1])
    assert np.concatenate([g["occ_blank"].reshape(-1) for g in got]).tobytes() == host[2].tobytes()
    assert np.concatenate([g["occ_emit"].reshape(-1) for g in got]).tobytes() == host[3].tobytes()
    for j, i in enumerate(small):                         # the one-slot kernel instance and a parity stride of its own widest window
        assert got_small[j]["loglik"] == got[i]["loglik"] and got_small[j]["loglik_bwd"] == got[i]["loglik_bwd"], i
        for k in POST_KEYS:
            assert got_small[j][k].tobytes() == got[i][k].tobytes(), (i, k)


# ------------------------------------------------------------------------------- (b) bit-equality
def test_loglik_is_lattice_band_dp_bit_for_bit():
    got, *_, dp = kernel_run()
    assert [g["loglik"] for g in got] == [d["loglik"] for d in dp]


def test_full_width_band_equals_lattice_post():
    shapes = [(1, 0), (1, 3), (5, 0), (2, 1), (3, 2), (64, 63), (65, 64), (70, 130), (300, 5)]        # test_dp_kernel_exact's
    rng = np.random.default_rng(2024)
    bs = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in shapes]
    es = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in shapes]
    crng = np.random.default_rng(7)                                      # continuous values: the same operations in the same order
    bs.append(-crng.random((50, 31)).astype(np.float32) * 8)
    es.append(-crng.random((50, 31)).astype(np.float32) * 8)
    shapes.append((50, 30))
    eng = make("tiny")
    try:
        full = eng.lattice_post(bs, es)
        band = eng.lattice_band_post(bs, es, [[0] * T for T, _ in shapes], [U for _, U in shapes])
    finally:
        eng.close()
    for i, (f, g) in enumerate(zip(full, band)):
        assert set(f) == set(g)
        for k in f:
            assert np.asarray(f[k]).tobytes() == np.asarray(g[k]).tobytes(), (i, k)


# ------------------------------------------------------------------------------- (c) the model path, f32
def post_call(eng, entry, ys, idx=(0, 1, 2), **kw):
    if entry == "feats":
        return eng.align_band_post_feats(SLOTS[:len(idx)], [feats_all()[i] for i in idx], ys, **kw)
    return eng.align_band_post_pcm(SLOTS[:len(idx)], [utterances()[i] for i in idx], ys, **kw)


def same_bits(a, b, keys, what):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def check_model(eng, res, plain, name, ys, what):
    """res: align_band_post_*; plain: the same align_*(band=...) call; then lattice_band_post on res's lattices and windows, and the
    float64 posteriors of the oracle's band lattice on the reported windows"""
    again = eng.lattice_band_post([r["blank_lp"] for r in res], [r["emit_lp"] for r in res], [r["lo"] for r in res], [len(y) for y in ys])
    worst, none = 0.0, 0
    for i, (r, q, a, y) in enumerate(zip(res, plain, again, ys)):
        U, lo, w = len(y), [int(v) for v in r["lo"]], int(r["width"])
        T = len(lo)
        assert set(q) | set(POST_KEYS) == set(r)
        same_bits(q, r, q.keys(), f"{what} {i}: the banded call's fields")
        same_bits(a, r, POST_KEYS, f"{what} {i}: the same kernels on the same inputs")
        assert a["loglik"] == r["loglik"]
        assert r["occ_blank"].shape == (T, w) and r["occ_emit"].shape == (T, w) and r["tok_peak_frame"].shape == (U,)
        bb, eb, ll, _, _ = band_reference(name, y, i, lo, w)
        key = ("post", name, tuple(y), i, tuple(lo), w)
        if key not in _CACHE:
            _CACHE[key] = Q.posteriors(bb, eb, lo, U)
        ref = _CACHE[key]
        if ll == -np.inf:                                 # the windows leave no path: the sentinel values on both sides
            none += 1
            check_no_path(r, T, w, U)
            assert ref["loglik"] == -np.inf and np.all(ref["occ_e"] == 0) and list(ref["tok_peak_frame"]) == [-1] * U
            continue
        sum_invariants(r, lo, U)
        for k_gpu, k_ref in (("occ_blank", "occ_b"), ("occ_emit", "occ_e")):
            m = ref[k_ref] >= 1e-3
            if not m.any():
                continue
            d = float(np.abs(np.log(r[k_gpu][m].astype(np.float64)) - np.log(ref[k_ref][m])).max())
            worst = max(worst, d)
            assert d <= 2 * (T + U) * TERM_TOL, (what, i, k_gpu, d)
        assert np.all((0 <= r["tok_mean"]) & (r["tok_mean"] <= T - 1 + 1e-9)) and np.all(r["tok_var"] >= 0)
    print(f"{what}: max |d log occ| over the cells with occupancy >= 1e-3: {worst:.3g}; utterances without a path: {none}")
    return none


@pytest.mark.parametrize("entry", ["feats", "pcm"])
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_model_path(name, entry):
    eng = make(name)
    try:
        none = 0
        for kind in ("greedy", "rand40"):
            ys = transcripts(name, kind)
            what = f"{name} {entry} {kind}"
            for passes in (1, 4):
                plain = align(eng, entry, ys, lattice=True, band=6, max_passes=passes)
                res = post_call(eng, entry, ys, lattice=True, band=6, max_passes=passes)
                none += check_model(eng, res, plain, name, ys, f"{what} band 6 passes {passes}")
            # a band at least as wide as every lattice: lasr_align_post_*'s bits
            wide = post_call(eng, entry, ys, lattice=True, band=max(len(y) for y in ys) + 1)
            full = align(eng, entry, ys, lattice=True, posteriors=True)
            for i, (a, b) in enumerate(zip(full, wide)):
                same_bits(a, b, a.keys(), f"{what} full width {i}")
                assert b["width"] == len(ys[i]) + 1 and not b["lo"].any()
        assert none > 0                                   # rand40 on the six-frame utterance: 6 frames of 6 columns, 41 to cover
    finally:
        eng.close()


def test_long_transcript():
    """1600 labels, past lasr_align_post_*'s limit of 1535, at band 64"""
    y = [int(v) for v in np.random.default_rng(1600).integers(1, oracle("tiny").cfg["vocab"], 1600)]
    eng = make("tiny")
    try:
        for entry in ("feats", "pcm"):
            r = post_call(eng, entry, [y], idx=(0,), band=64)[0]
            assert r["width"] == 64 and r["lo"].tolist() == B.linear(37, 1600, 64) and np.isfinite(r["loglik"])
            s = sum_invariants(r, r["lo"], 1600)
            assert np.all((r["tok_peak_frame"] >= 0) & (r["tok_peak_frame"] < 37))
            print(f"1600 labels {entry}: sum invariants to {s:.3g}")
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (d) errors and the state afterwards
def test_errors_and_state():
    eng = make("tiny")
    try:
        f, ys = feats_all(), transcripts("tiny", "rand40")
        eng.transcribe_pcm(SLOTS, utterances())
        fresh = [eng.fetch(s)[0] for s in SLOTS]
        plain = eng.align_feats(SLOTS, f, ys, lattice=True, band=6, max_passes=3)
        ref = eng.align_band_post_feats(SLOTS, f, ys, 6, max_passes=3, lattice=True)

        def refused(code, fn, *a, **kw):
            with pytest.raises(N.LasrError) as ei:
                fn(*a, **kw)
            assert ei.value.code == code, ei.value

        # more than 2^24 band cells: refused before a lattice is read (dummy buffers), and through the model entry point before the audio
        dummy = np.zeros(4, np.float32)
        T_big = 10923                                     # x 1536 columns = 2^24 + 512 band cells
        assert T_big * 1536 > 1 << 24 >= (T_big - 1) * 1536
        refused(N.LASR_EINVAL, raw_post, eng, dummy, dummy, [T_big], [1600], [1536], B.linear(T_big, 1600, 1536), False)
        big = np.zeros((T_big, eng.desc.feat), np.float32)
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [big], [[3] * 1600], 1536)
        # every LASR_EINVAL of the band call
        y0, T0 = list(ys[0]), f[0].shape[0]
        lin = B.linear(T0, 40, 6)
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [y0], 0)
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [y0], -3)
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [y0], 6, max_passes=0)
        refused(N.LASR_EINVAL, eng.align_band_post_pcm, [5], [utterances()[0]], [y0], 6, max_passes=-1)
        for bad in ([1] + lin[1:], lin[:-1] + [lin[-1] - 1], lin[:5] + [lin[5] + 30] + lin[6:], lin[:3] + [-1] + lin[4:],
                    lin[:10] + [lin[9] - 1 if lin[9] else 40] + lin[11:]):
            refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [y0], 6, windows=[bad])
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [y0], 6, windows=[lin[:-1]])      # one start per frame
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [y0[:2] + [0] + y0[2:]], 6)       # a blank label
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [y0[:2] + [64]], 6)               # out of range
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [[3] * 32768], 6)                 # more than 32767 labels
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0][:1]], [[3] * 1536], 6)              # a single frame needs w = 1537
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5], [f[0]], [[3] * 1600], 1537)               # w beyond 1536
        refused(N.LASR_EINVAL, eng.align_band_post_feats, [5, 5], [f[0], f[1]], [y0, y0], 6)             # a slot listed twice
        b1 = np.zeros((4, 2), np.float32)                                                                # lasr_lattice_band_dp's own checks
        refused(N.LASR_EINVAL, eng.lattice_band_post, [b1], [b1], [[0, 0, 1, 1]], [3])                   # lo[T-1] != U + 1 - w
        refused(N.LASR_EINVAL, eng.lattice_band_post, [b1], [b1], [[0, 1, 0, 2]], [3])                   # decreasing
        refused(N.LASR_EINVAL, eng.lattice_band_post, [b1], [b1], [[0, 0, 0, 0]], [0])                   # W > U + 1
        refused(N.LASR_EINVAL, eng.lattice_band_post, [b1[:1]], [b1[:1]], [[0]], [3])                    # T == 1 needs W == U + 1
        refused(N.LASR_EINVAL, eng.lattice_band_post, [b1], [b1], [[0, 0, 1, 2]], [40000])               # U beyond 32767
        # nothing changed: the same calls as before give the same bits
        again = eng.align_band_post_feats(SLOTS, f, ys, 6, max_passes=3, lattice=True)
        plain2 = eng.align_feats(SLOTS, f, ys, lattice=True, band=6, max_passes=3)
        for a, b, p, q in zip(ref, again, plain, plain2):
            same_bits(a, b, a.keys(), "again")
            same_bits(p, q, p.keys(), "the plain band call, before and after")
            same_bits(p, a, p.keys(), "the plain band call inside the posterior call")
        # all six posterior outputs null: the plain call (every other optional output null too: scoring only)
        sl, nf = np.array(SLOTS, np.int32), np.array([x.shape[0] for x in f], np.int32)
        tok, nt = np.array([t for y in ys for t in y], np.int32), np.array([len(y) for y in ys], np.int32)
        x, ll = np.ascontiguousarray(np.concatenate(f), np.float32), np.zeros(3)
        eng._chk(eng.lib.lasr_align_band_post_feats(eng.ctx, vp(sl), 3, vp(x), vp(nf), vp(tok), vp(nt), 6, 3, None, vp(ll), *([None] * 14)))
        assert ll.tolist() == [r["loglik"] for r in plain]
        # a transcribe on the same slots afterwards: what a fresh engine returns; no result is left from the align call
        assert all(eng.fetch(s)[0] == [] for s in SLOTS)
        eng.transcribe_pcm(SLOTS, utterances())
        assert [eng.fetch(s)[0] for s in SLOTS] == fresh
        # a submitted, uncollected step
        pcm = utterances()[0]
        from libreasr_amd import synth
        eng.reset(1, 15)
        for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=0):
            eng.push([1], ch[None])
            eng.submit([1])
            if eng.pending():
                break
        assert eng.pending()
        refused(N.LASR_ESTATE, eng.align_band_post_feats, [5], [f[0]], [y0], 6)
        while eng.pending():
            eng.wait()
        eng.fetch(1)
        one = eng.align_band_post_feats([5], [f[0]], [y0], 6, max_passes=3)[0]
        assert one["loglik"] == ref[0]["loglik"] and one["occ_emit"].tobytes() == ref[0]["occ_emit"].tobytes()
    finally:
        eng.close()


def test_beam_context_is_refused():
    eng = make("tiny", beam=2)
    try:
        with pytest.raises(N.LasrError) as ei:
            eng.align_band_post_feats([0], [feats_all()[0]], [transcripts("tiny", "rand40")[0]], 6)
        assert ei.value.code == N.LASR_EINVAL
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (e) bf16 context
def test_bf16_context():
    """structure and the sum invariants (the recursions are double whatever the operands)"""
    eng = make("tiny", dtype="bf16")
    try:
        ys = transcripts("tiny", "rand40")
        res = eng.align_band_post_feats(SLOTS, feats_all(), ys, 6, max_passes=4, lattice=True)
    finally:
        eng.close()
    for i, (r, y) in enumerate(zip(res, ys)):
        T, U, w = feats_all()[i].shape[0], len(y), r["width"]
        assert w == 6 and B.valid(T, U, w, r["lo"])
        assert r["occ_blank"].shape == (T, w) and r["occ_emit"].shape == (T, w)
        for k in POST_KEYS:
            assert r[k].shape[0] == (T if k.startswith("occ") else U) and np.all(np.isfinite(r[k])), k
        if not np.isfinite(r["loglik"]):
            check_no_path(r, T, w, U)
            continue
        assert np.all((r["occ_blank"] >= 0) & (r["occ_blank"] <= 1)) and np.all((r["occ_emit"] >= 0) & (r["occ_emit"] <= 1))
        sum_invariants(r, r["lo"], U)
        assert np.all((0 <= r["tok_peak_frame"]) & (r["tok_peak_frame"] < T))
        for u in range(U):
            t = int(r["tok_peak_frame"][u])
            col = [r["occ_emit"][s, u - r["lo"][s]] for s in range(T) if 0 <= u - r["lo"][s] < w]
            assert np.float32(r["tok_peak"][u]) == r["occ_emit"][t, u - r["lo"][t]] == max(col)


# ------------------------------------------------------------------------------- (f) the facade
def test_facade_align_band():
    import __graft_entry__ as graft
    graft.build()
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", config_path="/nonexistent.yaml", synthetic="tiny", max_streams=8)
    try:
        pcm, ys = utterances(), transcripts("tiny", "rand40")
        out = asr.align_band(pcm, ys, band=6)
        plain = asr.align(pcm, ys, band=6)
        eng = asr.engine
        slots = [eng.open() for _ in pcm]
        raw = eng.align_band_post_pcm(slots, pcm, ys, 6, max_passes=4)
        for s in slots:
            eng.close_slot(s)
        none = 0
        for o, q, r, y in zip(out, plain, raw, ys):
            assert o["score"] == q["score"] == r["loglik"] and o["viterbi"] == q["viterbi"] and o["tokens"] == q["tokens"] and o["band"] == q["band"]
            assert o["band"] == {"width": 6, "passes": r["passes"], "touch": bool(r["touch"])}
            assert len(o["posteriors"]) == len(y)
            for k, d in enumerate(o["posteriors"]):
                fr = int(r["frames"][k])
                if fr < 0:
                    none += 1
                    assert d == {"posterior": 0.0, "time_mean_s": None, "time_std_s": None, "peak_time_s": None, "peak": 0.0}
                    continue
                assert d["posterior"] == float(r["occ_emit"][fr, k - int(r["lo"][fr])])
                assert 0 <= d["posterior"] <= d["peak"] <= 1
                assert d["time_mean_s"] >= 0 and d["time_std_s"] >= 0
                assert d["peak_time_s"] == float(r["tok_peak_frame"][k]) * 0.08
        assert none > 0
        one = asr.align_band(pcm[0], ys[0], band=6)
        assert one["posteriors"] == out[0]["posteriors"]
        assert "posteriors" not in asr.align_band(pcm[0], ys[0], band=6, posteriors=False)
        d = asr.align_band(pcm[0], ys[0])                 # the defaults: band 64 holds the whole lattice of 40 labels
        assert d["band"]["width"] == 41 and d["posteriors"] == asr.align(pcm[0], ys[0], posteriors=True)["posteriors"]
    finally:
        asr.engine.close()
