"""The banded RNN-T lattice on the GPU (lasr_align_band_pcm / lasr_align_band_feats / lasr_lattice_band_dp).

Expected values: tests/lattice_band_ref.py (float64, pinned in test_lattice_band_cpu.py).  The dynamic programme is checked exactly
on lattices of multiples of 1/64 (every partial sum is exact in double: Viterbi scores and paths must be EQUAL, loglik within 1e-8,
the bound of test_gpu_lattice.py); with w = U + 1 against lasr_lattice_dp bit for bit.  The model tests use test_gpu_lattice.py's
bounds: a term within 2e-3 of the oracle's, a path sums T + U terms.

Shapes of (a): the issue's list, in which (2200, 2000, 32) and (2100, 40, 64) have 70 400 and 86 100 band cells and so keep their
back-pointers in LDS (lat_bp_words * 32 = 131 072 bits); (2200, 2000, 64) and (2100, 100, 64) are added for the global workspace,
and (300, 400, 300) for the kernel instance with more than one window slot per thread (w > 256)."""
import ctypes as C

import numpy as np
import pytest

import bf16_exact as X
import lattice_band_ref as B
import lattice_ref as R
from libreasr_amd import _native as N
from test_alignment_cpu import utterances
from test_gpu_lattice import SLOTS, TERM_TOL, feats_all, make, oracle, transcripts

pytestmark = pytest.mark.gpu

_REF = {}


def rand64(rng, T, U):
    return (-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32), -(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32))


# ------------------------------------------------------------------------------- (a) the DP kernel, exact
DP_SHAPES = [(1, 0, 1), (1, 3, 2), (5, 0, 4), (64, 63, 8), (70, 130, 17), (300, 5, 3), (2200, 2000, 32), (2100, 40, 64),
             (2200, 2000, 64), (2100, 100, 64), (300, 400, 300)]


def dp_cases():
    """(T, U, w, lo, band b, band e) of every lattice of the mixed batch, with the float64 results -- computed once"""
    if "dp" not in _REF:
        rng = np.random.default_rng(5656)
        cases = []
        for T, U, band in DP_SHAPES:
            b, e = rand64(rng, T, U)
            w, lo = B.width(T, U, band), B.linear(T, U, band)
            cases.append((T, U, w, lo, B.cut(b, lo, w), B.cut(e, lo, w)))
        lo = B.linear(9, 7, 3)                                           # every in-band path ties
        cases.append((9, 7, 3, lo, np.full((9, 3), -0.5, np.float32), np.full((9, 3), -0.5, np.float32)))
        b, e = rand64(rng, 3, 4)                                         # column 2 belongs to no frame: no path
        cases.append((3, 4, 2, [0, 0, 3], B.cut(b, [0, 0, 3], 2), B.cut(e, [0, 0, 3], 2)))
        want = [(B.forward(bb, eb, lo, U), *B.viterbi(bb, eb, lo, U)) for T, U, w, lo, bb, eb in cases]
        _REF["dp"] = (cases, want)
    return _REF["dp"]


def test_band_dp_kernel_exact():
    cases, want = dp_cases()
    eng = make("tiny")
    try:
        words = eng.config("lat_bp_words")
        in_lds = [(T * w + 31) // 32 <= words for T, U, w, *_ in cases]
        assert in_lds[6] and in_lds[7] and not in_lds[8] and not in_lds[9]       # both homes of the back-pointers are in the batch
        assert max(c[2] for c in cases) > 256 >= cases[9][2]
        got = eng.lattice_band_dp([c[4] for c in cases], [c[5] for c in cases], [c[3] for c in cases], [c[1] for c in cases])
        small = [i for i, c in enumerate(cases) if c[2] <= 256]           # the one-slot kernel instance on its own
        got_small = eng.lattice_band_dp([cases[i][4] for i in small], [cases[i][5] for i in small], [cases[i][3] for i in small],
                                        [cases[i][1] for i in small])
        # device-resident lattices, no Viterbi half: the same forward sum
        import torch
        cat_b = torch.as_tensor(np.concatenate([c[4].reshape(-1) for c in cases])).to(eng.device)
        cat_e = torch.as_tensor(np.concatenate([c[5].reshape(-1) for c in cases])).to(eng.device)
        arr = lambda xs: np.ascontiguousarray(np.array(xs, np.int32))
        Ts, Us, Ws = arr([c[0] for c in cases]), arr([c[1] for c in cases]), arr([c[2] for c in cases])
        los = arr([v for c in cases for v in c[3]])
        ll_d = np.zeros(len(cases))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        eng._chk(eng.lib.lasr_lattice_band_dp(eng.ctx, C.c_void_p(cat_b.data_ptr()), C.c_void_p(cat_e.data_ptr()), p(Ts), p(Us), p(Ws), p(los),
                                              len(cases), p(ll_d), None, None))
    finally:
        eng.close()
    for i, ((T, U, w, lo, bb, eb), (ll, v, fr), g) in enumerate(zip(cases, want, got)):
        print(f"band lattice {i} T {T} U {U} w {w}: loglik {g['loglik']:.6f} dloglik {g['loglik'] - ll if np.isfinite(ll) else 0.0:.3g} viterbi {g['viterbi']}")
        assert g["viterbi"] == v, (i, g["viterbi"], v)
        assert [int(t) for t in g["frames"]] == fr, i
        if np.isfinite(ll):
            assert abs(g["loglik"] - ll) <= 1e-8, (i, g["loglik"], ll)
        else:
            assert g["loglik"] == ll, (i, g["loglik"])
        assert ll_d[i] == g["loglik"], i
    for j, i in enumerate(small):
        assert got_small[j]["loglik"] == got[i]["loglik"] and got_small[j]["viterbi"] == got[i]["viterbi"], i
        assert np.array_equal(got_small[j]["frames"], got[i]["frames"]), i
    assert want[-1][0] == -np.inf and want[-1][2] == [-1] * 4            # the disconnected windows
    assert np.isfinite(want[-2][1])                                      # the all-tie lattice has a path


# ------------------------------------------------------------------------------- (b) full width = lasr_lattice_dp, bit for bit
def test_full_width_band_equals_lattice_dp():
    shapes = [(1, 0), (1, 3), (5, 0), (2, 1), (3, 2), (64, 63), (65, 64), (70, 130), (300, 5)]        # test_dp_kernel_exact's
    rng = np.random.default_rng(2024)
    bs = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in shapes]
    es = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in shapes]
    bs.append(np.full((4, 4), -0.5, np.float32))
    es.append(np.full((4, 4), -0.5, np.float32))
    shapes.append((4, 3))
    crng = np.random.default_rng(7)                                      # continuous values too: the same operations in the same order
    bs.append(-crng.random((50, 31)).astype(np.float32) * 8)
    es.append(-crng.random((50, 31)).astype(np.float32) * 8)
    shapes.append((50, 30))
    eng = make("tiny")
    try:
        full = eng.lattice_dp(bs, es)
        band = eng.lattice_band_dp(bs, es, [[0] * T for T, _ in shapes], [U for _, U in shapes])
        full_ll = eng.lattice_dp(bs, es, viterbi=False)
        band_ll = eng.lattice_band_dp(bs, es, [[0] * T for T, _ in shapes], [U for _, U in shapes], viterbi=False)
    finally:
        eng.close()
    for i, (f, g) in enumerate(zip(full, band)):
        assert f["loglik"] == g["loglik"] and f["viterbi"] == g["viterbi"], (i, f, g)
        assert np.array_equal(f["frames"], g["frames"]), i
        assert full_ll[i]["loglik"] == band_ll[i]["loglik"] == f["loglik"], i


# ------------------------------------------------------------------------------- (c) the planted path through a Python loop
def test_planted_path_pass_loop():
    eng = make("tiny")
    try:
        for T, U, band, seed in B.PLANTED:
            b, e, planted = B.planted(T, U, band, seed)
            ref = B.pass_loop(b, e, U, band, B.PLANTED_MAX_PASSES)
            assert ref[-1][3] == 0 and ref[-1][2] == planted and len(ref) <= B.PLANTED_MAX_PASSES
            w = B.width(T, U, band)
            lo, touch = eng.band_windows(T, U, band)
            lo = lo.tolist()
            for k, (rlo, rscore, rframes, rtouch) in enumerate(ref):
                assert lo == rlo, (T, U, k)
                g = eng.lattice_band_dp([B.cut(b, lo, w)], [B.cut(e, lo, w)], [lo], [U])[0]
                frames = [int(t) for t in g["frames"]]
                assert frames == rframes and g["viterbi"] == rscore, (T, U, k)
                new, touch = eng.band_windows(T, U, band, frames, lo)
                assert touch == rtouch, (T, U, k)
                lo = new.tolist()
            assert touch == 0
            full = eng.lattice_dp([b], [e])[0]
            assert [int(t) for t in full["frames"]] == frames == planted and full["viterbi"] == g["viterbi"]
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (d) the model path
def align(eng, entry, ys, idx=(0, 1, 2), **kw):
    if entry == "feats":
        return eng.align_feats(SLOTS[:len(idx)], [feats_all()[i] for i in idx], ys, **kw)
    return eng.align_pcm(SLOTS[:len(idx)], [utterances()[i] for i in idx], ys, **kw)


def same_result(a, b, what):
    assert a["loglik"] == b["loglik"] and a["viterbi"] == b["viterbi"], (what, a["loglik"], b["loglik"])
    for key in ("frames", "logps", "blank_lp", "emit_lp"):
        assert np.array_equal(a[key], b[key]), (what, key)


def band_reference(name, y, i, lo, w):
    key = (name, tuple(y), i, tuple(lo), w)
    if key not in _REF:
        bb, eb = B.band_lattice(oracle(name), feats_all()[i], y, lo, w)
        _REF[key] = (bb, eb, B.forward(bb, eb, lo, len(y)), *B.viterbi(bb, eb, lo, len(y)))
    return _REF[key]


def check_band_against(res, name, y, i, what):
    """the bounds of test_gpu_lattice.check_against, on the engine-reported windows"""
    lo, w, U = [int(v) for v in res["lo"]], int(res["width"]), len(y)
    T = len(lo)
    assert B.valid(T, U, w, lo) and res["blank_lp"].shape == (T, w) and res["emit_lp"].shape == (T, w), what
    bb, eb, ll, v, _ = band_reference(name, y, i, lo, w)
    at_U = np.array([[lo[t] + k == U for k in range(w)] for t in range(T)])
    db = float(np.abs(res["blank_lp"].astype(np.float64) - bb).max())
    de = float(np.abs(res["emit_lp"].astype(np.float64) - eb)[~at_U].max()) if (~at_U).any() else 0.0
    assert np.all(res["emit_lp"][at_U] == 0), what
    print(f"{what}: T {T} U {U} w {w} max |db| {db:.3g} max |de| {de:.3g} dloglik {res['loglik'] - ll:.3g} touch {res['touch']}")
    assert db <= TERM_TOL and de <= TERM_TOL, (what, db, de)
    if ll == -np.inf:                                                     # the windows leave no path (6 frames of 6 columns, 41 to cover)
        assert res["loglik"] == -np.inf and res["viterbi"] == -np.inf and res["touch"] == 0, what
        assert np.all(res["frames"] == -1) and np.all(res["logps"] == 0), what
        return False
    assert abs(res["loglik"] - ll) <= (T + U) * TERM_TOL, (what, res["loglik"], ll)
    fr = [int(t) for t in res["frames"]]
    assert len(fr) == U and fr == sorted(fr) and all(0 <= t < T for t in fr), (what, fr)
    full_b, full_e = B.spread(bb, lo, U), B.spread(eb, lo, U)             # -inf outside the windows: a path that leaves them scores -inf
    assert R.path_score(full_b, full_e, fr) >= v - 2 * (T + U) * TERM_TOL, (what, R.path_score(full_b, full_e, fr), v)
    for u in range(U):
        assert abs(float(res["logps"][u]) - float(full_e[fr[u], u])) <= TERM_TOL, (what, u)
    assert res["viterbi"] <= res["loglik"] + 1e-9, what
    assert res["touch"] == B.recentre(T, U, w if T > 1 else U + 1, fr, lo)[1], what
    return True


@pytest.mark.parametrize("entry", ["feats", "pcm"])
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_model_path(name, entry):
    eng = make(name)
    try:
        for kind in ("greedy", "wrong", "rand40"):
            ys = transcripts(name, kind)
            what = f"{name} {entry} {kind}"
            # a band at least as wide as every lattice: lasr_align_*'s bits
            full = align(eng, entry, ys, lattice=True)
            wide = align(eng, entry, ys, lattice=True, band=max(len(y) for y in ys) + 1, max_passes=1)
            for i, (a, b) in enumerate(zip(full, wide)):
                same_result(a, b, f"{what} full width {i}")
                assert b["passes"] == 1 and b["touch"] == 0 and b["width"] == len(ys[i]) + 1 and not b["lo"].any()
            # band = 6, one pass, linear windows
            one = align(eng, entry, ys, lattice=True, band=6, max_passes=1)
            for i, r in enumerate(one):
                T = feats_all()[i].shape[0]
                assert r["passes"] == 1 and r["lo"].tolist() == B.linear(T, len(ys[i]), 6)
                check_band_against(r, name, ys[i], i, f"{what} band 6 utterance {i}")
            # band = 6, up to four passes = feeding lo_out back by hand
            multi = align(eng, entry, ys, lattice=True, band=6, max_passes=4)
            lo, passes = [r["lo"] for r in one], 0
            while True:
                hand = one if passes == 0 else align(eng, entry, ys, lattice=True, band=6, max_passes=1, windows=lo)
                passes += 1
                new, touch = [], []
                for i, r in enumerate(hand):
                    assert np.array_equal(r["lo"], lo[i])
                    if r["viterbi"] == -np.inf:
                        new.append(lo[i]); touch.append(0)
                        continue
                    nw, tc = eng.band_windows(len(lo[i]), len(ys[i]), 6, r["frames"], lo[i])
                    new.append(nw); touch.append(tc)
                assert touch == [r["touch"] for r in hand]
                if not any(touch) or all(np.array_equal(a, b) for a, b in zip(new, lo)) or passes >= 4:
                    break
                lo = new
            print(f"{what}: {passes} passes, touch {touch}")
            for i, (a, b) in enumerate(zip(hand, multi)):
                same_result(a, b, f"{what} multi-pass {i}")
                assert np.array_equal(a["lo"], b["lo"]) and a["touch"] == b["touch"] and b["passes"] == passes <= 4
    finally:
        eng.close()


def test_long_transcript():
    """1600 labels: past lasr_align_*'s limit of 1535 (which refuses them), one frame count of 37 and windows of 64"""
    m = oracle("tiny")
    y = [int(v) for v in np.random.default_rng(1600).integers(1, m.cfg["vocab"], 1600)]
    eng = make("tiny")
    try:
        with pytest.raises(N.LasrError) as ei:
            eng.align_feats([5], [feats_all()[0]], [y])
        assert ei.value.code == N.LASR_EINVAL
        for entry in ("feats", "pcm"):
            r = align(eng, entry, [y], idx=(0,), lattice=True, band=64, max_passes=1)[0]
            assert r["width"] == 64 and r["lo"].tolist() == B.linear(37, 1600, 64)
            assert check_band_against(r, "tiny", y, 0, f"tiny {entry} 1600 labels")
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (e) errors and state
def test_errors_and_state():
    eng = make("tiny")
    try:
        f, ys = feats_all(), transcripts("tiny", "rand40")
        eng.transcribe_pcm(SLOTS, utterances())
        fresh = [eng.fetch(s)[0] for s in SLOTS]
        ref = eng.align_feats(SLOTS, f, ys, lattice=True, band=6, max_passes=3)

        def refused(code, fn, *a, **kw):
            with pytest.raises(N.LasrError) as ei:
                fn(*a, **kw)
            assert ei.value.code == code, ei.value

        y0, T0 = list(ys[0]), f[0].shape[0]
        lin = B.linear(T0, 40, 6)
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0], band=0)
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0], band=-3)
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0], band=6, max_passes=0)
        refused(N.LASR_EINVAL, eng.align_pcm, [5], [utterances()[0]], [y0], band=6, max_passes=-1)
        for bad in ([1] + lin[1:], lin[:-1] + [lin[-1] - 1], lin[:5] + [lin[5] + 30] + lin[6:], lin[:3] + [-1] + lin[4:],
                    lin[:10] + [lin[9] - 1 if lin[9] else 40] + lin[11:]):
            refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0], band=6, windows=[bad])
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0], band=6, windows=[lin[:-1]])         # one start per frame
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0[:2] + [0] + y0[2:]], band=6)          # a blank label
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0[:2] + [64]], band=6)                  # out of range
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [[3] * 32768], band=6)                    # more than 32767 labels
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0][:1]], [[3] * 1536], band=6)                 # a single frame needs w = U + 1 = 1537
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [[3] * 1600], band=1537)                  # w beyond 1536
        refused(N.LASR_EINVAL, eng.align_feats, [5, 5], [f[0], f[1]], [y0, y0], band=6)                # a slot listed twice
        with pytest.raises(ValueError):
            eng.align_feats([5], [f[0]], [y0], band=6, posteriors=True)
        # the DP entry point's own checks
        b1 = np.zeros((4, 2), np.float32)
        refused(N.LASR_EINVAL, eng.lattice_band_dp, [b1], [b1], [[0, 0, 1, 1]], [3])                    # lo[T-1] != U + 1 - w
        refused(N.LASR_EINVAL, eng.lattice_band_dp, [b1], [b1], [[0, 1, 0, 2]], [3])                    # decreasing
        refused(N.LASR_EINVAL, eng.lattice_band_dp, [b1], [b1], [[0, 0, 0, 0]], [0])                    # W > U + 1
        refused(N.LASR_EINVAL, eng.lattice_band_dp, [b1[:1]], [b1[:1]], [[0]], [3])                     # T == 1 needs W == U + 1
        refused(N.LASR_EINVAL, eng.lattice_band_dp, [b1], [b1], [[0, 0, 1, 2]], [40000])                # U beyond 32767
        # nothing changed: the same call as before gives the same bits
        again = eng.align_feats(SLOTS, f, ys, lattice=True, band=6, max_passes=3)
        for a, b in zip(ref, again):
            same_result(a, b, "again")
            assert np.array_equal(a["lo"], b["lo"]) and a["passes"] == b["passes"] and a["touch"] == b["touch"]
        # every optional output may be null: scoring only (no Viterbi pass), no lattice
        one = eng.align_feats(SLOTS, f, ys, band=6, lattice=True)
        sl, nf = np.array(SLOTS, np.int32), np.array([x.shape[0] for x in f], np.int32)
        tok, nt = np.array([t for y in ys for t in y], np.int32), np.array([len(y) for y in ys], np.int32)
        x, ll = np.ascontiguousarray(np.concatenate(f), np.float32), np.zeros(3)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        eng._chk(eng.lib.lasr_align_band_feats(eng.ctx, p(sl), 3, p(x), p(nf), p(tok), p(nt), 6, 1, None, p(ll), *([None] * 8)))
        assert ll.tolist() == [r["loglik"] for r in one]
        # a transcribe on the same slots afterwards: what a fresh engine returns; no result is left from the align call
        assert all(eng.fetch(s)[0] == [] for s in SLOTS)
        eng.transcribe_pcm(SLOTS, utterances())
        assert [eng.fetch(s)[0] for s in SLOTS] == fresh
        # the full-lattice call is what it was
        full = eng.align_feats(SLOTS, f, ys, lattice=True)
        assert all(fr["loglik"] >= r["loglik"] - 1e-9 for fr, r in zip(full, one))
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
        refused(N.LASR_ESTATE, eng.align_feats, [5], [f[0]], [y0], band=6)
        while eng.pending():
            eng.wait()
        eng.fetch(1)
        assert eng.align_feats([5], [f[0]], [y0], band=6, max_passes=3)[0]["loglik"] == ref[0]["loglik"]
    finally:
        eng.close()


def test_beam_context_is_refused():
    eng = make("tiny", beam=2)
    try:
        with pytest.raises(N.LasrError) as ei:
            eng.align_feats([0], [feats_all()[0]], [transcripts("tiny", "rand40")[0]], band=6)
        assert ei.value.code == N.LASR_EINVAL
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (f) bf16 context
def test_bf16_context():
    """the first frame's first label row within the bound of tests/bf16_exact.py, the rest structure only, as
    test_gpu_lattice.test_bf16_context (row 0 of the band layout starts at label 0)"""
    eng = make("tiny", dtype="bf16")
    try:
        ys = transcripts("tiny", "rand40")
        res = eng.align_feats(SLOTS, feats_all(), ys, lattice=True, band=6, max_passes=4)
    finally:
        eng.close()
    for i, (r, y) in enumerate(zip(res, ys)):
        T, U, w = feats_all()[i].shape[0], len(y), r["width"]
        assert w == 6 and r["blank_lp"].shape == (T, w) and r["emit_lp"].shape == (T, w) and r["lo"].shape == (T,)
        assert B.valid(T, U, w, r["lo"]) and 1 <= r["passes"] <= 4 and r["touch"] in (0, 1)
        assert np.all(np.isfinite(r["blank_lp"])) and np.all(np.isfinite(r["emit_lp"]))
        assert r["lo"][0] == 0
        X.check_first_cell("tiny", feats_all()[i][0], r["blank_lp"][0, 0], {y[0]: r["emit_lp"][0, 0]} if U else {}, f"bf16 band utterance {i}")
        assert r["viterbi"] <= r["loglik"] + 1e-9
        if np.isfinite(r["viterbi"]):                                     # the windows connect
            assert np.isfinite(r["loglik"])
            fr = [int(t) for t in r["frames"]]
            assert len(fr) == U and fr == sorted(fr) and all(0 <= t < T for t in fr)
            for u in range(U):
                assert r["logps"][u] == r["emit_lp"][fr[u], u - r["lo"][fr[u]]]
        else:
            assert r["loglik"] == -np.inf and np.all(r["frames"] == -1)
        print(f"bf16 band utterance {i}: T {T} U {U} loglik {r['loglik']:.4f} viterbi {r['viterbi']:.4f} passes {r['passes']} touch {r['touch']}")


# ------------------------------------------------------------------------------- (g) the facade
def test_facade_align_with_a_band():
    import __graft_entry__ as graft
    graft.build()
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", config_path="/nonexistent.yaml", synthetic="tiny", max_streams=8)
    try:
        pcm, ys = utterances(), transcripts("tiny", "rand40")
        out = asr.align([pcm[0], pcm[1]], [ys[0], ys[1]], band=6)
        eng = asr.engine
        slots = [eng.open(), eng.open()]
        raw = eng.align_pcm(slots, [pcm[0], pcm[1]], [ys[0], ys[1]], band=6, max_passes=4)
        for s in slots:
            eng.close_slot(s)
        for o, r, y in zip(out, raw, ys):
            assert o["score"] == r["loglik"] and o["viterbi"] == r["viterbi"]
            assert o["band"] == {"width": 6, "passes": r["passes"], "touch": bool(r["touch"])}
            assert [t for t, _, _ in o["tokens"]] == list(y)
            assert [ts for _, ts, _ in o["tokens"]] == [float(f) * 0.08 for f in r["frames"]]
        one = asr.align(pcm[0], ys[0], band=6, max_passes=1)
        assert one["band"]["passes"] == 1 and one["score"] <= asr.align(pcm[0], ys[0])["score"] + 1e-9
        assert "band" not in asr.align(pcm[0], ys[0])
        with pytest.raises(ValueError):
            asr.align(pcm[0], ys[0], band=6, posteriors=True)
    finally:
        asr.engine.close()
