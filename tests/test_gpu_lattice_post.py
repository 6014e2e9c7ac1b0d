"""Lattice posteriors on the GPU (lasr_align_post_pcm / lasr_align_post_feats / lasr_lattice_post): the occupancy of every edge of the
teacher-forced RNN-T lattice over all alignments, and per label the statistics of its emission frame.

Expected values: tests/lattice_post_ref.py (float64, pinned in test_lattice_post_cpu.py).  Bounds of the kernel tests: the kernels
compute in double, and float64 rounding over T + U steps stays below 1e-12 in the reference's own invariants, so 1e-9 (1e-8 for
loglik, the project's DP bound) leaves three orders and an f32 accumulation misses it by four; occupancies are <= 1 and rounded once to
f32 (6e-8), bound 2e-7.  Model tests: a lattice term is within 2e-3 of the float64 one (the project's logits bound, doubled: z_k - lse);
log occ is a log-sum over paths of T + U terms minus loglik, another such, so |d log occ| <= 2 (T + U) 2e-3."""
import ctypes as C

import numpy as np
import pytest

import bf16_exact as X
import lattice_post_ref as P
import lattice_ref as R
from libreasr_amd import _native as N
from libreasr_amd import synth
from test_alignment_cpu import utterances
from test_gpu_lattice import SLOTS, TERM_TOL, feats_all, make, reference, transcripts

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (1, 3), (5, 0), (2, 1), (3, 2), (64, 63), (65, 64), (70, 130), (300, 5), (4, 300)]
N_RANDOM = len(SHAPES)
POST_KEYS = ("occ_blank", "occ_emit", "tok_mean", "tok_var", "tok_peak_frame", "tok_peak")
_CACHE = {}


def vp(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def batch():
    """the lattices of (a): the random shapes (test_gpu_lattice's generator), then all-tie, all-zero, -inf entries, impossible"""
    if "batch" not in _CACHE:
        rng = np.random.default_rng(2024)
        bs = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in SHAPES]
        es = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in SHAPES]
        extra = [(np.full((4, 4), -0.5, np.float32),) * 2, (np.zeros((6, 5), np.float32),) * 2, P.minus_inf_lattice(), P.impossible_lattice()]
        bs += [x[0] for x in extra]
        es += [x[1] for x in extra]
        _CACHE["batch"] = (bs, es, [P.posteriors(b, e, b.shape[1] - 1) for b, e in zip(bs, es)])
    return _CACHE["batch"]


def raw_post(eng, b, e, Ts, Us, full=True):
    """lasr_lattice_post on concatenated lattices (numpy arrays or device tensors) -> the output arrays, in the order of the C arguments"""
    n, cells, su = len(Ts), int(sum(int(t) * (int(u) + 1) for t, u in zip(Ts, Us))), max(int(sum(Us)), 1)
    ll = np.zeros(n)
    outs = [np.zeros(n), np.zeros(cells, np.float32), np.zeros(cells, np.float32), np.zeros(su), np.zeros(su), np.zeros(su, np.int32),
            np.zeros(su)] if full else [None] * 7
    ptr = lambda x: C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else vp(x)
    eng._chk(eng.lib.lasr_lattice_post(eng.ctx, ptr(b), ptr(e), vp(np.asarray(Ts, np.int32)), vp(np.asarray(Us, np.int32)), n, vp(ll),
                                       *[vp(x) for x in outs]))
    return [ll] + outs


def kernel_run():
    """one engine, the batch of (a) through every way in: the Python wrapper, raw with host inputs, raw with device inputs, raw with only
    loglik asked for, and lasr_lattice_dp"""
    if "run" not in _CACHE:
        import torch
        bs, es, _ = batch()
        Ts, Us = [x.shape[0] for x in bs], [x.shape[1] - 1 for x in bs]
        cat_b, cat_e = np.concatenate([x.reshape(-1) for x in bs]), np.concatenate([x.reshape(-1) for x in es])
        eng = make("tiny")
        try:
            got = eng.lattice_post(bs, es)
            host = raw_post(eng, cat_b, cat_e, Ts, Us)
            dev = raw_post(eng, torch.as_tensor(cat_b).to(eng.device), torch.as_tensor(cat_e).to(eng.device), Ts, Us)
            only = raw_post(eng, cat_b, cat_e, Ts, Us, full=False)
            dp = eng.lattice_dp(bs, es, viterbi=False)
        finally:
            eng.close()
        _CACHE["run"] = (got, host, dev, only, dp)
    return _CACHE["run"]


def sum_invariants(r, U, tol=1e-6):
    ob, oe = r["occ_blank"].astype(np.float64), r["occ_emit"].astype(np.float64)
    worst = float(np.abs(ob.sum(axis=1) - 1).max())
    if U:
        worst = max(worst, float(np.abs(oe[:, :U].sum(axis=0) - 1).max()))
    assert worst <= tol, worst
    assert np.all(oe[:, U] == 0) and np.all(ob[-1, :U] == 0) and ob[-1, U] == 1
    return worst


# ------------------------------------------------------------------------------- (a) the kernels against float64
def test_kernels_against_float64():
    bs, es, refs = batch()
    got = kernel_run()[0]
    worst = dict(loglik=0.0, occ=0.0, mean=0.0, var=0.0, peak=0.0, sums=0.0)
    margin = np.inf
    for i, (b, g, ref) in enumerate(zip(bs, got, refs)):
        T, U = b.shape[0], b.shape[1] - 1
        assert g["occ_blank"].shape == (T, U + 1) and g["occ_emit"].shape == (T, U + 1) and g["occ_blank"].dtype == np.float32
        for k in POST_KEYS:
            assert not np.any(np.isnan(g[k])), (i, k)
        if ref["loglik"] == -np.inf:                      # the impossible lattice: the -inf convention
            assert g["loglik"] == -np.inf and g["loglik_bwd"] == -np.inf
            assert np.all(g["occ_blank"] == 0) and np.all(g["occ_emit"] == 0)
            assert list(g["tok_mean"]) == [-1.0] * U and list(g["tok_var"]) == [0.0] * U
            assert list(g["tok_peak_frame"]) == [-1] * U and list(g["tok_peak"]) == [0.0] * U
            continue
        d_ll = max(abs(g["loglik"] - ref["loglik"]), abs(g["loglik_bwd"] - ref["loglik_bwd"]))
        d_occ = max(float(np.abs(g["occ_blank"] - ref["occ_b"]).max()), float(np.abs(g["occ_emit"] - ref["occ_e"]).max()))
        d_mean = float(np.abs(g["tok_mean"] - ref["tok_mean"]).max()) if U else 0.0
        d_var = float(np.abs(g["tok_var"] - ref["tok_var"]).max()) if U else 0.0
        d_peak = float(np.abs(g["tok_peak"] - ref["tok_peak"]).max()) if U else 0.0
        s = sum_invariants(g, U)
        print(f"lattice {i} T {T} U {U}: dloglik {d_ll:.3g} docc {d_occ:.3g} dmean {d_mean:.3g} dvar {d_var:.3g} dpeak {d_peak:.3g} sums {s:.3g}")
        assert d_ll <= 1e-8, (i, d_ll)
        assert d_occ <= 2e-7, (i, d_occ)
        assert d_mean <= 1e-9 * max(1, T) and d_var <= 1e-9 * max(1, T) ** 2 and d_peak <= 1e-9, (i, d_mean, d_var, d_peak)
        worst = dict(loglik=max(worst["loglik"], d_ll), occ=max(worst["occ"], d_occ), mean=max(worst["mean"], d_mean / max(1, T)),
                     var=max(worst["var"], d_var / max(1, T) ** 2), peak=max(worst["peak"], d_peak), sums=max(worst["sums"], s))
        if i < N_RANDOM:                                  # every label of the random shapes: the peak's frame, given a clear winner
            for u in range(U):
                top = np.sort(ref["occ_e"][:, u])[::-1]
                if T > 1:
                    margin = min(margin, float(top[0] - top[1]))
            assert margin > 1e-6, (i, margin)
            assert [int(t) for t in g["tok_peak_frame"]] == [int(t) for t in ref["tok_peak_frame"]], i
    print(f"maxima: {worst}; smallest margin between the two largest posteriors of a label: {margin:.3g}")
    # -inf entries: occupancy 0 on the impossible edges
    g = got[N_RANDOM + 2]
    assert g["occ_emit"][0, 0] == 0 and g["occ_blank"][2, 1] == 0
    # the all-zero (6,4) lattice against the closed form: counts of paths into the cell x out of the edge's head / all paths
    from math import comb
    g, T, U = got[N_RANDOM + 1], 6, 4
    n_paths = comb(T - 1 + U, U)
    for t in range(T):
        for u in range(U):
            assert abs(g["occ_emit"][t, u] - comb(t + u, u) * comb(T - 1 - t + U - u - 1, U - u - 1) / n_paths) <= 2e-7, (t, u)
        for u in range(U + 1 if t < T - 1 else 0):
            assert abs(g["occ_blank"][t, u] - comb(t + u, u) * comb(T - 2 - t + U - u, U - u) / n_paths) <= 2e-7, (t, u)


def test_device_inputs_and_null_outputs():
    got, host, dev, only, _ = kernel_run()
    for h, d in zip(host, dev):
        assert h.tobytes() == d.tobytes()
    assert only[0].tobytes() == host[0].tobytes()         # every posterior output null: loglik alone
    assert [g["loglik"] for g in got] == list(host[0]) and [g["loglik_bwd"] for g in got] == list(host[1])
    assert np.concatenate([g["occ_emit"].reshape(-1) for g in got]).tobytes() == host[3].tobytes()


# ------------------------------------------------------------------------------- (b) the forward half is k_lat_dp's
def test_loglik_is_lattice_dp_bit_for_bit():
    got, _, _, _, dp = kernel_run()
    assert [g["loglik"] for g in got] == [d["loglik"] for d in dp]


# ------------------------------------------------------------------------------- (c) the model path, f32
def post_reference(name):
    key = ("post", name)
    if key not in _CACHE:
        _CACHE[key] = [P.posteriors(b, e, len(y)) for y, b, e, _, _, _ in reference(name, "greedy")]
    return _CACHE[key]


def check_model(res, plain, again, name, what):
    """res: with posteriors; plain: the same call without; again: lattice_post on res's lattices"""
    worst = 0.0
    for i, (r, q, a, ref) in enumerate(zip(res, plain, again, post_reference(name))):
        T, U = r["blank_lp"].shape[0], r["blank_lp"].shape[1] - 1
        assert set(q) | set(POST_KEYS) == set(r)
        for k in q:                                       # every field of the plain call, bit for bit
            assert np.asarray(q[k]).tobytes() == np.asarray(r[k]).tobytes(), (what, i, k)
        for k in POST_KEYS:                               # the same kernels on the same inputs
            assert r[k].tobytes() == a[k].tobytes(), (what, i, k)
        assert a["loglik"] == r["loglik"]
        sum_invariants(r, U)
        for k_gpu, k_ref in (("occ_blank", "occ_b"), ("occ_emit", "occ_e")):
            m = ref[k_ref] >= 1e-3
            if not m.any():                               # (occ_e of a transcript without labels)
                continue
            d = float(np.abs(np.log(r[k_gpu][m].astype(np.float64)) - np.log(ref[k_ref][m])).max())
            worst = max(worst, d)
            assert d <= 2 * (T + U) * TERM_TOL, (what, i, k_gpu, d)
        assert r["tok_peak_frame"].shape == (U,) and np.all((0 <= r["tok_mean"]) & (r["tok_mean"] <= T - 1 + 1e-9)) and np.all(r["tok_var"] >= 0)
    print(f"{what}: max |d log occ| over the cells with occupancy >= 1e-3: {worst:.3g}")


@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_model_path(name):
    ys, f = transcripts(name, "greedy"), feats_all()
    eng = make(name)
    try:
        plain = eng.align_feats(SLOTS, f, ys, lattice=True)
        res = eng.align_feats(SLOTS, f, ys, lattice=True, posteriors=True)
        again = eng.lattice_post([r["blank_lp"] for r in res], [r["emit_lp"] for r in res])
        check_model(res, plain, again, name, f"{name} feats")
        if name == "tiny":
            plain = eng.align_pcm(SLOTS, utterances(), ys, lattice=True)
            res = eng.align_pcm(SLOTS, utterances(), ys, lattice=True, posteriors=True)
            again = eng.lattice_post([r["blank_lp"] for r in res], [r["emit_lp"] for r in res])
            check_model(res, plain, again, name, f"{name} pcm")
            # no Viterbi pass and no lattice asked for: loglik then comes from the posterior kernels' forward half
            lean = eng.align_feats(SLOTS, f, ys, viterbi=False, posteriors=True)
            full = eng.align_feats(SLOTS, f, ys, lattice=True, posteriors=True)
            for a, b in zip(lean, full):
                assert a["loglik"] == b["loglik"] and all(a[k].tobytes() == b[k].tobytes() for k in POST_KEYS) and "frames" not in a
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (d) errors and the state afterwards
def test_errors_and_state():
    eng = make("tiny")
    try:
        f, ys = feats_all(), transcripts("tiny", "greedy")
        eng.transcribe_feats(SLOTS, f)
        fresh = [eng.fetch(s)[0] for s in SLOTS]
        assert fresh == ys
        ref = eng.align_feats(SLOTS, f, ys, posteriors=True)

        def refused(code, fn, *a, **kw):
            with pytest.raises(N.LasrError) as ei:
                fn(*a, **kw)
            assert ei.value.code == code, ei.value

        dummy = np.zeros(4, np.float32)
        refused(N.LASR_EINVAL, raw_post, eng, dummy, dummy, [16384], [1024], False)       # 16384 x 1025 > 2^24 cells: before any read
        refused(N.LASR_EINVAL, raw_post, eng, dummy, dummy, [1], [1536], False)           # U > 1535
        refused(N.LASR_EINVAL, raw_post, eng, dummy, dummy, [0], [1], False)              # T < 1
        y0 = list(ys[0])
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0[:2] + [0] + y0[2:]], posteriors=True)      # a blank label
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0[:2] + [64]], posteriors=True)              # out of range
        refused(N.LASR_EINVAL, eng.align_pcm, [5], [utterances()[0]], [[0]], posteriors=True)
        # 2^24 cells through the model entry point: T x (U + 1) is checked before the audio is touched
        T_big = 1 << 14
        big = np.zeros((T_big, eng.desc.feat), np.float32)
        refused(N.LASR_EINVAL, eng.align_feats, [5], [big], [[3] * 1024], posteriors=True)
        # nothing changed: the same call as before gives the same bits, and a transcribe gives what it gives without these calls
        again = eng.align_feats(SLOTS, f, ys, posteriors=True)
        for a, b in zip(ref, again):
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
        assert all(eng.fetch(s)[0] == [] for s in SLOTS)
        eng.transcribe_feats(SLOTS, f)
        assert [eng.fetch(s)[0] for s in SLOTS] == fresh
        # ... and a streaming run, before and after a good posterior call on the same slot
        pcm = utterances()[0]
        want = None
        for rep in range(2):
            eng.reset(1, 15)
            got = []
            for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=4):
                eng.push([1], ch[None])
                eng.step([1])
                got += eng.fetch(1)[0]
            if rep == 0:
                want = got
                eng.align_pcm([1], [pcm], [ys[0]], posteriors=True)
        assert got == want and len(want) > 0
        # a submitted, uncollected step
        eng.reset(1, 15)
        n_sub = 0
        for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=0):
            eng.push([1], ch[None])
            eng.submit([1])
            if eng.pending():
                n_sub += 1
                break
        assert n_sub == 1
        refused(N.LASR_ESTATE, eng.align_feats, [5], [f[0]], [y0], posteriors=True)
        while eng.pending():
            eng.wait()
        eng.fetch(1)
        one = eng.align_feats([5], [f[0]], [y0], posteriors=True)[0]
        assert one["loglik"] == ref[0]["loglik"] and one["occ_emit"].tobytes() == ref[0]["occ_emit"].tobytes()
    finally:
        eng.close()


def test_beam_context_is_refused():
    eng = make("tiny", beam=2)
    try:
        with pytest.raises(N.LasrError) as ei:
            eng.align_feats([0], [feats_all()[0]], [transcripts("tiny", "greedy")[0]], posteriors=True)
        assert ei.value.code == N.LASR_EINVAL
        eng.transcribe_feats([0], [feats_all()[0]])
        after = eng.fetch(0)[0]
    finally:
        eng.close()
    eng = make("tiny", beam=2)
    try:
        eng.transcribe_feats([0], [feats_all()[0]])
        assert eng.fetch(0)[0] == after                   # what the context gives without the refused call
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (e) bf16 context
def test_bf16_context():
    """the first frame's first label row within the bound of tests/bf16_exact.py (as, and as loose as, in
    test_gpu_lattice.test_bf16_context); beyond it structure and the sum invariants (the recursions are double whatever the operands)"""
    eng = make("tiny", dtype="bf16")
    try:
        ys = transcripts("tiny", "greedy")
        res = eng.align_feats(SLOTS, feats_all(), ys, lattice=True, posteriors=True)
    finally:
        eng.close()
    for i, (r, y) in enumerate(zip(res, ys)):
        T, U = r["blank_lp"].shape[0], len(y)
        X.check_first_cell("tiny", feats_all()[i][0], r["blank_lp"][0, 0], {y[0]: r["emit_lp"][0, 0]} if U else {}, f"bf16 post utterance {i}")
        assert r["occ_blank"].shape == (T, U + 1) and r["occ_emit"].shape == (T, U + 1)
        for k in POST_KEYS:
            assert r[k].shape[0] == (T if k.startswith("occ") else U) and np.all(np.isfinite(r[k])), k
        assert np.all((r["occ_blank"] >= 0) & (r["occ_blank"] <= 1)) and np.all((r["occ_emit"] >= 0) & (r["occ_emit"] <= 1))
        sum_invariants(r, U)
        assert np.all((0 <= r["tok_peak_frame"]) & (r["tok_peak_frame"] < T))
        for u in range(U):
            assert np.float32(r["tok_peak"][u]) == r["occ_emit"][r["tok_peak_frame"][u], u] == r["occ_emit"][:, u].max()


# ------------------------------------------------------------------------------- (f) the facade
def test_facade_posteriors():
    import __graft_entry__ as graft
    graft.build()
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", config_path="/nonexistent.yaml", synthetic="tiny", max_streams=8)
    pcm, ys = utterances(), transcripts("tiny", "greedy")
    try:
        plain = asr.align([pcm[0], pcm[1]], [ys[0], ys[1]])
        out = asr.align([pcm[0], pcm[1]], [ys[0], ys[1]], posteriors=True)
        eng = asr.engine
        slots = [eng.open(), eng.open()]
        raw = eng.align_pcm(slots, [pcm[0], pcm[1]], [ys[0], ys[1]], posteriors=True)
        for s in slots:
            eng.close_slot(s)
        assert "posteriors" not in plain[0]
        for o, q, r, y, p in zip(out, plain, raw, ys, pcm):
            assert o["tokens"] == q["tokens"] and o["score"] == q["score"] and o["viterbi"] == q["viterbi"]
            assert len(o["posteriors"]) == len(y)
            for k, d in enumerate(o["posteriors"]):
                assert d["posterior"] == float(r["occ_emit"][int(r["frames"][k]), k])
                assert 0 <= d["posterior"] <= d["peak"] <= 1
                assert 0 <= d["time_mean_s"] <= len(p) / 16000 and d["time_std_s"] >= 0
                assert d["peak_time_s"] == float(r["tok_peak_frame"][k]) * 0.08
        one = asr.align(pcm[0], ys[0], posteriors=True)
        assert one["posteriors"] == out[0]["posteriors"]
    finally:
        asr.engine.close()
