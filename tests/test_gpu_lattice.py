"""The teacher-forced RNN-T lattice on the GPU (lasr_align_pcm / lasr_align_feats / lasr_lattice_dp): forced alignment and
log P(y | x) of a transcript the caller already has.

Expected values: tests/lattice_ref.py (float64 recursions, pinned in test_lattice_cpu.py; the lattice terms from the numpy oracle's
encoder / predictor / joint).  Bounds of the model tests follow from the project's own logits bound of 1e-3 (DESIGN section 0,
test_gpu_parity): a lattice term is z_k - lse, so its error is at most 2e-3; a path adds T + U terms."""
import numpy as np
import pytest

import bf16_exact as X
import lattice_ref as R
from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O
from test_alignment_cpu import utterances

pytestmark = pytest.mark.gpu

TERM_TOL = 2e-3
SLOTS = [5, 0, 3]


def make(name, dtype="f32", **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    cfg = synth.model_cfg(name)
    sd = synth.synth_state_dict(cfg, seed=0)
    eng = Engine(sd, cfg, max_streams=8, dtype=dtype, **kw)
    for _ in range(8):
        eng.open()
    return eng


_ORACLE, _FEATS, _REF = {}, [], {}


def oracle(name, operand="f32"):
    if (name, operand) not in _ORACLE:
        cfg = synth.model_cfg(name)
        _ORACLE[name, operand] = O.OracleTransducer(synth.synth_state_dict(cfg, seed=0), cfg, operand=operand)
    return _ORACLE[name, operand]


def feats_all():
    if not _FEATS:
        _FEATS.extend(O.features_offline(p) for p in utterances())
    return _FEATS


def transcripts(name, kind):
    """per utterance: the oracle's greedy tokens ("greedy"), a deliberately wrong transcript ("wrong"), 40 random labels ("rand40")"""
    key = (name, kind)
    if key not in _REF:
        m = oracle(name)
        if kind == "rand40":
            rng = np.random.default_rng(40)
            ys = [[int(v) for v in rng.integers(1, m.cfg["vocab"], 40)] for _ in feats_all()]
        else:
            ys = [m.decode_greedy(f, max_iters=3)[0] for f in feats_all()]
            if kind == "wrong":
                ys = [[(t % 60) + 3 for t in y][::-1] for y in ys]
        _REF[key] = ys
    return _REF[key]


def reference(name, kind, operand="f32"):
    """per utterance (y, b, e, loglik, viterbi, frames) from the float64 reference, computed once"""
    key = (name, kind, operand, "lat")
    if key not in _REF:
        m = oracle(name, operand)
        out = []
        for f, y in zip(feats_all(), transcripts(name, kind)):
            b, e = R.lattice(m, f, y)
            v, fr = R.viterbi(b, e, len(y))
            out.append((y, b, e, R.forward(b, e, len(y)), v, fr))
        _REF[key] = out
    return _REF[key]


def check_against(res, ref, what):
    """the bounds of the issue for one utterance: res = the engine's dict (with the lattice), ref = reference(..)[i]"""
    y, b, e, ll, v, _ = ref
    T, U = b.shape[0], len(y)
    assert res["blank_lp"].shape == (T, U + 1) and res["emit_lp"].shape == (T, U + 1), what
    eb = float(np.abs(res["blank_lp"].astype(np.float64) - b).max())
    ee = float(np.abs(res["emit_lp"][:, :U].astype(np.float64) - e[:, :U]).max()) if U else 0.0
    assert np.all(res["emit_lp"][:, U] == 0), what
    print(f"{what}: T {T} U {U} max |db| {eb:.3g} max |de| {ee:.3g} dloglik {res['loglik'] - ll:.3g}")
    assert eb <= TERM_TOL and ee <= TERM_TOL, (what, eb, ee)
    assert abs(res["loglik"] - ll) <= (T + U) * TERM_TOL, (what, res["loglik"], ll)
    fr = [int(t) for t in res["frames"]]
    assert len(fr) == U and fr == sorted(fr) and all(0 <= t < T for t in fr), (what, fr)
    for u in range(U):
        assert abs(float(res["logps"][u]) - float(e[fr[u], u])) <= TERM_TOL, (what, u)
    assert R.path_score(b, e, fr) >= v - 2 * (T + U) * TERM_TOL, (what, R.path_score(b, e, fr), v)
    assert res["viterbi"] <= res["loglik"] + 1e-9, what


# ------------------------------------------------------------------------------- (a) the DP kernel, exact
def test_dp_kernel_exact():
    shapes = [(1, 0), (1, 3), (5, 0), (2, 1), (3, 2), (64, 63), (65, 64), (70, 130), (300, 5)]
    rng = np.random.default_rng(2024)
    bs = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in shapes]
    es = [-(rng.integers(0, 513, (T, U + 1)) / 64.0).astype(np.float32) for T, U in shapes]
    bs.append(np.full((4, 4), -0.5, np.float32))          # every path ties
    es.append(np.full((4, 4), -0.5, np.float32))
    shapes.append((4, 3))
    eng = make("tiny")
    try:
        import torch
        got = eng.lattice_dp(bs, es)
        # device-resident lattices through the same entry point
        import ctypes as C
        cat_b = torch.as_tensor(np.concatenate([x.reshape(-1) for x in bs])).to(eng.device)
        cat_e = torch.as_tensor(np.concatenate([x.reshape(-1) for x in es])).to(eng.device)
        Ts = np.array([s[0] for s in shapes], np.int32)
        Us = np.array([s[1] for s in shapes], np.int32)
        ll_d = np.zeros(len(shapes))
        eng._chk(eng.lib.lasr_lattice_dp(eng.ctx, C.c_void_p(cat_b.data_ptr()), C.c_void_p(cat_e.data_ptr()), Ts.ctypes.data_as(C.c_void_p),
                                         Us.ctypes.data_as(C.c_void_p), len(shapes), ll_d.ctypes.data_as(C.c_void_p), None, None))
    finally:
        eng.close()
    for i, ((T, U), b, e, g) in enumerate(zip(shapes, bs, es, got)):
        v, fr = R.viterbi(b, e, U)
        ll = R.forward(b, e, U)
        print(f"lattice {i} T {T} U {U}: dloglik {g['loglik'] - ll:.3g}")
        assert g["viterbi"] == v, (i, g["viterbi"], v)
        assert [int(t) for t in g["frames"]] == fr, i
        assert abs(g["loglik"] - ll) <= 1e-8, (i, g["loglik"], ll)
        assert ll_d[i] == g["loglik"], i                   # no Viterbi pass, device input: the same forward sum
    assert [int(t) for t in got[-1]["frames"]] == [0, 0, 0]


def test_dp_kernel_more_labels_than_threads():
    """U + 1 > 256: every thread of the workgroup owns more than one u of a diagonal."""
    rng = np.random.default_rng(300)
    b = -(rng.integers(0, 513, (8, 301)) / 64.0).astype(np.float32)
    e = -(rng.integers(0, 513, (8, 301)) / 64.0).astype(np.float32)
    eng = make("tiny")
    try:
        g = eng.lattice_dp([b], [e])[0]
    finally:
        eng.close()
    v, fr = R.viterbi(b, e, 300)
    assert g["viterbi"] == v and [int(t) for t in g["frames"]] == fr
    assert abs(g["loglik"] - R.forward(b, e, 300)) <= 1e-8


# ------------------------------------------------------------------------------- (b) model parity, f32
@pytest.mark.parametrize("entry", ["feats", "pcm"])
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_model_parity(name, entry):
    eng = make(name)
    try:
        for kind in ("greedy", "wrong"):
            ys = transcripts(name, kind)
            if entry == "feats":
                res = eng.align_feats(SLOTS, feats_all(), ys, lattice=True)
            else:
                res = eng.align_pcm(SLOTS, utterances(), ys, lattice=True)
            ref = reference(name, kind)
            assert [r[1].shape[0] for r in ref] == [37, 25, 6] and len(ref[2][0]) == 0
            for i in range(3):
                check_against(res[i], ref[i], f"{name} {entry} {kind} utterance {i}")
    finally:
        eng.close()


def test_terms_against_the_decode_records():
    """A token greedy decode emits as its k-th on frame t was scored against g_k and f_t: its recorded log p is e[t, k] of the lattice
    of greedy's own transcript (whatever the per-frame cap did).  Both are within 1e-3 of the truth (the project's bound), so
    within 2e-3 of each other; the log-softmax arithmetic is the same, the logits GEMM may run on another tiling."""
    eng = make("tiny_lstm")
    try:
        eng.set_alignments(True)
        eng.transcribe_pcm(SLOTS, utterances())
        recs = [eng.fetch_aligned(s)[:3] for s in SLOTS]
        eng.set_alignments(False)
        res = eng.align_pcm(SLOTS, utterances(), [r[0] for r in recs], lattice=True)
    finally:
        eng.close()
    n = worst = 0
    for (tok, fr, lp), r in zip(recs, res):
        for k in range(len(tok)):
            worst = max(worst, abs(float(r["emit_lp"][fr[k], k]) - float(lp[k])))
            n += 1
    print(f"{n} decode records against the lattice: max |d| {worst:.3g}")
    assert n >= 30 and worst <= TERM_TOL


# ------------------------------------------------------------------------------- (c) block boundaries
def test_block_boundaries():
    eng = make("tiny")
    try:
        Rb = eng.config("lat_R")
        ys = transcripts("tiny", "rand40")
        cells = sum(f.shape[0] * 41 for f in feats_all())
        assert cells > 2 * Rb and cells % Rb != 0          # two block boundaries at least, and a partial last block
        res = eng.align_feats(SLOTS, feats_all(), ys, lattice=True)
        for i, ref in enumerate(reference("tiny", "rand40")):
            check_against(res[i], ref, f"tiny rand40 utterance {i}")
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (d) a real shape once
def test_cfg2_wide_logits_tiling():
    m = oracle("cfg2")
    pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
    f = O.features_offline(pcm)
    y = [int(v) for v in np.random.default_rng(12).integers(1, m.cfg["vocab"], 12)]
    b, e = R.lattice(m, f, y)
    assert b.shape[0] * 13 < 512       # one partial block: the narrow tiling; the wide one (>= 512 rows, V % 64 == 0) needs a second call
    eng = make("cfg2")
    try:
        res = eng.align_pcm([2], [pcm], [y], lattice=True)[0]
        check_against(res, (y, b, e, R.forward(b, e, 12), *R.viterbi(b, e, 12)), "cfg2")
        # the same utterance on four slots: 4 x 37 x 13 = 1924 rows, a full block of lat_R rows on the 64 x 64 tiling + a partial one
        assert 4 * b.shape[0] * 13 > eng.config("lat_R") >= 512
        res4 = eng.align_pcm([1, 7, 0, 4], [pcm] * 4, [y] * 4, lattice=True)
        for i, r in enumerate(res4):
            check_against(r, (y, b, e, R.forward(b, e, 12), *R.viterbi(b, e, 12)), f"cfg2 x4 row {i}")
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (e) state and errors
def test_state_and_errors():
    eng = make("tiny")
    try:
        f, ys = feats_all(), transcripts("tiny", "greedy")
        fresh = []
        eng.transcribe_pcm(SLOTS, utterances())
        fresh = [eng.fetch(s)[0] for s in SLOTS]
        assert fresh == ys
        ref = eng.align_feats(SLOTS, f, ys, lattice=True)

        def refused(code, fn, *a, **kw):
            with pytest.raises(N.LasrError) as ei:
                fn(*a, **kw)
            assert ei.value.code == code, ei.value

        y0 = list(ys[0])
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0[:2] + [0] + y0[2:]])              # a blank label
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [y0[:2] + [64]])                      # out of range
        refused(N.LASR_EINVAL, eng.align_feats, [5], [f[0]], [[-1]])
        refused(N.LASR_EINVAL, eng.align_pcm, [5], [utterances()[0]], [[0]])
        import ctypes as C
        sl, nf, nt = np.array([5], np.int32), np.array([f[0].shape[0]], np.int32), np.array([-1], np.int32)
        ll = np.zeros(1)
        x = np.ascontiguousarray(f[0], np.float32)
        rc = eng.lib.lasr_align_feats(eng.ctx, sl.ctypes.data_as(C.c_void_p), 1, x.ctypes.data_as(C.c_void_p), nf.ctypes.data_as(C.c_void_p),
                                      None, nt.ctypes.data_as(C.c_void_p), ll.ctypes.data_as(C.c_void_p), None, None, None, None, None)
        assert rc == N.LASR_EINVAL                                                                 # a negative n_tokens
        # nothing changed: the same call as before gives the same bits
        again = eng.align_feats(SLOTS, f, ys, lattice=True)
        for a, b in zip(ref, again):
            assert a["loglik"] == b["loglik"] and a["viterbi"] == b["viterbi"]
            assert np.array_equal(a["blank_lp"], b["blank_lp"]) and np.array_equal(a["emit_lp"], b["emit_lp"])
            assert np.array_equal(a["frames"], b["frames"]) and np.array_equal(a["logps"], b["logps"])
        # every optional output may be null: scoring only (no Viterbi pass), no lattice
        only = eng.align_feats(SLOTS, f, ys, viterbi=False)
        assert [r["loglik"] for r in only] == [r["loglik"] for r in ref] and "frames" not in only[0]
        # a transcribe on the same slots afterwards: what a fresh engine returns; no result is left from the align call
        assert all(eng.fetch(s)[0] == [] for s in SLOTS)
        eng.transcribe_pcm(SLOTS, utterances())
        assert [eng.fetch(s)[0] for s in SLOTS] == fresh
        # ... and a streaming run
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
                eng.align_pcm([1], [pcm], [ys[0]])
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
        refused(N.LASR_ESTATE, eng.align_feats, [5], [f[0]], [y0])
        while eng.pending():
            eng.wait()
        eng.fetch(1)
        assert eng.align_feats([5], [f[0]], [y0])[0]["loglik"] == ref[0]["loglik"]
    finally:
        eng.close()


def test_beam_context_is_refused():
    eng = make("tiny", beam=2)
    try:
        with pytest.raises(N.LasrError) as ei:
            eng.align_feats([0], [feats_all()[0]], [transcripts("tiny", "greedy")[0]])
        assert ei.value.code == N.LASR_EINVAL
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (f) bf16 context
def test_bf16_context():
    """The first frame's first label row (the encoder on one frame, the predictor after BOS, the joint: the depth
    test_gpu_bf16_exact.py bounds stage by stage) is held to the float64 model of tests/bf16_exact.py: |engine - value| <= tol + flip
    (bf16_exact.check_first_cell).  Behind the encoder's K = 1280 GEMM every element inherits a flip allowance, and on these
    utterances (an x0 with tie-sensitive elements, two encoder layers) the allowance adds up to a few units of log p: the assertion
    catches a wrong row or a wrong sign, not a subtle fault (docs/bf16_bound.md).  Longer dependence -- every other cell, loglik,
    the paths -- stays structure-only; the distance to the oracle's operand="bf16" emulation is printed (DESIGN 5.3 records it)."""
    eng = make("tiny", dtype="bf16")
    try:
        ys = transcripts("tiny", "greedy")
        res = eng.align_feats(SLOTS, feats_all(), ys, lattice=True)
    finally:
        eng.close()
    ref = reference("tiny", "greedy", "bf16")
    for i, (r, y) in enumerate(zip(res, ys)):
        T, U = r["blank_lp"].shape[0], len(y)
        assert np.all(np.isfinite(r["blank_lp"])) and np.all(np.isfinite(r["emit_lp"])) and np.isfinite(r["loglik"]) and np.isfinite(r["viterbi"])
        fr = [int(t) for t in r["frames"]]
        assert len(fr) == U and fr == sorted(fr) and all(0 <= t < T for t in fr)
        assert r["viterbi"] <= r["loglik"] + 1e-9
        for u in range(U):
            assert r["logps"][u] == r["emit_lp"][fr[u], u]
        db = float(np.abs(r["blank_lp"].astype(np.float64) - ref[i][1]).max())
        de = float(np.abs(r["emit_lp"][:, :U].astype(np.float64) - ref[i][2][:, :U]).max()) if U else 0.0
        print(f"bf16 utterance {i}: T {T} U {U} max |db| {db:.3g} max |de| {de:.3g} dloglik {r['loglik'] - ref[i][3]:.3g}")
        X.check_first_cell("tiny", feats_all()[i][0], r["blank_lp"][0, 0], {y[0]: r["emit_lp"][0, 0]} if U else {}, f"bf16 utterance {i}")


# ------------------------------------------------------------------------------- (g) the facade
def test_facade_align_and_score():
    import __graft_entry__ as graft
    graft.build()
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", config_path="/nonexistent.yaml", synthetic="tiny", max_streams=8)
    pcm = utterances()
    ys, wrong = transcripts("tiny", "greedy"), transcripts("tiny", "wrong")
    ref = reference("tiny", "greedy")
    out = asr.align([pcm[0], pcm[1]], [ys[0], ys[1]])
    eng = asr.engine
    slots = [eng.open(), eng.open()]
    raw = eng.align_pcm(slots, [pcm[0], pcm[1]], [ys[0], ys[1]])
    for s in slots:
        eng.close_slot(s)
    for o, r, y in zip(out, raw, ys):
        assert o["score"] == r["loglik"] and o["viterbi"] == r["viterbi"]
        assert [t for t, _, _ in o["tokens"]] == list(y)
        assert [ts for _, ts, _ in o["tokens"]] == [float(f) * 0.08 for f in r["frames"]]
        assert [cf for _, _, cf in o["tokens"]] == [float(np.exp(np.float64(lp))) for lp in r["logps"]]
    one = asr.align(pcm[0], ys[0])
    assert one["score"] == out[0]["score"]
    assert abs(one["score"] - ref[0][3]) <= (ref[0][1].shape[0] + len(ys[0])) * TERM_TOL
    # rescoring: more candidates than slots (two engine calls), the greedy transcript wins
    cands = [ys[0], wrong[0]] + [wrong[0][:k] for k in range(1, 9)]
    sc = asr.score(pcm[0], cands)
    assert len(sc) == 10 and sc[0] == one["score"] and sc[0] > sc[1]
    wr = reference("tiny", "wrong")[0]                 # (the oracle: -18.3 against -122.7)
    assert abs(sc[1] - wr[3]) <= (wr[1].shape[0] + len(wrong[0])) * TERM_TOL
    asr.engine.close()
