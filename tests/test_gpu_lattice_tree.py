"""N-best rescoring over a prefix tree on the GPU (lasr_score_pcm / lasr_score_feats / lasr_lattice_tree_dp): one encoder pass per
utterance, one joint row per distinct (frame, prefix), one dynamic programme for every candidate.

Expected values: tests/lattice_tree_ref.py and tests/lattice_ref.py (float64 recursions, pinned in test_lattice_tree_cpu.py and
test_lattice_cpu.py; the terms from the numpy oracle's encoder / predictor / joint).  The bounds of the model tests are those of
test_gpu_lattice.py: a lattice term is z_k - lse of logits within 1e-3, so within TERM_TOL = 2e-3; a path adds T + U terms."""
import ctypes as C

import numpy as np
import pytest

import bf16_exact as X
import lattice_ref as R
import lattice_tree_ref as TR
from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O
from test_alignment_cpu import utterances

pytestmark = pytest.mark.gpu

TERM_TOL = 2e-3


def make(name, dtype="f32", max_streams=16, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    cfg = synth.model_cfg(name)
    sd = synth.synth_state_dict(cfg, seed=0)
    eng = Engine(sd, cfg, max_streams=max_streams, dtype=dtype, **kw)
    for _ in range(max_streams):
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


def candidates(name):
    """per utterance the 8 candidates of the issue, from the oracle's greedy tokens y (max_iters = 3)"""
    if (name, "cands") not in _REF:
        out = []
        for f in feats_all():
            y = [int(t) for t in oracle(name).decode_greedy(f, max_iters=3)[0]]
            h = len(y) // 2
            out.append([list(y), list(y), [], y[:h], (y[:-1] + [(y[-1] % 61) + 3]) if y else [3],
                        y[:h] + [((t + 7) % 61) + 3 for t in y[h:]], [(t % 60) + 3 for t in y][::-1], y + [5, 6]])
        _REF[name, "cands"] = out
    return _REF[name, "cands"]


def reference(name, operand="f32"):
    """per utterance, per candidate (y, b, e, loglik, viterbi) from tests/lattice_ref.py, computed once"""
    if (name, operand) not in _REF:
        m = oracle(name, operand)
        out = []
        for f, cs in zip(feats_all(), candidates(name)):
            done, per = {}, []
            for y in cs:
                if tuple(y) not in done:
                    b, e = R.lattice(m, f, y)
                    done[tuple(y)] = (y, b, e, R.forward(b, e, len(y)), R.viterbi(b, e, len(y))[0])
                per.append(done[tuple(y)])
            out.append(per)
        _REF[name, operand] = out
    return _REF[name, operand]


def gathered(res, j):
    """candidate j's chain out of the tree lattice of one utterance: (b [T, U + 1], e [T, U])"""
    p = TR.path(res["tree"]["parent"].tolist(), int(res["tree"]["term"][j]))
    return res["blank_lp"][:, p], res["emit_lp"][:, p[1:]]


# ------------------------------------------------------------------------------- (a) the tree DP kernel, exact
def level_tree(widths):
    """parent array of a tree in the library's order whose level d + 1 gives every node of level d widths[d] children"""
    parent, level = [-1], [0]
    for w in widths:
        nxt = []
        for p in level:
            for _ in range(w):
                nxt.append(len(parent))
                parent.append(p)
        level = nxt
    return parent


def dp_cases():
    rng = np.random.default_rng(2025)
    rnd = lambda T, n: -(rng.integers(0, 513, (T, n)) / 64.0).astype(np.float32)
    trees = [
        (5, level_tree([13, 22])),                                                   # 300 nodes, 286 of them on one depth: more than threads
        (1, TR.trie([[1, 2, 3], [1, 3], [2]])[0]),                                   # T = 1: every emission on frame 0
        (4, level_tree([5])),                                                        # a root with 5 children
        (7, TR.trie([[1, 2], [3] * 40])[0]),                                         # terminal depths 2 and 40: the saved final
        (33, TR.trie([[1, 2, 3, 4], [1, 2, 4], [1, 3], [2, 2, 2, 2, 2, 2]])[0]),     # another T and N in the same call
    ]
    assert len(trees[0][1]) == 300 and len(trees[3][1]) == 43
    cases = [(rnd(T, len(p)), rnd(T, len(p)), p) for T, p in trees]
    tie = TR.trie([[1, 2, 3], [1, 4], [5]])[0]
    cases.append((np.full((4, len(tie)), -0.5, np.float32), np.full((4, len(tie)), -0.5, np.float32), tie))      # every path ties
    return cases


def test_tree_dp_kernel_exact():
    cases = dp_cases()
    bs, es, ps = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    eng = make("tiny")
    try:
        import torch
        got = eng.lattice_tree_dp(bs, es, ps)
        # device-resident lattices, no Viterbi half: the same forward sums
        cat_b = torch.as_tensor(np.concatenate([x.reshape(-1) for x in bs])).to(eng.device)
        cat_e = torch.as_tensor(np.concatenate([x.reshape(-1) for x in es])).to(eng.device)
        Ts = np.array([x.shape[0] for x in bs], np.int32)
        Ns = np.array([x.shape[1] for x in bs], np.int32)
        par = np.concatenate([np.asarray(p, np.int32) for p in ps])
        ll_d = np.zeros(int(Ns.sum()))
        eng._chk(eng.lib.lasr_lattice_tree_dp(eng.ctx, C.c_void_p(cat_b.data_ptr()), C.c_void_p(cat_e.data_ptr()), Ts.ctypes.data_as(C.c_void_p),
                                              Ns.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p), len(cases),
                                              ll_d.ctypes.data_as(C.c_void_p), None))
        # what the call refuses
        one = lambda p, T=2: eng.lattice_tree_dp([np.zeros((T, len(p)), np.float32)], [np.zeros((T, len(p)), np.float32)], [p])
        for bad in ([0, 0], [-1, 1], [-1, -1], [-1, 0, 1, 0]):        # no root, parent >= node, no parent, depth decreases
            with pytest.raises(N.LasrError) as ei:
                one(bad)
            assert ei.value.code == N.LASR_EINVAL, bad
        with pytest.raises(N.LasrError):
            one(level_tree([2048]))                                                  # 2049 nodes
        assert len(one(level_tree([2047]))[0]["loglik"]) == 2048                     # the largest tree: 64 KB of LDS
    finally:
        eng.close()
    o = 0
    for i, ((b, e, p), g) in enumerate(zip(cases, got)):
        ll, vit = TR.tree_dp(b, e, p), TR.tree_dp(b, e, p, best=True)
        print(f"tree {i} T {b.shape[0]} N {len(p)}: max |dloglik| {np.abs(g['loglik'] - ll).max():.3g}")
        assert np.array_equal(g["viterbi"], vit), i
        assert np.abs(g["loglik"] - ll).max() <= 1e-8, i
        assert np.array_equal(ll_d[o:o + len(p)], g["loglik"]), i
        o += len(p)
    assert np.all(got[-1]["viterbi"] == -0.5 * (4 + np.asarray(TR.trie([[1, 2, 3], [1, 4], [5]])[2])))


# ------------------------------------------------------------------------------- (b) a chain is the existing kernel
def test_chain_equals_lattice_dp():
    rng = np.random.default_rng(77)
    shapes = [(1, 0), (1, 4), (5, 3), (37, 40), (8, 300)]
    bs = [(-rng.random((T, U + 1)) * 9).astype(np.float32) for T, U in shapes]
    es = [(-rng.random((T, U + 1)) * 9).astype(np.float32) for T, U in shapes]
    tes = [np.concatenate([np.zeros((e.shape[0], 1), np.float32), e[:, :-1]], axis=1) for e in es]      # the emission that enters v
    eng = make("tiny")
    try:
        want = eng.lattice_dp(bs, es)
        got = eng.lattice_tree_dp(bs, tes, [[-1] + list(range(U)) for _, U in shapes])
    finally:
        eng.close()
    for (T, U), w, g in zip(shapes, want, got):
        assert g["loglik"][U] == w["loglik"] and g["viterbi"][U] == w["viterbi"], (T, U, g["loglik"][U], w["loglik"])


# ------------------------------------------------------------------------------- (c) one candidate is lasr_align_feats
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_one_candidate_equals_align(name):
    ys = [c[0] for c in candidates(name)]
    slots = [5, 0, 3]
    eng = make(name)
    try:
        want = eng.align_feats(slots, feats_all(), ys, lattice=True)
        got = eng.score_feats([[s] for s in slots], feats_all(), [[y] for y in ys], viterbi=True, lattice=True)
    finally:
        eng.close()
    for w, g, y in zip(want, got, ys):
        U = len(y)
        assert g["tree"]["parent"].tolist() == [-1] + list(range(U))
        assert np.array_equal(g["blank_lp"], w["blank_lp"])
        assert np.array_equal(g["emit_lp"][:, 1:], w["emit_lp"][:, :U]) and np.all(g["emit_lp"][:, 0] == 0)
        assert g["loglik"][0] == w["loglik"] and g["viterbi"][0] == w["viterbi"]


# ------------------------------------------------------------------------------- (d) model parity, f32
@pytest.mark.parametrize("entry", ["feats", "pcm"])
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_model_parity(name, entry):
    """All three utterances in ONE call: 24 slots (three groups of 8) of a 32-slot engine."""
    cands, ref = candidates(name), reference(name)
    groups = [[3 * q + i for q in range(8)] for i in range(3)]           # interleaved: a group's rows are not adjacent
    eng = make(name, max_streams=32)
    try:
        if entry == "feats":
            res = eng.score_feats(groups, feats_all(), cands, viterbi=True, lattice=True)
        else:
            res = eng.score_pcm(groups, utterances(), cands, viterbi=True, lattice=True)
        Rb = eng.config("lat_R")
    finally:
        eng.close()
    Ts = [r["blank_lp"].shape[0] for r in res]
    nodes = [int(r["tree"]["parent"].size) for r in res]
    assert Ts == [37, 25, 6] and nodes == {"tiny": [34, 6, 4], "tiny_lstm": [79, 29, 4]}[name]
    assert Ts[0] * nodes[0] == {"tiny": 1258, "tiny_lstm": 2923}[name] and Ts[0] * nodes[0] > (Rb if name == "tiny" else 2 * Rb)
    worst_t = worst_l = 0.0
    for i, (r, per) in enumerate(zip(res, ref)):
        T = Ts[i]
        for j, (y, b, e, ll, vit) in enumerate(per):
            U = len(y)
            assert np.isfinite(ll) and np.isfinite(vit)
            gb, ge = gathered(r, j)
            assert gb.shape == (T, U + 1) and ge.shape == (T, U)
            db = float(np.abs(gb.astype(np.float64) - b).max())
            de = float(np.abs(ge.astype(np.float64) - e[:, :U]).max()) if U else 0.0
            dl = abs(float(r["loglik"][j]) - ll)
            worst_t, worst_l = max(worst_t, db, de), max(worst_l, dl / (T + U))
            assert db <= TERM_TOL and de <= TERM_TOL, (name, entry, i, j, db, de)
            assert dl <= (T + U) * TERM_TOL, (name, entry, i, j, r["loglik"][j], ll)
            assert r["viterbi"][j] <= r["loglik"][j] + 1e-9
        assert r["loglik"][0] == r["loglik"][1] and r["viterbi"][0] == r["viterbi"][1]      # the duplicate candidates
        assert np.all(r["emit_lp"][:, 0] == 0)
    print(f"{name} {entry}: max term error {worst_t:.3g}, max |dloglik| / (T + U) {worst_l:.3g}")


# ------------------------------------------------------------------------------- (e) state and errors
def test_state_and_errors():
    eng = make("tiny")
    try:
        f, cands = feats_all(), candidates("tiny")
        slots3 = [5, 0, 3]
        y0 = list(cands[0][0])

        def fresh_tokens():
            eng.transcribe_feats(slots3, f)
            return [eng.fetch(s)[0] for s in slots3]

        fresh = fresh_tokens()
        assert fresh == [c[0] for c in cands]
        groups = [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15]]
        ref = eng.score_feats(groups, f[:2], cands[:2], viterbi=True, lattice=True)

        def refused(code, *a, **kw):
            with pytest.raises(N.LasrError) as ei:
                eng.score_feats(*a, **kw)
            assert ei.value.code == code, ei.value
            if code == N.LASR_EINVAL:
                assert fresh_tokens() == fresh                                      # nothing changed

        refused(N.LASR_EINVAL, [[5, 6]], [f[0]], [[y0, y0[:2] + [0]]])                           # a blank label
        refused(N.LASR_EINVAL, [[5, 6]], [f[0]], [[y0, [64]]])                                   # out of range
        refused(N.LASR_EINVAL, [[5], []], f[:2], [[y0], []])                                     # n_cands < 1
        refused(N.LASR_EINVAL, [[5, 6], [7, 5]], f[:2], [[y0, []], [y0, [3]]])                   # a slot listed twice
        refused(N.LASR_EINVAL, [list(range(16)), [0]], f[:2], [[[3]] * 16, [[4]]])               # more candidates than max_streams
        refused(N.LASR_EINVAL, [[5, 6]], [f[0]], [[y0, [3] * 1536]])                             # U > 1535
        refused(N.LASR_EINVAL, [[5, 6]], [f[0]], [[[3] * 1100, [4] * 1100]])                     # 2201 nodes
        with pytest.raises(N.LasrError) as ei:
            eng.score_pcm([[5, 6]], [utterances()[0]], [[y0, [0]]])
        assert ei.value.code == N.LASR_EINVAL and fresh_tokens() == fresh
        # the same call as before gives the same bits
        again = eng.score_feats(groups, f[:2], cands[:2], viterbi=True, lattice=True)
        for a, b in zip(ref, again):
            assert np.array_equal(a["loglik"], b["loglik"]) and np.array_equal(a["viterbi"], b["viterbi"])
            assert np.array_equal(a["blank_lp"], b["blank_lp"]) and np.array_equal(a["emit_lp"], b["emit_lp"])
        # every optional output may be null: no Viterbi half, no lattice
        only = eng.score_feats(groups, f[:2], cands[:2])
        assert all(np.array_equal(o["loglik"], r["loglik"]) for o, r in zip(only, ref)) and "viterbi" not in only[0]
        # a transcribe on slots of the call afterwards: what a fresh engine returns; no result is left from the call
        assert all(eng.fetch(s)[0] == [] for s in slots3)
        assert fresh_tokens() == fresh
        # ... and a streaming run, on the slot that held the audio and on one that held only a candidate
        pcm = utterances()[0]
        for slot in (1, 2):
            want = None
            for rep in range(2):
                eng.reset(slot, 15)
                got = []
                for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=4):
                    eng.push([slot], ch[None])
                    eng.step([slot])
                    got += eng.fetch(slot)[0]
                if rep == 0:
                    want = got
                    eng.score_pcm([[1, 2, 4]], [pcm], [[y0, y0[:3], []]])
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
        refused(N.LASR_ESTATE, [[5, 6]], [f[0]], [[y0, []]])
        while eng.pending():
            eng.wait()
        eng.fetch(1)
        assert np.array_equal(eng.score_feats(groups, f[:2], cands[:2])[0]["loglik"], ref[0]["loglik"])
    finally:
        eng.close()


def test_beam_context_is_refused():
    eng = make("tiny", beam=2)
    try:
        def tokens():
            eng.transcribe_feats([0, 1], feats_all()[:2])
            return [eng.fetch(s)[0] for s in (0, 1)]

        before = tokens()
        with pytest.raises(N.LasrError) as ei:
            eng.score_feats([[0, 1]], [feats_all()[0]], [[[3], [4]]])
        assert ei.value.code == N.LASR_EINVAL
        assert tokens() == before and len(before[0]) > 0               # nothing changed
    finally:
        eng.close()


# ------------------------------------------------------------------------------- (f) bf16 context
def test_bf16_context():
    """The root's row on the first frame (blank, and the emission into every child of the root) within the bound of
    tests/bf16_exact.py, as -- and as loose as -- in test_gpu_lattice.test_bf16_context; beyond it structure only; the distance to
    the oracle's operand="bf16" emulation is printed (DESIGN 5.4 records it)."""
    cands = candidates("tiny")
    eng = make("tiny", dtype="bf16", max_streams=32)
    try:
        res = eng.score_feats([[3 * q + i for q in range(8)] for i in range(3)], feats_all(), cands, viterbi=True, lattice=True)
    finally:
        eng.close()
    ref = reference("tiny", "bf16")
    for i, (r, per) in enumerate(zip(res, ref)):
        assert np.all(np.isfinite(r["blank_lp"])) and np.all(np.isfinite(r["emit_lp"]))
        assert np.all(np.isfinite(r["loglik"])) and np.all(np.isfinite(r["viterbi"]))
        assert np.all(r["viterbi"] <= r["loglik"] + 1e-9)
        assert r["loglik"][0] == r["loglik"][1] and r["viterbi"][0] == r["viterbi"][1]
        tree = r["tree"]
        kids = {int(tree["label"][v]): r["emit_lp"][0, v] for v in range(1, len(tree["parent"])) if tree["parent"][v] == 0}
        X.check_first_cell("tiny", feats_all()[i][0], r["blank_lp"][0, 0], kids, f"bf16 tree utterance {i}")
        dt = dl = 0.0
        for j, (y, b, e, ll, vit) in enumerate(per):
            gb, ge = gathered(r, j)
            dt = max(dt, float(np.abs(gb.astype(np.float64) - b).max()), float(np.abs(ge.astype(np.float64) - e[:, :len(y)]).max()) if y else 0.0)
            dl = max(dl, abs(float(r["loglik"][j]) - ll))
        print(f"bf16 utterance {i}: T {r['blank_lp'].shape[0]} N {r['blank_lp'].shape[1]} max term distance {dt:.3g} max |dloglik| {dl:.3g}")


# ------------------------------------------------------------------------------- (g) the facade
def test_facade_rescore():
    import __graft_entry__ as graft
    graft.build()
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", config_path="/nonexistent.yaml", synthetic="tiny", max_streams=8)
    try:
        pcm = utterances()[0]
        cs = candidates("tiny")[0]
        y = cs[0]
        # 10 candidates on 8 slots: two engine calls.  The two extra ones are wrong continuations (float64 reference: -47.6 and -44.6
        # against -18.3 for y); a short prefix of y would not do: the reference gives y[:2] -18.19, above y itself
        cands = cs + [cs[6][:4], y[:1] + [7, 8, 9]]
        new, old = asr.rescore(pcm, cands), asr.score(pcm, cands)
        T = feats_all()[0].shape[0]
        assert len(new) == 10
        for c, a, b in zip(cands, new, old):
            assert abs(a - b) <= (T + len(c)) * 2 * TERM_TOL, (c, a, b)
        assert int(np.argmax(new)) == 0 and new[0] == new[1]
        sc, vit = asr.rescore(pcm, cands[:3], viterbi=True)
        assert all(abs(a - b) <= (T + len(c)) * 2 * TERM_TOL for c, a, b in zip(cands, sc, new))      # (another tree: other blocks)
        assert all(v <= s + 1e-9 for v, s in zip(vit, sc))
    finally:
        asr.engine.close()
