"""The decision side of the decoder at its edges (needs an MI355X): a nonzero blank id, BOS 1, the per-frame symbol cap at 1, 2 and
3 (also inside a lookahead window), vocabularies on every path of k_select / k_lat_pick* (2064: 16 register slots with padding;
4096: the LM limit and the wide lattice tiling; 4112: the re-read tail, not a multiple of 64) and exact ties between logits, which
must go to the lowest index.

Models and utterances: tests/decision_edges.py; test_decision_edges_cpu.py asserts on the oracle alone that the edges occur on them
and that no decision is closer than 5e-3.  Expected values: OracleTransducer(sd, cfg, blank=.., bos=1) and the float64
tests/lattice_ref.py, never the engine.  Bounds: tokens and frames equal; log p and logits within 1e-3 (test_gpu_parity,
test_gpu_alignment); lattice terms within TERM_TOL, loglik / viterbi as test_gpu_lattice.check_against."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import decision_edges as D
import lattice_post_ref as P
import lattice_ref as R
from libreasr_amd import _native as N
from test_gpu_alignment import LOGP_TOL, align_from_frames, check_records
from test_gpu_lattice import TERM_TOL, check_against
from test_gpu_lattice_post import sum_invariants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGITS_TOL = 1e-3
IDS = [f"{n}-V{v}-blank{b}" for n, v, b in D.MODELS]
_ENGINES = {}


def make(mod, off=3, st=10, dtype="f32", max_streams=8, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    return Engine(mod.sd, mod.cfg, max_streams=max_streams, max_iters_offline=off, max_iters_stream=st, blank=mod.blank, bos=mod.bos,
                  dtype=dtype, **kw)


def engine(key, dtype="f32"):
    """one engine per model and operand type for the op-level and lattice tests (caps 3 / 10), kept for the module"""
    if (key, dtype) not in _ENGINES:
        eng = make(D.model(*key), dtype=dtype, max_streams=16)
        for _ in range(16):
            eng.open()
        _ENGINES[key, dtype] = eng
    return _ENGINES[key, dtype]


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------- 1. op-level joint (k_select<PLAIN>)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("key", D.MODELS[::2], ids=IDS[::2])
def test_joint_ties_go_to_the_lowest_index(key, dtype):
    mod = D.model(*key)
    eng = engine(key, dtype)
    hp, he, _ = D.states(mod, 2)
    parts = [[x.cpu().numpy() for x in eng.joint(dev(hp[r:r + 16]), dev(he[r:r + 16]))] for r in range(0, 64, 16)]      # B <= max_streams
    logits, lp, am = (np.concatenate([p[k] for p in parts]) for k in range(3))
    assert logits.shape == (64, mod.V)
    # the premise of every test of this file: a copy is bit-equal to its source on the GPU as well
    for g in mod.groups:
        for j in g[1:]:
            assert np.array_equal(logits[:, j].view(np.int32), logits[:, g[0]].view(np.int32)), (g, j)
    first = {j: g[0] for g in mod.groups for j in g}
    if dtype == "bf16":
        # no oracle needed: wherever the argmax falls in a group it is the group's lowest index, and it is a first maximum
        assert sum(int(a) in first for a in am) >= 5
        for r, a in enumerate(am):
            assert first.get(int(a), int(a)) == int(a), (r, int(a))
            assert int(a) == int(np.argmax(logits[r])), r
        return
    ref_lp, ref_z = mod.m.joint_logp(hp, he)
    want = ref_z.argmax(-1)
    assert {int(a) for a in want if int(a) in first} == {g[0] for g in mod.groups}
    assert [int(a) for a in am] == [int(a) for a in want]
    dz = float(np.abs(logits.astype(np.float64) - ref_z).max())
    dl = float(np.abs(lp.astype(np.float64) - ref_lp.max(-1)).max())
    print(f"{key}: max |d logits| {dz:.3g} max |d lp| {dl:.3g}")
    assert dz < LOGITS_TOL and dl < LOGP_TOL


# ------------------------------------------------------------------------------- 2. greedy decode against the oracle
def check_offline(eng, mod, cap, what):
    slots = [eng.open() for _ in range(4)]
    use = [slots[3], slots[1]]
    eng.transcribe_pcm(use, D.utterances())
    worst = 0.0
    for i, (s, r) in enumerate(zip(use, D.offline(mod, cap))):
        tok, fr, lp, neg_logp, align = eng.fetch_aligned(s)
        check_records((tok, fr, lp), (r.tokens, r.frames, r.logps), (what, i))
        if len(lp):
            worst = max(worst, float(np.abs(np.asarray(lp, np.float64) - np.asarray(r.logps)).max()))
        T = len(r.evals)
        assert abs(neg_logp - r.neg_logp) < 1e-2 * max(1.0, abs(r.neg_logp)), (what, i, neg_logp, r.neg_logp)
        assert abs(neg_logp - r.neg_logp) <= r.sum_iters * LOGP_TOL, (what, i)          # one log p per decision, each within the bound
        # the alignment score is (sum_iters - n_ones) / (sum_iters + 1e-4) of the row's own counters: both follow from the oracle's
        assert abs(align - (r.sum_iters - r.n_ones) / (r.sum_iters + 1e-4)) < 1e-9, (what, i, align)
        assert abs(align - r.score) < 1e-9 and abs(align_from_frames(fr, T, cap) - align) < 1e-9, (what, i)
    for s in slots:
        eng.close_slot(s)
    return worst


@pytest.mark.parametrize("cap", D.OFFLINE_CAPS)
@pytest.mark.parametrize("key", D.MODELS, ids=IDS)
def test_offline_greedy(key, cap):
    mod = D.model(*key)
    eng = make(mod, off=cap)
    try:
        eng.set_alignments(True)
        worst = check_offline(eng, mod, cap, (key, "cap", cap))
        print(f"{key} cap {cap}: max |d lp| {worst:.3g}")
    finally:
        eng.close()


@pytest.mark.parametrize("tie", ["plus", "minus"])
def test_offline_blank_tie_rows(tie):
    """a row bit-equal to the blank: behind it (blank + 1) it is never emitted, in front of it (blank - 1) it takes every decision the
    blank would have won, so every frame runs into the cap"""
    mod = D.model(*D.TIE_MODEL, tie)
    eng = make(mod, off=2, st=2)
    try:
        eng.set_alignments(True)
        check_offline(eng, mod, 2, ("blank tie", tie))
        check_stream(eng, mod, 2, [0, 1], "sync", ("blank tie", tie))
    finally:
        eng.close()


def check_stream(eng, mod, cap, rows, mode, what, reset=None):
    """rows of decision_edges.utterances() as streams on non-contiguous slots; reset = {row: model step} (synchronous only)"""
    reset = reset or {}
    refs = [D.stream(mod, cap, row, reset.get(row)) for row in rows]
    chunks = [D.chunks(row) for row in rows]
    slots = [eng.open() for _ in range(4)]
    use = [slots[3], slots[1]][:len(rows)]
    done = [0]

    def collect():
        for i, got in enumerate(eng.fetch_many_aligned(use, 64)):
            check_records(got, refs[i].steps[done[0]], (what, mode, "step", done[0], "row", rows[i]))
        done[0] += 1
        for i, row in enumerate(rows):
            if reset.get(row) == done[0]:
                eng.reset(use[i], 7)                     # model state only: BOS through k_reset_rows, the frame count runs on

    for k in range(len(chunks[0])):
        x = np.stack([c[k] for c in chunks])
        if mode == "sync":
            eng.push(use, x)
            if eng.step(use):
                collect()
        else:
            eng.push_submit(use, x)
            if eng.pending() >= 3 and eng.wait():
                collect()
    while eng.pending():
        if eng.wait():
            collect()
    assert done[0] == len(refs[0].steps) and sum(len(r.tokens) for r in refs) >= 20, what
    for s in slots:
        eng.close_slot(s)


@pytest.mark.parametrize("key", D.STREAM_MODELS, ids=IDS[:2])
def test_streaming_greedy(key):
    mod = D.model(*key)
    for cap in (2, 10):
        eng = make(mod, off=3, st=cap)
        try:
            eng.set_alignments(True)
            for c, reset in D.STREAM_RUNS:                 # every run is both utterances as two streams
                if c == cap:
                    check_stream(eng, mod, cap, [0, 1], "sync", (key, cap), reset=reset)
            check_stream(eng, mod, cap, [0, 1], "pipelined", (key, cap))
        finally:
            eng.close()


def test_bos_pass_per_reset():
    """LASR_BOS_CACHE=0 (read once per process, hence the child): a reset runs the predictor on BOS = 1 instead of storing the state
    captured at create; the same stream with a reset in the middle"""
    key = D.STREAM_MODELS[0]
    code = r'''
import json, sys
sys.path[:0] = [%r, %r]
import numpy as np
import decision_edges as D
import test_gpu_decision_edges as G
mod = D.model(*%r)
eng = G.make(mod, st=2)
use = [eng.open() for _ in range(3)][1:]
chunks = [D.chunks(0), D.chunks(1)]
got, step = [[], []], 0
for k in range(len(chunks[0])):
    eng.push(use, np.stack([c[k] for c in chunks]))
    if eng.step(use):
        for i, t in enumerate(eng.fetch_many(use, 64)):
            got[i].append(t)
        step += 1
        if step == 3:
            eng.reset(use[1], 7)
eng.close()
print("RESULT" + json.dumps(got))
''' % (ROOT, os.path.join(ROOT, "tests"), key)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, LASR_BOS_CACHE="0"))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(line[0][6:])
    mod = D.model(*key)
    for i, ref in enumerate((D.stream(mod, 2, 0), D.stream(mod, 2, 1, 3))):
        assert got[i] == [s[0] for s in ref.steps], i


# ------------------------------------------------------------------------------- 3. lookahead
def test_lookahead_is_invisible_at_the_cap(monkeypatch):
    """cap 2 inside a lookahead window of 2 or 4 frames: the CPU conditions guarantee capped frames that are not the first of
    their window.  The same tokens, frames, log p, log-p sum and alignment score (sum_iters, n_ones) whatever the window."""
    key = D.MODELS[0]
    mod = D.model(*key)
    seen = {}
    for la in (1, 2, 4):
        monkeypatch.setenv("LASR_LOOKAHEAD", str(la))
        eng = make(mod, off=2, st=2)
        try:
            assert eng.config("la_offline") == la
            eng.set_alignments(True)
            check_offline(eng, mod, 2, (key, "lookahead", la))
            check_stream(eng, mod, 2, [0, 1], "sync", (key, "lookahead", la), reset={1: 3})
            check_stream(eng, mod, 2, [0, 1], "pipelined", (key, "lookahead", la))
            slots = [eng.open(), eng.open()]
            eng.transcribe_pcm(slots, D.utterances())
            seen[la] = [(tok, fr.tobytes(), lp.tobytes(), nl, al) for tok, fr, lp, nl, al in (eng.fetch_aligned(s) for s in slots)]
        finally:
            eng.close()
    assert seen[1] == seen[2] == seen[4]                   # bit for bit, not only within the bounds


# ------------------------------------------------------------------------------- 4. lattice
LAT_MODELS = [D.MODELS[5], D.MODELS[0]]                   # V = 4096 (wide logits tiling), V = 4112; blank 300
LAT_SLOTS = [5, 0]
_LAT = {}


def lat_reference(key, kind):
    """per utterance (y, b, e, loglik, viterbi, frames) from the float64 reference, computed once"""
    if (key, kind) not in _LAT:
        mod = D.model(*key)
        ys = [r.tokens for r in D.offline(mod, 3)] if kind == "greedy" else [D.rand_labels(mod, 40, 40 + i) for i in range(2)]
        if kind == "rand40":
            ys[0][7] = 0                                   # id 0 is a token here
        out = []
        for f, y in zip(D.feats_all(), ys):
            b, e = R.lattice(mod.m, f, y)
            out.append((y, b, e, R.forward(b, e, len(y)), *R.viterbi(b, e, len(y))))
        _LAT[key, kind] = out
    return _LAT[key, kind]


@pytest.mark.parametrize("key", LAT_MODELS, ids=[IDS[5], IDS[0]])
def test_lattice_terms_and_scores(key):
    import lattice_band_ref as B
    mod, eng = D.model(*key), engine(key)
    f = D.feats_all()
    for kind in ("greedy", "rand40"):
        ref = lat_reference(key, kind)
        ys = [r[0] for r in ref]
        assert all(mod.blank not in y for y in ys) and (kind == "greedy" or 0 in ys[0])
        res = eng.align_feats(LAT_SLOTS, f, ys, lattice=True)
        for i in range(2):
            check_against(res[i], ref[i], f"{key} {kind} utterance {i}")
        if kind == "rand40":
            # 2 x 37 x 41 rows: more than one block of the logits GEMM (the wide tiling needs >= 512 rows and V % 64 == 0)
            assert sum(r[1].size for r in ref) > eng.config("lat_R") >= 512
            pcm = eng.align_pcm(LAT_SLOTS, D.utterances(), ys, lattice=True)
            for i in range(2):                         # (the GPU front-end's features: the same bounds, not the same bits)
                check_against(pcm[i], ref[i], f"{key} {kind} pcm utterance {i}")
        # posteriors: every field of the plain call bit for bit; the occupancies against the float64 forward-backward with the
        # bound of test_gpu_lattice_post.check_model; the per-token fields follow from the occupancies
        post = eng.align_feats(LAT_SLOTS, f, ys, lattice=True, posteriors=True)
        for i, (p, q) in enumerate(zip(post, res)):
            for k in q:
                assert np.asarray(q[k]).tobytes() == np.asarray(p[k]).tobytes(), (key, kind, i, k)
            T, U = ref[i][1].shape[0], len(ys[i])
            sum_invariants(p, U)
            pr = P.posteriors(ref[i][1], ref[i][2], U)
            for k_gpu, k_ref in (("occ_blank", "occ_b"), ("occ_emit", "occ_e")):
                m = pr[k_ref] >= 1e-3
                d = float(np.abs(np.log(p[k_gpu][m].astype(np.float64)) - np.log(pr[k_ref][m])).max())
                assert d <= 2 * (T + U) * TERM_TOL, (key, kind, i, k_gpu, d)
            oe = p["occ_emit"].astype(np.float64)
            assert [int(t) for t in p["tok_peak_frame"]] == [int(t) for t in oe[:, :U].argmax(0)], (key, kind, i)
            assert np.array_equal(np.asarray(p["tok_peak"], np.float32), p["occ_emit"][:, :U].max(0)), (key, kind, i)
            # a float32 sum of T terms t * occ, each at most T - 1: within T * T * 2^-23 of the float64 sum, far below 1e-3
            assert float(np.abs(p["tok_mean"] - (np.arange(T)[:, None] * oe[:, :U]).sum(0)).max()) <= 1e-3, (key, kind, i)
            assert np.all(p["tok_var"] >= 0)
        # scoring through the prefix tree (k_lat_pick_tree): both transcripts as candidates of each utterance
        sc = eng.score_feats([[1, 2], [3, 4]], f, [ys, ys])
        for i in range(2):
            T = ref[i][1].shape[0]
            assert abs(sc[i]["loglik"][i] - ref[i][3]) <= (T + len(ys[i])) * TERM_TOL, (key, kind, i)
            b, e = R.lattice(mod.m, f[i], ys[1 - i])
            assert abs(sc[i]["loglik"][1 - i] - R.forward(b, e, len(ys[1 - i]))) <= (T + len(ys[1 - i])) * TERM_TOL, (key, kind, i)
        # a band (k_lat_pick_band): the terms inside the windows are the full lattice's
        band = eng.align_feats(LAT_SLOTS, f, ys, lattice=True, band=6, max_passes=1)
        for i, r in enumerate(band):
            lo, w, U = [int(v) for v in r["lo"]], int(r["width"]), len(ys[i])
            bb, eb = B.cut(ref[i][1], lo, w), B.cut(ref[i][2], lo, w)
            at_U = np.array([[lo[t] + k >= U for k in range(w)] for t in range(len(lo))])
            assert float(np.abs(r["blank_lp"].astype(np.float64) - bb).max()) <= TERM_TOL, (key, kind, i)
            assert float(np.abs(r["emit_lp"].astype(np.float64) - eb)[~at_U].max()) <= TERM_TOL, (key, kind, i)
            ll = B.forward(bb, eb, lo, U)
            if ll > -np.inf:
                assert abs(r["loglik"] - ll) <= (len(lo) + U) * TERM_TOL, (key, kind, i)
            else:
                assert r["loglik"] == -np.inf
    # a transcript with the blank in it is refused, one with id 0 was accepted above
    y0 = list(lat_reference(key, "greedy")[0][0])
    with pytest.raises(N.LasrError) as ei:
        eng.align_feats([5], [f[0]], [y0[:2] + [mod.blank] + y0[2:]])
    assert ei.value.code == N.LASR_EINVAL
    with pytest.raises(N.LasrError) as ei:
        eng.score_feats([[1, 2]], [f[0]], [[y0, [mod.blank]]])
    assert ei.value.code == N.LASR_EINVAL
    assert eng.align_feats([5], [f[0]], [[0] + y0])[0]["loglik"] < 0


@pytest.mark.parametrize("key", LAT_MODELS, ids=[IDS[5], IDS[0]])
def test_lattice_terms_are_the_decode_records(key):
    """test_gpu_lattice.test_terms_against_the_decode_records where a virtual thread of k_lat_pick holds up to 17 terms: the emit term
    of greedy's k-th token on its frame is the decode path's log p of that decision, bit for bit -- k_lat_pick's stride loops
    reproduce k_select's sum, and at these shapes both paths' logits come out of the same dot products."""
    mod = D.model(*key)
    eng = make(mod, off=3)
    try:
        eng.set_alignments(True)
        slots = [eng.open() for _ in range(6)]
        use = [slots[5], slots[0]]
        eng.transcribe_pcm(use, D.utterances())
        recs = [eng.fetch_aligned(s)[:3] for s in use]
        eng.set_alignments(False)
        res = eng.align_pcm(use, D.utterances(), [r[0] for r in recs], lattice=True)
    finally:
        eng.close()
    n = worst = 0
    for (tok, fr, lp), r in zip(recs, res):
        for k in range(len(tok)):
            worst = max(worst, abs(float(r["emit_lp"][fr[k], k]) - float(lp[k])))
            n += 1
    print(f"{key}: {n} decode records against the lattice: max |d| {worst:.3g}")
    assert n >= 30 and worst == 0.0


# ------------------------------------------------------------------------------- 5. LM fusion
@pytest.mark.parametrize("int8", [False, True], ids=["fp32", "int8"])
def test_lm_fusion_masks_entry_zero_not_the_blank(int8):
    """LMFuser writes MIN_VAL to entry 0 of both standardised vectors (lm.py:59-79) whatever the blank id is: with blank = 300 token 0
    can never be the fused pick, and neither can the blank (the re-pick only runs behind a non-blank decision)"""
    mod = D.model(*D.LM_MODEL)
    runs, picks = D.lm_offline(int8)
    plain = D.offline(mod, 3)
    assert sum(1 for r, q in zip(runs, plain) for a, b in zip(r.tokens, q.tokens) if a != b) >= 3      # the re-pick runs
    eng = make(mod, off=3, st=3)
    try:
        eng.attach_lm(D.lm_state_dict(), int8=int8)
        eng.set_alignments(True)
        slots = [eng.open() for _ in range(3)]
        use = [slots[2], slots[0]]
        eng.transcribe_pcm(use, D.utterances())
        for i, (s, r) in enumerate(zip(use, runs)):
            tok, fr, lp, _, _ = eng.fetch_aligned(s)
            assert 0 not in tok and mod.blank not in tok
            check_records((tok, fr, lp), (r.tokens, r.frames, r.logps), ("lm offline", int8, i))
        for s in slots:
            eng.close_slot(s)
        # synchronous streaming through the GPU front-end against the oracle's stream decoder with its own LMFuser
        sruns, spicks = D.lm_stream(int8)
        assert sum(1 for ps in spicks for a, b, _ in ps if a != b) >= 3
        slots = [eng.open() for _ in range(3)]
        use = [slots[2], slots[0]]
        chunks = [D.chunks(row) for row in range(2)]
        step = 0
        for k in range(len(chunks[0])):
            eng.push(use, np.stack([c[k] for c in chunks]))
            if eng.step(use):
                for i, got in enumerate(eng.fetch_many_aligned(use, 64)):
                    assert 0 not in got[0] and mod.blank not in got[0]
                    check_records(got, sruns[i].steps[step], ("lm stream", int8, "step", step, "row", i))
                step += 1
        assert step == len(sruns[0].steps)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 7. contract
def test_vocabulary_limits():
    import ctypes as C
    mod = D.model(*D.MODELS[3])                           # V = 2064
    with pytest.raises(ValueError):                       # the Python side asks lasr_weight_count first
        make(mod, beam=2)
    ok = make(mod)                                        # ... and lasr_create itself refuses the same description with beam = 2
    try:
        d = N.ModelDesc.from_buffer_copy(ok.desc)
        d.beam = 2
        blob = np.zeros(16, np.float32)
        ctx = C.c_void_p()
        rc = ok.lib.lasr_create(0, C.byref(d), blob.ctypes.data_as(C.c_void_p), blob.size, None, C.byref(ctx))
        if ctx:
            ok.lib.lasr_destroy(ctx)
        assert rc == N.LASR_EINVAL
        d.beam, d.vocab = 2, 2048                         # the limit itself is a valid description
        assert ok.lib.lasr_weight_count(C.byref(d)) > 0
    finally:
        ok.close()
    mod = D.model(*D.MODELS[0])                           # V = 4112
    eng = make(mod, off=2)
    try:
        lm = dict(D.LM_CFG, vocab=4112)
        from libreasr_amd import synth
        with pytest.raises(N.LasrError) as ei:
            eng.attach_lm(synth.synth_lm_state_dict(lm))
        assert ei.value.code == N.LASR_EINVAL
        eng.set_alignments(True)
        check_offline(eng, mod, 2, "after the refused LM")           # the context stays usable
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 6. beam
@pytest.mark.parametrize("W", D.BEAM_WIDTHS)
def test_beam_whole_nbest_with_ties(W):
    """blank 7, cap 2, tie groups in the beam's layout: the whole N-best against the oracle's beam rank by rank.  Hypotheses whose
    scores are bit-equal (two members of a group, emitted in a frame's last round) rank by slot, i.e. in ascending token order."""
    from test_gpu_beam_records import check_rank, check_structure
    mod = D.beam_model(W, "offline")
    ref = D.beam_offline(W)
    eng = make(mod, off=D.BEAM_CAP, st=D.BEAM_CAP, beam=W)
    try:
        eng.set_beam_records(True)
        slots = [eng.open() for _ in range(4)]
        use = [slots[3], slots[1]]
        eng.transcribe_pcm(use, D.utterances())
        for i, s in enumerate(use):
            got = eng.fetch_nbest(s)
            what = ("beam", W, "utt", i)
            check_structure(got, ref[i]["T"], W, D.BEAM_CAP, what)
            assert len(got) == len(ref[i]["beam"]) == W, what
            for k in range(W):
                check_rank(got[k], ref[i]["beam"][k], what + (k,))
                assert mod.blank not in got[k][0]
    finally:
        eng.close()
    # both utterances as pipelined streams (submit / wait, k_beam_select_rw fed step by step, `inb = round >= max_iters` across
    # model steps): the whole beam after every model step against the oracle's stream decode (the model of that run)
    mod = D.beam_model(W, "streams")
    sref = D.beam_stream(W)
    eng = make(mod, off=D.BEAM_CAP, st=D.BEAM_CAP, beam=W)
    try:
        eng.set_beam_records(True)
        slots = [eng.open() for _ in range(4)]
        use = [slots[3], slots[1]]
        chunks = [D.chunks(row) for row in range(2)]
        done = [0]

        def collect():
            j = done[0]
            for i, s in enumerate(use):
                got = eng.fetch_nbest(s)
                what = ("beam", W, "pipelined stream", i, "step", j)
                check_structure(got, sref[i]["T"][j], W, D.BEAM_CAP, what)
                assert len(got) == len(sref[i]["steps"][j]), what
                for k in range(len(got)):
                    check_rank(got[k], sref[i]["steps"][j][k], what + (k,))
                    assert mod.blank not in got[k][0]
            done[0] += 1

        for k in range(len(chunks[0])):
            eng.push_submit(use, np.stack([c[k] for c in chunks]))
            if eng.pending() >= 3:
                assert eng.wait() == 2
                collect()
        while eng.pending():
            assert eng.wait() == 2
            collect()
        assert done[0] == len(sref[0]["steps"]) >= 10
    finally:
        eng.close()
