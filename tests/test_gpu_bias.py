"""Contextual biasing (hotwords) on the GPU: lasr_set_bias / lasr_bias_state / lasr_bias_pick and k_select<.., BIAS = true>.

Expected values: the restatements of bias_ref.py (pinned to the numpy oracle in test_bias_cpu.py, which also asserts the input
conditions of the parity tests below -- every compared decision has a margin >= 1e-3 in the restatement, so nothing is skipped
or truncated here).  Tokens, frames and nodes must be equal; log p within 1e-3 (LOGP_TOL, the project's fp32 bound); neg_logp
within 2e-3 * max(1, |neg_logp|), the bound test_gpu_beam_records.py uses for sums of such terms.

The issue asks for V = 4100 in the op-level test; lasr_create refuses a vocabulary that is no multiple of 16, so the test runs
at 4112, the smallest valid vocabulary past both KEEP ranges (8 x 256, 16 x 256) that is still no multiple of 256."""
import numpy as np
import pytest

import bias_ref as B
from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O
from test_alignment_cpu import oracle, utterances
from test_gpu_alignment import LOGP_TOL, check_structure

pytestmark = pytest.mark.gpu

BLANK = 0
PCM = synth.synth_pcm(1, 48000, seed=1234)[0]
CHUNKS = synth.stream_chunks(PCM, 1280, lead=1, tail=10)


def make(name="tiny", vocab=None, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    cfg = synth.model_cfg(name)
    if vocab is not None:
        cfg["vocab"] = vocab
    sd = synth.synth_state_dict(cfg, seed=0)
    return Engine(sd, cfg, max_streams=8, **kw)


def native(g):
    """a bias_ref.Graph in lasr_set_bias' layout"""
    from libreasr_amd.engine import BiasGraph
    return BiasGraph(g.off, g.tok, g.nxt, g.bonus, g.depth)


def feats_all():
    return [O.features_offline(p) for p in utterances()]


def records(run):
    """(tokens, frames, lps) of the emissions of a bias_ref.decode_greedy run"""
    em = [d for d in run[4] if d[0] != BLANK]
    return [d[0] for d in em], [d[1] for d in em], [d[2] for d in em]


def check_records(got, want, what):
    tok, fr, lp = got
    wt, wf, wl = want
    assert list(tok) == list(wt), (what, "tokens", list(tok), list(wt))
    assert list(fr) == list(wf), (what, "frames", list(fr), list(wf))
    assert np.asarray(lp).dtype == np.float32 and len(lp) == len(wl)
    if len(wl):
        err = float(np.abs(np.asarray(lp, np.float64) - np.asarray(wl, np.float64)).max())
        print(what, "max log p error", err)
        assert err < LOGP_TOL, (what, "log p", err)


def bits(lp):
    return np.asarray(lp, np.float32).view(np.int32).tolist()


def run_offline(eng, slots):
    """-> per slot (tokens, frames, lp bits, neg_logp) of test_alignment_cpu.utterances() (records on)"""
    eng.transcribe_pcm(slots, utterances())
    out = []
    for s in slots:
        tok, fr, lp, neg, _ = eng.fetch_aligned(s)
        out.append((list(tok), list(fr), bits(lp), float(neg)))
    return out


def run_stream(eng, slot, mode):
    """the 3.0 s stream on `slot` (records on): per model step (tokens, frames, lp float32).  mode "sync": lasr_step_stream;
    "pipelined": lasr_push_submit / lasr_step_wait with up to 5 steps in flight."""
    steps = []
    if mode == "sync":
        for ch in CHUNKS:
            eng.push([slot], ch[None])
            if eng.step([slot]):
                tok, fr, lp, _, _ = eng.fetch_aligned(slot)
                steps.append((list(tok), list(fr), np.asarray(lp, np.float32)))
        return steps
    depth = 0

    def collect():
        if eng.wait():
            tok, fr, lp = eng.fetch_many_aligned([slot], 256)[0]
            steps.append((list(tok), list(fr), np.asarray(lp, np.float32)))

    for ch in CHUNKS:
        eng.push_submit([slot], ch[None])
        depth = max(depth, eng.pending())
        if eng.pending() >= 5:
            collect()
    while eng.pending():
        collect()
    assert depth >= 5                                       # several steps were in flight
    return steps


def same_steps(a, b, what):
    assert len(a) == len(b), what
    for j, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0] and x[1] == y[1] and bits(x[2]) == bits(y[2]), (what, "step", j, x, y)


# ------------------------------------------------------------------------------- 1. op-level, exact
A_, B_, C_, D_ = 5, 9, 7, 3


def base_row(V):
    return (-20.0 - 0.5 * (np.arange(V) % 7)).astype(np.float32)


def pick_case(eng, g, rows, loose=()):
    """rows: (node, {token: logit}) on top of base_row; expected values from bias_ref.pick.  loose: rows with non-finite logits
    -- ranges only"""
    import torch
    V = eng.desc.vocab
    z = np.stack([base_row(V) for _ in rows])
    for r, (_, put) in enumerate(rows):
        for t, val in put.items():
            z[r, t] = val
    nodes = [v for v, _ in rows]
    tok, nxt, lp = eng.bias_pick(torch.as_tensor(z).to(eng.device), nodes)
    for r, v in enumerate(nodes):
        assert 0 <= tok[r] < V and 0 <= nxt[r] < g.n_nodes, (r, tok[r], nxt[r])
        if r in loose:
            continue
        wt, wn, margin = B.pick(z[r], g, v, BLANK)
        assert margin >= 0.5 or margin == 0.0, (r, margin)           # a clear gap, or an exact tie that the index decides
        assert (int(tok[r]), int(nxt[r])) == (wt, wn), (r, int(tok[r]), int(nxt[r]), wt, wn)
        assert abs(float(lp[r]) - B.pick_logp(z[r], wt)) < 1e-3, (r, float(lp[r]), B.pick_logp(z[r], wt))
    return tok, nxt, lp


@pytest.mark.parametrize("V", [64, 320, 4112])
def test_bias_pick_is_exact(V):
    eng = make(vocab=V)
    try:
        E_ = V - 1                                           # the last token: past the registers' range at V = 4112
        phrases, weights = [[A_, A_, B_], [C_], [D_, E_]], [2.0, 0.0, 1.5]
        g = B.automaton(phrases, weights)
        idx = {p: i for i, p in enumerate(g.paths)}
        cg = eng.bias_compile(phrases, weights)
        assert cg.edge_off.tolist() == g.off.tolist() and cg.edge_tok.tolist() == g.tok.tolist() and cg.edge_next.tolist() == g.nxt.tolist()
        assert cg.edge_bonus.tobytes() == g.bonus.tobytes()
        eng.set_bias(cg)
        rows = [
            (0, {BLANK: 1.0, A_: 0.0}),                      # an edge token wins over blank (0 + 2 > 1)
            (0, {BLANK: 1.0, A_: -1.5}),                     # an edge token loses (-1.5 + 2 < 1)
            (0, {A_: 3.0, BLANK: 1.0}),                      # arg itself is listed
            (0, {D_: 0.5, 20: 2.0}),                         # exact tie, the edge has the lower id: the edge wins
            (0, {1: 2.0, A_: 0.0}),                          # exact tie, arg has the lower id: arg wins, unlisted -> root
            (idx[(A_, A_)], {A_: 1.0}),                      # failure transition: a a . a stays in a a
            (0, {BLANK: 1.0, C_: 0.5}),                      # a bonus of 0 changes nothing
            (idx[(D_,)], {BLANK: 1.0, E_: 0.0}),             # the last token of the vocabulary as an edge
        ]
        tok, nxt, _ = pick_case(eng, g, rows)
        assert tok.tolist() == [A_, BLANK, A_, D_, 1, A_, BLANK, E_]
        assert nxt.tolist() == [idx[(A_,)], 0, idx[(A_,)], idx[(D_,)], 0, idx[(A_, A_)], 0, idx[(D_, E_)]]
        # one row of NaN and one of +-inf logits among finite rows: ranges for those, the others exact
        rows = [
            (0, {C_: 1.5, BLANK: 1.0}),                      # arg listed with bonus 0: taken, and the row moves
            (idx[(A_,)], {A_: float("nan"), 11: float("nan"), BLANK: 1.0}),
            (0, {BLANK: 1.0, A_: 0.0}),
            (idx[(A_, A_)], {B_: float("inf"), 2: float("inf"), A_: float("-inf")}),
            (idx[(A_, A_)], {BLANK: 1.0, B_: -0.25}),        # a a . b completes the phrase
        ]
        tok, nxt, _ = pick_case(eng, g, rows, loose=(1, 3))
        assert (tok[0], nxt[0]) == (C_, idx[(C_,)]) and (tok[4], nxt[4]) == (B_, idx[(A_, A_, B_)])
        # a node without edges: only a hand-made graph has one (every node of a compiled automaton lists the root's edges)
        hand = B.Graph([0, 1, 1], [A_], [1], [1.0], [0, 1])
        eng.set_bias(native(hand))
        tok, nxt, _ = pick_case(eng, hand, [(1, {BLANK: 1.0, A_: 0.5}), (1, {A_: 1.0, BLANK: 0.0}), (0, {BLANK: 1.0, A_: 0.5})])
        assert tok.tolist() == [BLANK, A_, A_] and nxt.tolist() == [1, 0, 1]
        if V == 320:
            # a root with 300 one-token phrases: a degree above the workgroup size, winners on either side of edge 256
            w = np.full(300, 1.0, np.float32)
            w[286] = 3.0                                     # token 287
            phrases = [[t] for t in range(1, 301)]
            wide = B.Graph(np.arange(302) * 300, np.tile(np.arange(1, 301), 301), np.tile(np.arange(1, 301), 301), np.tile(w, 301),
                           [0] + [1] * 300)
            cg = eng.bias_compile(phrases, w.tolist())
            assert cg.edge_off.tolist() == wide.off.tolist() and cg.edge_tok.tolist() == wide.tok.tolist()
            assert cg.edge_next.tolist() == wide.nxt.tolist() and cg.edge_bonus.tobytes() == wide.bonus.tobytes()
            eng.set_bias(cg)
            tok, nxt, _ = pick_case(eng, wide, [(0, {BLANK: 1.0, 287: -1.0}), (5, {BLANK: 1.0, 17: 0.5}), (299, {BLANK: 1.0, 287: -2.5}),
                                                (0, {BLANK: 1.0, 310: 0.5}), (0, {310: 2.0, BLANK: 1.0})])
            assert tok.tolist() == [287, 17, BLANK, BLANK, 310] and nxt.tolist() == [287, 17, 299, 0, 0]
        # the op-level calls touched no slot: one opened now is at the root
        s = eng.open()
        assert eng.bias_state([s]).tolist() == [0]
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 2. offline parity
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_offline_parity_with_the_restatement(name):
    eng = make(name)
    try:
        g, runs = B.offline_ref(name, oracle(name), feats_all())
        eng.set_alignments(True)
        eng.set_bias(eng.bias_compile(*B.OFFLINE_CASES[name]))
        slots = [eng.open() for _ in range(6)]
        use = [slots[4], slots[0], slots[2]]                 # non-contiguous rows
        eng.transcribe_pcm(use, utterances())
        nodes = eng.bias_state(use)
        for i, s in enumerate(use):
            tok, fr, lp, neg, _ = eng.fetch_aligned(s)
            check_records((tok, fr, lp), records(runs[i]), (name, i))
            want = runs[i][1]
            print(name, i, "neg_logp", neg, want)
            assert abs(neg - want) <= 2e-3 * max(1.0, abs(want)), (name, i, neg, want)
            assert int(nodes[i]) == runs[i][5], (name, i, int(nodes[i]), runs[i][5])
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 3. streaming, both protocols
def test_streaming_parity_on_both_protocols():
    eng = make()
    try:
        g, ref = B.stream_ref(oracle("tiny"), PCM)
        eng.set_alignments(True)
        eng.set_bias(eng.bias_compile(*B.STREAM_CASE))
        n_buffer = eng.desc.n_buffer
        got = {}
        for mode in ("sync", "pipelined"):
            slot = eng.open()
            got[mode] = run_stream(eng, slot, mode)
            assert len(got[mode]) == len(ref["steps"]) == 23 and ref["speech"] == 19
            for j, st in enumerate(got[mode]):
                if j < ref["speech"]:
                    check_records(st, ref["steps"][j], (mode, "step", j))
                check_structure(st, j * n_buffer, (j + 1) * n_buffer, (mode, "step", j))      # the silent tail: structure only
            assert eng.bias_state([slot]).tolist() == [ref["nodes"][-1]]
            eng.close_slot(slot)
        same_steps(got["sync"], got["pipelined"], "sync vs pipelined")                        # every step, tail included
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 4. state rules
def test_node_state_rules():
    eng = make()
    try:
        R = B.STREAM_RESET_AT
        m = oracle("tiny")
        g, ref = B.stream_ref(m, PCM)
        _, ref_reset = B.stream_ref(m, PCM, reset_at=R)
        deep = ref["nodes"][R - 1]
        assert deep != 0
        graph = eng.bias_compile(*B.STREAM_CASE)
        eng.set_alignments(True)
        eng.set_bias(graph)
        # reset bits 1 | 2 before model step R: the node is 0 and the stream goes on as the restatement does after reset()
        s = eng.open()
        steps = []
        for ch in CHUNKS:
            eng.push([s], ch[None])
            if not eng.step([s]):
                continue
            tok, fr, lp, _, _ = eng.fetch_aligned(s)
            steps.append((list(tok), list(fr), np.asarray(lp, np.float32)))
            if len(steps) == R:
                assert int(eng.bias_state([s])[0]) == deep
                eng.reset(s, 3)
                assert int(eng.bias_state([s])[0]) == 0
        for j in range(ref_reset["speech"]):
            check_records(steps[j], ref_reset["steps"][j], ("reset stream step", j))
        assert eng.bias_state([s]).tolist() == [ref_reset["nodes"][-1]]
        eng.close_slot(s)

        def go_deep():
            slot, n = eng.open(), 0
            for ch in CHUNKS:
                eng.push([slot], ch[None])
                if eng.step([slot]):
                    eng.fetch_aligned(slot)
                    n += 1
                    if n == R:
                        break
            assert int(eng.bias_state([slot])[0]) == deep
            return slot

        # bits 1, 4 and 8 alone leave the node; lasr_set_bias zeroes every slot's
        s2 = go_deep()
        for what in (1, 4, 8, 1 | 4 | 8):
            eng.reset(s2, what)
            assert int(eng.bias_state([s2])[0]) == deep, what
        other = eng.open()
        eng.set_bias(graph)
        assert eng.bias_state([s2, other]).tolist() == [0, 0]
        eng.close_slot(s2)
        eng.close_slot(other)
        # lasr_transcribe_* starts from the root on a slot that was left in a deep node: the same as on a fresh slot
        s3 = go_deep()
        fresh = eng.open()
        utt = utterances()[0]
        eng.transcribe_pcm([s3, fresh], [utt, utt])
        n3, nf = eng.bias_state([s3, fresh]).tolist()
        a, b = eng.fetch_aligned(s3), eng.fetch_aligned(fresh)
        assert list(a[0]) == list(b[0]) and list(a[1]) == list(b[1]) and bits(a[2]) == bits(b[2]) and a[3] == b[3] and n3 == nf
        # ... and as the restatement decodes that utterance from the root (tokens; its margins are not part of the searched set)
        want = B.decode_greedy(m, O.features_offline(utt), g, 3)
        if min(d[4] for d in want[4]) >= B.MARGIN:
            assert list(a[0]) == want[0] and n3 == want[5]
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 5. / 6. off is off, zero bonuses are no bonuses
def all_paths(eng):
    """offline, synchronous and pipelined results of one context, records on: what tests 5 and 6 compare bit for bit"""
    slots = [eng.open() for _ in range(3)]
    out = {"offline": run_offline(eng, slots)}
    for s in slots:
        eng.close_slot(s)
    for mode in ("sync", "pipelined"):
        s = eng.open()
        steps = run_stream(eng, s, mode)
        out[mode] = [(t, f, bits(lp)) for t, f, lp in steps]
        out[mode + " neg_logp"] = float(eng.fetch(s)[1])
        eng.close_slot(s)
    return out


_TWIN = {}


def twin(dtype):
    """what a context that never sets a graph produces (computed once per operand type)"""
    if dtype not in _TWIN:
        eng = make(dtype=dtype)
        try:
            eng.set_alignments(True)
            _TWIN[dtype] = all_paths(eng)
        finally:
            eng.close()
    return _TWIN[dtype]


def test_off_is_off_after_clearing():
    eng = make()
    try:
        eng.set_alignments(True)
        eng.set_bias(eng.bias_compile(*B.STREAM_CASE))
        biased = all_paths(eng)
        assert biased["sync"] != twin("f32")["sync"]                  # the graph did change the decode ...
        eng.set_bias(None)
        with pytest.raises(N.LasrError) as e:
            eng.bias_state([0])
        assert e.value.code == N.LASR_ESTATE
        assert all_paths(eng) == twin("f32")                          # ... and from the clear onwards nothing is left of it
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_bonus_graph_is_bit_identical(dtype):
    eng = make(dtype=dtype)
    try:
        m = oracle("tiny")
        g = B.automaton(*B.STREAM_CASE).zeroed()
        eng.set_alignments(True)
        eng.set_bias(native(g))
        assert all_paths(eng) == twin(dtype)                           # BIAS = true against BIAS = false, bit for bit
        if dtype == "f32":
            # the state walks the automaton: nodes as in the restatement (offline final nodes; per synchronous step while the
            # stream still sees audio)
            slots = [eng.open() for _ in range(3)]
            eng.transcribe_pcm(slots, utterances())
            want = [B.decode_greedy(m, f, g, 3)[5] for f in feats_all()]
            assert eng.bias_state(slots).tolist() == want
            for s in slots:
                eng.fetch_aligned(s)
                eng.close_slot(s)
            _, ref = B.stream_ref(m, PCM, zero=True)
            s, n = eng.open(), 0
            for ch in CHUNKS:
                eng.push([s], ch[None])
                if eng.step([s]):
                    eng.fetch_aligned(s)
                    if n < ref["speech"]:
                        assert int(eng.bias_state([s])[0]) == ref["nodes"][n], n
                    n += 1
        # a graph whose phrases the decode does walk (zero bonuses): the transcript's own tokens as phrases
        toks = twin(dtype)["offline"][0][0]
        if len(toks) >= 3:
            own = B.automaton([toks[:3], toks[1:4]], [0.0, 0.0])
            eng2 = make(dtype=dtype)
            try:
                eng2.set_alignments(True)
                eng2.set_bias(native(own))
                slots = [eng2.open() for _ in range(3)]
                assert run_offline(eng2, slots) == twin(dtype)["offline"]
                v = 0
                for t in toks:
                    tk, nx, _ = own.edges(v)
                    hit = np.nonzero(tk == t)[0]
                    v = int(nx[hit[0]]) if len(hit) else 0
                assert int(eng2.bias_state([slots[0]])[0]) == v
            finally:
                eng2.close()
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing():
    def code(fn, *a, **kw):
        with pytest.raises(N.LasrError) as e:
            fn(*a, **kw)
        return e.value.code

    good = B.automaton(*B.STREAM_CASE)
    beam = make(beam=4)
    try:
        assert code(beam.set_bias, native(good)) == N.LASR_EINVAL
    finally:
        beam.close()
    for int8 in (False, True):
        eng = make()
        try:
            lsd = synth.synth_lm_state_dict("tiny_lm")
            eng.set_bias(native(good))
            assert code(eng.attach_lm, lsd, int8=int8) == N.LASR_ESTATE        # a graph is set: no LM
            assert eng.lm_cfg is None
            eng.set_bias(None)
            eng.attach_lm(lsd, int8=int8)
            assert code(eng.set_bias, native(good)) == N.LASR_ESTATE            # an LM is attached: no graph
        finally:
            eng.close()
    eng = make()
    try:
        eng.set_alignments(True)
        s = eng.open()
        for ch in CHUNKS[:8]:
            eng.push_submit([s], ch[None])
        assert eng.pending() > 0
        assert code(eng.set_bias, native(good)) == N.LASR_ESTATE                # a step in flight
        while eng.pending():
            eng.wait()
        eng.fetch_many_aligned([s], 256)
        eng.close_slot(s)
        V = eng.desc.vocab

        def variant(**kw):
            a = dict(off=good.off.copy(), tok=good.tok.copy(), nxt=good.nxt.copy(), bonus=good.bonus.copy())
            for k, (i, v) in kw.items():
                a[k][i] = v
            return B.Graph(a["off"], a["tok"], a["nxt"], a["bonus"], good.depth)

        e0 = int(good.off[1])                                                     # edges of the root: [0, e0), e0 >= 2
        assert e0 >= 2
        bad = {
            "edge_off[0] != 0": variant(off=(0, 1)),
            "offsets decrease": variant(off=(1, int(good.off[2]) + 1)),
            "tokens not ascending": variant(tok=(1, int(good.tok[0]))),
            "token >= vocab": variant(tok=(e0 - 1, V)),
            "token < 0": variant(tok=(0, -1)),
            "blank listed": variant(tok=(0, BLANK)),
            "next = 0": variant(nxt=(0, 0)),
            "next >= n_nodes": variant(nxt=(0, good.n_nodes)),
            "negative bonus": variant(bonus=(0, -1.0)),
            "infinite bonus": variant(bonus=(0, np.inf)),
            "nan bonus": variant(bonus=(0, np.nan)),
        }
        for what, g in bad.items():
            assert code(eng.set_bias, native(g)) == N.LASR_EINVAL, what
        from libreasr_amd.engine import BiasGraph
        big = BiasGraph(np.zeros(65538, np.int32), [], [], [])
        assert big.n_nodes == 65537 and code(eng.set_bias, big) == N.LASR_EINVAL
        from libreasr_amd.engine import BeamBiasGraph
        with pytest.raises(ValueError):                                           # a graph of the beam form: it carries node_back
            eng.set_bias(BeamBiasGraph(good.off, good.tok, good.nxt, good.bonus, np.zeros(good.n_nodes, np.float32), good.depth))
        # nothing changed: biasing is still off, and the context decodes as its twin
        assert code(eng.bias_state, [0]) == N.LASR_ESTATE
        assert all_paths(eng) == twin("f32")
        # ... and with a graph set, a refused graph leaves the set one in place
        eng.set_bias(native(good))
        s = eng.open()
        for what, g in bad.items():
            assert code(eng.set_bias, native(g)) == N.LASR_EINVAL, what
        assert eng.bias_state([s]).tolist() == [0]
        _, ref = B.stream_ref(oracle("tiny"), PCM)
        steps = run_stream(eng, s, "sync")
        for j in range(ref["speech"]):
            check_records(steps[j], ref["steps"][j], ("after refusals, step", j))
    finally:
        eng.close()
