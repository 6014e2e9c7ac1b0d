"""Contextual biasing in beam search on the GPU (lasr_set_beam_bias) against the restatement of beam_bias_ref.py:
the op-level round exact on crafted logits; offline, synchronous and pipelined parity on the committed cases (whose input
conditions test_beam_bias_cpu.py asserts on the restatement alone); merging and records with a graph; the state rules; a
zero-gain graph, a cleared graph and every refusal against a twin context that never heard of a graph."""
import numpy as np
import pytest

import beam_bias_ref as BB
import beam_merge_ref as BM
import beam_records_ref as R
from libreasr_amd import _native as N
from libreasr_amd import synth

pytestmark = pytest.mark.gpu

BLANK = 0
LOGP_TOL = 1e-3                      # test_gpu_beam_records.py's bounds
F32 = np.float32


def score_ok(got, want):
    return abs(got - want) < 2e-3 * max(1.0, abs(want))


def make(name="tiny", W=4, vocab=None, records=True, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    cfg = synth.model_cfg(name)
    if vocab is not None:
        cfg["vocab"] = vocab
    sd = synth.synth_state_dict(cfg, seed=0)
    eng = Engine(sd, cfg, max_streams=8, beam=W, **kw)
    if records:
        eng.set_beam_records(True)
    return eng


def native(g):
    """a beam_bias_ref.Graph in lasr_set_beam_bias' layout"""
    from libreasr_amd.engine import BeamBiasGraph
    return BeamBiasGraph(g.off, g.tok, g.nxt, g.gain, g.back, g.depth)


def bits(lp):
    return np.asarray(lp, np.float32).view(np.int32).tolist()


def code(fn, *a, **kw):
    with pytest.raises(N.LasrError) as e:
        fn(*a, **kw)
    return e.value.code


# ------------------------------------------------------------------------------- 1. the op-level round, exact on crafted logits
A_, B_, C_, D_, E_ = 5, 9, 7, 3, 12
MAX_ITERS = 3


def round_graph(V):
    """a wide node (A followed by any of up to 70 tokens, token V - 1 among them: more than 64 edges where the vocabulary has
    them; weights 2 to 5, so a row in node (A) holds 5.0), and B C D with 3.0 per token, so that a row in node (B, C) holds 6.0
    it hands back on anything but D"""
    wide = [t for t in range(20, min(V - 1, 20 + 69))] + [V - 1]
    phrases = [[A_, t] for t in wide] + [[B_, C_, D_]]
    weights = [2.0 + 1.0 * (i % 4) for i in range(len(wide))] + [3.0]
    return BB.automaton(phrases, weights), len(wide)


def row(V, peaks, base=-60.0):
    z = np.full(V, base, F32)
    for t, x in peaks.items():
        z[t] = x
    return z


def log_softmax32(z):
    z = np.asarray(z, np.float64)
    m = z.max()
    return ((z - m) - np.log(np.exp(z - m).sum())).astype(F32)


def round_ref(z, score, alive, inB, node, rounds, g, W, max_iters):
    """one biased selection round of every stream, from the spec; -> dict like Engine.beam_bias_round's, plus "gap": the smallest
    gap between two candidates that the selection or a row's offer separates, exact ties (equal floats) aside"""
    V = z.shape[1]
    n = len(rounds)
    out = {k: np.zeros(n * W, np.int32) for k in ("parent", "token", "emit", "alive", "inB", "node")}
    out["score"], out["term"] = np.full(n * W, -np.inf), np.zeros(n * W, F32)
    out["token"][:] = -1
    gap = np.inf
    for q in range(n):
        cands = []
        for b in range(W):
            r = q * W + b
            if not alive[r]:
                continue
            if inB[r]:
                cands.append((-score[r], b, 0, -1, 0.0, node[r]))
                continue
            lp = log_softmax32(z[r])
            gv = g.row(int(node[r]), V, BLANK)
            s = (lp + gv).astype(F32)
            order = np.argsort(-s, kind="stable")
            if s[order[W - 1]] != s[order[W]]:
                gap = min(gap, float(s[order[W - 1]]) - float(s[order[W]]))
            for v in order[:W]:
                cands.append((-((score[r] + float(lp[v])) + float(gv[v])), b, 1, int(v), float(lp[v]), node[r]))
        cands.sort(key=lambda c: c[:4])
        for x, y in zip(cands[:W], cands[1:W + 1]):
            if x[0] != y[0]:
                gap = min(gap, y[0] - x[0])
        at_cap = rounds[q] + 1 >= max_iters
        inb = []
        for j, (negs, b, kind, v, lpv, nd) in enumerate(cands[:W]):
            r = q * W + j
            out["alive"][r], out["parent"][r], out["score"][r] = 1, b, -negs
            if kind == 1 and v != BLANK:
                out["emit"][r], out["token"][r], out["term"][r] = 1, v, lpv
                out["node"][r] = g.step(int(nd), v, BLANK)[0]
                inb.append(1 if at_cap else 0)
            else:
                out["node"][r] = nd
                inb.append(1)
        for j in range(len(cands[:W]), W):
            out["parent"][q * W + j] = j
        done = all(inb)
        for j, x in enumerate(inb):
            out["inB"][q * W + j] = 0 if done else x
    out["gap"] = gap
    return out


def round_case(V, W):
    """-> (g, z [n W, V], score, alive, inB, node, rounds, names): one stream per scenario"""
    g, n_wide = round_graph(V)
    idx = {p: i for i, p in enumerate(g.paths)}
    nA, nBC = idx[(A_,)], idx[(B_, C_)]
    last = V - 1
    streams, names = [], []

    def stream(name, slots, rounds=0):
        """slots: W entries (z row, score, alive, inB, node)"""
        assert len(slots) == W
        streams.append((slots, rounds))
        names.append(name)

    dead = (row(V, {}), -np.inf, 0, 0, 0)
    # tokens a row of width W offers beside its peaks: distinct levels, 2 apart, far below
    fill = {(100 if V > 64 else 54) + i: -12.0 - 2.0 * i for i in range(W + 1)}

    def live(peaks, score, node=0):
        return (row(V, {**fill, **peaks}), score, 1, 0, node)

    # the wide node: every lane's scatter trip and the edge on token V - 1 -- the last token wins only through its gain
    edges = dict(zip(*[x.tolist() for x in g.edges(nA)[::2]]))
    stream("wide node, edge on V - 1",
           [live({last: 2.0, 30 if V > 64 else 25: 2.0 + edges[last] - 1.0 - edges[30 if V > 64 else 25], BLANK: 0.0}, 0.0, nA)] +
           [live({BLANK: 3.0, E_: 1.0}, -60.0 - 3.0 * b) for b in range(1, W)])
    # a negative gain pushes the row's best token out of its top W: E leads in log p, is not listed at (A) and hands 5 back,
    # while W listed tokens gain 5 each
    peaks = {E_: 6.0, BLANK: 2.0}
    peaks.update({23 + 4 * i: 5.0 - 0.75 * i for i in range(W)})
    assert all(edges[t] == 5.0 for t in peaks if t not in (E_, BLANK))
    stream("negative gain out of the top W", [live(peaks, 0.0, nA)] + [live({BLANK: 3.0, E_: 0.5}, -40.0 - 3.0 * b) for b in range(1, W)])
    # back on every unlisted token, blank unshifted: blank trails the best tokens by 2 and wins by 4
    stream("back on unlisted, blank unshifted",
           [live({E_: 4.0, A_: 2.0, BLANK: 2.0}, -1.0, nBC)] + [live({BLANK: 1.0, E_: 3.5}, -50.0 - 3.0 * b) for b in range(1, W)])
    # ties: slots 0 and 1 are twins (between rows: the lower slot first), E and E + 1 tie inside every row (the lower id first)
    twin_ = live({E_: 3.0, E_ + 1: 3.0, BLANK: 1.0}, -2.0, idx[(B_, C_, D_)])
    stream("ties", [twin_, twin_] + [live({BLANK: 2.0, A_: 1.0}, -30.0 - 3.0 * b) for b in range(2, W)])
    # a carried slot (and, from width 4, a dead one) among live ones
    mixed = [live({B_: 3.0, BLANK: 2.0}, -1.0), (row(V, {}), -1.75, 1, 1, nBC)]
    mixed += [live({BLANK: 2.0, A_: 1.5}, -6.0 - 1.75 * b) for b in range(2, W)]
    if W > 2:
        mixed[-1] = dead
    stream("carried and dead slots", mixed)
    stream("one live slot", [live({B_: 3.0, BLANK: 2.5}, 0.0, nA)] + [dead] * (W - 1))
    # the round at the cap: every extension joins B, the frame is finished
    stream("at the cap", [live({C_: 3.0, BLANK: 1.0}, -0.5 - 2.75 * b, idx[(B_,)] if b == 0 else 0) for b in range(W)], MAX_ITERS - 1)
    z = np.stack([s[0] for slots, _ in streams for s in slots])
    score = np.array([s[1] for slots, _ in streams for s in slots], np.float64)
    alive, inB, node = (np.array([s[k] for slots, _ in streams for s in slots], np.int32) for k in (2, 3, 4))
    return g, z, score, alive, inB, node, np.array([r for _, r in streams], np.int32), names


def check_round(got, want, rows, what):
    for k in ("parent", "token", "emit", "alive", "inB", "node"):
        assert got[k][rows].tolist() == want[k][rows].tolist(), (what, k, got[k][rows].tolist(), want[k][rows].tolist())
    for r in rows:
        if want["alive"][r]:
            assert abs(got["score"][r] - want["score"][r]) < 1e-4, (what, r, got["score"][r], want["score"][r])
        else:
            assert got["score"][r] == -np.inf, (what, r)
        assert abs(float(got["term"][r]) - float(want["term"][r])) < 1e-4, (what, r)


def round_expected(V, W):
    """the crafted case, its expected values, and -- read off those values alone -- that every scenario is what its name says"""
    case = round_case(V, W)
    g, z, score, alive, inB, node, rounds, names = case
    want = round_ref(z, score, alive, inB, node, rounds, g, W, MAX_ITERS)
    assert want["gap"] >= 0.5, want["gap"]                              # every decision is a clear one or an exact tie
    if V > 64:
        assert int(np.diff(g.off).max()) > 64                           # more than one scatter trip
    assert (V - 1) in g.tok.tolist()
    rows = lambda name: slice(names.index(name) * W, (names.index(name) + 1) * W)
    q = rows("wide node, edge on V - 1")
    assert want["token"][q][0] == V - 1 and want["node"][q][0] == {p: i for i, p in enumerate(g.paths)}[(A_, V - 1)]
    q = rows("negative gain out of the top W")
    assert E_ not in want["token"][q].tolist() and int(np.argmax(z[q][0])) == E_ and (want["parent"][q] == 0).sum() >= min(W, 3)
    q = rows("back on unlisted, blank unshifted")
    assert want["emit"][q][0] == 0 and want["parent"][q][0] == 0
    assert abs(want["score"][q][0] - (-1.0 + float(log_softmax32(z[q][0])[BLANK]))) < 1e-9
    q = rows("ties")
    assert want["score"][q][0] == want["score"][q][1]                   # (equal floats: the order is the tie rule's alone)
    assert want["parent"][q][:2].tolist() == [0, 0] and want["token"][q][:2].tolist() == [E_, E_ + 1]      # inside a row: the lower id
    if W > 2:                                                           # between rows: the lower slot
        assert want["score"][q][2] == want["score"][q][0]
        assert want["parent"][q][2:4].tolist() == [1, 1] and want["token"][q][2:4].tolist() == [E_, E_ + 1]
    q = rows("carried and dead slots")
    assert 1 in want["parent"][q][want["emit"][q] == 0].tolist()       # the carried slot survives as it is
    q = rows("one live slot")
    assert want["alive"][q].sum() == min(W, int(want["alive"][q].sum())) and (want["parent"][q][want["alive"][q] == 1] == 0).all()
    q = rows("at the cap")
    assert want["emit"][q].any() and not want["inB"][q].any()            # extended slots join B too: the frame is finished
    return case, want


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("V", [64, 320, 2048])
def test_beam_bias_round_is_exact(V, W):
    import torch
    (g, z, score, alive, inB, node, rounds, names), want = round_expected(V, W)
    eng = make(W=W, vocab=V, records=False)
    try:
        assert code(eng.beam_bias_round, torch.from_numpy(z).cuda(), score, alive, inB, node, rounds, MAX_ITERS) == N.LASR_ESTATE
        eng.set_beam_bias(native(g))
        got = eng.beam_bias_round(torch.from_numpy(z).cuda(), score, alive, inB, node, rounds, MAX_ITERS)
        for q, name in enumerate(names):
            check_round(got, want, list(range(q * W, (q + 1) * W)), (V, W, name))
        # a NaN row and a row with +inf beside finite rows, as one more stream: in-range results there, the others untouched
        zz = np.concatenate([z, z[:W]])
        zz[-W] = np.nan
        zz[-1, 7] = np.inf
        ext = lambda a, tail: np.concatenate([a, tail])
        got2 = eng.beam_bias_round(torch.from_numpy(zz).cuda(), ext(score, score[:W]), ext(alive, alive[:W]), ext(inB, inB[:W]),
                                   ext(node, node[:W]), ext(rounds, rounds[:1]), MAX_ITERS)
        for k in ("parent", "token", "emit", "alive", "inB", "node"):
            assert got2[k][:-W].tolist() == got[k].tolist(), k
        assert got2["score"][:-W].tolist() == got["score"].tolist() and bits(got2["term"][:-W]) == bits(got["term"])
        tail = slice(len(z), len(zz))
        assert np.all((got2["token"][tail] >= -1) & (got2["token"][tail] < V)) and np.all((got2["node"][tail] >= 0) & (got2["node"][tail] < g.n_nodes))
        assert np.all((got2["parent"][tail] >= 0) & (got2["parent"][tail] < W))
        assert code(eng.beam_bias_round, torch.from_numpy(z).cuda(), score, alive, inB, node + g.n_nodes, rounds, MAX_ITERS) == N.LASR_EINVAL
        # a live graph replaced by one of another size, and back: a hand-made graph of two nodes and one edge (A gains 1.5 at the
        # root and leads to node 1, where every other non-blank token hands it back) on the same logits, rows off the root in node 1
        small = BB.Graph([0, 1, 1], [A_], [1], [1.5], [0.0, -1.5])
        node1 = np.minimum(node, 1).astype(np.int32)
        want1 = round_ref(z, score, alive, inB, node1, rounds, small, W, MAX_ITERS)
        assert want1["gap"] >= 0.25, want1["gap"]      # (f32 log-softmax plus a gain errs by some 1e-5 at these sizes: every decision is clear)
        assert set(want1["node"].tolist()) == {0, 1} and want1["emit"].any()
        eng.set_beam_bias(native(small))
        got1 = eng.beam_bias_round(torch.from_numpy(z).cuda(), score, alive, inB, node1, rounds, MAX_ITERS)
        for q, name in enumerate(names):
            check_round(got1, want1, list(range(q * W, (q + 1) * W)), (V, W, name, "two nodes"))
        assert code(eng.beam_bias_round, torch.from_numpy(z).cuda(), score, alive, inB, node, rounds, MAX_ITERS) == N.LASR_EINVAL      # (g's nodes)
        eng.set_beam_bias(native(g))
        again = eng.beam_bias_round(torch.from_numpy(z).cuda(), score, alive, inB, node, rounds, MAX_ITERS)
        assert sorted(again) == sorted(got) and len(got) == 8
        for k in got:
            assert again[k].dtype == got[k].dtype and again[k].tobytes() == got[k].tobytes(), (V, W, k)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 2. offline parity on the committed cases
def check_rank(got, ref, what):
    (tok, fr, lp, sc), (rt, rf, rl, rs) = got, ref
    assert list(tok) == rt, (what, list(tok), rt)
    assert list(fr) == rf, (what, list(fr), rf)
    if rl:
        assert float(np.abs(np.asarray(lp, np.float64) - np.asarray(rl)).max()) < LOGP_TOL, (what, list(lp), rl)
    assert score_ok(sc, rs), (what, sc, rs)


def check_beam(eng, got, ref_beam, ref_bon, full, what):
    if full:
        assert len(got) == len(ref_beam), (what, len(got), len(ref_beam))
    for k in range(len(ref_beam) if full else 1):
        check_rank(got[k], ref_beam[k], what + (k,))
        if ref_bon is not None:                   # score - walk total = the restatement's score - bon: the acoustic score
            total = eng.bias_walk(got[k][0])[1]
            assert score_ok(got[k][3] - total, ref_beam[k][3] - ref_bon[k]), (what, k)
            assert abs(total - ref_bon[k]) < 1e-6, (what, k, total, ref_bon[k])


@pytest.mark.parametrize("name,W", BB.SHAPES)
def test_offline_parity_with_the_restatement(name, W):
    g, ref = BB.offline_ref(name, W)
    eng, plain = make(name, W), make(name, W, records=False)
    try:
        graph = eng.beam_bias_compile(*BB.OFFLINE_CASES[(name, W)])
        eng.set_beam_bias(graph)
        plain.set_beam_bias(graph)
        pcm = R.offline_pcm(name)
        slots, pslots = [eng.open() for _ in range(3)], [plain.open() for _ in range(3)]
        assert eng.beam_bias_state(slots[0]).tolist() == [0] + [-1] * (W - 1)
        eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
        plain.transcribe_pcm(pslots, [pcm[i] for i in range(3)])
        for i in range(3):
            what = (name, W, "utt", i)
            assert ref[i]["margin"] >= BB.MARGIN                        # (test_beam_bias_cpu.py: every utterance in full)
            assert eng.beam_bias_state(slots[i]).tolist() == ref[i]["nodes"], what
            got = eng.fetch_nbest(slots[i])
            print(what, len(got), "hypotheses,", len(got[0][0]), "tokens, margin", ref[i]["margin"])
            check_beam(eng, got, ref[i]["beam"], ref[i]["bon"], True, what)
            # records off (the REC = false instantiation): the same best hypothesis, bit for bit
            toks, neg_logp, _ = plain.fetch(pslots[i])
            assert toks == got[0][0] and -neg_logp == got[0][3], what
    finally:
        eng.close()
        plain.close()


# ------------------------------------------------------------------------------- 3. streaming parity, both protocols, with a reset
CHUNKS = R.stream_inputs()


def run_streams(eng, pipelined, reset_at=None, on_step=None, n_chunks=None):
    """the three streams side by side -> per stream the list of fetch_nbest results per model step.  pipelined: up to 4 model
    steps in flight.  reset_at: reset(1 | 2) of every stream before that model step (everything collected first).  on_step(i, j,
    slot) after stream i's step j was fetched; on_step(-1, reset_at, slots) just behind the reset."""
    slots = [eng.open() for _ in range(3)]
    hist = [[] for _ in range(3)]
    queue, was_reset = 0, False

    def collect():
        if pipelined:
            assert eng.wait() == 3
        for i in range(3):
            hist[i].append(eng.fetch_nbest(slots[i]))
            if on_step is not None:
                on_step(i, len(hist[i]) - 1, slots[i])

    for k in range(len(CHUNKS[0]) if n_chunks is None else n_chunks):
        batch = np.stack([CHUNKS[i][k] for i in range(3)])
        if pipelined:
            before = eng.pending()
            eng.push_submit(slots, batch)
            queue += 1 if eng.pending() > before else 0
        else:
            eng.push(slots, batch)
            ran = eng.step(slots)
            assert ran in (0, 3)
            queue += 1 if ran else 0
        due = reset_at is not None and not was_reset and len(hist[0]) + queue == reset_at
        while queue and (not pipelined or due or queue >= 4):
            collect()
            queue -= 1
        if due and queue == 0:
            for s in slots:
                eng.reset(s, 3)
            was_reset = True
            if on_step is not None:
                on_step(-1, reset_at, slots)
    while queue:
        collect()
        queue -= 1
    for s in slots:
        eng.close_slot(s)
    return hist


def compare_streams(eng, hist, ref, what):
    for i in range(3):
        n = BB.full_upto(ref[i])
        print(what, "stream", i, "compared in full up to step", n, "of", ref[i]["speech"])
        for j in range(n):
            for k, (gh, rh) in enumerate(zip(hist[i][j], ref[i]["steps"][j])):
                check_rank(gh, rh, what + (i, j, k))
            assert len(hist[i][j]) == len(ref[i]["steps"][j]), what + (i, j)


@pytest.mark.parametrize("reset_at", [None, BB.STREAM_RESET_AT])
@pytest.mark.parametrize("pipelined", [False, True])
def test_streaming_parity_with_the_restatement(pipelined, reset_at):
    g, ref = BB.stream_ref(reset_at)
    eng = make("tiny", 4)
    try:
        eng.set_beam_bias(eng.beam_bias_compile(*BB.STREAM_CASE))

        def on_step(i, j, slot):
            if i < 0:                                   # just behind the reset: every slot of every stream is at the root
                for s in slot:
                    assert eng.beam_bias_state(s).tolist() == [0, -1, -1, -1]
                return
            if not pipelined and j < BB.full_upto(ref[i]):
                assert eng.beam_bias_state(slot).tolist() == ref[i]["nodes"][j], (i, j)      # carried across model steps

        hist = run_streams(eng, pipelined, reset_at, on_step)
        assert [len(h) for h in hist] == [len(r["steps"]) for r in ref]
        compare_streams(eng, hist, ref, ("pipelined" if pipelined else "synchronous", reset_at))
        if reset_at is not None:
            assert all(BB.full_upto(r) > reset_at for r in ref)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 4. merging with a graph
def test_merge_on_with_bias_follows_the_restatement():
    g, ref = BB.offline_ref("tiny", 4, merge=True)
    eng = make("tiny", 4)
    try:
        eng.set_beam_merge(True)
        eng.set_beam_bias(eng.beam_bias_compile(*BB.OFFLINE_CASES[("tiny", 4)]))
        pcm = R.offline_pcm("tiny")
        slots = [eng.open() for _ in range(3)]
        eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
        merges = 0
        for i in range(3):
            full = ref[i]["margin"] >= BB.MARGIN
            nodes = eng.beam_bias_state(slots[i]).tolist()
            got = eng.fetch_nbest(slots[i])
            print(("merge", i), "margin", ref[i]["margin"], "merges", ref[i]["stats"].get("merges", 0), "full" if full else "rank 0")
            assert len({tuple(h[0]) for h in got}) == len(got)                 # pairwise distinct
            check_beam(eng, got, ref[i]["beam"], ref[i]["bon"] if full else None, full, ("merge", i))
            if full:
                assert nodes == ref[i]["nodes"]
            for h in got:                                                       # equal tokens, equal node: the node is the walk's
                assert eng.bias_walk(h[0])[0] in nodes
            merges += ref[i]["stats"].get("merges", 0)
        assert merges > 0
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 5. the state rules
def test_node_state_rules():
    g, ref = BB.stream_ref()
    eng = make("tiny", 4)
    try:
        graph = eng.beam_bias_compile(*BB.STREAM_CASE)
        assert code(eng.beam_bias_state, 0) == N.LASR_ESTATE                    # biasing is off
        eng.set_beam_bias(graph)
        K = BB.STREAM_RESET_AT

        def go_deep(steps=K, slot=None, k0=0):
            """`steps` model steps of stream 0's chunks from chunk k0 -> (slot, the next chunk, the last whole beam)"""
            if slot is None:
                slot = eng.open()
                assert eng.beam_bias_state(slot).tolist() == [0, -1, -1, -1]    # lasr_stream_open
            n = 0
            for k in range(k0, len(CHUNKS[0])):
                eng.push([slot], CHUNKS[0][k][None])
                if eng.step([slot]):
                    beam = eng.fetch_nbest(slot)
                    n += 1
                    if n == steps:
                        return slot, k + 1, beam
            raise AssertionError("the stream is too short")

        deep = ref[0]["nodes"][K - 1]
        assert any(v > 0 for v in deep) and BB.full_upto(ref[0]) >= K
        s = go_deep()[0]
        assert eng.beam_bias_state(s).tolist() == deep
        for what in (1, 4, 8, 1 | 4 | 8):                                        # bits 1, 4 and 8 alone leave the nodes
            eng.reset(s, what)
            assert eng.beam_bias_state(s).tolist() == deep, what
        eng.reset(s, 2)                                                          # bit 2: all W slots
        assert eng.beam_bias_state(s).tolist() == [0, -1, -1, -1]
        eng.close_slot(s)
        s2, other = go_deep()[0], eng.open()
        assert eng.beam_bias_state(s2).tolist() == deep
        eng.set_beam_bias(graph)                                                 # lasr_set_beam_bias: every slot back at the root,
        nodes = eng.beam_bias_state(s2).tolist()                                 # dead slots stay dead, the scores stay
        assert nodes == [0 if v >= 0 else -1 for v in deep] and eng.beam_bias_state(other).tolist() == [0, -1, -1, -1]
        eng.close_slot(other)
        # lasr_transcribe_* starts from the root on a slot that was left in deep nodes: the same as on a fresh slot
        s3, fresh = go_deep()[0], eng.open()
        utt = R.offline_pcm("tiny")[0]
        eng.transcribe_pcm([s3, fresh], [utt, utt])
        assert eng.beam_bias_state(s3).tolist() == eng.beam_bias_state(fresh).tolist()
        a, b = eng.fetch_nbest(s3), eng.fetch_nbest(fresh)
        assert [(h[0], list(h[1]), bits(h[2]), h[3]) for h in a] == [(h[0], list(h[1]), bits(h[2]), h[3]) for h in b]
        # clearing in mid-stream leaves the scores as they are, held bonuses included: the stream goes on as the restatement
        # does when its graph is taken away before model step 8 (margins of the next three steps: 0.04 each)
        from oracle import rnnt_oracle as O
        for s_ in (s2, s3, fresh):
            eng.close_slot(s_)
        K2 = 8
        fe, dec, want = O.StreamFrontend(), BB.StreamBeamBias(R.model("tiny")[0], 4, g), []
        for ch in CHUNKS[0]:
            o = fe.push(ch)
            if o is None:
                continue
            if len(dec.step_margin) == K2:
                assert any(h is not None and h["bon"] > 0 and g.back[h["node"]] < 0 for h in dec.hyps)      # a held bonus is at stake
                dec.g = None
            beam = dec.step(o)
            if len(dec.step_margin) > K2:
                assert dec.step_margin[-1] >= BB.MARGIN
                want.append(beam)
            if len(want) == 3:
                break
        s4, k, _ = go_deep(K2)
        eng.set_beam_bias(None)
        assert code(eng.beam_bias_state, s4) == N.LASR_ESTATE
        for j in range(3):
            _, k, beam = go_deep(1, s4, k)
            assert len(beam) == len(want[j])
            for r, (gh, rh) in enumerate(zip(beam, want[j])):
                check_rank(gh, rh, ("after the clear", j, r))
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 6. / 7. / 8. against a twin context
def all_paths(eng, W=4):
    """offline, synchronous and pipelined whole beams of one context (records on): what the twin tests compare bit for bit"""
    def flat(beam):
        return [(list(h[0]), list(h[1]), bits(h[2]), float(h[3])) for h in beam]
    pcm = R.offline_pcm("tiny")
    slots = [eng.open() for _ in range(3)]
    eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
    out = {"offline": [flat(eng.fetch_nbest(s)) for s in slots]}
    for s in slots:
        eng.close_slot(s)
    for mode in (False, True):
        out["pipelined" if mode else "sync"] = [[flat(b) for b in h] for h in run_streams(eng, mode, n_chunks=16)]
    return out


_TWIN = {}


def twin(dtype):
    """what a context that never sets a graph produces (computed once per operand type)"""
    if dtype not in _TWIN:
        eng = make("tiny", 4, dtype=dtype)
        try:
            _TWIN[dtype] = all_paths(eng)
        finally:
            eng.close()
    return _TWIN[dtype]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_gain_graph_is_bit_identical(dtype):
    eng = make("tiny", 4, dtype=dtype)
    try:
        g = BB.automaton(*BB.STREAM_CASE)
        eng.set_beam_bias(native(g.zeroed()))
        assert all_paths(eng) == twin(dtype)                           # BIAS = true against BIAS = false, bit for bit
        if dtype == "f32":                                             # ... while the nodes walk the automaton
            pcm = R.offline_pcm("tiny")
            s = eng.open()
            eng.transcribe_pcm([s], [pcm[0]])
            nodes = eng.beam_bias_state(s).tolist()
            beam = eng.fetch_nbest(s)
            assert sorted(v for v in nodes if v >= 0) == sorted(BB.walk(g, h[0], BLANK)[0] for h in beam)
    finally:
        eng.close()


def test_set_decode_clear_equals_a_twin_that_never_did():
    eng = make("tiny", 4)
    try:
        eng.set_beam_bias(eng.beam_bias_compile(*BB.STREAM_CASE))
        biased = all_paths(eng)
        assert biased["sync"] != twin("f32")["sync"] and biased["offline"] != twin("f32")["offline"]      # the graph did change the decode
        eng.set_beam_bias(None)
        assert code(eng.beam_bias_state, 0) == N.LASR_ESTATE
        assert all_paths(eng) == twin("f32")                           # ... and from the clear onwards nothing is left of it
    finally:
        eng.close()


def test_refusals_change_nothing():
    good = BB.automaton(*BB.STREAM_CASE)
    greedy = make("tiny", 1, records=False)
    try:
        assert code(greedy.set_beam_bias, native(good)) == N.LASR_EINVAL          # a greedy context has lasr_set_bias
        assert code(greedy.beam_bias_state, 0) == N.LASR_EINVAL
    finally:
        greedy.close()
    eng = make("tiny", 4)
    try:
        lsd = synth.synth_lm_state_dict("tiny_lm")
        eng.set_beam_bias(native(good))
        assert code(eng.attach_lm, lsd) == N.LASR_ESTATE                          # a beam graph is set: no LM
        assert eng.lm_cfg is None
        eng.set_beam_bias(None)
        eng.attach_lm(lsd)
        assert code(eng.set_beam_bias, native(good)) == N.LASR_ESTATE             # an LM is attached: no graph
        assert eng.beam_bias is None
    finally:
        eng.close()
    eng = make("tiny", 4)
    try:
        s = eng.open()
        for k in range(8):
            eng.push_submit([s], CHUNKS[0][k][None])
        assert eng.pending() > 0
        assert code(eng.set_beam_bias, native(good)) == N.LASR_ESTATE             # a step in flight
        while eng.pending():
            eng.wait()
        assert code(eng.set_beam_bias, native(good)) == N.LASR_ESTATE             # an unfetched result
        eng.fetch_nbest(s)
        eng.close_slot(s)
        V = eng.desc.vocab

        def variant(**kw):
            a = dict(off=good.off.copy(), tok=good.tok.copy(), nxt=good.nxt.copy(), gain=good.gain.copy(), back=good.back.copy())
            for k, (i, v) in kw.items():
                a[k][i] = v
            return BB.Graph(a["off"], a["tok"], a["nxt"], a["gain"], a["back"], good.depth)

        e0 = int(good.off[1])
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
            "gain beyond 1000": variant(gain=(0, 1000.5)),
            "gain below -1000": variant(gain=(0, -1000.5)),
            "infinite gain": variant(gain=(0, np.inf)),
            "nan gain": variant(gain=(0, np.nan)),
            "positive back": variant(back=(1, 0.5)),
            "back[0] != 0": variant(back=(0, -0.5)),
            "nan back": variant(back=(1, np.nan)),
            "back below -1000": variant(back=(1, -1000.5)),
        }
        for what, g in bad.items():
            assert code(eng.set_beam_bias, native(g)) == N.LASR_EINVAL, what
        from libreasr_amd.engine import BiasGraph
        with pytest.raises(ValueError):                                           # a graph of the greedy form: no node_back
            eng.set_beam_bias(BiasGraph(good.off, good.tok, good.nxt, np.abs(good.gain), good.depth))
        # nothing changed: biasing is still off, and the context decodes as its twin
        assert code(eng.beam_bias_state, 0) == N.LASR_ESTATE
        assert all_paths(eng) == twin("f32")
        # ... and with a graph set, a refused graph leaves the set one in place
        eng.set_beam_bias(native(good))
        for what, g in bad.items():
            assert code(eng.set_beam_bias, native(g)) == N.LASR_EINVAL, what
        _, ref = BB.stream_ref()
        hist = run_streams(eng, False, n_chunks=16)
        for i in range(3):
            for j in range(min(len(hist[i]), BB.full_upto(ref[i]))):
                check_rank(hist[i][j][0], ref[i]["steps"][j][0], ("after refusals", i, j))
    finally:
        eng.close()


def test_libreasr_facade_beam_hotwords():
    from libreasr_amd.api import LibreASR
    eng = make("tiny", 4)
    try:
        class Model:
            engine = eng
        asr = LibreASR(None, None, Model(), None, None)
        pcm = R.offline_pcm("tiny")[0]
        before = asr.transcribe(pcm, nbest=4)
        assert all("bonus" not in h for h in before)
        asr.set_beam_hotwords(BB.OFFLINE_CASES[("tiny", 4)][0], boost=BB.OFFLINE_CASES[("tiny", 4)][1])
        g, ref = BB.offline_ref("tiny", 4)
        out = asr.transcribe(pcm, nbest=4)
        assert [[t[0] for t in h["tokens"]] for h in out] == [b[0] for b in ref[0]["beam"]]
        for h, b, bon in zip(out, ref[0]["beam"], ref[0]["bon"]):
            assert score_ok(h["score"], b[3]) and abs(h["bonus"] - bon) < 1e-6
        asr.set_beam_hotwords(None)
        assert asr.transcribe(pcm, nbest=4) == before
    finally:
        eng.close()
