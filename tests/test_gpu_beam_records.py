"""Beam search on the GPU with lasr_set_beam_records on: every model step's result is the whole beam (lasr_fetch_nbest), every token
of every hypothesis carries its emission frame and the joint's log p of that extension.

Expected values: tests/beam_records_ref.py -- the oracle's _beam_frame restated with records (pinned to the spec on the CPU in
tests/test_beam_records_cpu.py).  Hypotheses are matched BY RANK (the beams of `tiny` hold the same token list on different frames):
n_hyps and the order equal, tokens and frames equal, log p within LOGP_TOL = 1e-3 (the project's fp32 bound for a log-prob), scores
within 2e-3 * max(1, |score|) (the bound of tests/test_gpu_beam.py).

The margin rule: GPU f32 and numpy f32 differ in the last bits, so a selection the oracle decides by less than 1e-3 is a tie.  A case
whose smallest selection-boundary gap and smallest gap between two kept hypotheses are both >= 1e-3 is compared in full; otherwise
in full up to the first model step below 1e-3, and from there on rank 0 (pinned without exception by tests/test_gpu_beam.py on these
inputs) plus structure, with the margin printed.  At most 3 of the 24 cases may fall back: counted on the CPU
(test_beam_records_cpu.test_margin_rule_lets_at_most_three_cases_fall_back)."""
import ctypes as C

import numpy as np
import pytest

import beam_records_ref as R
from libreasr_amd import _native as N
from libreasr_amd import synth

pytestmark = pytest.mark.gpu

LOGP_TOL = 1e-3
_ENGINES = {}


def engine(name, W, dtype="f32", records=True, lm=None):
    """(engine, oracle): one engine per (shape, width, type, switch, LM), kept for the module"""
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    key = (name, W, dtype, records, lm)
    if key not in _ENGINES:
        graft.build()
        m, sd, cfg = R.model(name, lm)
        eng = Engine(sd, cfg, max_streams=8, beam=W, dtype=dtype)
        if lm:
            eng.attach_lm(synth.synth_lm_state_dict(lm), int8=False)
        if records:
            eng.set_beam_records(True)
        _ENGINES[key] = (eng, m)
    return _ENGINES[key]


def check_structure(beam, T, W, max_iters, what):
    """whatever the records are: well-formed"""
    assert 1 <= len(beam) <= W, what
    sc = [h[3] for h in beam]
    assert all(a >= b for a, b in zip(sc, sc[1:])), (what, sc)
    for tok, fr, lp, score in beam:
        assert len(tok) == len(fr) == len(lp), what
        fr = np.asarray(fr, np.int64)
        assert np.all((0 <= fr) & (fr < T)) and np.all(np.diff(fr) >= 0), (what, fr.tolist(), T)
        assert np.bincount(fr, minlength=1).max() <= max_iters, what
        assert np.all(np.isfinite(lp)) and np.all(np.asarray(lp) <= 0), what
        assert np.isfinite(score)


def check_rank(got, ref, what):
    (tok, fr, lp, sc), (rt, rf, rl, rs) = got, ref
    assert tok == rt, (what, tok, rt)
    assert list(fr) == rf, (what, list(fr), rf)
    if rl:
        assert float(np.abs(np.asarray(lp, np.float64) - np.asarray(rl)).max()) < LOGP_TOL, (what, list(lp), rl)
    assert abs(sc - rs) < 2e-3 * max(1.0, abs(rs)), (what, sc, rs)


def check_beam(got, ref, full, what):
    """full: the whole beam rank by rank; else rank 0 only (the margin rule's fall-back)"""
    if full:
        assert len(got) == len(ref), (what, len(got), len(ref))
    for k in range(len(ref) if full else 1):
        check_rank(got[k], ref[k], what + (k,))


def same_as_fetch(beam, fetched, what):
    """hypothesis 0 is exactly what lasr_fetch returns on an engine that never heard of the switch"""
    toks, neg_logp, _ = fetched
    assert beam[0][0] == toks, (what, beam[0][0], toks)
    assert beam[0][3] == -neg_logp, (what, beam[0][3], -neg_logp)


# ------------------------------------------------------------------------------- 1. offline
@pytest.mark.parametrize("name,W", R.SHAPES)
def test_offline_whole_beam_equals_the_restatement(name, W):
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, records=False)
    ref = R.offline_ref(name, W)
    pcm = R.offline_pcm(name)
    slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]
    eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
    twin.transcribe_pcm(tslots, [pcm[i] for i in range(3)])
    for i in range(3):
        got = eng.fetch_nbest(slots[i])
        what = (name, W, "utt", i)
        same_as_fetch(got, twin.fetch(tslots[i]), what)
        check_structure(got, ref[i]["T"], W, 3, what)
        full = ref[i]["margin"] >= R.MARGIN
        print(f"{what}: {len(got)} hypotheses, {len(got[0][0])} tokens, oracle margin {ref[i]['margin']:.2e}{'' if full else ' -> rank 0 + structure'}")
        check_beam(got, ref[i]["beam"], full, what)
        assert eng.fetch_nbest(slots[i]) == []          # consumed, like lasr_fetch
    for s in slots:
        eng.close_slot(s)
    for s in tslots:
        twin.close_slot(s)


# ------------------------------------------------------------------------------- 2. / 3. streaming
def compare_step(got, ref_stream, j, W, what):
    """model step j of a stream under the margin rule; the silent tail: structure only"""
    T = ref_stream["T"][j]
    check_structure(got, T, W, 10, what)
    if j >= ref_stream["speech"]:
        return
    full = j < R.full_upto(ref_stream)
    if not full:
        print(f"{what}: oracle margin {ref_stream['margin'][j]:.2e} (first below at step {R.full_upto(ref_stream)}) -> rank 0 + structure")
    check_beam(got, ref_stream["steps"][j], full, what)


def drive(eng, twin, slots, tslots, chunks, pipelined, on_step, depth=4, fetch=None, every_third=None):
    """the streams join at chunks 0, 1, 3; on_step(i, fetch(slot i), twin's fetch) per stream and model step, in model-step order.
    every_third(): called after every third model step with everything collected and fetched (an idle engine)."""
    from oracle import rnnt_oracle as O
    fetch = fetch or eng.fetch_nbest
    n = len(chunks)
    fes = [O.StreamFrontend() for _ in range(n)]       # (tells which streams complete a model step with a chunk)
    order = []
    steps = 0

    def collect():
        rows = order.pop(0)
        if pipelined:
            assert eng.wait() == len(rows) and twin.wait() == len(rows)
        for i in rows:
            on_step(i, fetch(slots[i]), twin.fetch(tslots[i]))

    for k in range(len(chunks[0]) + max(R.START)):
        act = [i for i in range(n) if 0 <= k - R.START[i] < len(chunks[i])]
        if not act:
            continue
        batch = np.stack([chunks[i][k - R.START[i]] for i in act])
        ran = [i for i in act if fes[i].push(chunks[i][k - R.START[i]]) is not None]
        if pipelined:
            before = eng.pending()
            eng.push_submit([slots[i] for i in act], batch)
            twin.push_submit([tslots[i] for i in act], batch)
            assert (eng.pending() > before) == bool(ran)
        else:
            eng.push([slots[i] for i in act], batch)
            twin.push([tslots[i] for i in act], batch)
            assert eng.step([slots[i] for i in act]) == len(ran) == twin.step([tslots[i] for i in act])
        if not ran:
            continue
        order.append(ran)
        steps += 1
        idle_now = every_third is not None and steps % 3 == 0
        while order and (not pipelined or idle_now or eng.pending() >= depth):
            collect()
        if idle_now:
            every_third()
    while order:
        collect()


def reset_then_continue(eng, twin, slot, tslot, frozen, T0, name, W, pipelined):
    """a predictor reset freezes the best hypothesis WITH its records; the beam restarts; the slot's frame count runs on.
    frozen: hypothesis 0 of the slot's last model step (everything collected and fetched); T0: the frames it had consumed by then."""
    eng.reset(slot, 1 | 2 | 4)
    twin.reset(tslot, 1 | 2 | 4)
    extra = synth.stream_chunks(synth.synth_pcm(3, 48000, seed=31)[1], 1280, lead=0, tail=2)[:12]
    n_after, T, k0 = 0, T0, len(frozen[0])
    for ch in extra:
        if pipelined:
            eng.push_submit([slot], ch[None])
            twin.push_submit([tslot], ch[None])
            ran = eng.pending()
            assert twin.pending() == ran and ran <= 1
            if ran:
                assert eng.wait() == 1 and twin.wait() == 1
        else:
            eng.push([slot], ch[None])
            twin.push([tslot], ch[None])
            ran = eng.step([slot])
            assert twin.step([tslot]) == ran
        if not ran:
            continue
        T += 2
        beam = eng.fetch_nbest(slot)
        what = (name, W, "pipelined" if pipelined else "synchronous", "after reset", n_after)
        same_as_fetch(beam, twin.fetch(tslot), what)          # scores[0] == -neg_logp, tokens those of the plain engine
        check_structure(beam, T, W, 10, what)
        for tok, fr, lp, sc in beam:
            assert tok[:k0] == frozen[0] and list(fr[:k0]) == list(frozen[1]) and list(lp[:k0]) == list(frozen[2]), what
            assert all(T0 <= f for f in fr[k0:]), (what, list(fr[k0:]), T0)
        n_after += 1
    assert max(len(h[0]) for h in beam) > k0, "no token after the reset: the frozen prefix was not continued"
    assert n_after >= 4


@pytest.mark.parametrize("name,W", R.SHAPES)
def test_synchronous_streaming_whole_beam_per_model_step_then_reset(name, W):
    eng, m = engine(name, W)
    twin, _ = engine(name, W, records=False)
    ref = R.stream_ref(name, W)
    chunks = R.stream_inputs()
    slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]
    hist = [[] for _ in range(3)]

    def on_step(i, beam, fetched):
        j = len(hist[i])
        same_as_fetch(beam, fetched, (name, W, "stream", i, "step", j))
        compare_step(beam, ref[i], j, W, (name, W, "stream", i, "step", j))
        hist[i].append(beam)

    drive(eng, twin, slots, tslots, chunks, False, on_step)
    assert [len(h) for h in hist] == [21, 21, 21]
    if name == "tiny":
        assert len(hist[2][-1][0][0]) > 50           # the bursty stream (84 to 136 tokens per hypothesis in 3 s)
    reset_then_continue(eng, twin, slots[0], tslots[0], hist[0][-1][0], ref[0]["T"][-1], name, W, False)
    for s in slots:
        eng.close_slot(s)
    for s in tslots:
        twin.close_slot(s)


@pytest.mark.parametrize("name,W", R.SHAPES)
def test_pipelined_whole_beam_per_collected_model_step(name, W):
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, records=False)
    ref = R.stream_ref(name, W)
    slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]
    n_steps = [0, 0, 0]
    last = [None, None, None]

    def on_step(i, beam, fetched):
        j = n_steps[i]
        same_as_fetch(beam, fetched, (name, W, "pipelined stream", i, "step", j))
        compare_step(beam, ref[i], j, W, (name, W, "pipelined stream", i, "step", j))
        n_steps[i] += 1
        last[i] = beam

    drive(eng, twin, slots, tslots, R.stream_inputs(), True, on_step)
    assert n_steps == [21, 21, 21]
    # everything is collected and fetched: the same reset tail as the synchronous test, through push_submit / wait
    assert eng.pending() == 0 and twin.pending() == 0
    reset_then_continue(eng, twin, slots[0], tslots[0], last[0][0], ref[0]["T"][-1], name, W, True)
    for s in slots:
        eng.close_slot(s)
    for s in tslots:
        twin.close_slot(s)


# ------------------------------------------------------------------------------- 4. the switch and the cached graphs
def test_toggling_the_switch_every_third_step_changes_no_token():
    """Both protocols: the decode groups are cached graphs that captured BeamState by value -- a stale one would keep storing (or
    not storing) records, or run on with the other kernel.  The toggled engine's tokens equal the untoggled twin's."""
    name, W = "tiny", 4
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, records=False)
    try:
        for pipelined in (False, True):
            slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]
            state = dict(on=True, seen=0, with_records=0)

            def fetch(slot):
                return eng.fetch_nbest(slot) if state["on"] else eng.fetch(slot)

            def on_step(i, got, fetched):
                state["seen"] += 1
                if state["on"]:
                    same_as_fetch(got, fetched, (pipelined, i, state["seen"]))
                    state["with_records"] += 1
                else:
                    assert got[0] == fetched[0] and got[1] == fetched[1], (pipelined, i, state["seen"])

            def toggle():
                state["on"] = not state["on"]
                eng.set_beam_records(state["on"])

            drive(eng, twin, slots, tslots, R.stream_inputs(), pipelined, on_step, fetch=fetch, every_third=toggle)
            assert state["seen"] == 63 and 20 <= state["with_records"] <= 45, state
            eng.set_beam_records(True)
            for sl in slots:
                eng.close_slot(sl)
            for sl in tslots:
                twin.close_slot(sl)
    finally:
        eng.set_beam_records(True)


def test_switch_on_after_the_trellis_grew_while_it_was_off():
    """The records are indexed like the trellis, which grows with the longest utterance seen.  On a fresh engine: on, a short utterance
    (both sized for it); off; a long utterance (the trellis grows alone); on; the same long utterance -- the records must hold every
    round of it: the whole beam equals the restatement's and the twin's answer."""
    from libreasr_amd.engine import Engine
    name, W = "tiny", 4
    m, sd, cfg = R.model(name)
    twin, _ = engine(name, W, records=False)
    ref = R.offline_ref(name, W)[1]
    assert ref["margin"] >= R.MARGIN                 # (compared in full)
    long_pcm = R.offline_pcm(name)[1]
    short_pcm = long_pcm[:8000]                      # 6 frames against 37
    eng = Engine(sd, cfg, max_streams=8, beam=W)
    try:
        s, ts = eng.open(), twin.open()
        eng.set_beam_records(True)
        eng.transcribe_pcm([s], [short_pcm])
        twin.transcribe_pcm([ts], [short_pcm])
        got = eng.fetch_nbest(s)
        same_as_fetch(got, twin.fetch(ts), ("short",))
        check_structure(got, 6, W, 3, ("short",))
        eng.set_beam_records(False)
        eng.transcribe_pcm([s], [long_pcm])
        twin.transcribe_pcm([ts], [long_pcm])
        fetched = twin.fetch(ts)
        assert eng.fetch(s)[:2] == fetched[:2]
        eng.set_beam_records(True)
        eng.transcribe_pcm([s], [long_pcm])
        got = eng.fetch_nbest(s)
        same_as_fetch(got, fetched, ("long",))
        check_structure(got, ref["T"], W, 3, ("long",))
        check_beam(got, ref["beam"], True, ("long",))
        twin.close_slot(ts)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 5. LM inside the beam
def test_lm_inside_the_beam_tokens_are_the_repicks_logp_stays_the_joints():
    """On these utterances the oracle's re-pick differs from the joint's best non-blank token inside an utterance that is compared in
    full (pinned on the CPU: test_lm_case_has_a_repick_that_differs_from_the_joints_token): a record that followed the re-pick, or a
    token that did not, fails the comparison."""
    name, lm, W = "tiny", "tiny_lm", 2
    eng, _ = engine(name, W, lm=lm)
    ref = R.offline_ref(name, W, lm, R.LM_PCM_SEED)
    pcm = R.offline_pcm(name, R.LM_PCM_SEED)
    slots = [eng.open() for _ in range(3)]
    eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
    pinned = 0
    for i in range(3):
        got = eng.fetch_nbest(slots[i])
        what = (name, lm, W, "utt", i)
        check_structure(got, ref[i]["T"], W, 3, what)
        full = ref[i]["margin"] >= R.MARGIN
        print(f"{what}: oracle margin {ref[i]['margin']:.2e}, re-picks that differ {ref[i]['repicked']}{'' if full else ' -> rank 0 + structure'}")
        check_beam(got, ref[i]["beam"], full, what)
        pinned += sum(ref[i]["repicked"]) if full else 0
        eng.close_slot(slots[i])
    assert pinned > 0, "no re-pick differs from the joint's token: the rule is not exercised"


# ------------------------------------------------------------------------------- 6. every register slot
def test_cfg2_width_8_fills_every_register_slot():
    name, W = "cfg2", 8
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, records=False)
    ref = R.offline_ref(name, W)[0]
    pcm = R.offline_pcm(name)[0]
    s, ts = eng.open(), twin.open()
    eng.transcribe_pcm([s], [pcm])
    twin.transcribe_pcm([ts], [pcm])
    got = eng.fetch_nbest(s)
    what = (name, W)
    same_as_fetch(got, twin.fetch(ts), what)
    check_structure(got, ref["T"], W, 3, what)
    full = ref["margin"] >= R.MARGIN
    print(f"{what}: {len(got)} hypotheses, {len(got[0][0])} tokens, oracle margin {ref['margin']:.2e}{'' if full else ' -> rank 0 + structure'}")
    check_beam(got, ref["beam"], full, what)
    eng.close_slot(s)
    twin.close_slot(ts)


# ------------------------------------------------------------------------------- 7. bf16
def test_bf16_records_are_well_formed():
    name, W = "tiny", 4
    eng, _ = engine(name, W, dtype="bf16")
    pcm = R.offline_pcm(name)
    slots = [eng.open() for _ in range(3)]
    eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
    n_tok = 0
    for i in range(3):
        got = eng.fetch_nbest(slots[i])
        check_structure(got, R.offline_ref(name, W)[i]["T"], W, 3, (name, W, "bf16", i))
        n_tok += len(got[0][0])
        eng.close_slot(slots[i])
    assert n_tok > 0


# ------------------------------------------------------------------------------- 9. errors
def test_errors_and_buffer_contract():
    from libreasr_amd.engine import Engine
    name, W = "tiny", 4
    eng, _ = engine(name, W)
    m, sd, cfg = R.model(name)
    greedy = Engine(sd, cfg, max_streams=2)
    try:
        with pytest.raises(N.LasrError) as e:
            greedy.set_beam_records(True)
        assert e.value.code == N.LASR_EINVAL
    finally:
        greedy.close()
    twin, _ = engine(name, W, records=False)
    ts = twin.open()
    with pytest.raises(N.LasrError) as e:
        twin.fetch_nbest(ts)
    assert e.value.code == N.LASR_ESTATE
    twin.close_slot(ts)
    # a switch needs an idle engine without unfetched results
    chunks = R.stream_inputs()[0]
    s = eng.open()
    k = 0
    while not eng.pending():
        eng.push_submit([s], chunks[k][None])
        k += 1
    with pytest.raises(N.LasrError) as e:
        eng.set_beam_records(False)
    assert e.value.code == N.LASR_ESTATE
    eng.set_beam_records(True)                       # (changes nothing: fine while a step is in flight)
    assert eng.wait() == 1
    with pytest.raises(N.LasrError) as e:            # collected, not fetched
        eng.set_beam_records(False)
    assert e.value.code == N.LASR_ESTATE
    assert len(eng.fetch_nbest(s)) >= 1
    eng.close_slot(s)
    # LASR_EFULL: nothing consumed, n_tokens[] = needed; max_hyps < n_hyps truncates from the back
    pcm = R.offline_pcm(name)[0]
    s = eng.open()
    eng.transcribe_pcm([s], [pcm])
    ref = R.offline_ref(name, W)[0]["beam"]
    need = [len(h[0]) for h in ref]
    assert min(need) > 2
    cap = max(need)
    tok = np.zeros((W, cap), np.int32)
    cnt = np.zeros(W, np.int32)
    sc = np.zeros(W, np.float64)
    nh = C.c_int(0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = eng.lib.lasr_fetch_nbest(eng.ctx, s, W, P(tok), None, None, 2, P(cnt), P(sc), C.byref(nh))
    assert rc == N.LASR_EFULL and nh.value == len(ref) and cnt[:nh.value].tolist() == need
    # nothing was consumed: the very next call, with the room the failed one asked for, returns every hypothesis (frames, logps optional)
    cap2 = int(cnt[:nh.value].max())
    tok2, cnt2 = np.zeros((W, cap2), np.int32), np.zeros(W, np.int32)
    rc = eng.lib.lasr_fetch_nbest(eng.ctx, s, W, P(tok2), None, None, cap2, P(cnt2), P(sc), C.byref(nh))
    assert rc == N.LASR_OK and nh.value == len(ref)
    assert [tok2[i, :cnt2[i]].tolist() for i in range(nh.value)] == [h[0] for h in ref]
    assert all(abs(sc[i] - ref[i][3]) < 2e-3 * max(1.0, abs(ref[i][3])) for i in range(nh.value))
    assert eng.fetch_nbest(s) == []                  # now it is consumed
    # a null tokens pointer is an argument error, not a size query
    eng.transcribe_pcm([s], [pcm])
    rc = eng.lib.lasr_fetch_nbest(eng.ctx, s, W, None, None, None, cap, P(cnt), P(sc), C.byref(nh))
    assert rc == N.LASR_EINVAL
    # max_hyps < n_hyps truncates from the back
    two = eng.fetch_nbest(s, max_hyps=2)             # frames / log p come along; the two best only
    assert len(two) == 2 and [h[0] for h in two] == [h[0] for h in ref[:2]]
    assert [list(h[1]) for h in two] == [h[1] for h in ref[:2]]
    assert eng.fetch_nbest(s) == []                  # the rest was dropped with the fetch
    eng.transcribe_pcm([s], [pcm])
    toks, neg_logp, _ = eng.fetch(s)                 # lasr_fetch keeps working and consumes the same result
    assert toks == ref[0][0] and eng.fetch_nbest(s) == []
    eng.close_slot(s)


# ------------------------------------------------------------------------------- 10. facade
def test_libreasr_facade_nbest():
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", synthetic="tiny", max_streams=4, beam=4)
    try:
        pcm = R.offline_pcm("tiny")[0]
        ref = R.offline_ref("tiny", 4)[0]
        out = asr.transcribe(pcm, nbest=2)
        assert len(out) == 2 and out[0]["score"] >= out[1]["score"]
        ids = asr.transcribe(pcm, return_ids=True)
        assert [t for t, _, _ in out[0]["tokens"]] == ids == ref["beam"][0][0]
        for h in out:
            assert all(abs(ts / 0.08 - round(ts / 0.08)) < 1e-9 and 0.0 < cf <= 1.0 for _, ts, cf in h["tokens"])
        assert [round(ts / 0.08) for _, ts, _ in out[0]["tokens"]] == ref["beam"][0][1]
        batch = asr.transcribe([pcm, pcm], nbest=1)
        assert len(batch) == 2 and all(len(b) == 1 and [t for t, _, _ in b[0]["tokens"]] == ids for b in batch)
        chunks = R.stream_inputs()[1]
        last_ids = None
        for last_ids in asr.stream(chunks, return_ids=True):
            pass
        last, n = None, 0
        for last in asr.stream(chunks, nbest=2):
            assert 1 <= len(last) <= 2
            n += 1
        assert n == 21 and [t for t, _, _ in last[0]["tokens"]] == last_ids
        fr = [round(ts / 0.08) for _, ts, _ in last[0]["tokens"]]
        assert fr == sorted(fr) and all(0.0 < cf <= 1.0 for _, _, cf in last[0]["tokens"])
    finally:
        asr.engine.close()
    greedy = LibreASR.load("en", synthetic="tiny", max_streams=4)
    try:
        with pytest.raises(ValueError):
            greedy.transcribe(R.offline_pcm("tiny")[0], nbest=2)
        with pytest.raises(ValueError):
            next(greedy.stream([np.zeros(1280, np.float32)], nbest=2))
    finally:
        greedy.engine.close()
