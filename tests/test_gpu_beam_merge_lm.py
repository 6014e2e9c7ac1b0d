"""Beam search on the GPU with an LM attached and lasr_set_beam_merge(c, LASR_BEAM_MERGE_LM): hypotheses that hold the same tokens
are merged, with identities chained from the fuser's re-picked tokens (k_beam_fuse_merge).

Expected values: tests/beam_merge_lm_ref.py (pinned on the CPU in tests/test_beam_merge_lm_cpu.py).  Structure, tolerances and the
margin rule are those of tests/test_gpu_beam_merge.py: compared rank by rank, tokens and frames equal, log p within 1e-3, scores
within 2e-3 * max(1, |score|); a case whose oracle margin is below 1e-3 (offline at max_iters 3: at most the three the CPU test names)
is compared in full up to its first model step below the margin and by rank 0 + structure from there.  The largest differences seen
are printed.

The cases compared in full include the inputs on which a plausible wrong build differs (test_beam_merge_lm_cpu.py, test 6): those
where grouping by an identity of the JOINT's token differs from the true grouping (max_iters_offline 3), and those where a merge
involves a differing re-pick made in the same round (max_iters_offline 1).  One of the former, (tiny, seed 1234, W = 8, utterance 1),
is excused by its margin (3.7e-4): seed 1233 stands in, all three of its W = 8 utterances are such inputs above the margin."""
import copy

import numpy as np
import pytest

import beam_merge_lm_ref as L
import beam_merge_ref as M
import beam_records_ref as R
from libreasr_amd import _native as N
from libreasr_amd import synth
from test_gpu_beam_merge import WORST, compare, distinct
from test_gpu_beam_records import check_structure, drive

pytestmark = pytest.mark.gpu

_ENGINES, _OFFLINE = {}, {}
OFF, ON, ON_LM = 0, 1, 2                            # the switch's three values


def engine(name, W, mode=ON_LM, lm=L.LM, dtype="f32", max_iters_offline=3):
    """(engine, oracle): records on, the LM attached (lm=None: none), the switch in `mode` (tests that toggle put it back)"""
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    key = (name, W, mode, lm, dtype, max_iters_offline)
    if key not in _ENGINES:
        graft.build()
        m, sd, cfg = R.model(name, lm)
        eng = Engine(sd, cfg, max_streams=8, beam=W, dtype=dtype, max_iters_offline=max_iters_offline)
        if lm:
            eng.attach_lm(synth.synth_lm_state_dict(lm), int8=False)
        eng.set_beam_records(True)
        if mode:
            eng.set_beam_merge(True, lm=(mode == ON_LM))
        _ENGINES[key] = (eng, m)
    return _ENGINES[key]


def run_offline(eng, pcm):
    slots = [eng.open() for _ in range(len(pcm))]
    eng.transcribe_pcm(slots, [pcm[i] for i in range(len(pcm))])
    out = [eng.fetch_nbest(s) for s in slots]
    for s in slots:
        eng.close_slot(s)
    return out


def offline_run(name, W, mode=ON_LM, seed=31, lm=L.LM, dtype="f32", max_iters_offline=3):
    """the final beams of the offline utterances, once per (engine, seed): [fetch_nbest per utterance]"""
    key = (name, W, mode, seed, lm, dtype, max_iters_offline)
    if key not in _OFFLINE:
        _OFFLINE[key] = run_offline(engine(name, W, mode, lm, dtype, max_iters_offline)[0], R.offline_pcm(name, seed))
    return _OFFLINE[key]


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for (t, f, lp, sc), (t2, f2, lp2, sc2) in zip(x, y):
            assert t == t2 and list(f) == list(f2) and np.array_equal(lp, lp2) and sc == sc2


def worst():
    print(f"largest differences so far: log p {WORST['logp']:.2e}, score (relative to max(1, |score|)) {WORST['score']:.2e}")


# ------------------------------------------------------------------------------- 1. fails without the feature
@pytest.mark.parametrize("seed", [31, 1234])
@pytest.mark.parametrize("name,W", L.SHAPES)
def test_offline_final_beams_are_pairwise_distinct_where_the_twin_holds_duplicates(name, W, seed):
    for i, beam in enumerate(offline_run(name, W, seed=seed)):
        distinct(beam, (name, W, seed, "utt", i))
    twin, ref, n = offline_run(name, W, OFF, seed), L.offline_ref(name, W, 3, False, seed), 0
    for i in range(3):
        if ref[i]["distinct"] < ref[i]["n"] and ref[i]["margin"] >= L.MARGIN:      # (the twin's beam is pinned rank by rank there)
            ys = [tuple(h[0]) for h in twin[i]]
            assert len(set(ys)) < len(ys), (name, W, seed, i, "no duplicate without merging: the case pins nothing")
            n += 1
    if (name, W) == ("tiny", 8):
        assert n >= 2, (seed, n)                                                    # seed 31: all three, seed 1234: utterances 1 and 2


# ------------------------------------------------------------------------------- 2. parity with the restatement
OFFLINE_CASES = [(n, w, mi, s) for n, w in L.SHAPES for mi in (3, 1) for s in (31, 1234)] + [("tiny", 8, 3, 1233)]


@pytest.mark.parametrize("name,W,max_iters,seed", OFFLINE_CASES)
def test_offline_parity_rank_by_rank(name, W, max_iters, seed):
    ref = L.offline_ref(name, W, max_iters, True, seed)
    for i, got in enumerate(offline_run(name, W, seed=seed, max_iters_offline=max_iters)):
        what = (name, W, "max_iters", max_iters, "seed", seed, "utt", i)
        check_structure(got, ref[i]["T"], W, max_iters, what)
        distinct(got, what)
        full = ref[i]["margin"] >= L.MARGIN
        w = ref[i]["watch"]
        print(f"{what}: {len(got)} hypotheses, {ref[i]['merges']} merges, joint-identity grouping differs in {w['jdiff_rounds']} rounds, "
              f"{w['rp_groups']} merges of a fresh re-pick, oracle margin {ref[i]['margin']:.2e}{'' if full else ' -> rank 0 + structure'}")
        compare(got, ref[i]["beam"], full, what)
    worst()


def compare_step(got, ref_stream, j, W, what):
    check_structure(got, ref_stream["T"][j], W, 10, what)
    distinct(got, what)
    if j >= ref_stream["speech"]:
        return
    full = j < L.full_upto(ref_stream)
    if not full:
        print(f"{what}: oracle margin {ref_stream['margin'][j]:.2e} (first below at step {L.full_upto(ref_stream)}) -> rank 0 + structure")
    compare(got, ref_stream["steps"][j], full, what)


def reset_then_continue(eng, twin, slot, tslot, ref0, frozen, name, W, pipelined):
    """test_gpu_beam_merge.reset_then_continue with one difference.  A reset with bits 1 | 2 | 4 restarts encoder, predictor, beam,
    identities and LM; all that is left of the stream is the frozen best hypothesis and the front-end.  The reset comes behind the
    stream's silent tail, whose model steps the margin rule never compares in full (the front-ends differ at the log-mel floor, and
    under the LM the tail's beams do differ: tiny_lstm, W = 4), so the restatement goes on from the ENGINE's frozen hypothesis
    (tokens, frames, log p, score) instead of its own: everything behind the reset is compared as usual, the frozen prefix must be
    the engine's own last rank 0."""
    eng.reset(slot, 1 | 2 | 4)
    twin.reset(tslot, 1 | 2 | 4)
    dec, fe = ref0["dec"].clone(), copy.deepcopy(ref0["fe"])
    dec.reset()
    dec.prefix = (list(frozen[0]), [int(f) for f in frozen[1]], [float(x) for x in frozen[2]], float(frozen[3]))
    extra = synth.stream_chunks(synth.synth_pcm(3, 48000, seed=31)[1], 1280, lead=0, tail=2)[:12]
    n_after, k0, ok = 0, len(frozen[0]), True
    for ch in extra:
        if pipelined:
            eng.push_submit([slot], ch[None])
            twin.push_submit([tslot], ch[None])
            ran = eng.pending()
            if ran:
                assert eng.wait() == 1 and twin.wait() == 1
        else:
            eng.push([slot], ch[None])
            twin.push([tslot], ch[None])
            ran = eng.step([slot])
            assert twin.step([tslot]) == ran
        o = fe.push(ch)
        assert (o is not None) == bool(ran)
        if not ran:
            continue
        want = dec.step(o)
        twin.fetch(tslot)
        beam = eng.fetch_nbest(slot)
        what = (name, W, "pipelined" if pipelined else "synchronous", "after reset", n_after)
        check_structure(beam, dec.t, W, 10, what)
        distinct(beam, what)
        for tok, fr, lp, sc in beam:
            assert tok[:k0] == frozen[0] and list(fr[:k0]) == list(frozen[1]) and list(lp[:k0]) == list(frozen[2]), what
        ok = ok and dec.step_margin[-1] >= L.MARGIN
        if ok:
            compare(beam, want, True, what)
        n_after += 1
    assert max(len(h[0]) for h in beam) > k0, "no token after the reset: the frozen prefix was not continued"
    assert n_after >= 4


def run_streams(name, W, pipelined):
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, OFF)
    ref = L.stream_ref(name, W)
    slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]
    hist = [[] for _ in range(3)]
    kind = "pipelined" if pipelined else "synchronous"

    def on_step(i, beam, fetched):
        compare_step(beam, ref[i], len(hist[i]), W, (name, W, kind, "stream", i, "step", len(hist[i])))
        hist[i].append(beam)

    drive(eng, twin, slots, tslots, L.stream_inputs(), pipelined, on_step)
    assert [len(h) for h in hist] == [21, 21, 21]
    assert eng.pending() == 0 and twin.pending() == 0
    # reset with bits 1 | 2 | 4 (encoder, predictor + beam + identities, LM), then going on
    reset_then_continue(eng, twin, slots[0], tslots[0], ref[0], hist[0][-1][0], name, W, pipelined)
    for s in slots:
        eng.close_slot(s)
    for s in tslots:
        twin.close_slot(s)
    worst()


@pytest.mark.parametrize("name,W", L.SHAPES)
def test_synchronous_streaming_parity_per_model_step_then_reset(name, W):
    run_streams(name, W, False)


@pytest.mark.parametrize("name,W", L.SHAPES)
def test_pipelined_parity_per_collected_model_step_then_reset(name, W):
    run_streams(name, W, True)


# ------------------------------------------------------------------------------- 3. toggling in mid-stream
@pytest.mark.parametrize("pipelined", [False, True])
def test_toggling_every_third_step_follows_the_restatement_toggled_at_the_same_steps(pipelined):
    """0 -> LASR_BEAM_MERGE_LM -> 0 every third model step with the LM attached: a switch-on in mid-stream takes the slots' identities
    from the host's trees, which hold the re-picked tokens.  The restatement toggles at the same steps."""
    name, W = "tiny", 4
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, OFF)
    eng.set_beam_merge(False)
    state = {"on": False}
    sched, hist = [[] for _ in range(3)], [[] for _ in range(3)]
    try:
        slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]

        def on_step(i, beam, fetched):
            sched[i].append(state["on"])
            hist[i].append(beam)

        def toggle():
            state["on"] = not state["on"]
            eng.set_beam_merge(state["on"], lm=True)

        drive(eng, twin, slots, tslots, L.stream_inputs(), pipelined, on_step, every_third=toggle)
        for s in slots:
            eng.close_slot(s)
        for s in tslots:
            twin.close_slot(s)
    finally:
        eng.set_beam_merge(True, lm=True)
    assert [len(h) for h in hist] == [21, 21, 21]
    n_on = sum(sum(s) for s in sched)
    assert 20 <= n_on <= 45, sched
    ref = L.stream_run(name, W, merge_at=lambda i, j: sched[i][j])
    for i in range(3):
        for j in range(21):
            what = (name, W, "pipelined" if pipelined else "synchronous", "toggled stream", i, "step", j, "on" if sched[i][j] else "off")
            check_structure(hist[i][j], ref[i]["T"][j], W, 10, what)
            if j < ref[i]["speech"]:
                compare(hist[i][j], ref[i]["steps"][j], j < L.full_upto(ref[i]), what)
    worst()


# ------------------------------------------------------------------------------- 4. / 5. the other modes are what they were
def test_mode_2_without_an_lm_is_mode_1_bit_for_bit():
    name, W = "tiny", 8
    for seed in (31, 1234):
        same_bits(offline_run(name, W, ON_LM, seed, lm=None), offline_run(name, W, ON, seed, lm=None))
    ref = M.offline_ref(name, W)                                # ... and both are 5.9's restatement
    for i, got in enumerate(offline_run(name, W, ON_LM, 1234, lm=None)):
        compare(got, ref[i]["beam"], ref[i]["margin"] >= M.MARGIN, (name, W, "mode 2, no LM", i))
    # streamed: 1 -> 2 -> 1 in mid-stream on one engine against an engine that stays in mode 1
    a, b = engine(name, W, ON_LM, None)[0], engine(name, W, ON, None)[0]
    sa, sb = a.open(), b.open()
    try:
        for k, ch in enumerate(R.stream_inputs()[2]):
            for e, s in ((a, sa), (b, sb)):
                e.push([s], ch[None])
            ran = a.step([sa])
            assert b.step([sb]) == ran
            if ran:
                same_bits([a.fetch_nbest(sa)], [b.fetch_nbest(sb)])
                if k % 4 == 0:
                    a.set_beam_merge(True, lm=(k % 8 == 0))
    finally:
        a.set_beam_merge(True, lm=True)
        a.close_slot(sa)
        b.close_slot(sb)


def test_with_the_lm_mode_2_switched_off_again_is_bit_equal_to_an_engine_never_switched():
    name, W = "tiny", 8
    eng, _ = engine(name, W)
    never = offline_run(name, W, OFF, 31)
    eng.set_beam_merge(False)
    try:
        got = run_offline(eng, R.offline_pcm(name, 31))
    finally:
        eng.set_beam_merge(True, lm=True)
    same_bits(got, never)
    ref = R.offline_ref(name, W, L.LM, 31)                      # ... which is the beam with an LM of before
    for i in range(3):
        compare(never[i], ref[i]["beam"], ref[i]["margin"] >= R.MARGIN, (name, W, "LM, never merged", i))


# ------------------------------------------------------------------------------- 6. contract
def test_contract_of_the_third_value():
    from libreasr_amd.engine import Engine
    name, W = "tiny", 4
    m, sd, cfg = R.model(name, L.LM)
    lm = synth.synth_lm_state_dict(L.LM)
    pcm = R.offline_pcm(name, 31)[1]
    want = L.offline_ref(name, W, 3, True, 31)[1]
    assert want["margin"] >= L.MARGIN

    def refused(code, f, *a, **kw):
        with pytest.raises(N.LasrError) as ei:
            f(*a, **kw)
        assert ei.value.code == code, (ei.value.code, code)

    def beam_of(e):
        return run_offline(e, [pcm])[0]

    e1 = Engine(sd, cfg, max_streams=2, beam=W)                 # mode 2 first, then the LM
    try:
        e1.set_beam_records(True)
        e1.set_beam_merge(True, lm=True)
        e1.set_beam_merge(True, lm=True)                        # (changes nothing)
        refused(N.LASR_ESTATE, lambda: e1.attach_lm(lm, int8=True))      # a beam context refuses the int8-served LM as before
        e1.attach_lm(lm, int8=False)                            # accepted while mode 2 is on
        got = beam_of(e1)
        distinct(got, "mode 2, LM attached afterwards")
        compare(got, want["beam"], True, (name, W, "mode 2 then attach_lm"))
        refused(N.LASR_ESTATE, e1.set_beam_merge, True)         # 2 -> 1 with an LM: refused, nothing changed
        same_bits([beam_of(e1)], [got])
        e1.set_beam_merge(False)                                # 2 -> 0
        refused(N.LASR_ESTATE, e1.set_beam_merge, True)         # 0 -> 1 with an LM: as before
        e1.set_beam_merge(True, lm=True)                        # 0 -> 2 with an LM attached
        same_bits([beam_of(e1)], [got])
    finally:
        e1.close()
    e2 = Engine(sd, cfg, max_streams=2, beam=W)                 # 1 -> 2 without an LM, then the LM
    try:
        e2.set_beam_records(True)
        e2.set_beam_merge(True)
        refused(N.LASR_ESTATE, lambda: e2.attach_lm(lm, int8=False))     # mode 1 still refuses
        e2.set_beam_merge(True, lm=True)
        e2.attach_lm(lm, int8=False)
        same_bits([beam_of(e2)], [got])
    finally:
        e2.close()
    greedy = Engine(sd, cfg, max_streams=2)
    try:
        refused(N.LASR_EINVAL, greedy.set_beam_merge, True, lm=True)
    finally:
        greedy.close()
    eng, _ = engine(name, W)                                    # a switch with an uncollected step
    chunks = L.stream_inputs()[0]
    s = eng.open()
    k = 0
    while not eng.pending():
        eng.push_submit([s], chunks[k][None])
        k += 1
    refused(N.LASR_ESTATE, eng.set_beam_merge, False)
    refused(N.LASR_ESTATE, eng.set_beam_merge, True)            # (2 -> 1: refused for the LM before anything else)
    eng.set_beam_merge(True, lm=True)                           # (changes nothing: fine while a step is in flight)
    assert eng.wait() == 1
    refused(N.LASR_ESTATE, eng.set_beam_merge, False)           # collected, not fetched
    assert len(eng.fetch_nbest(s)) >= 1
    eng.close_slot(s)
    same_bits([beam_of(eng)], [got])


# ------------------------------------------------------------------------------- 7. bf16: structure
def test_bf16_beams_are_distinct_and_well_formed():
    name, W = "tiny", 4
    ref = L.offline_ref(name, W, 3, True, 31)
    for i, got in enumerate(offline_run(name, W, seed=31, dtype="bf16")):
        check_structure(got, ref[i]["T"], W, 3, (name, W, "bf16", i))
        distinct(got, (name, W, "bf16", i))
        print((name, W, "bf16", i), "live", len(got), "scores", [round(h[3], 4) for h in got], "f32 restatement", [round(h[3], 4) for h in ref[i]["beam"]])


# ------------------------------------------------------------------------------- 8. the facade
def test_libreasr_facade_merge_lm():
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", synthetic="tiny", synthetic_lm=L.LM, max_streams=4, beam=4)
    try:
        pcm = R.offline_pcm("tiny", 31)[0]
        ref = L.offline_ref("tiny", 4, 3, True, 31)[0]
        with pytest.raises(N.LasrError):
            asr.transcribe(pcm, nbest=4, merge=True)            # mode 1 still refuses the LM
        out = asr.transcribe(pcm, nbest=4, merge="lm")
        ys = [tuple(t for t, _, _ in h["tokens"]) for h in out]
        assert len(out) == 4 and len(set(ys)) == 4
        assert list(ys[0]) == ref["beam"][0][0]
        assert abs(out[0]["score"] - ref["beam"][0][3]) < 2e-3 * max(1.0, abs(ref["beam"][0][3]))
        n = 0
        for beam in asr.stream(L.stream_inputs()[1], nbest=4, merge="lm"):
            ys = [tuple(t for t, _, _ in h["tokens"]) for h in beam]
            assert len(set(ys)) == len(ys)
            n += 1
        assert n == 21
        off = asr.transcribe(pcm, nbest=4, merge=False)
        ys = [tuple(t for t, _, _ in h["tokens"]) for h in off]
        assert len(set(ys)) < len(ys)                           # (2 distinct lists of 4 without merging)
    finally:
        asr.engine.close()
