"""Beam search on the GPU with lasr_set_beam_merge on: hypotheses that hold the same tokens are merged.

Expected values: tests/beam_merge_ref.py (pinned on the CPU in tests/test_beam_merge_cpu.py).  Compared rank by rank under the margin
rule of tests/test_gpu_beam_records.py: tokens and frames equal, log p within 1e-3, scores within 2e-3 * max(1, |score|); a case the
CPU test counted below the margin (at most 2 offline, 2 streamed) is compared in full up to its first model step below 1e-3 and by
rank 0 + structure from there.  The largest differences seen are printed.

(a) fails without the feature: merge on, the token lists of every final beam are pairwise distinct; a twin with merge off holds
duplicates in the named cases."""
import copy

import numpy as np
import pytest

import beam_merge_ref as M
import beam_records_ref as R
from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O
from test_gpu_beam_records import check_beam, check_structure, drive

pytestmark = pytest.mark.gpu

_ENGINES, _OFFLINE = {}, {}
WORST = {"logp": 0.0, "score": 0.0}


def engine(name, W, dtype="f32", merge=True, max_iters_offline=3):
    """(engine, oracle): records on; merge: the switch's state when the engine is made (tests that toggle put it back)"""
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    key = (name, W, dtype, merge, max_iters_offline)
    if key not in _ENGINES:
        graft.build()
        m, sd, cfg = R.model(name)
        eng = Engine(sd, cfg, max_streams=8, beam=W, dtype=dtype, max_iters_offline=max_iters_offline)
        eng.set_beam_records(True)
        if merge:
            eng.set_beam_merge(True)
        _ENGINES[key] = (eng, m)
    return _ENGINES[key]


def offline_run(name, W, merge=True, dtype="f32", max_iters_offline=3):
    """the final beams of the offline utterances, once per (engine): [fetch_nbest per utterance]"""
    key = (name, W, merge, dtype, max_iters_offline)
    if key not in _OFFLINE:
        eng, _ = engine(name, W, dtype, merge, max_iters_offline)
        pcm = R.offline_pcm(name)
        slots = [eng.open() for _ in range(len(pcm))]
        eng.transcribe_pcm(slots, [pcm[i] for i in range(len(pcm))])
        _OFFLINE[key] = [eng.fetch_nbest(s) for s in slots]
        for s in slots:
            eng.close_slot(s)
    return _OFFLINE[key]


def distinct(beam, what):
    ys = [tuple(h[0]) for h in beam]
    assert len(set(ys)) == len(ys), (what, "the beam holds a token list twice", ys)


def note(got, ref, n):
    """the largest differences of the ranks compared (printed; the bounds themselves are check_rank's)"""
    for (_, _, lp, sc), (_, _, rl, rs) in list(zip(got, ref))[:n]:
        if rl:
            WORST["logp"] = max(WORST["logp"], float(np.abs(np.asarray(lp, np.float64) - np.asarray(rl)).max()))
        WORST["score"] = max(WORST["score"], abs(sc - rs) / max(1.0, abs(rs)))


def compare(got, ref_beam, full, what):
    check_beam(got, ref_beam, full, what)
    note(got, ref_beam, len(ref_beam) if full else 1)


# ------------------------------------------------------------------------------- (a) fails without the feature
DUPLICATES_WITHOUT = {("tiny", 8): [0, 1, 2], ("tiny", 4): [0, 2], ("tiny", 2): [1]}


@pytest.mark.parametrize("name,W", M.SHAPES)
def test_offline_final_beams_are_pairwise_distinct(name, W):
    for i, beam in enumerate(offline_run(name, W)):
        distinct(beam, (name, W, "utt", i))
    off = offline_run(name, W, merge=False)
    for i in DUPLICATES_WITHOUT.get((name, W), []):                 # the inputs exercise the rule
        ys = [tuple(h[0]) for h in off[i]]
        assert len(set(ys)) < len(ys), (name, W, i, "no duplicate without merging: the case pins nothing")


# ------------------------------------------------------------------------------- (b) parity with the restatement
@pytest.mark.parametrize("name,W", M.SHAPES)
def test_offline_parity_rank_by_rank(name, W):
    ref = M.offline_ref(name, W)
    for i, got in enumerate(offline_run(name, W)):
        what = (name, W, "utt", i)
        check_structure(got, ref[i]["T"], W, 3, what)
        full = ref[i]["margin"] >= M.MARGIN
        print(f"{what}: {len(got)} hypotheses, {ref[i]['merges']} merges, oracle margin {ref[i]['margin']:.2e}{'' if full else ' -> rank 0 + structure'}")
        compare(got, ref[i]["beam"], full, what)
    print(f"largest differences so far: log p {WORST['logp']:.2e}, score (relative to max(1, |score|)) {WORST['score']:.2e}")


def compare_step(got, ref_stream, j, W, what):
    check_structure(got, ref_stream["T"][j], W, 10, what)
    distinct(got, what)
    if j >= ref_stream["speech"]:
        return
    full = j < M.full_upto(ref_stream)
    if not full:
        print(f"{what}: oracle margin {ref_stream['margin'][j]:.2e} (first below at step {M.full_upto(ref_stream)}) -> rank 0 + structure")
    compare(got, ref_stream["steps"][j], full, what)


def reset_then_continue(eng, twin, slot, tslot, ref0, frozen, name, W, pipelined):
    """predictor reset: the best hypothesis is frozen, the identities restart with the beam, the frame count runs on.  The
    restatement goes on from the same state (its front-end is not reset, like the engine's: bits 1 | 2 | 4)."""
    eng.reset(slot, 1 | 2 | 4)
    twin.reset(tslot, 1 | 2 | 4)
    dec, fe = ref0["dec"].clone(), copy.deepcopy(ref0["fe"])
    dec.reset()
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
        ok = ok and dec.step_margin[-1] >= M.MARGIN
        if ok:
            compare(beam, want, True, what)
        n_after += 1
    assert max(len(h[0]) for h in beam) > k0, "no token after the reset: the frozen prefix was not continued"
    assert n_after >= 4


def run_streams(name, W, pipelined):
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, merge=False)
    ref = M.stream_ref(name, W)
    slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]
    hist = [[] for _ in range(3)]
    kind = "pipelined" if pipelined else "synchronous"

    def on_step(i, beam, fetched):
        compare_step(beam, ref[i], len(hist[i]), W, (name, W, kind, "stream", i, "step", len(hist[i])))
        hist[i].append(beam)

    drive(eng, twin, slots, tslots, R.stream_inputs(), pipelined, on_step)
    assert [len(h) for h in hist] == [21, 21, 21]
    assert eng.pending() == 0 and twin.pending() == 0
    reset_then_continue(eng, twin, slots[0], tslots[0], ref[0], hist[0][-1][0], name, W, pipelined)
    for s in slots:
        eng.close_slot(s)
    for s in tslots:
        twin.close_slot(s)
    print(f"largest differences so far: log p {WORST['logp']:.2e}, score (relative to max(1, |score|)) {WORST['score']:.2e}")


@pytest.mark.parametrize("name,W", M.SHAPES)
def test_synchronous_streaming_parity_per_model_step_then_reset(name, W):
    run_streams(name, W, False)


@pytest.mark.parametrize("name,W", M.SHAPES)
def test_pipelined_parity_per_collected_model_step_then_reset(name, W):
    run_streams(name, W, True)


# ------------------------------------------------------------------------------- (c) merge off is today
@pytest.mark.parametrize("pipelined", [False, True])
def test_toggling_every_third_step_follows_the_restatement_toggled_at_the_same_steps(pipelined):
    """on -> off -> on every third model step: the decode groups are cached graphs that captured BeamState by value, and a
    switch-on in mid-stream takes the slots' identities from the host's trees.  The restatement toggles at the same steps (in its
    off regions it is the records-only restatement continued from the same state); the twin that never heard of the switch runs
    beside it and must equal the records-only restatement's tokens throughout."""
    name, W = "tiny", 4
    eng, _ = engine(name, W)
    twin, _ = engine(name, W, merge=False)
    plain = R.stream_ref(name, W)
    eng.set_beam_merge(False)
    state = {"on": False}
    sched, hist, thist = [[] for _ in range(3)], [[] for _ in range(3)], [[] for _ in range(3)]
    try:
        slots, tslots = [eng.open() for _ in range(3)], [twin.open() for _ in range(3)]

        def on_step(i, beam, fetched):
            sched[i].append(state["on"])
            hist[i].append(beam)
            thist[i].append(fetched)

        def toggle():
            state["on"] = not state["on"]
            eng.set_beam_merge(state["on"])

        drive(eng, twin, slots, tslots, R.stream_inputs(), pipelined, on_step, every_third=toggle)
        for s in slots:
            eng.close_slot(s)
        for s in tslots:
            twin.close_slot(s)
    finally:
        eng.set_beam_merge(True)
    assert [len(h) for h in hist] == [21, 21, 21]
    n_on = sum(sum(s) for s in sched)
    assert 20 <= n_on <= 45, sched
    ref = M.stream_run(name, W, merge_at=lambda i, j: sched[i][j])
    for i in range(3):
        for j in range(21):
            what = (name, W, "pipelined" if pipelined else "synchronous", "toggled stream", i, "step", j, "on" if sched[i][j] else "off")
            check_structure(hist[i][j], ref[i]["T"][j], W, 10, what)
            if j < ref[i]["speech"]:
                compare(hist[i][j], ref[i]["steps"][j], j < M.full_upto(ref[i]), what)
                # the twin: the best hypothesis of the records-only restatement (rank 0 is pinned without exception)
                assert thist[i][j][0] == plain[i]["steps"][j][0][0], what


def test_an_engine_switched_off_again_is_bit_equal_to_one_never_switched():
    name, W = "tiny", 8
    eng, _ = engine(name, W)
    never = offline_run(name, W, merge=False)
    pcm = R.offline_pcm(name)
    eng.set_beam_merge(False)
    try:
        slots = [eng.open() for _ in range(3)]
        eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
        got = [eng.fetch_nbest(s) for s in slots]
        for s in slots:
            eng.close_slot(s)
    finally:
        eng.set_beam_merge(True)
    for a, b in zip(got, never):
        assert len(a) == len(b)
        for (t, f, lp, sc), (t2, f2, lp2, sc2) in zip(a, b):
            assert t == t2 and list(f) == list(f2) and np.array_equal(lp, lp2) and sc == sc2


# ------------------------------------------------------------------------------- (d) cross-check with the lattice
def test_merged_scores_stay_below_the_lattice_total_and_exceed_the_unmerged():
    from libreasr_amd.engine import Engine
    gains, checked = [], 0
    for name, W in M.SHAPES:
        m, sd, cfg = R.model(name)
        ref = M.offline_ref(name, W, max_iters=10)
        got = offline_run(name, W, max_iters_offline=10)
        off = offline_run(name, W, merge=False, max_iters_offline=10)
        pcm = R.offline_pcm(name)
        greedy = Engine(sd, cfg, max_streams=8)
        try:
            for i in range(3):
                what = (name, W, "max_iters 10, utt", i)
                check_structure(got[i], ref[i]["T"], W, 10, what)
                distinct(got[i], what)
                full = ref[i]["margin"] >= M.MARGIN
                compare(got[i], ref[i]["beam"], full, what)
                use = [k for k in range(len(ref[i]["beam"]) if full else 1) if not ref[i]["capped"][k]]
                if use:
                    slots = [greedy.open() for _ in use]
                    res = greedy.align_pcm(slots, [pcm[i]] * len(use), [got[i][k][0] for k in use], viterbi=False)
                    for s in slots:
                        greedy.close_slot(s)
                    for k, r in zip(use, res):
                        ll = float(r["loglik"])
                        assert got[i][k][3] <= ll + 2e-3 * max(1.0, abs(ll)), (what, k, got[i][k][3], ll)
                        checked += 1
                if got[i][0][0] == off[i][0][0]:
                    gains.append((name, W, i, got[i][0][3], off[i][0][3]))
        finally:
            greedy.close()
    print("rank 0, merged against unmerged score:", [(n, w, i, round(a, 3), round(b, 3)) for n, w, i, a, b in gains])
    assert checked > 0
    assert any(a - b > 1e-2 for _, _, _, a, b in gains), gains


# ------------------------------------------------------------------------------- (e) other widths and dtype
def test_cfg2_width_8_fills_every_register_slot():
    name, W = "cfg2", 8
    ref = M.offline_ref(name, W)[0]
    got = offline_run(name, W)[0]
    what = (name, W)
    check_structure(got, ref["T"], W, 3, what)
    distinct(got, what)
    print(f"{what}: {len(got)} hypotheses, {ref['merges']} merges in the restatement, oracle margin {ref['margin']:.2e}")
    compare(got, ref["beam"], False, what)


def test_bf16_beams_are_distinct_and_well_formed():
    name, W = "tiny", 4
    for i, got in enumerate(offline_run(name, W, dtype="bf16")):
        check_structure(got, M.offline_ref(name, W)[i]["T"], W, 3, (name, W, "bf16", i))
        distinct(got, (name, W, "bf16", i))
        print((name, W, "bf16", i), "scores", [round(h[3], 4) for h in got], "f32 restatement", [round(h[3], 4) for h in M.offline_ref(name, W)[i]["beam"]])


# ------------------------------------------------------------------------------- (f) errors
def test_errors_leave_the_engine_as_it_was():
    from libreasr_amd.engine import Engine
    name, W = "tiny", 4
    m, sd, cfg = R.model(name)
    pcm = R.offline_pcm(name)[1]
    want = M.offline_ref(name, W)[1]["beam"][0][0]

    def unchanged(e, toks):
        s = e.open()
        e.transcribe_pcm([s], [pcm])
        assert e.fetch(s)[0] == toks
        e.close_slot(s)

    def refused(code, f, *a):
        with pytest.raises(N.LasrError) as ei:
            f(*a)
        assert ei.value.code == code, (ei.value.code, code)

    greedy = Engine(sd, cfg, max_streams=2)
    try:
        refused(N.LASR_EINVAL, greedy.set_beam_merge, True)
        refused(N.LASR_EINVAL, greedy.set_beam_merge, False)
        unchanged(greedy, m.decode_greedy(O.features_offline(pcm))[0])
    finally:
        greedy.close()
    eng, _ = engine(name, W)
    chunks = R.stream_inputs()[0]
    s = eng.open()
    k = 0
    while not eng.pending():
        eng.push_submit([s], chunks[k][None])
        k += 1
    refused(N.LASR_ESTATE, eng.set_beam_merge, False)               # a submitted step is uncollected
    eng.set_beam_merge(True)                                        # (changes nothing: fine while a step is in flight)
    assert eng.wait() == 1
    refused(N.LASR_ESTATE, eng.set_beam_merge, False)               # collected, not fetched
    assert len(eng.fetch_nbest(s)) >= 1
    eng.close_slot(s)
    unchanged(eng, want)
    # not with an LM: attached, then on; on, then attach (both forms)
    lm = synth.synth_lm_state_dict("tiny_lm")
    e2 = Engine(sd, cfg, max_streams=2, beam=W)
    try:
        e2.set_beam_merge(True)
        refused(N.LASR_ESTATE, e2.attach_lm, lm)
        refused(N.LASR_ESTATE, lambda: e2.attach_lm(lm, int8=True))
        unchanged(e2, want)                                         # still merging, still no LM
        e2.set_beam_merge(False)
        e2.attach_lm(lm)
        s = e2.open()
        e2.transcribe_pcm([s], [pcm])
        with_lm = e2.fetch(s)[0]
        e2.close_slot(s)
        refused(N.LASR_ESTATE, e2.set_beam_merge, True)
        e2.set_beam_merge(False)                                    # (changes nothing)
        unchanged(e2, with_lm)
    finally:
        e2.close()


# ------------------------------------------------------------------------------- (g) the facade
def test_libreasr_facade_merge():
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", synthetic="tiny", max_streams=4, beam=8)
    try:
        pcm = R.offline_pcm("tiny")[0]
        ref = M.offline_ref("tiny", 8)[0]
        off = asr.transcribe(pcm, nbest=8)
        ys = [tuple(t for t, _, _ in h["tokens"]) for h in off]
        assert len(set(ys)) < len(ys)                               # default off: the beam of today, with its duplicates
        out = asr.transcribe(pcm, nbest=8, merge=True)
        ys = [tuple(t for t, _, _ in h["tokens"]) for h in out]
        assert len(set(ys)) == len(ys) and list(ys[0]) == ref["beam"][0][0]
        assert abs(out[0]["score"] - ref["beam"][0][3]) < 2e-3 * max(1.0, abs(ref["beam"][0][3]))
        again = asr.transcribe(pcm, nbest=8)                        # None: the engine keeps the setting
        assert [h["score"] for h in again] == [h["score"] for h in out]
        n = 0
        for beam in asr.stream(R.stream_inputs()[1], nbest=8, merge=True):
            ys = [tuple(t for t, _, _ in h["tokens"]) for h in beam]
            assert len(set(ys)) == len(ys)
            n += 1
        assert n == 21
        back = asr.transcribe(pcm, nbest=8, merge=False)
        assert [h["score"] for h in back] == [h["score"] for h in off]
    finally:
        asr.engine.close()
    greedy = LibreASR.load("en", synthetic="tiny", max_streams=4)
    try:
        with pytest.raises(ValueError):
            greedy.transcribe(R.offline_pcm("tiny")[0], merge=True)
        with pytest.raises(ValueError):
            next(greedy.stream([np.zeros(1280, np.float32)], merge=False))
    finally:
        greedy.engine.close()
