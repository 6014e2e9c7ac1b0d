"""The conditions under which test_gpu_decision_edges.py means something, asserted on the numpy oracle alone: on the crafted models of
decision_edges.py and the utterances the GPU tests decode, the tie groups really win, the blank is neither rare nor dominant, the
per-frame symbol cap is reached (also on a frame that is not the first of a lookahead window) and no decision is closer than
MIN_MARGIN to one the GPU may legitimately take differently.  These are conditions, not measurements; the figures are printed.

A "run" is one decode of both utterances in one configuration (offline at one cap; two streams at one cap with or without a reset);
every run the GPU tests compare is checked by check_run on its own: a run in which a tie group never won would leave the GPU
comparison of that run vacuous for that group's boundary."""
import numpy as np
import pytest

import decision_edges as D

IDS = [f"{n}-V{v}-blank{b}" for n, v, b in D.MODELS]


def check_run(mod, runs, cap, what, blank_wins=True):
    """the conditions every run has to meet; -> its events"""
    ev = D.events(mod, runs, cap)
    print(f"{what}: {ev['n']} evaluations, {sum(len(r.tokens) for r in runs)} tokens, wins {list(ev['wins'].values())}, blank share "
          f"{ev['blank_share']:.2f}, frames {ev['frames']} emitting {ev['emitting']} capped {ev['capped']} (odd frame "
          f"{ev['capped_odd']}), min margin {ev['min_margin']:.4f}")
    assert ev["copies_equal"], what                              # copies are bit-equal to their source in the oracle's logits
    assert min(ev["wins"].values()) >= 2, (what, ev["wins"])     # every tie group wins at least 2 evaluations ...
    assert ev["lowest"], what                                    # ... each decided for the group's lowest index
    assert ev["min_margin"] >= D.MIN_MARGIN, what
    if blank_wins:
        assert 0.3 <= ev["blank_share"] <= 0.9, what
    assert ev["emitting"] > 0
    if cap == 1:
        assert ev["capped"] == ev["emitting"], what              # every emitting frame reaches the cap
    if cap == 2:
        assert ev["capped"] >= 5, what
    if cap >= 2 and blank_wins:
        assert ev["uncapped_emitting"] >= 1, what
    return ev


def offline_checks(mod, what):
    for cap in D.OFFLINE_CAPS:
        ev = check_run(mod, D.offline(mod, cap), cap, f"{what} offline cap {cap}")
        if cap == 2:
            assert ev["capped_odd"] >= 1                         # ... also behind a blank frame of the same lookahead window


def stream_checks(mod, what):
    for cap, reset in D.STREAM_RUNS:
        runs = D.stream_run(mod, cap, reset)
        check_run(mod, runs, cap, f"{what} streams cap {cap} reset {reset}")
        assert sum(len(r.tokens) for r in runs) >= 20
        for row, at in reset.items():
            r = runs[row]
            assert len(r.steps) > at + 2 and sum(len(s[0]) for s in r.steps[at:]) >= 5          # tokens behind the reset


def tie_checks(key):
    mod, plus, minus = D.model(*key), D.model(*key, "plus"), D.model(*key, "minus")
    assert plus.blank_bias == minus.blank_bias == mod.blank_bias
    for tm, j in ((plus, mod.blank + 1), (minus, mod.blank - 1)):
        b, w = tm.sd["joint.joint.2.bias"], tm.sd["joint.joint.2.weight"]
        assert b[j] == b[mod.blank] and not w[j].any()
        check_run(tm, D.offline(tm, 2), 2, f"{key} {tm.tie} offline cap 2", blank_wins=tm is plus)
        check_run(tm, D.stream_run(tm, 2), 2, f"{key} {tm.tie} streams cap 2", blank_wins=tm is plus)
    # blank + 1: never emitted, the same tokens as the plain model
    for a, b in zip(D.offline(plus, 2) + D.stream_run(plus, 2), D.offline(mod, 2) + D.stream_run(mod, 2)):
        assert a.tokens == b.tokens and a.frames == b.frames and mod.blank + 1 not in a.tokens
    # blank - 1: wins every tie with the blank, so no frame ends on a blank: every frame reaches the cap, and the token is emitted
    # on at least half of them
    for runs in (D.offline(minus, 2), D.stream_run(minus, 2)):
        frames = sum(len(r.evals) for r in runs)
        hit = sum(1 for r in runs for t in range(len(r.evals)) if mod.blank - 1 in [k for k, f in zip(r.tokens, r.frames) if f == t])
        print(f"blank - 1 variant: {hit} of {frames} frames emit the tie row; all reach the cap")
        assert all(e == 2 for r in runs for e in r.evals)
        assert 2 * hit >= frames
        assert D.events(minus, runs, 2)["blank"] == 0


def lm_checks(int8):
    mod = D.model(*D.LM_MODEL)
    for kind, (runs, picks), plain in (("offline", D.lm_offline(int8), D.offline(mod, 3)),
                                       ("streams", D.lm_stream(int8), D.stream_run(mod, 3))):
        ev = check_run(mod, runs, 3, f"LM int8={int8} {kind}")
        flat = [p for ps in picks for p in ps]
        changed = sum(1 for a, b, _ in flat if a != b)
        print(f"LM int8={int8} {kind}: {len(flat)} fused decisions, {changed} re-picked, min fused margin {min(g for _, _, g in flat):.4f}, "
              f"min joint margin {ev['min_margin']:.4f}")
        assert changed >= 3
        assert sum(1 for r, q in zip(runs, plain) for a, b in zip(r.tokens, q.tokens) if a != b) >= 3
        assert all(b not in (0, mod.blank) for _, b, _ in flat)
        assert min(g for _, _, g in flat) >= D.LM_MIN_MARGIN


def beam_checks(W, kinds=("offline", "streams")):
    for kind in kinds:
        mod = D.beam_model(W, kind)
        assert mod.blank == 7 and [len(g) for g in mod.groups] == [2, 2, 2, 2]
        runs = D.beam_offline(W) if kind == "offline" else D.beam_stream(W)
        gaps = [g for u in runs for g in u["gaps"]]
        print(f"beam W {W} {kind}: {sum(u['pairs'] for u in runs)} surviving pairs, {sum(u['ties'] for u in runs)} still tied at the end of "
              f"their frame, {sum(1 for g in gaps if g == 0)} exact ties among {len(gaps)} gaps, smallest other gap "
              f"{min(g for g in gaps if g != 0):.5f}")
        assert sum(u["pairs"] for u in runs) >= 1 and sum(u["ties"] for u in runs) >= 1
        assert min(g for g in gaps if g != 0) >= D.BEAM_MARGIN
        beams = [[u["beam"]] if kind == "offline" else u["steps"] for u in runs]
        assert all(len(b[-1]) == W for b in beams) and sum(len(b[-1][0][0]) for b in beams) >= 16
        beams = [b for u in beams for b in u]
        assert all(mod.blank not in h[0] for b in beams for h in b)              # the blank never appears in a hypothesis


@pytest.mark.parametrize("key", D.MODELS, ids=IDS)
def test_offline_conditions(key):
    mod = D.model(*key)
    assert mod.m.blank == key[2] != 0 and mod.m.bos == 1
    w, b = mod.sd["joint.joint.2.weight"], mod.sd["joint.joint.2.bias"]
    assert not w[mod.blank].any() and w[0].any()                   # the constant row sits at `blank`, entry 0 is a token
    for g in mod.groups:
        for j in g[1:]:
            assert np.array_equal(w[j], w[g[0]]) and b[j] == b[g[0]]
    offline_checks(mod, key)


@pytest.mark.parametrize("key", D.MODELS[::2], ids=IDS[::2])
def test_states_replay_the_decode(key):
    """decision_edges.states (the op-level joint test's inputs) is the oracle's own decode: same logits, and groups win on its rows"""
    mod = D.model(*key)
    hp, he, zs = D.states(mod, 2)
    assert hp.shape == he.shape == (64, 64) and zs.shape == (64, mod.V)
    outs = [z for r in D.offline(mod, 2) for z in r.outs]
    for z in zs:
        assert any(np.array_equal(z, o) for o in outs)
    lp, z2 = mod.m.joint_logp(hp, he)
    member = {j for g in mod.groups for j in g}
    won = [int(a) for a in z2.argmax(-1) if int(a) in member]
    assert {a for a in won} == {g[0] for g in mod.groups}          # every group wins a row, decided for its lowest index
    assert all(won.count(g[0]) >= 2 for g in mod.groups)
    assert min(D.margin(z) for z in z2) >= D.MIN_MARGIN


@pytest.mark.parametrize("key", D.STREAM_MODELS, ids=IDS[:2])
def test_stream_conditions(key):
    stream_checks(D.model(*key), key)


def test_blank_tie_variants():
    tie_checks(D.TIE_MODEL)


def test_rand_labels_avoid_the_blank_and_reach_zero():
    mod = D.model(*D.MODELS[0])
    y = D.rand_labels(mod, 40000, 0)
    assert mod.blank not in y and min(y) == 0 and max(y) == mod.V - 1
    assert mod.blank - 1 in y and mod.blank + 1 in y


@pytest.mark.parametrize("int8", [False, True], ids=["fp32", "int8"])
def test_lm_fusion_conditions(int8):
    """offline and streamed: every tie group still wins, the re-pick runs and differs from the joint's token, entry 0 (MIN_VAL) is
    never picked although it is a token here, and no fused decision is closer than LM_MIN_MARGIN; the joint's own decisions keep
    MIN_MARGIN on the path the fused tokens lead to"""
    lm_checks(int8)


@pytest.mark.parametrize("W", D.BEAM_WIDTHS)
def test_beam_conditions(W):
    """blank 7, cap 2, the V = 2048 tie groups, offline and streamed: rounds in which two members of a group both survive exist, some
    of them still with bit-equal scores at the end of the frame (then the lower token holds the lower slot); every other selection
    is decided by at least BEAM_MARGIN"""
    beam_checks(W)
