"""tests/f32_exact.py is right, and it bites (no GPU): the float32 evaluation of its yardstick is the numpy oracle's bit for bit, the
float64 model lies within its own bound of it, nine subtly wrong kernels are rejected in every model, and the K schedule each GPU
case is said to reach is the one gemm_body's list gives it."""
import numpy as np
import pytest

import f32_exact as S
from bf16_exact import StandIn, bf16_trunc

ROWS = 17       # rows of the CPU cases: an m-tile and one row (the GPU cases have their own)


def inputs(name):
    """the 17-row cases of the GPU file: two frames, two tokens, the joint"""
    return S.case("enc", name, ROWS, 2)[0], S.case("pred", name, ROWS, 2)[0], S.case("joint", name, ROWS)[0]


def traces(name):
    return dict(enc=S.case("enc", name, ROWS, 2)[1], pred=S.case("pred", name, ROWS, 2)[1], joint=S.case("joint", name, ROWS)[1])


@pytest.mark.parametrize("name", S.MODELS)
def test_stand_in_is_the_oracle(name):
    """StandIn on an operand="f32" oracle is OracleTransducer.encoder / .predictor / .joint_logp, bit for bit, and the stage it
    names ".pre" is the stage itself (nothing is rounded)"""
    m = S.model(name)[0]
    o, s = m.o, m.ref
    x, toks, (a, b) = inputs(name)
    e = s.encoder(x)
    out, st = o.encoder(x)
    L = o.Le
    assert np.array_equal(e[f"enc{L - 1}.y"], out)
    for l in range(L):
        assert np.array_equal(e[f"enc{l}.t1.h"], st[l][0]) and np.array_equal(e[f"enc{l}.t1.c"], st[l][1])
    p = s.predictor(toks)
    stp = None
    for u in range(2):
        y, stp = o.predictor(toks[:, u], stp)
    assert np.array_equal(p[f"pred{o.Lp - 1}.u1.y"], y)
    for l in range(o.Lp):
        assert np.array_equal(p[f"pred{l}.u1.h"], stp[l][0] if o.pred_lstm else stp[l])
        if o.pred_lstm:
            assert np.array_equal(p[f"pred{l}.u1.c"], stp[l][1])
    j = s.joint(a, b)
    lp, z = o.joint_logp(a, b)
    assert np.array_equal(j["logits"], z) and np.array_equal(j["lp"], lp.max(-1))
    for d in (e, p, j):
        for k in d:
            if k.endswith(".pre"):
                assert np.array_equal(d[k], d[k[:-4]]), k


@pytest.mark.parametrize("name", S.MODELS)
def test_model_against_oracle(name):
    """every stage of the oracle lies within tol of the float64 model (Y <= 8 Y: this pins the plumbing), no stage carries a flip
    or a tie mask, and tol is the rule's: 8 Y or the floor of 4 ulps"""
    for part, tr in traces(name).items():
        worst = 0.0
        for k, s in tr.items():
            r = s.ratio(s.ref32)
            worst = max(worst, r)
            assert r <= 1.0, (name, k, r)
            assert s.tie is None and not s.flip.any() and s.tol > 0
            if k != "lp":
                floor = S.FLOOR_ULPS * float(np.spacing(np.float32(np.abs(s.value).max())))
                assert s.tol == max(S.MARGIN * s.Y, floor), k
                assert s.Y == float(np.abs(s.ref32.astype(np.float64) - s.value).max()), k
        if part == "joint":
            assert tr["lp"].tol == tr["logits"].tol + tr.tol_reduction
        print(f"{name} {part}: worst |oracle - model| / tol {worst:.3g}; Y " + ", ".join(f"{k} {s.Y:.2g}" for k, s in tr.items()))


# ----------------------------------------------------------------------------- sensitivity
ENC_SEEN = lambda L, T: ["x0"] + [f"enc{l}.t{T - 1}.{k}" for l in range(L) for k in ("c", "h")] + [f"enc{L - 1}.y"]
PRED_SEEN = lambda L, U: [f"pred{l}.u{U - 1}.h" for l in range(L)] + [f"pred{L - 1}.u{U - 1}.y"]
JOINT_SEEN = ["pp", "pe", "logits", "lp"]

MUTATIONS = {
    "a_activations_truncated_to_bf16": dict(q=bf16_trunc),
    "b_recurrent_k_tail_dropped": dict(weights="k_tail"),
    "c_k_chunk_dropped": dict(weights="chunk_dropped"),
    "c_k_chunk_twice": dict(weights="chunk_twice"),
    "d_layer0_operand_13_bits_cleared": dict(weights="tf32"),
    "e_bias_twice_in_pp": dict(weights="bias_twice"),
    "f_second_step_on_the_initial_cell_state": dict(stale_c_t=1),
}
# the parts of the model in which the fault must show (it touches no other: (d) is encoder layer 0, (e) the joint; (f) needs a cell
# state, which the NBRC predictor does not have)
CAUGHT_IN = {
    "a_activations_truncated_to_bf16": lambda lstm: ("enc", "pred", "joint"),
    "b_recurrent_k_tail_dropped": lambda lstm: ("enc", "pred"),
    "c_k_chunk_dropped": lambda lstm: ("enc", "pred", "joint"),
    "c_k_chunk_twice": lambda lstm: ("enc", "pred", "joint"),
    "d_layer0_operand_13_bits_cleared": lambda lstm: ("enc",),
    "e_bias_twice_in_pp": lambda lstm: ("joint",),
    "f_second_step_on_the_initial_cell_state": lambda lstm: ("enc", "pred") if lstm else ("enc",),
}


@pytest.mark.parametrize("name", S.MODELS)
@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_is_caught(mut, name):
    """a copy of the float32 oracle's stages with one fault, playing the kernel: at least one element of one stage the GPU tests
    read lands outside tol, in every part of the model the fault touches"""
    m, _, cfg = S.model(name)
    kw = dict(MUTATIONS[mut])
    o = S.mutated(m.o, kw.pop("weights")) if "weights" in kw else m.o
    bad = StandIn(o, **kw)
    x, toks, (a, b) = inputs(name)
    tr = traces(name)
    got = dict(enc=bad.encoder(x), pred=bad.predictor(toks), joint=bad.joint(a, b))
    seen = dict(enc=ENC_SEEN(cfg["enc_layers"], 2), pred=PRED_SEEN(cfg["pred_layers"], 2), joint=JOINT_SEEN)
    over = {}
    for part in ("enc", "pred", "joint"):
        for k in seen[part]:
            s = tr[part][k]
            d = np.abs(got[part][k].astype(np.float64) - s.value)
            if (d > s.tol).any():
                over[f"{part}:{k}"] = f"{int((d > s.tol).sum())} (worst {float(d.max() / s.tol):.3g} tol)"
    print(f"{mut} on {name}: elements outside the bound {over}")
    for part in CAUGHT_IN[mut](cfg["pred_cell"] == "LSTM"):
        assert any(k.startswith(part + ":") for k in over), (mut, name, part, over)


# ----------------------------------------------------------------------------- the K schedule
UNREACHED = set()       # entries of the f32 list that no GPU case runs (docs/f32_bound.md names the reason for each)


def test_schedule_of_every_gpu_case():
    """the static entry each GPU case names is the one the restated list gives its (launcher, model, wave count), and every entry
    of the f32 list is run by at least one case"""
    reached = {}
    for what, launcher, name, nw, want in S.gpu_schedules():
        assert S.schedule(launcher, name, nw) == want, (what, S.schedule(launcher, name, nw), want)
        for e in want:
            if e is not None:
                reached.setdefault(e, []).append(f"{what} ({nw} waves)")
    for e in S.F32_TRY:
        print(f"{e}: " + ("; ".join(reached[e]) if e in reached else "no GPU case"))
    assert set(S.F32_TRY) - set(reached) == UNREACHED
    # the dynamic loop is run too, with idle waves (4 chunks on 8 waves) and with a tail in the split (6 chunks on 4 and on 8)
    assert S.schedule("pred_cell", "tiny", 8) == [None, None] and S.launches("pred_cell", S.model_cfg("tiny"))[1] == (4, 4)
    assert S.schedule("enc_cell", "d96", 4) == [None, None] and S.launches("enc_cell", S.model_cfg("d96"))[1] == (6, 6)


def test_static_entry_is_first_fit():
    """the list as gemm_body reads it: both phases must fit where the epilogue has both, an absent phase fits anything, the first
    entry wins, anything else is the dynamic loop"""
    assert S.static_entry(80, 64, 4) == (20, 16) and S.static_entry(80, 64, 8) == (10, 8)
    assert S.static_entry(64, 64, 4) == (16, 16) and S.static_entry(64, 64, 8) == (8, 8)
    assert S.static_entry(80, 96, 8) == (10, 12) and S.static_entry(96, 96, 8) == (12, 12)
    assert S.static_entry(None, 64, 8) == (8, 8) and S.static_entry(64, None, 4) == (16, 16)
    assert S.static_entry(80, 96, 4) is None and S.static_entry(96, 96, 4) is None           # hidden 1536 on 4 waves
    assert S.static_entry(80, 4, 4) is None and S.static_entry(80, 6, 8) is None               # tiny, d96
    assert S.static_entry(20, 16, 4) == (5, 4) and S.static_entry(16, 16, 4) == (4, 4)         # K = 320 / 256 on 4 waves
    assert S.static_entry(40, 32, 8) == (5, 4)                                                 # (K = 640 / 512 on 8: the same entry)
