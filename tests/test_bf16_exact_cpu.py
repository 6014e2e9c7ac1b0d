"""tests/bf16_exact.py is right, and it bites (no GPU): the float64 model of the dtype=bf16 contract agrees with the numpy oracle's
operand="bf16" emulation stage by stage within its own bound, rounds what the oracle rounds, keeps the tie caps on every case the
GPU file uses, and rejects six subtly wrong kernels."""
import numpy as np
import pytest

import bf16_exact as X
from oracle import rnnt_oracle as O

MODELS = ["tiny", "tiny_lstm", "cfg2", "cfg2_lstm"]


def inputs(name):
    """plain seeded inputs (not picked for the caps: these never go to the GPU): 3 rows, two frames, two tokens; 5 joint rows"""
    cfg = X.model_cfg(name)
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((3, 2, cfg["feat"])) * rng.uniform(0.5, 2.0, (3, 1, 1))).astype(np.float32)
    toks = rng.integers(1, cfg["vocab"], (3, 2)).astype(np.int32)
    a, b = rng.standard_normal((5, cfg["hidden"])).astype(np.float32), rng.standard_normal((5, cfg["hidden"])).astype(np.float32)
    return x, toks, a, b


_TR = {}


def traces(name):
    if name not in _TR:
        m = X.model(name)[0]
        x, toks, a, b = inputs(name)
        _TR[name] = dict(enc=m.encoder(x), pred=m.predictor(toks), joint=m.joint(a, b))
    return _TR[name]


@pytest.mark.parametrize("name", MODELS)
def test_stand_in_is_the_oracle(name):
    """the float32 evaluation of the yardstick is OracleTransducer's, bit for bit"""
    m = X.model(name)[0]
    o, s = m.o, m.ref
    x, toks, a, b = inputs(name)
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
    j = s.joint(a, b)
    lp, z = o.joint_logp(a, b)
    assert np.array_equal(j["logits"], z) and np.array_equal(j["lp"], lp.max(-1))


@pytest.mark.parametrize("name", MODELS)
def test_rounded_weights_are_the_oracles(name):
    """the model rounds its weights itself, from the state dict: the same set as the oracle, to the same values"""
    m, sd, cfg = X.model(name)
    o, f32 = m.o, O.OracleTransducer(sd, cfg)
    changed = set()
    for prefix, mine, theirs, plain in (("encoder", m.enc, o.enc, f32.enc), ("predictor", m.pred, o.pred, f32.pred)):
        for i, (a, b, c) in enumerate(zip(mine, theirs, plain)):
            for k, w in b["rnn"].items():
                assert np.array_equal(a["rnn"][k], w.astype(np.float64)), (prefix, i, k)
                if not np.array_equal(w, c["rnn"][k]):
                    changed.add(f"{prefix}.rnn_stack.rnns.{i}.{k}")
    for k, a, b, c in (("joint.joint.0.weight", m.j0_w, o.j0_w, f32.j0_w), ("joint.joint.2.weight", m.j2_w, o.j2_w, f32.j2_w),
                       ("joint.joint.0.bias", m.j0_b, o.j0_b, f32.j0_b), ("joint.joint.2.bias", m.j2_b, o.j2_b, f32.j2_b),
                       ("predictor.embed.weight", m.embed, o.embed, f32.embed)):
        assert np.array_equal(a, b.astype(np.float64)), k
        if not np.array_equal(b, c):
            changed.add(k)
    assert changed == set(m.rounded_weights)
    # the docstring's list: every recurrent weight, every input weight but the predictor's layer 0, both joint weights
    n_cells = cfg["enc_layers"] + cfg["pred_layers"]
    assert len(changed) == 2 * n_cells - 1 + 2 and not any("bias" in k for k in changed)
    assert not {"predictor.rnn_stack.rnns.0.weight_ih_l0", "predictor.rnn_stack.rnns.0.kernel"} & changed


@pytest.mark.parametrize("name", MODELS)
def test_rounded_activations_are_the_oracles(name):
    """the set of activations the model rounds against the set the oracle passes to its rounding function: the same tensors, in
    the same order (LayerNorm output, every h, every BN(h); the joint's input and its activation), nothing else"""
    m = X.model(name)[0]
    o = m.o
    x, toks, a, b = inputs(name)
    tr = traces(name)
    es, ps = o.enc_init_state(len(x)), o.pred_init_state(len(toks))       # (rounded at load: not part of the set)
    seen, q = [], o.q

    def rec(v):
        seen.append(np.array(v, np.float32))
        return q(v)

    o.q = rec
    try:
        o.encoder(x, es)
        n_enc = len(seen)
        for u in range(2):
            _, ps = o.predictor(toks[:, u], ps)
        n_pred = len(seen)
        o.joint_logp(a, b)
    finally:
        o.q = q
    groups = ((seen[:n_enc], tr["enc"]), (seen[n_enc:n_pred], tr["pred"]), (seen[n_pred + 1:], tr["joint"]))
    assert np.array_equal(seen[n_pred], np.concatenate([a, b], -1))      # the joint's input: rounded once, no allowance
    for got, t in groups:
        assert len(got) == len(t.rounded), (len(got), t.rounded)
        for v, k in zip(got, t.rounded):
            s = t[k + ".pre"]
            assert v.shape == s.value.shape, k
            assert s.ratio(v) <= 1.0, (k, s.ratio(v))
    # and what must stay f32 is continuous in the model: cell state, pp / pe, logits
    assert all(tr["joint"][k].tie is None for k in ("pp", "pe", "logits", "lp"))
    assert all(s.tie is None for k, s in list(tr["enc"].items()) + list(tr["pred"].items()) if k.endswith(".c"))


@pytest.mark.parametrize("name", MODELS)
def test_model_against_oracle(name):
    """every stage of the oracle's emulation lies within tol + flip of the float64 model -- rounded stages included, where tol is
    zero: away from a tie the two round to the same bf16 number"""
    worst = {}
    for part, tr in traces(name).items():
        for k, s in tr.items():
            r = s.ratio(s.ref32)
            worst[part] = max(worst.get(part, 0.0), r)
            assert r <= 1.0, (name, k, r)
            assert s.tol > 0 or s.tie is not None
    print(f"{name}: worst |oracle - model| / (tol + flip) {worst}")


def test_a_flip_is_bounded_where_it_happens():
    """the allowance is one bf16 ulp of the element where nothing is inherited, and zero off a tie"""
    tr = traces("tiny")["joint"]
    s = tr["act"]
    assert np.all(s.flip[~s.tie] == 0) and np.all(s.flip[s.tie] > 0)
    assert np.all(s.flip[s.tie] <= 2 * X.bf16_ulp(s.value[s.tie].astype(np.float32)) + 1e-30)
    # through the vocabulary GEMM: |W| . flip
    want = s.flip @ np.abs(X.model("tiny")[0].j2_w).T
    assert np.array_equal(tr["logits"].flip, want)


CASES = [("enc",) + c for c in X.ENC_CASES] + [("pred", n, X.PRED_ROWS, U) for n, U in X.PRED_CASES] + [("joint",) + c for c in X.JOINT_CASES]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_caps_hold_for_every_gpu_case(case):
    _, tr = X.case(*case)
    tie, flip = X.check_caps(tr)
    print(f"{case}: tie-sensitive {tie:.4f} (cap {X.TIE_CAP}), carrying a flip {flip:.4f} (cap {X.FLIP_CAP})")
    for k, s in tr.items():
        assert s.ratio(s.ref32) <= 1.0, k


def test_the_flip_rule_is_exercised():
    """not only permitted: of the encoder's and of the joint's cases some carry an inherited flip"""
    for kind, cases in (("enc", X.ENC_CASES), ("joint", X.JOINT_CASES)):
        n = sum(max(float((s.flip > 0).mean()) for s in X.case(kind, *c)[1].values() if s.tie is None) > 0 for c in cases)
        assert n >= len(cases) // 2, (kind, n)


# ----------------------------------------------------------------------------- sensitivity
ENC_SEEN = lambda L, T: ["x0"] + [f"enc{l}.t{T - 1}.{k}" for l in range(L) for k in ("c", "h")] + [f"enc{L - 1}.y"]
PRED_SEEN = lambda L, U: [f"pred{l}.u{U - 1}.h" for l in range(L)] + [f"pred{L - 1}.u{U - 1}.y"]
JOINT_SEEN = ["pp", "pe", "logits", "lp"]

MUTATIONS = {
    "a_truncated_activations": dict(q=X.bf16_trunc),
    "b_recurrent_k_tail_dropped": dict(weights="k_tail"),
    "c_weight_row_one_ulp_off": dict(weights="w_ulp"),
    "d_h_fed_back_unrounded": dict(raw_h_t=1),
    "e_joint_activation_unrounded": dict(raw_act=True),
    "f_bias_twice_in_pp": dict(weights="bias_twice"),
}


# The parts of the model in which the fault must show.  The fault touches more: docs/bf16_bound.md lists where it escapes and why
# (a rounded h hides what is smaller than its bf16 ulp; behind the encoder's K = 1280 GEMM every row of a second frame carries a flip).
CAUGHT_IN = {
    "a_truncated_activations": ("enc", "pred", "joint"),
    "b_recurrent_k_tail_dropped": ("enc", "pred"),
    "c_weight_row_one_ulp_off": ("joint",),
    "d_h_fed_back_unrounded": ("pred",),
    "e_joint_activation_unrounded": ("joint",),
    "f_bias_twice_in_pp": ("joint",),
}


@pytest.mark.parametrize("name", MODELS + ["d96", "d96_lstm"])
@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_is_caught(mut, name):
    """a copy of the float32 oracle's stages with one fault, playing the kernel: at least one element of one stage the GPU tests
    read lands outside tol + flip"""
    m, _, cfg = X.model(name)
    kw = dict(MUTATIONS[mut])
    o = X.mutated(m.o, kw.pop("weights")) if "weights" in kw else m.o
    bad = X.StandIn(o, **kw)
    x, toks, a, b = inputs(name)
    tr = traces(name)
    got = dict(enc=bad.encoder(x), pred=bad.predictor(toks), joint=bad.joint(a, b))
    seen = dict(enc=ENC_SEEN(cfg["enc_layers"], 2), pred=PRED_SEEN(cfg["pred_layers"], 2), joint=JOINT_SEEN)
    over = {}
    for part in ("enc", "pred", "joint"):
        for k in seen[part]:
            s = tr[part][k]
            n = int((np.abs(got[part][k].astype(np.float64) - s.value) > s.bound()).sum())
            if n:
                over[f"{part}:{k}"] = n
    print(f"{mut} on {name}: elements outside the bound {over}")
    for part in CAUGHT_IN[mut]:
        assert any(k.startswith(part + ":") for k in over), (mut, name, part, over)


@pytest.mark.parametrize("name", ["tiny", "d96"])
@pytest.mark.parametrize("mut", ["a_truncated_activations", "b_recurrent_k_tail_dropped", "c_weight_row_one_ulp_off", "d_h_fed_back_unrounded"])
def test_mutation_is_caught_on_the_encoder_case(mut, name):
    """the same on the GPU's encoder cases (a settled x0, 17 rows): one frame -- the recurrent GEMM runs on the learned initial h --
    and, for the h fed back unrounded, two.  On these inputs (d) shows in the encoder too: in layer 0's cell state of the second frame."""
    m = X.model(name)[0]
    T = 2 if mut == "d_h_fed_back_unrounded" else 1
    x, tr = X.case("enc", name, 17, T)
    kw = dict(MUTATIONS[mut])
    o = X.mutated(m.o, kw.pop("weights")) if "weights" in kw else m.o
    got = X.StandIn(o, **kw).encoder(x)
    c = f"enc0.t{T - 1}.c"
    over = {k: int((np.abs(got[k].astype(np.float64) - tr[k].value) > tr[k].bound()).sum()) for k in ("x0", c, f"enc0.t{T - 1}.h", "enc1.y")}
    print(f"{mut} on the encoder case of {name}: elements outside the bound {over}")
    if mut != "c_weight_row_one_ulp_off":          # (one ulp in one row moves 4 or 5 elements of c just past the K = 1280 stage's tol:
        assert over[c] > 0                         #  printed; the joint weights are where test_mutation_is_caught holds it)
    assert (over["x0"] > 0) == (mut == "a_truncated_activations")
    if mut == "a_truncated_activations":           # a truncating store of h or of BN(h) alone would show here
        assert over["enc0.t0.h"] > 0 and over["enc1.y"] > 0
