"""The dtype=bf16 kernels against the float64 model of tests/bf16_exact.py, element by element: |engine - value| <= tol + flip, at the
smallest shapes that reach each tiling the bf16 launchers select by themselves (docs/bf16_bound.md has the rule, the yardsticks and
the measured ratios; every test prints its own, so the table can be regenerated with -s).

Models: tiny and tiny_lstm as they are, and tiny with hidden = joint = 96 (three 32-wide K chunks: every K split has a tail), with
a vocabulary of 64 (a multiple of 64: the 64 x 64 logits tiling) and of 80; for the runtime-shaped k_stack_ln tiny with 64 mels x 12
stacked frames (g768).  Inputs: bf16_exact.case -- picked on the CPU by the
reference alone so that the tie caps hold, which is asserted before anything is compared."""
import numpy as np
import pytest
import torch

import bf16_exact as X

pytestmark = pytest.mark.gpu


def make(name, monkeypatch=None, env=None, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)                       # read by lasr_create
    _, sd, cfg = X.model(name)
    return Engine(sd, cfg, dtype="bf16", **kw, **X.FRONTEND.get(name, {}))


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def held(tr, what):
    """the caps first: a case outside them fails here, it is not skipped"""
    tie, flip = X.check_caps(tr)
    print(f"{what}: tie-sensitive {tie:.4f}, carrying a flip {flip:.4f}")


def compare(tr, name, got, what, worst):
    """one stage of the trace against the engine's values; for a rounded stage Y is the yardstick of the value before rounding"""
    stage = tr[name]
    r = stage.ratio(got)
    d = float(np.abs(np.asarray(got, np.float64) - stage.value).max())
    Y = tr[name + ".pre"].Y if name + ".pre" in tr else stage.Y
    exact = float((stage.bound() == 0).mean())       # share of elements that must be bit-equal (rounded stages)
    print(f"  {what:44s} {stage.name:14s} Y {Y:.3g} tol {stage.tol:.3g} max flip {float(stage.flip.max()):.3g} zero bound {exact:.2f} max |d| {d:.3g} ratio {r:.3g}")
    worst.append((r, what, stage.name))


def settle(worst):
    over = [w for w in worst if not w[0] <= 1.0]
    assert not over, over


# ----------------------------------------------------------------------------- LayerNorm into x0, encoder cell of layer 0
ENC_TILINGS = {
    "default": ({}, dict(enc_wave=1, cell_nw=8, enc_u12=0)),
    "plain_launches": ({"LASR_ENC_WAVE": "0"}, dict(enc_wave=0, cell_nw=8, enc_u12=0)),
    "four_waves": ({"LASR_CELL_NW": "4"}, dict(enc_wave=1, cell_nw=4, enc_u12=0)),
    "tiling_d": ({"LASR_ENC_U12": "1"}, dict(enc_wave=0, cell_nw=8, enc_u12=1)),
}


# tiling D needs hidden % 12 == 0 (lasr_create): of these models d96 alone admits it; g768 is there for the runtime-shaped k_stack_ln
ENC_PARAMS = [("tiny", t) for t in ("default", "plain_launches", "four_waves")] + [("d96", t) for t in ENC_TILINGS] + [("g768", "default")]


@pytest.mark.parametrize("name,tiling", ENC_PARAMS)
def test_encoder(name, tiling, monkeypatch):
    """One frame and two (the recurrent path on a rounded h), rows 1, 16, 17, 64 -- an m-tile boundary and a full row group: x0
    (the static k_stack_ln<20, 10> where feat is 1280, the runtime-shaped one for g768), and of every layer the f32 cell state and
    the rounded h after the last frame, and the rounded BN(h) of the last layer for every frame.  The caps hold, and are asserted,
    for x0 and for layer 0's first frame up to the rounding of its h; that h and (one frame) its BN(h) inherit nothing, so off a
    tie they are bit-equal, but 13 .. 16 % of their elements are tie-sensitive behind the K = feat GEMM, whatever the input: held
    to 25 % instead of the 2 % cap.  Everything behind them is held to tol + flip all the same, outside the caps -- every row
    carries a flip there, and the printed share of elements with a zero bound says how sharp each stage still is
    (docs/bf16_bound.md)."""
    env, want = ENC_TILINGS[tiling]
    eng = make(name, monkeypatch, env, max_streams=64)
    worst = []
    try:
        assert eng.config("M") == 64 and {k: eng.config(k) for k in want} == want
        L = eng.cfg["enc_layers"]
        for nm, B, T in X.ENC_CASES:
            if nm != name:
                continue
            x, tr = X.case("enc", name, B, T)
            what = f"encoder {name} {tiling} rows {B} T' {T}"
            held(tr, what)
            for k in ["enc0.t0.h"] + (["enc0.y"] if T == 1 else []):
                assert tr[k].tie.mean() <= X.ENC_H_TIE_CAP and np.all(tr[k + ".pre"].flip[:B - B // 16] == 0), k
            out, h, c = eng.encoder(dev(x), return_state=True)
            compare(tr, "x0", np.stack([eng.debug_read("x0", t)[:B] for t in range(T)], 1), what, worst)
            h, c = h.cpu().numpy(), c.cpu().numpy()
            for l in range(L):
                compare(tr, f"enc{l}.t{T - 1}.c", c[l], what, worst)
                compare(tr, f"enc{l}.t{T - 1}.h", h[l], what, worst)
            compare(tr, f"enc{L - 1}.y", out.cpu().numpy(), what, worst)
    finally:
        eng.close()
    settle(worst)


# ----------------------------------------------------------------------------- predictor cells
# (four units: 64 rows need max_streams 64; M is 64 from 1 stream on, whole 64-row groups)
PRED_TILINGS = {"units4": (dict(max_streams=64), 64), "wide8": (dict(max_streams=64, beam=4), 256), "wide_k16": (dict(max_streams=64, beam=8), 512)}


@pytest.mark.parametrize("tiling", list(PRED_TILINGS))
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm", "d96", "d96_lstm"])
def test_predictor_cells(name, tiling):
    """U = 1 and 2 tokens from the learned initial state, 64 rows (a whole row group: all four m-tiles of a wide workgroup): the rounded h of both layers (layer 0 on the f32 table, layer 1 on
    the rounded BN(h) of layer 0; at U = 2 on a rounded recurrent h) and the rounded BN(h) of the last layer, with the flip rule.
    The tiling follows the decoder row count Md = M x beam: < 256 four units per workgroup, 256 .. 511 wide8, >= 512 the 16-unit
    tiling on the k16 instruction (thresholds read from launch_predictor_t at this commit: nothing reports the tiling taken)."""
    kw, Md = PRED_TILINGS[tiling]
    eng = make(name, **kw)
    worst = []
    try:
        assert eng.config("M") * eng.beam == Md
        L = eng.cfg["pred_layers"]
        for nm, U in X.PRED_CASES:
            if nm != name:
                continue
            toks, tr = X.case("pred", name, X.PRED_ROWS, U)
            B = len(toks)
            what = f"predictor {name} {tiling} U {U}"
            held(tr, what)
            y = eng.predictor(toks).cpu().numpy()
            for l in range(L):
                compare(tr, f"pred{l}.u{U - 1}.h", eng.debug_read("pred_h", l)[:B], what, worst)
            compare(tr, f"pred{L - 1}.u{U - 1}.y", y, what, worst)
    finally:
        eng.close()
    settle(worst)


# ----------------------------------------------------------------------------- joint
# (model, max_streams, rows, the logits tiling launch_logits_ops takes: logits_mt is 2 in every context -- nothing sets it, nothing reports it)
JOINT_ENGINES = [
    ("tiny", 64, (5, 16, 17, 64), "32 rows x 16 columns"),
    ("d96", 64, (5, 16, 17, 64), "32 rows x 16 columns"),
    ("d96", 512, (512,), "64 x 64 (rows >= 512, vocab % 64 == 0)"),
    ("d96_v80", 512, (17, 512), "32 x 16 below 512 rows, 64 x 16 from 512 (vocab 80)"),
]


@pytest.mark.parametrize("name,max_streams,rows,tiling", JOINT_ENGINES, ids=[f"{e[0]}-{e[1]}" for e in JOINT_ENGINES])
def test_joint(name, max_streams, rows, tiling):
    """pp and pe one GEMM deep on inputs rounded once (no flip term), the logits with the flip budget of the joint activation, lp
    against the float64 log-softmax maximum within the logits' bound plus the reduction's own yardstick."""
    eng = make(name, max_streams=max_streams)
    worst = []
    try:
        assert eng.config("M") == max_streams
        V = eng.cfg["vocab"]
        for B in rows:
            assert (name, B) in X.JOINT_CASES
            (a, b), tr = X.case("joint", name, B)
            what = f"joint {name} rows {B} [{tiling}]"
            assert (B >= 512 and V % 64 == 0) == tiling.startswith("64 x 64")
            held(tr, what)
            logits, lp, am = eng.joint(dev(a), dev(b))
            compare(tr, "pp", eng.debug_read("pp")[:B], what, worst)
            compare(tr, "pe", eng.debug_read("pe", 0)[:B], what, worst)
            compare(tr, "logits", logits.cpu().numpy(), what, worst)
            compare(tr, "lp", lp.cpu().numpy(), what, worst)
            z = tr["logits"]
            top2 = np.sort(z.value, -1)[:, -2:]
            clear = top2[:, 1] - top2[:, 0] > 2 * z.bound().max(-1)
            assert np.array_equal(am.cpu().numpy()[clear], z.value.argmax(-1)[clear])
    finally:
        eng.close()
    settle(worst)
