"""The dtype=f32 kernels against the float64 model of tests/f32_exact.py, element by element: |engine - value| <= tol, in every
tiling and K schedule the f32 launchers take (docs/f32_bound.md has the rule, the schedule each case reaches and the measured
ratios; every test prints its own, so the table can be regenerated with -s).

Models: tiny, tiny_lstm and the hidden-96 models of the bf16 tests (the dynamic K loop, with idle waves and with a tail in every
split), g768 (the runtime-shaped k_stack_ln), and four models whose K meets the static schedules: s256 (K = 320 / 256), s1024,
s1024_lstm (1280 / 1024) and s1536_lstm (1280 / 1536, and tiling D).  Nothing reports the schedule a launch takes: each test asserts
the parameters that imply it (Engine.config, M x beam, the row count) and that f32_exact's restatement of gemm_body's list gives
the entry the case names."""
import numpy as np
import pytest
import torch

import f32_exact as S

pytestmark = pytest.mark.gpu


def make(name, monkeypatch=None, env=None, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)                       # read by lasr_create
    _, sd, cfg = S.model(name)
    return Engine(sd, cfg, dtype="f32", **kw, **S.FRONTEND.get(name, {}))


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def compare(tr, name, got, what, worst):
    """one stage of the trace against the engine's values"""
    stage = tr[name]
    r = stage.ratio(got)
    d = float(np.abs(np.asarray(got, np.float64) - stage.value).max())
    print(f"  {what:52s} {stage.name:12s} Y {stage.Y:.3g} tol {stage.tol:.3g} max |d| {d:.3g} ratio {r:.3g}")
    worst.append((r, what, stage.name))


def settle(worst):
    over = [w for w in worst if not w[0] <= 1.0]
    assert not over, over


# ----------------------------------------------------------------------------- LayerNorm into x0, the encoder cells
def run_encoder(eng, name, tiling, B, T, worst):
    L = eng.cfg["enc_layers"]
    x, tr = S.case("enc", name, B, T)
    what = f"encoder {name} {tiling} rows {B} T' {T}"
    out, h, c = eng.encoder(dev(x), return_state=True)
    compare(tr, "x0", np.stack([eng.debug_read("x0", t)[:B] for t in range(T)], 1), what, worst)
    h, c = h.cpu().numpy(), c.cpu().numpy()
    for l in range(L):
        compare(tr, f"enc{l}.t{T - 1}.c", c[l], what, worst)
        compare(tr, f"enc{l}.t{T - 1}.h", h[l], what, worst)
    compare(tr, f"enc{L - 1}.y", out.cpu().numpy(), what, worst)


@pytest.mark.parametrize("name,tiling,rows,entries", S.ENC_PARAMS, ids=[f"{p[0]}-{p[1]}" for p in S.ENC_PARAMS])
def test_encoder(name, tiling, rows, entries, monkeypatch):
    """One frame and two (the recurrent path), at the rows 1, 16, 17, 33, 64 for the dynamic-loop models -- m-tile boundaries and
    a full row group -- and 17, 64 for the static schedules (which do not depend on the row count): x0, c and h of every layer
    after the last frame, BN(h) of the last layer for every frame."""
    env, want, nw = S.ENC_TILINGS[tiling]
    assert S.schedule("enc_cell", name, nw) == entries
    eng = make(name, monkeypatch, env, max_streams=64)
    worst = []
    try:
        assert eng.config("M") == 64 and {k: eng.config(k) for k in want} == want
        for B in rows:
            for T in S.ENC_FRAMES:
                run_encoder(eng, name, tiling, B, T, worst)
    finally:
        eng.close()
    settle(worst)


@pytest.mark.parametrize("tiling", S.ENC_GROUP2[3])
def test_encoder_second_row_group(tiling, monkeypatch):
    """80 rows of a 128-row engine: a second m-group behind the 32-row grid of tiling C and the 64-row grid of tiling D"""
    name, M, B, _ = S.ENC_GROUP2
    env, want, nw = S.ENC_TILINGS[tiling]
    eng = make(name, monkeypatch, env, max_streams=M)
    worst = []
    try:
        assert eng.config("M") == M and {k: eng.config(k) for k in want} == want
        for T in S.ENC_FRAMES:
            run_encoder(eng, name, tiling, B, T, worst)
    finally:
        eng.close()
    settle(worst)


# ----------------------------------------------------------------------------- predictor cells
@pytest.mark.parametrize("tiling", list(S.PRED_TILINGS))
@pytest.mark.parametrize("name", S.PRED_MODELS)
def test_predictor_cells(name, tiling):
    """U = 1 and 2 tokens from the learned initial state: h of both layers (layer 0 on the token table, layer 1 on BN(h) of layer
    0; at U = 2 on a recurrent h) and BN(h) of the last layer.  Four units per workgroup (Md = 64) at 5, 17, 33 and 64 rows -- 1,
    2, 3 and 4 of a workgroup's m-tiles in play, every P branch of gemm_body for MT = 4 -- and the 16-unit tiling (Md = 512) at 64.
    f32 has no wide8 tiling (launch_predictor_t asks for it with bf16 operands only): Md is asserted, nothing reports the tiling
    taken.  The s1024 models take a static schedule in both tilings, the others the dynamic loop."""
    kw, Md, nw, rows = S.PRED_TILINGS[tiling]
    eng = make(name, **kw)
    worst = []
    try:
        assert eng.config("M") * eng.beam == Md and eng.dtype == "f32"
        assert all((e is not None) == name.startswith("s1024") for e in S.schedule("pred_cell", name, nw))
        L = eng.cfg["pred_layers"]
        for B in rows:
            for U in S.PRED_TOKENS:
                toks, tr = S.case("pred", name, B, U)
                what = f"predictor {name} {tiling} rows {B} U {U}"
                y = eng.predictor(toks).cpu().numpy()
                for l in range(L):
                    compare(tr, f"pred{l}.u{U - 1}.h", eng.debug_read("pred_h", l)[:B], what, worst)
                compare(tr, f"pred{L - 1}.u{U - 1}.y", y, what, worst)
    finally:
        eng.close()
    settle(worst)


# ----------------------------------------------------------------------------- joint
@pytest.mark.parametrize("name,max_streams,rows,nw,tiling", S.JOINT_ENGINES, ids=[f"{e[0]}-{e[1]}" for e in S.JOINT_ENGINES])
def test_joint(name, max_streams, rows, nw, tiling):
    """pp and pe one GEMM deep, the logits behind tanh, lp against the float64 log-softmax maximum within the logits' bound plus
    the reduction's own yardstick, and the argmax wherever the float64 top-2 margin exceeds twice the bound."""
    eng = make(name, max_streams=max_streams)
    worst = []
    try:
        assert eng.config("M") == max_streams
        assert all((e is not None) == (name == "s1024") for e in S.schedule("joint_half", name, 8) + S.schedule("logits", name, nw))
        V = eng.cfg["vocab"]
        for B in rows:
            (a, b), tr = S.case("joint", name, B)
            what = f"joint {name} rows {B} [{tiling}]"
            assert (B >= 512 and V % 64 == 0) == tiling.startswith("64 x 64")
            logits, lp, am = eng.joint(dev(a), dev(b))
            compare(tr, "pp", eng.debug_read("pp")[:B], what, worst)
            compare(tr, "pe", eng.debug_read("pe", 0)[:B], what, worst)
            compare(tr, "logits", logits.cpu().numpy(), what, worst)
            compare(tr, "lp", lp.cpu().numpy(), what, worst)
            z = tr["logits"]
            top2 = np.sort(z.value, -1)[:, -2:]
            clear = top2[:, 1] - top2[:, 0] > 2 * z.tol
            assert clear.any() and np.array_equal(am.cpu().numpy()[clear], z.value.argmax(-1)[clear])
    finally:
        eng.close()
    settle(worst)
