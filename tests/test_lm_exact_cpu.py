"""tests/lm_exact.py is right, and it bites (no GPU): the float32 evaluation of its yardstick is OracleLM / LMFuser.advance bit for
bit, the float64 model lies within its own bound of it, the bf16 cases stay inside the caps, every subtly wrong LM is rejected, the K
schedule each GPU case is said to reach is the one gemm_body's list gives it, and the saturating int8 case has the integer sums it
says it has."""
import numpy as np
import pytest

import bf16_exact as X
import f32_exact as S
import lm_exact as E
from oracle import rnnt_oracle as O

F32, F64 = np.float32, np.float64
ROWS = 17       # rows of the CPU cases: an m-tile and one row


@pytest.mark.parametrize("lm", ["h32", "h32u", "h96", "v272", "tiny_lm"])
def test_stand_in_is_the_oracle(lm):
    """StandInLM on f32 operands is OracleLM.step chained by LMFuser.advance, row by row and bit for bit: h and c of every layer and
    the standardised vector after each of the three passes"""
    labels, n, tr = E.case(lm, "f32", ROWS)
    x = E.lm_inputs(labels)
    got = E.chain(lm).ref.run(x)
    lm_o = O.OracleLM(E.state_dict(lm))
    for r in range(ROWS):
        f = O.LMFuser(lm_o)
        for u in range(E.UMAX):
            f.advance(int(x[r, u]))
            assert np.array_equal(got[f"u{u}.lmz"][r], f.lm_logits), (r, u)
            for l, (h, c) in enumerate(f.lm_state):
                assert np.array_equal(got[f"l{l}.u{u}.h"][r], h[0]) and np.array_equal(got[f"l{l}.u{u}.c"][r], c[0]), (r, u, l)
                assert np.array_equal(got[f"l{l}.u{u}.h.pre"][r], h[0])
    assert got["valid"].all() and np.array_equal(got["lmz"], got[f"u{E.UMAX - 1}.lmz"])


def gpu_cases():
    """(LM, operand type, rows, ragged) of every lm_score case of tests/test_gpu_lm_exact.py"""
    out = []
    for dtype in ("f32", "bf16"):
        for lm in E.SCORE_LMS[dtype]:
            out += [(lm, dtype, B, False) for B in E.ROWS64] + [(lm, dtype, 33, True)]
        out += [("h96", dtype, E.ROWS128[0], False)] + [(f"v{V}", dtype, E.POST_ROWS, False) for V in E.VOCABS]
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_against_oracle(dtype):
    """every stage of the float32 chain lies within tol + flip of the float64 model (Y <= 8 Y: this pins the plumbing); f32: no stage
    carries a flip or a tie mask and tol is the rule's, 8 Y or the floor of 4 ulps"""
    for lm, d, B, ragged in gpu_cases():
        if d != dtype:
            continue
        labels, n, tr = E.case(lm, dtype, B, ragged=ragged)
        worst = 0.0
        for k, s in tr.items():
            r = s.ratio(s.ref32)
            worst = max(worst, r)
            assert r <= 1.0, (lm, B, k, r)
            if dtype == "f32":
                assert s.tie is None and not s.flip.any() and s.tol > 0
                floor = E.FLOOR_ULPS * float(np.spacing(F32(np.abs(s.value).max())))
                assert s.tol == max(E.MARGIN * s.Y, floor) and s.Y == float(np.abs(s.ref32.astype(F64) - s.value).max()), k
        print(f"{dtype} {lm} rows {B}{' ragged' if ragged else ''}: worst |oracle - model| / bound {worst:.3g}")


def test_bf16_cases_stay_within_the_caps():
    """at most 2 % of the elements of any rounded tensor tie-sensitive, at most 10 % of any stage with a flip: the rows were picked
    by the reference alone (lm_exact.case); the cases that cannot be (hidden 1024, the flat row) are named as such"""
    for lm, dtype, B, ragged in gpu_cases():
        if dtype != "bf16":
            continue
        labels, n, tr = E.case(lm, dtype, B, ragged=ragged)
        if E.capped(lm):
            tie, flip = X.check_caps(tr)
            print(f"bf16 {lm} rows {B}{' ragged' if ragged else ''}: tie-sensitive <= {tie:.4f}, flip <= {flip:.4f}")
        else:
            s = tr["raw"]
            print(f"bf16 {lm} rows {B}: outside the caps, {float((s.flip > 0).mean()):.2f} of raw carries a flip (median {float(np.median(s.flip)):.2g})")
    assert [lm for lm in E.SCORE_LMS["bf16"] if not E.capped(lm)] == ["h1024"]


# ----------------------------------------------------------------------------- sensitivity
SCORE_SEEN = [f"u{u}.{k}" for u in range(E.UMAX) for k in ("raw", "lmz")]          # what the lm_score tests read, U = 1, 2, 3
FINAL_SEEN = ["l0.h", "l0.c", "l1.h", "l1.c", "raw", "lmz"]                        # what the decode tests read
W = 4


def beam_parents(B, U, seed=5):
    """parent[r, u]: the row of r's group of W whose state r continues at pass u (pass 0: itself)"""
    rng = np.random.default_rng(seed)
    par = (np.arange(B)[:, None] // W) * W + rng.integers(0, W, (B, U))
    par[:, 0] = np.arange(B)
    return par


def outside(tr, got, seen):
    over = {}
    for k in seen:
        s = tr[k]
        d = np.abs(got[k].astype(F64) - s.value)
        bad = d > s.bound()
        if bad.any():
            over[k] = f"{int(bad.sum())} (worst {float((d / np.maximum(s.bound(), 1e-300))[bad].max()):.3g} bound)"
    return over


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", E.WEIGHT_FAULTS + E.RUN_FAULTS + E.POST_FAULTS)
def test_mutation_is_caught(kind, dtype):
    """a copy of the float32 chain with one fault, playing the kernel: at least one element of one stage the GPU tests read lands
    outside the bound -- in the 17-row lm_score case of every LM for the weight and standardisation faults, in the ragged case for
    the row that is stepped although it is done, in a chain with parent indirection for the beam fault"""
    caught = {}
    for lm in ("h32", "h32u", "h96", "v272"):
        ref = E.chain(lm, dtype).ref
        if kind == "parent_plus_one":
            B = 16
            toks = E.lm_inputs(E.seeded_tokens(E.lm_cfg(lm)["vocab"], B, 9))
            par = beam_parents(B, E.UMAX)
            tr = E.chain(lm, dtype).run(toks, parent=par)
            got, seen = E.mutated(ref, kind, W=W).run(toks, parent=par), FINAL_SEEN
        else:
            labels, n, tr = E.case(lm, dtype, ROWS if kind != "idle_row_stepped" else 33, ragged=kind == "idle_row_stepped")
            got = E.mutated(ref, kind).run(E.lm_inputs(labels), n)
            seen = FINAL_SEEN if kind == "idle_row_stepped" else SCORE_SEEN
        caught[lm] = outside(tr, got, seen)
    print(f"{kind} ({dtype}): elements outside the bound {caught}")
    assert all(caught.values()), (kind, caught)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["bias_dropped", "h_k_tail_dropped", "row16_takes_row0"])
def test_mutation_is_caught_at_hidden_1024(kind, dtype):
    """hidden 1024: in the lm_score stages (raw, lmz) the bf16 bound is all allowance and these faults stay inside it -- recorded
    here, so that a case whose bound cannot bite is seen on the CPU; the stages that do bite are h and c of rows a few tokens long,
    which tests/test_gpu_lm_exact.py::test_state_after_short_decode_hidden_1024 reads: there each fault must be caught"""
    labels, n, tr = E.case("h1024", dtype, ROWS, ragged=True)
    got = E.mutated(E.chain("h1024", dtype).ref, kind).run(E.lm_inputs(labels), n)
    state = outside(tr, got, ["l0.h", "l0.c", "l1.h", "l1.c"])
    score = outside(tr, got, ["raw", "lmz"])
    print(f"{kind} ({dtype}) at hidden 1024: outside the bound in h / c {state}; in raw / lmz {score}")
    assert state, (kind, dtype)
    if dtype == "f32":
        assert score, kind


def test_post_faults_are_caught_by_the_isolated_check():
    """k_lm_post alone (lmz against the float64 standardisation of the same raw; the flat row is a stage of its own, as in the GPU
    test: its yardstick is a hundred times the other rows'): every standardisation fault lands outside the bound in both, and
    the omitted + 1e-5 moves the flat row a hundred times further than any other"""
    labels, n, tr = E.case("v272", "f32", ROWS)
    raw = tr["raw"].ref32
    rest, flat = E.post_stage(raw[:-1]), E.post_stage(raw[-1:])
    assert rest.ratio(rest.ref32) <= 1.0 and flat.ratio(flat.ref32) <= 1.0 and flat.Y > 10 * rest.Y
    for kind in E.POST_FAULTS:
        got = np.stack([E.post32(z, kind) for z in raw]).astype(F64)
        d, df = np.abs(got[:-1] - rest.value), np.abs(got[-1:] - flat.value)
        print(f"{kind}: worst {float(d.max() / rest.tol):.3g} tol, flat row {float(df.max() / flat.tol):.3g} tol")
        assert (d > rest.tol).any() and (df > flat.tol).any(), kind
        if kind == "no_eps":
            assert df.max() > 100 * d.max() and df.max() > 20 * flat.tol


# ----------------------------------------------------------------------------- the int8-served form
def quant_rows():
    rng = np.random.default_rng(3)
    H = 36
    rows = [rng.uniform(-1, 1, H).astype(F32) * F32(s) for s in (1.0, 0.3, 1e-3, 0.9)]
    rows += [np.abs(rows[0]), -np.abs(rows[1]), np.zeros(H, F32)]              # one-sided ranges (zero point 0 / 127), the row that emitted nothing
    return rows, 64


def test_quantise_is_dq_linear():
    """quantise() is the activation side of oracle.rnnt_oracle.dq_linear: the integer sums against the same weights agree exactly"""
    rows, Kp = quant_rows()
    rng = np.random.default_rng(4)
    qw = rng.integers(-128, 128, (8, len(rows[0])))
    for x in rows:
        q, s = E.quantise(x, Kp)
        want = O.dq_linear(x, qw, F32(0.01), np.zeros(8, F32))
        got = ((q[:len(x)].astype(np.int64) @ qw.T).astype(F32) * F32(s * F32(0.01))).astype(F32)
        assert np.array_equal(got, want) and not q[len(x):].any()
    assert E.quantise(rows[-1], Kp)[1] == F32(0.1)


@pytest.mark.parametrize("kind", E.QUANT_FAULTS)
def test_quantisation_fault_is_caught(kind):
    """the int8 rule is bit for bit, so a fault is caught when its image or scale differs from the reference's on some row.  The
    zero point's clamp to [0, 127] is the exception: min(x, 0) <= 0 <= max(x, 0) puts the unclamped value inside that interval
    for every finite row, so no input can tell a kernel without it apart -- asserted as such, over 2000 rows of every magnitude"""
    rows, Kp = quant_rows()
    differs = []
    for i, x in enumerate(rows):
        q, s = E.quantise(x, Kp)
        fq, fs = E.quantise(x, Kp, kind, nxt=rows[(i + 1) % len(rows)])
        differs.append(not (np.array_equal(q, fq, equal_nan=True) and s == fs))
    print(f"{kind}: rows on which the image or the scale differs {differs}")
    if kind == "zero_point_unclamped":
        rng = np.random.default_rng(5)
        for _ in range(2000):
            x = (rng.standard_normal(8) * 10.0 ** rng.uniform(-30, 30)).astype(F32)
            assert np.array_equal(E.quantise(x, 8)[0], E.quantise(x, 8, kind)[0])
        assert not any(differs)
    else:
        assert any(differs), kind
        if kind == "scale_zero_kept":
            assert differs[-1]                    # the all-zero row


def test_saturating_case_has_the_sums_it_says():
    sd = E.saturating_lm()
    qw, sw = O.dq_weight(sd["rnn.weight_ih_l0"])
    assert np.all(qw == -128)
    q, s = E.quantise(sd["embed.weight"][3], E.SAT_CFG["embed"])
    assert np.all(q == 127)
    v, bound, acc = E.tab_int8(sd)
    assert np.all(acc == E.SAT_SUM) and E.SAT_SUM == -1024 * 127 * 128 and abs(E.SAT_SUM) < 2 ** 24
    assert 1032 * 127 * 128 < 2 ** 24 < 1033 * 127 * 128       # "exact below K = 1032": the last K whose worst sum is an f32 integer
    assert F32(E.SAT_SUM) == E.SAT_SUM                 # exact in f32, as every partial sum on the way is
    assert np.all(bound > 0) and np.all(np.abs(v) > 100 * bound)


# ----------------------------------------------------------------------------- the K schedule
def test_schedule_of_every_lm_case():
    """launch_lm_t: every cell in the four-unit tiling on 8 waves (layer 0 has no x phase), the output layer on 8 waves; hidden 1024
    is gemm_body's (8, 8) entry in both, everything smaller the dynamic loop -- with idle waves (2 chunks) and with a tail (6)"""
    for lm, nw, cells, out in E.LM_SCHEDULES:
        cfg = E.lm_cfg(lm)
        assert S.schedule("lm_cell", cfg, nw) == cells and S.schedule("lm_out", cfg, nw) == out, lm
    assert S.launches("lm_cell", E.lm_cfg("h96")) == [(None, 6), (6, 6)] and S.launches("lm_out", E.lm_cfg("h96")) == [(6, None)]
    assert S.launches("lm_cell", E.lm_cfg("h1024"))[1] == (64, 64)
    assert sorted(n for n, *_ in E.LM_SCHEDULES) == sorted(E.SCORE_LMS["f32"])
