"""The language model's kernels against the float64 model of tests/lm_exact.py, element by element: the output layer's logits, the
standardised vector k_lm_post makes of them, h and c of every layer -- f32 and bf16 operands and the int8-served form, at more than one
m-tile, in a second 64-row group, with rows left out of a call, through lasr_lm_score, both greedy protocols and the beam
(docs/lm_bound.md has the rule, the schedule each case reaches and the measured ratios; every test prints its own with -s).

The read-outs are lasr_debug_read's LM matrices (include/lasr_debug.h): behind lasr_lm_score `lm_raw` / `lmz` hold the last pass of every
listed row (its closing reset zeroes h, c and the rows' flags and leaves those two), behind a decode h, c and the quantised images hold
the LM run over the tokens the row has emitted."""
import itertools

import numpy as np
import pytest

import f32_exact as S
import lm_exact as E
from libreasr_amd import synth
from oracle import rnnt_oracle as O

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64

# int8-served form: h and c against the oracle's emulation, OracleLM(quantized=True) replayed over the row's own tokens (integer
# accumulation exact on both sides; the device's expf / tanhf against numpy's, carried through the recurrence): 4 x the largest
# deviation measured on the GPU over every int8 case of this file (see docs/lm_bound.md), rounded up to one significant digit
# (measured: 1.13e-4 in c, 5.9e-5 in h, both protocols of test_state_after_greedy_decode[int8] -- a quantised value of h that
# rounds the other way moves a gate by sx * sw; the four shapes of test_int8_shapes stay below 2.4e-7)
INT8_STATE_TOL = 5e-4


def make(lm, dtype="f32", am="tiny", int8=False, sd=None, **kw):
    """an engine on the smallest acoustic model that carries the LM's vocabulary, the LM attached (sd: its weights, if not the
    config's own) -> (engine, acoustic config)"""
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    cfg = dict(synth.model_cfg(am), vocab=E.lm_cfg(lm)["vocab"])
    eng = Engine(synth.synth_state_dict(cfg, seed=0), cfg, dtype=dtype, **kw)
    eng.attach_lm(E.state_dict(lm) if sd is None else sd, int8=int8)
    return eng, cfg


def open_all(eng):
    M = eng.config("M")
    assert [eng.open() for _ in range(M)] == list(range(M))
    return M


def compare(stage, got, what, worst, rows=Ellipsis, name=None):
    """one stage against the engine's values: stage, Y, tol, max |d|, ratio"""
    got = np.asarray(got, F64)
    r = stage.ratio(got, rows)
    d = float(np.abs(got - stage.value[rows]).max()) if got.size else 0.0
    fl = stage.flip[rows]
    note = "" if not fl.any() else f" (flip: {float((fl > 0).mean()):.2f} of the elements, median {float(np.median(fl)):.2g})"
    print(f"  {what:44s} {name or stage.name:10s} Y {stage.Y:.3g} tol {stage.tol:.3g} max |d| {d:.3g} ratio {r:.3g}{note}")
    worst.append((r, what, name or stage.name))


def settle(worst):
    over = [w for w in worst if not w[0] <= 1.0]
    assert not over, over


def listed_slots(B, M):
    """B of the M open slots for a call: every third slot left out while the rest still holds B, in a seeded order"""
    keep = [s for s in range(M) if s % 3 != 2]
    pool = keep if len(keep) >= B else list(range(M))
    rows = pool[:B - 1] + [pool[-1]] if B > 1 else [pool[len(pool) // 2]]       # (the last m-tile of the engine takes part)
    np.random.default_rng(B).shuffle(rows)
    return rows, [s for s in range(M) if s not in rows]


def score_and_read(eng, labels, n, slots, U=None):
    """lasr_lm_score on the rows' first U (or n[r]) labels -> (per-candidate results, lm_raw, lmz of the listed rows, lm_valid)"""
    M = eng.config("M")
    others = [s for s in range(M) if s not in slots]
    before = eng.debug_read("lmz")[others]
    got = eng.lm_score(slots, [labels[r, :(U or n[r])].tolist() for r in range(len(slots))], start=E.START)
    raw, lmz, valid = eng.debug_read("lm_raw"), eng.debug_read("lmz"), eng.debug_read("lm_valid")[0]
    # rows that take no part keep what they had; the closing reset has zeroed the flags and the state of the listed rows
    assert np.array_equal(eng.debug_read("lmz")[others], before)
    assert not valid.any()
    for l in range(eng.lm_cfg["layers"]):
        assert not eng.debug_read("lm_h", l)[slots].any() and not eng.debug_read("lm_c", l)[slots].any()
    return got, raw[slots], lmz[slots]


def check_post(raw, lmz, what, worst, flat=False):
    """k_lm_post alone: lmz against the float64 standardisation of the engine's own raw; entry 0 is min_val exactly.  flat: the
    last row is lm_exact.flat_lm's and a stage of its own (its yardstick is a hundred times the other rows')"""
    assert np.all(lmz[:, 0] == F32(E.MIN_VAL)), what
    if flat:
        compare(E.post_stage(raw[-1:]), lmz[-1:], what, worst, name="lmz|raw flat")
        raw, lmz = raw[:-1], lmz[:-1]
    compare(E.post_stage(raw), lmz, what, worst)


def run_score_case(eng, lm, dtype, B, worst, passes=E.PASSES, ragged=False):
    M = eng.config("M")
    labels, n, tr = E.case(lm, dtype, B, ragged=ragged)
    slots, _ = listed_slots(B, M)
    for U in ((None,) if ragged else passes):
        what = f"{dtype} {lm} M {M} rows {B} " + ("ragged" if ragged else f"U {U}")
        _, raw, lmz = score_and_read(eng, labels, n, slots, U)
        pre = "" if ragged else f"u{U - 1}."
        compare(tr[pre + "raw"], raw, what, worst)
        compare(tr[pre + "lmz"], lmz, what, worst)
        check_post(raw, lmz, what, worst, flat=lm.startswith("v"))


# ----------------------------------------------------------------------------- lasr_lm_score, then raw and lmz
@pytest.mark.parametrize("lm", E.SCORE_LMS["f32"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_score_rows_and_passes(dtype, lm):
    """64-row engine, 1 / 16 / 17 / 33 / 64 rows listed
    in a scrambled order with every third slot left out while there is room, U = 1, 2, 3 passes (zero state, a recurrent h, the
    ping-pong parity both ways), and one ragged call in which the rows have 1 .. 3 passes: a row that is done is carried while the
    others step, and its raw / lmz stay its own last pass."""
    waves, cells, out = next((w, c, o) for name, w, c, o in E.LM_SCHEDULES if name == lm)
    if dtype == "f32":          # (the list restated in f32_exact is the f32 one: 16-wide K chunks)
        assert S.schedule("lm_cell", E.lm_cfg(lm), waves) == cells and S.schedule("lm_out", E.lm_cfg(lm), waves) == out
    eng, _ = make(lm, dtype, max_streams=64)
    worst = []
    try:
        assert open_all(eng) == 64
        for B in E.ROWS64:
            run_score_case(eng, lm, dtype, B, worst)
        run_score_case(eng, lm, dtype, 33, worst, ragged=True)
    finally:
        eng.close()
    settle(worst)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_score_second_row_group(dtype):
    """80 rows of a 128-row engine: a second 64-row group behind the cell launch (R / 64 workgroup rows) and m-tiles 4 .. 7 of the
    output layer"""
    eng, _ = make("h96", dtype, max_streams=128)
    worst = []
    try:
        assert open_all(eng) == 128
        run_score_case(eng, "h96", dtype, E.ROWS128[0], worst)
    finally:
        eng.close()
    settle(worst)


@pytest.mark.parametrize("V", E.VOCABS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_vocabulary_edges(dtype, V):
    """k_lm_post at V = 64 (fewer than 256 columns), 272 (a ragged last slot), 2048 (KEEP 8 full), 2064 (the first KEEP 16 shape)
    and 4096 (the maximum), 17 rows; the last row is the flat one (lm_exact.flat_lm: raw is the output bias, constant to within 2^-13 apart
    from one entry: an std of 1e-3 against which the + 1e-5 shows) and at U = 1 every row is"""
    lm = f"v{V}"
    eng, _ = make(lm, dtype, max_streams=64)
    worst = []
    try:
        assert open_all(eng) == 64
        run_score_case(eng, lm, dtype, E.POST_ROWS, worst)
        labels, n, tr = E.case(lm, dtype, E.POST_ROWS)
        b = E.state_dict(lm)["linear.bias"].astype(F64)
        assert np.array_equal(tr["u2.raw"].value[-1], b) and np.array_equal(tr["u0.raw"].value[0], b)
    finally:
        eng.close()
    settle(worst)


# ----------------------------------------------------------------------------- state behind a greedy decode
def decode_push_step(eng, slots, pcm, n_chunks=None):
    eng.reset_many(slots, 15)
    chunks = [synth.stream_chunks(p, 1280, lead=1, tail=10) for p in pcm]
    got = [[] for _ in slots]
    for k in range(n_chunks or len(chunks[0])):
        eng.push(slots, np.stack([c[k] for c in chunks]))
        if eng.step(slots):
            for i, t in enumerate(eng.fetch_many(slots, cap=512)):
                got[i] += t
    return got


def decode_submit_wait(eng, slots, pcm):
    eng.reset_many(slots, 15)
    chunks = [synth.stream_chunks(p, 1280, lead=1, tail=10) for p in pcm]
    got = [[] for _ in slots]

    def collect():
        for i, t in enumerate(eng.fetch_many(slots, cap=512)):
            got[i] += t

    for k in range(len(chunks[0])):
        eng.push(slots, np.stack([c[k] for c in chunks]))
        eng.submit(slots)
        if eng.pending() >= 3 and eng.wait():
            collect()
    while eng.pending():
        if eng.wait():
            collect()
    return got


def decode_offline(eng, slots, pcm):
    eng.transcribe_pcm(slots, list(pcm))
    return [eng.fetch(s)[0] for s in slots]


def oracle_tokens(m, pcm, streaming):
    out = []
    for p in pcm:
        if streaming:
            fe, dec = O.StreamFrontend(), m.stream_decoder()
            for ch in synth.stream_chunks(p, 1280, lead=1, tail=10):
                o = fe.push(ch)
                if o is not None:
                    dec.step(o)
            out.append(list(dec.y))
        else:
            out.append(list(m.decode_greedy(O.features_offline(p))[0]))
    return out


def check_int8_rows(eng, sd, slots, seqs, what, worst):
    """the int8 rule on the rows `slots` whose emitted tokens are `seqs`"""
    L, H = eng.lm_cfg["layers"], eng.lm_cfg["hidden"]
    Kp = (H + 31) // 32 * 32
    sxh = eng.debug_read("lm_sxh")
    assert sxh.shape[0] == L
    hs, cs = [eng.debug_read("lm_h", l) for l in range(L)], [eng.debug_read("lm_c", l) for l in range(L)]
    qhs = [eng.debug_read("lm_qh", l) for l in range(L)]
    for l in range(L):
        assert qhs[l].shape[1] == Kp
        for s, seq in zip(slots, seqs):
            q, sc = E.quantise(hs[l][s], Kp)
            # bit for bit: the image k_lm_cell_q stored is the reference quantisation of the h it stored beside it
            assert np.array_equal(qhs[l][s], q) and sxh[l, s] == sc, (what, l, s)
            assert not qhs[l][s, H:].any()
            if not seq:
                assert not qhs[l][s].any() and sxh[l, s] == F32(0.1) and not hs[l][s].any() and not cs[l][s].any()
    live = [i for i, seq in enumerate(seqs) if seq]
    rows = [slots[i] for i in live]
    raw, lmz, valid = eng.debug_read("lm_raw"), eng.debug_read("lmz"), eng.debug_read("lm_valid")[0]
    assert [int(valid[s]) for s in slots] == [1 if seq else 0 for seq in seqs]
    v, bound = E.raw_int8(qhs[L - 1][rows], sxh[L - 1][rows], sd)
    d = np.abs(raw[rows].astype(F64) - v)
    r = float((d / bound).max())
    print(f"  {what:44s} {'raw|qh':10s} 2 ulps: bound up to {float(bound.max()):.3g} max |d| {float(d.max()):.3g} ratio {r:.3g}")
    worst.append((r, what, "raw|qh"))
    check_post(raw[rows], lmz[rows], what, worst)
    rh, rc = E.replay_int8(sd, [seqs[i] for i in live])
    dh = max(float(np.abs(hs[l][rows].astype(F64) - rh[l]).max()) for l in range(L))
    dc = max(float(np.abs(cs[l][rows].astype(F64) - rc[l]).max()) for l in range(L))
    print(f"  {what:44s} {'h, c':10s} against the oracle's int8 emulation: max |d| h {dh:.3g} c {dc:.3g} (bound {INT8_STATE_TOL:.0e})")
    worst.append((max(dh, dc) / INT8_STATE_TOL, what, "h, c"))


def check_state_rows(eng, lm, dtype, slots, seqs, what, worst, sharp=(0.0, 0.0)):
    """f32 / bf16: h, c of every layer, raw and lmz of every row against the float64 LM replayed over the row's own tokens (the
    tolerance is the whole-chain Y of that replay); the output layer alone against the engine's own h; k_lm_post alone"""
    L = eng.lm_cfg["layers"]
    tr, n = E.replay(lm, dtype, seqs)
    live = np.nonzero(n > 0)[0]
    rows = [slots[i] for i in live]
    valid = eng.debug_read("lm_valid")[0]
    assert [int(valid[s]) for s in slots] == [int(k > 0) for k in n]
    for l in range(L):
        compare(tr[f"l{l}.h"], eng.debug_read("lm_h", l)[slots], what, worst, name=f"l{l}.h")
        compare(tr[f"l{l}.c"], eng.debug_read("lm_c", l)[slots], what, worst, name=f"l{l}.c")
    # how much of the state the bound still holds sharply (bf16: an allowance that has outgrown the values checks nothing): the
    # share of layer 0's h that must be bit-equal (bound 0: bf16 without a flip), and of c inside a bound below 1e-4 -- `sharp` is
    # what the caller requires of the two
    h0, cs = tr["l0.h"].bound()[live], np.concatenate([tr[f"l{l}.c"].bound()[live] for l in range(L)], 1)
    eq, small = float((h0 == 0).mean()), float((cs < 1e-4).mean())
    print(f"  {what:44s} sharp      layer-0 h bit-equal by the bound in {eq:.2f} of the elements, c bounded below 1e-4 in {small:.2f}")
    assert eq >= sharp[0] and small >= sharp[1], (what, eq, small, sharp)
    raw, lmz = eng.debug_read("lm_raw")[rows], eng.debug_read("lmz")[rows]
    compare(tr["raw"], raw, what, worst, rows=live, name="raw")
    compare(tr["lmz"], lmz, what, worst, rows=live, name="lmz")
    # the output layer alone: the engine's raw against its own h of the last layer (exact operands: the f32 rule, no flip)
    m = E.chain(lm, dtype).m
    h = eng.debug_read("lm_h", L - 1)[rows]
    v = h.astype(F64) @ m.w.T + m.b
    r32 = (h @ m.w.astype(F32).T + m.b.astype(F32)).astype(F32)
    tol, Y = E._tol(r32, v, np.zeros(v.shape))
    compare(E.Stage("raw|h", v, tol, np.zeros(v.shape), Y, r32), raw, what, worst)
    check_post(raw, lmz, what, worst)


@pytest.mark.parametrize("form", ["f32", "bf16", "int8"])
def test_state_after_greedy_decode(form):
    """40 streams of tiny_soft + tiny_lm (three m-tiles), 2 s of audio each, once through push / step and once through submit / wait
    (whose groups carry the LM cell as the second half of paired launches): the tokens are the oracle's (f32 and int8; the bf16
    engine's tokens follow no float32 oracle and are taken as they are), and the LM state of every stream is the LM run over that
    stream's own tokens"""
    dtype, int8 = ("f32", True) if form == "int8" else (form, False)
    eng, cfg = make("tiny_lm", dtype, am="tiny_soft", int8=int8, max_streams=64)
    sd = E.state_dict("tiny_lm")
    worst = []
    try:
        n = 40
        pcm = synth.synth_pcm(n, 16000 * 2, seed=1234)
        slots = [eng.open() for _ in range(n)]
        want = None
        if form != "bf16":
            m = O.OracleTransducer(synth.synth_state_dict(cfg, seed=0), cfg)
            m.lm = O.OracleLM(sd, quantized=int8)
            want = oracle_tokens(m, pcm, True)
        for name, run in (("push / step", decode_push_step), ("submit / wait", decode_submit_wait)):
            seqs = run(eng, slots, pcm)
            if want is not None:
                assert seqs == want, name
            assert sum(1 for s in seqs if s) >= n // 2
            what = f"{form} greedy {name}, {n} streams"
            if int8:
                check_int8_rows(eng, sd, slots, seqs, what, worst)
            else:
                # (f32: no flip anywhere, nothing to require.  bf16: tiny_lm's gates saturate and the rows hold up to a dozen tokens; a quarter of
                # layer 0's h and a twentieth of c are still held sharply -- the short rows)
                check_state_rows(eng, "tiny_lm", dtype, slots, seqs, what, worst, sharp=(0.0, 0.0) if dtype == "f32" else (0.25, 0.05))
    finally:
        eng.close()
    settle(worst)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_state_after_short_decode_hidden_1024(dtype):
    """The LM cells and the output layer at K = 1024 (f32: the (8, 8) schedule; bf16: the only LM shape with more than one K chunk
    per wave), where the lm_score chain of the bf16 case is all allowance: 17 streams of tiny_soft + h1024 through the first 8
    chunks of push / step with at most one token per frame, which leaves rows of one to five tokens -- h and c of both layers
    against the float64 replay (short rows: on the float32 oracle's tokens 0.75 of layer 0's h carries no flip and must be
    bit-equal and 0.77 of c has a bound below 1e-4; half of each is required), and raw against the engine's own h"""
    eng, cfg = make("h1024", dtype, am="tiny_soft", max_streams=32, max_iters_stream=1)
    worst = []
    try:
        n = 17
        pcm = synth.synth_pcm(n, 16000 * 2, seed=1234)
        slots = [eng.open() for _ in range(n)]
        seqs = decode_push_step(eng, slots, pcm, n_chunks=8)
        print(f"  tokens per row {[len(s) for s in seqs]}")
        assert sum(1 for s in seqs if 1 <= len(s) <= 3) >= n // 2
        check_state_rows(eng, "h1024", dtype, slots, seqs, f"{dtype} h1024 push / step, {n} streams", worst,
                         sharp=(0.0, 0.0) if dtype == "f32" else (0.5, 0.5))
    finally:
        eng.close()
    settle(worst)


@pytest.mark.parametrize("V", E.VOCABS)
def test_exactly_constant_row(V):
    """the flat row without its jitter: raw is 0.5 in every entry but one, exactly.  Every rounding error of such a row is the same
    one V - 1 times over, so numpy's own error is one draw of the summation order (3.8e-5 at V = 2064, 9.7e-4 at 4096) and no
    yardstick; the row is held to the conditioning bound of lm_exact.post_conditioning instead -- 4 f32 ulps of |log p|,
    amplified by 1 / (std + 1e-5) -- and its figure is printed (at V = 2064 the 8 Y rule would read 1.71)"""
    lm = f"c{V}"
    eng, _ = make(lm, "f32", max_streams=64)
    try:
        assert open_all(eng) == 64
        slots, _ = listed_slots(E.POST_ROWS, 64)
        eng.lm_score(slots, [[E.FLAT_TOKEN]] * len(slots), start=E.START)
        raw, lmz = eng.debug_read("lm_raw")[slots], eng.debug_read("lmz")[slots]
        assert np.array_equal(raw, np.repeat(E.state_dict(lm)["linear.bias"][None], len(slots), 0))
        v, bound = E.post_conditioning(raw)
        d = np.abs(lmz.astype(F64) - v)
        Y = float(np.abs(np.stack([E.post32(z) for z in raw]).astype(F64) - v).max())
        print(f"  exactly constant row V {V}: max |d| {float(d.max()):.3g}, conditioning bound {float(bound.min()):.3g} "
              f"(ratio {float((d / bound).max()):.3g}); numpy f32 itself {Y:.3g}")
        assert np.all(lmz[:, 0] == F32(E.MIN_VAL)) and np.all(d <= bound)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_readout_errors_and_the_table(dtype):
    """lasr_debug_read's LM matrices: LASR_ESTATE without an LM and for the int8 images of an LM that is not int8-served,
    LASR_EINVAL for a layer out of range; lm_tab (exact f32 with either operand type) against embed x W_ih^T + b_ih + b_hh in
    float64 by the f32 rule"""
    from libreasr_amd import _native as N
    from libreasr_amd.engine import Engine
    cfg = synth.model_cfg("tiny")
    bare = Engine(synth.synth_state_dict(cfg, seed=0), cfg, dtype=dtype, max_streams=8)
    try:
        for what in ("lm_h", "lm_c", "lm_raw", "lmz", "lm_valid", "lm_tab", "lm_qh", "lm_sxh"):
            with pytest.raises(N.LasrError) as ei:
                bare.debug_read(what)
            assert ei.value.code == N.LASR_ESTATE, what
    finally:
        bare.close()
    eng, _ = make("h96", dtype, max_streams=8)
    try:
        for what in ("lm_qh", "lm_sxh"):
            with pytest.raises(N.LasrError) as ei:
                eng.debug_read(what)
            assert ei.value.code == N.LASR_ESTATE, what
        for what in ("lm_h", "lm_c"):
            for index in (-1, 2):
                with pytest.raises(N.LasrError) as ei:
                    eng.debug_read(what, index)
                assert ei.value.code == N.LASR_EINVAL, (what, index)
        sd = E.state_dict("h96")
        emb, w, b = sd["embed.weight"], sd["rnn.weight_ih_l0"], sd["rnn.bias_ih_l0"] + sd["rnn.bias_hh_l0"]
        v = emb.astype(F64) @ w.astype(F64).T + sd["rnn.bias_ih_l0"].astype(F64) + sd["rnn.bias_hh_l0"].astype(F64)
        r32 = (emb @ w.T + b).astype(F32)
        tol, Y = E._tol(r32, v, np.zeros(v.shape))
        worst = []
        compare(E.Stage("lm_tab", v, tol, np.zeros(v.shape), Y, r32), eng.debug_read("lm_tab"), f"{dtype} h96 layer-0 table", worst)
        assert eng.debug_read("lm_valid").shape == (1, eng.config("M")) and eng.debug_read("lm_raw").shape == (eng.config("M"), 64)
    finally:
        eng.close()
    settle(worst)
    q8, _ = make("h96", int8=True, max_streams=8)
    try:
        with pytest.raises(N.LasrError) as ei:
            q8.debug_read("lm_qh", 2)
        assert ei.value.code == N.LASR_EINVAL
        assert q8.debug_read("lm_qh", 1).shape == (q8.config("M"), 96) and q8.debug_read("lm_sxh").shape == (2, q8.config("M"))
    finally:
        q8.close()


# ----------------------------------------------------------------------------- the int8-served form's shapes
INT8_SHAPES = {
    "H36": dict(vocab=64, embed=16, hidden=36, layers=2),            # Kp_h = 64: one register slot, 28 padding columns
    "H260": dict(vocab=64, embed=32, hidden=260, layers=2),          # Kp_h = 288: the second slot ragged
    "H1024": dict(vocab=64, embed=1024, hidden=1024, layers=2),      # all four slots, K = 1024: the limit of exact accumulation
    "E20": dict(vocab=64, embed=20, hidden=32, layers=2),            # Kp_ih = 32
}


@pytest.mark.parametrize("shape", list(INT8_SHAPES))
def test_int8_shapes(shape):
    """a short offline greedy decode on 17 streams (an m-tile and one row) with an 18th slot that emits nothing"""
    lm = INT8_SHAPES[shape]
    eng, cfg = make(lm, am="tiny_soft", int8=True, max_streams=32)
    sd = E.state_dict(lm)
    worst = []
    try:
        n = 17
        pcm = synth.synth_pcm(n, 16000 // 2, seed=1234)
        slots = [eng.open() for _ in range(n + 1)]
        seqs = decode_offline(eng, slots[:n], pcm) + [[]]
        m = O.OracleTransducer(synth.synth_state_dict(cfg, seed=0), cfg)
        m.lm = O.OracleLM(sd, quantized=True)
        assert seqs[:n] == oracle_tokens(m, pcm, False)
        assert sum(1 for s in seqs if s) >= n // 2
        check_int8_rows(eng, sd, slots, seqs, f"int8 {shape} offline, {n} streams", worst)
    finally:
        eng.close()
    settle(worst)


def test_int8_saturation():
    """the comment above lm_qparams at its limit: E = 1024, every quantised activation 127, every quantised weight -128, every
    integer sum of the layer-0 table -16 646 144 = -(2^24 - 131 072): lm_tab = sum * (sx * sw) + b within the 2-ulp rule"""
    sd = E.saturating_lm()
    eng, _ = make(E.SAT_CFG, int8=True, sd=sd, max_streams=8)
    try:
        v, bound, acc = E.tab_int8(sd)
        assert np.all(acc == E.SAT_SUM)
        tab = eng.debug_read("lm_tab")
        assert tab.shape == v.shape
        d = np.abs(tab.astype(F64) - v)
        print(f"  int8 saturation: lm_tab max |d| {float(d.max()):.3g}, bound {float(bound.min()):.3g} (ratio {float((d / bound).max()):.3g})")
        assert np.all(d <= bound)
    finally:
        eng.close()


# ----------------------------------------------------------------------------- the beam: LM rows are hypothesis slots
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_state_after_beam_decode(dtype):
    """beam 4, 8 streams of tiny + tiny_lm, offline: h, c and lmz of the hypothesis slots of every stream against the float64
    replays of that stream's fetch_nbest hypotheses.  k_beam_select leaves the survivors in slots 0 .. in score order and fetch_nbest
    lists the alive hypotheses by score, then slot: hypothesis j is slot j, so the identity assignment is asserted -- every pair
    within the bound in every stage -- and the best of all one-to-one assignments is printed beside it (a slot that had copied
    another parent's state would show there as a better one).  Dead slots are not compared."""
    W, n = 4, 8
    eng, cfg = make("tiny_lm", dtype, am="tiny", beam=W, max_streams=n)
    worst = []
    try:
        pcm = synth.synth_pcm(n, 16000 * 2, seed=1234)
        slots = [eng.open() for _ in range(n)]
        eng.set_beam_records(True)
        eng.transcribe_pcm(slots, list(pcm))
        hyps = [[h[0] for h in eng.fetch_nbest(s)] for s in slots]
        flat = [h for hs in hyps for h in hs]
        assert sum(1 for h in flat if h) >= n
        tr, cnt = E.replay("tiny_lm", dtype, flat)
        L = eng.lm_cfg["layers"]
        hs, cs = [eng.debug_read("lm_h", l) for l in range(L)], [eng.debug_read("lm_c", l) for l in range(L)]
        lmz, valid = eng.debug_read("lmz"), eng.debug_read("lm_valid")[0]
        assert hs[0].shape[0] == eng.config("M") * W
        at, identity = 0, 0
        for i, s in enumerate(slots):
            k = len(hyps[i])
            assert 1 <= k <= W
            rows = [s * W + b for b in range(W)]

            def ratio(b, j):
                """slot b of the stream against hypothesis j: the largest ratio over the stages"""
                r, g = rows[b], at + j
                out = max(max(tr[f"l{l}.h"].ratio(hs[l][r], g), tr[f"l{l}.c"].ratio(cs[l][r], g)) for l in range(L))
                if cnt[g] == 0:
                    return out if valid[r] == 0 else np.inf
                return max(out, tr["lmz"].ratio(lmz[r], g)) if valid[r] == 1 else np.inf

            cost = np.array([[ratio(b, j) for j in range(k)] for b in range(W)])
            best = min(itertools.permutations(range(W), k), key=lambda p: max(cost[p[j], j] for j in range(k)))
            r = max(cost[j, j] for j in range(k))
            identity += best == tuple(range(k))
            print(f"  {dtype} beam stream {i}: {k} hypotheses, lengths {[len(h) for h in hyps[i]]}, worst ratio {r:.3g} (best assignment: slots {best})")
            worst.append((r, f"beam stream {i}", "h, c, lmz"))
            at += k
        print(f"  {dtype} beam: the identity is the best assignment in {identity} of {n} streams")
        assert identity == n
    finally:
        eng.close()
    settle(worst)
