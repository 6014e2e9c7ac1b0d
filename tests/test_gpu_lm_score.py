"""LM sequence scoring on the GPU (lasr_lm_score): log P_LM of candidate transcripts by the attached LM, teacher-forced
through the decode path's LM step, against the float64 restatement of tests/lm_score_ref.py (f32), bit for bit where the definition
says so (every operand mode), against the oracle's int8 emulation (the int8-served form); the state it must leave alone; its error
codes; LibreASR.lm_score / rescore_lm."""
import ctypes as C
import os

import numpy as np
import pytest

import lm_exact as E
import lm_score_ref as LR
from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O

pytestmark = pytest.mark.gpu

TERM_TOL = 2e-3          # f32 terms against float64: the project's bound for lattice terms
# int8-served LM against the oracle's emulation (integer accumulation exact on both sides; the device's expf / tanhf / logf against
# numpy's): 4 x the largest per-term deviation measured on the GPU (1.431e-6 over the terms of test_int8_served_lm, either start
# form), rounded up to one significant digit
INT8_TERM_TOL = 6e-6
SLOTS = (1, 3, 4, 6, 7, 0, 2)          # interleaved: the 7 candidates' rows
_ENGINES, _REFS = {}, {}


def engine(name, lm_name, dtype="f32", int8=False):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    key = (name, lm_name, dtype, int8)
    if key not in _ENGINES:
        graft.build()
        cfg = synth.model_cfg(name)
        eng = Engine(synth.synth_state_dict(cfg, seed=0), cfg, max_streams=8, dtype=dtype)
        eng.attach_lm(synth.synth_lm_state_dict(lm_name), int8=int8)
        _ENGINES[key] = eng
    return _ENGINES[key]


def candidates(vocab=64, seed=7):
    """U = 0, 1, 2, 17, 40, a duplicate of the 17, the 9-label prefix of the 40; labels from [1, vocab), blank is 0"""
    rng = np.random.default_rng(seed)
    c = {u: [int(t) for t in rng.integers(1, vocab, u)] for u in (0, 1, 2, 17, 40)}
    return [c[0], c[1], c[2], c[17], c[40], list(c[17]), c[40][:9]]


def reference(lm_name, cands, start):
    """float64 (total, lp) per candidate, computed once per (LM, candidates, start)"""
    key = (lm_name, tuple(map(tuple, cands)), start)
    if key not in _REFS:
        if lm_name not in _REFS:
            _REFS[lm_name] = LR.LmRef(synth.synth_lm_state_dict(lm_name))
        _REFS[key] = [_REFS[lm_name].score(y, start) for y in cands]
    return _REFS[key]


class open_slots:
    """all 8 slots of an engine, open for the body"""

    def __init__(self, eng, n=8):
        self.eng, self.n = eng, n

    def __enter__(self):
        self.slots = [self.eng.open() for _ in range(self.n)]
        assert self.slots == list(range(self.n))
        return self.slots

    def __exit__(self, *exc):
        for s in self.slots:
            self.eng.close_slot(s)


def check_values(got, ref, label):
    """every term within TERM_TOL of the reference, |total - ref| <= U TERM_TOL; -> (max term deviation, max total deviation)"""
    dt, dT = 0.0, 0.0
    for i, (g, (rt, rlp)) in enumerate(zip(got, ref)):
        U = len(rlp)
        assert g["logps"].shape == (U,) and g["logps"].dtype == np.float32
        if U:
            dt = max(dt, float(np.abs(g["logps"].astype(np.float64) - rlp).max()))
        dT = max(dT, abs(g["total"] - rt))
    print(f"{label}: max |term - ref| {dt:.3e}, max |total - ref| {dT:.3e}")
    for i, (g, (rt, rlp)) in enumerate(zip(got, ref)):
        U = len(rlp)
        if U:
            assert np.abs(g["logps"].astype(np.float64) - rlp).max() <= TERM_TOL, (label, i)
        assert abs(g["total"] - rt) <= U * TERM_TOL, (label, i)
    return dt, dT


def check_exact(eng, got, cands, start):
    """what holds bit for bit in every operand mode"""
    g17, g40, gdup, gpre = got[3], got[4], got[5], got[6]
    assert gdup["total"] == g17["total"] and np.array_equal(gdup["logps"], g17["logps"])
    assert np.array_equal(gpre["logps"], g40["logps"][:9])
    alone = eng.lm_score([5], [cands[3]], start=start)[0]          # slot 5: not one of the batch's
    assert alone["total"] == g17["total"] and np.array_equal(alone["logps"], g17["logps"])
    for i, g in enumerate(got):
        tot = 0.0
        for v in g["logps"]:
            tot += float(v)
        assert g["total"] == tot, i
        assert np.all(np.isfinite(g["logps"])) and np.all(g["logps"] <= 0.0), i
    assert got[0]["total"] == 0.0 and got[0]["logps"].size == 0
    if start is None:
        assert got[1]["total"] == 0.0 and got[1]["logps"].tolist() == [0.0]
        assert all(g["logps"][0] == 0.0 for g in got[1:])


def check_derived(got, lm_name, dtype, cands, start, label):
    """every term within its derived bound (lm_exact.term_bounds: the bound of raw in that pass, twice, plus the log-sum-exp
    reduction's own 8 Y) of the float64 chain on the operands the engine holds; |total - sum| within the sum of the bounds"""
    ref = _REFS.setdefault(("derived", lm_name, dtype, tuple(map(tuple, cands)), start), E.term_bounds(lm_name, dtype, cands, start))
    worst, loose = 0.0, 0
    for i, (g, (lp, bound)) in enumerate(zip(got, ref)):
        d = np.abs(g["logps"].astype(np.float64) - lp)
        if len(d):
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0)).max()))
            loose += int((bound > TERM_TOL).sum())
    n = sum(len(r[0]) for r in ref)
    print(f"{label}: max |term - float64| / derived bound {worst:.3g} over {n} terms ({loose} of them with a bound above {TERM_TOL:g}: what the flips allow)")
    for i, (g, (lp, bound)) in enumerate(zip(got, ref)):
        assert np.all(np.abs(g["logps"].astype(np.float64) - lp) <= bound), (label, i)
        assert abs(g["total"] - lp.sum()) <= bound.sum() + 1e-12, (label, i)


# ------------------------------------------------------------------------------- (a) f32 parity, (b) exact properties
@pytest.mark.parametrize("start", [None, 2])
@pytest.mark.parametrize("name,lm_name", [("tiny_soft", "tiny_lm"), ("tiny_lstm", "tiny_lm_untied")])
def test_f32_terms_against_float64(name, lm_name, start):
    eng = engine(name, lm_name)
    cands = candidates()
    with open_slots(eng):
        got = eng.lm_score(SLOTS, cands, start=start)
        check_values(got, reference(lm_name, cands, start), f"f32 {name}+{lm_name} start={start}")
        check_derived(got, lm_name, "f32", cands, start, f"f32 {name}+{lm_name} start={start}")
        check_exact(eng, got, cands, start)


@pytest.mark.parametrize("start", [None, 2])
def test_bf16_exact_properties(start):
    """the bit-for-bit properties with bf16 operands, and every term within its derived bound (docs/lm_bound.md) of the float64
    chain on the bf16 operands; the deviation from the f32-weight reference is still printed"""
    eng = engine("tiny_soft", "tiny_lm", dtype="bf16")
    cands = candidates()
    with open_slots(eng):
        got = eng.lm_score(SLOTS, cands, start=start)
        check_exact(eng, got, cands, start)
    ref = reference("tiny_lm", cands, start)
    dt = max(float(np.abs(g["logps"].astype(np.float64) - r[1]).max()) for g, r in zip(got, ref) if len(r[1]))
    dT = max(abs(g["total"] - r[0]) for g, r in zip(got, ref))
    print(f"bf16 tiny_soft+tiny_lm start={start}: max |term - ref| {dt:.3e}, max |total - ref| {dT:.3e} (against unrounded weights: recorded)")
    check_derived(got, "tiny_lm", "bf16", cands, start, f"bf16 tiny_soft+tiny_lm start={start}")


# ------------------------------------------------------------------------------- (c) the shipped shape
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_shipped_shape(dtype):
    """cfg2 + lm768 (V = 2048, 4 x 768): f32 within the bound of (a); both types within the derived bound"""
    eng = engine("cfg2", "lm768", dtype=dtype)
    rng = np.random.default_rng(11)
    cands = [[int(t) for t in rng.integers(1, 2048, u)] for u in (12, 5)]
    ref = reference("lm768", cands, 2)
    with open_slots(eng, 2) as slots:
        got = eng.lm_score(slots, cands, start=2)
    if dtype == "f32":
        check_values(got, ref, "f32 cfg2+lm768 start=2")
    else:
        dt = max(float(np.abs(g["logps"].astype(np.float64) - r[1]).max()) for g, r in zip(got, ref))
        dT = max(abs(g["total"] - r[0]) for g, r in zip(got, ref))
        print(f"bf16 cfg2+lm768 start=2: max |term - ref| {dt:.3e}, max |total - ref| {dT:.3e} (against unrounded weights: recorded)")
    check_derived(got, "lm768", dtype, cands, 2, f"{dtype} cfg2+lm768 start=2")
    for g in got:
        assert np.all(np.isfinite(g["logps"])) and np.all(g["logps"] <= 0.0)


# ------------------------------------------------------------------------------- (d) the int8-served LM
def oracle_terms(lm, y, start):
    """OracleLM.step chained over the input sequence of the definition -> float32 terms"""
    lp = np.zeros(len(y), np.float32)
    x = (list(y[:-1]) if start is None else [start] + list(y[:-1])) if len(y) else []
    state = None
    for k, tok in enumerate(x):
        row, state = lm.step(tok, state)
        u = k + (1 if start is None else 0)
        lp[u] = row[y[u]]
    return lp


@pytest.mark.parametrize("start", [None, 2])
def test_int8_served_lm(start):
    eng = engine("tiny_soft", "tiny_lm", int8=True)
    cands = candidates()
    with open_slots(eng):
        got = eng.lm_score(SLOTS, cands, start=start)
        check_exact(eng, got, cands, start)
    lm = O.OracleLM(synth.synth_lm_state_dict("tiny_lm"), quantized=True)
    dev = 0.0
    want = [oracle_terms(lm, y, start) for y in cands]
    for g, w in zip(got, want):
        if len(w):
            dev = max(dev, float(np.abs(g["logps"].astype(np.float64) - w.astype(np.float64)).max()))
    print(f"int8 tiny_soft+tiny_lm start={start}: max |term - oracle int8 emulation| {dev:.3e} (bound {INT8_TERM_TOL:.0e})")
    for i, (g, w) in enumerate(zip(got, want)):
        if len(w):
            assert np.abs(g["logps"].astype(np.float64) - w.astype(np.float64)).max() <= INT8_TERM_TOL, i
    f32 = engine("tiny_soft", "tiny_lm")
    with open_slots(f32):
        ref = f32.lm_score(SLOTS, cands, start=start)
    assert any(g["total"] != r["total"] for g, r in zip(got, ref))


# ------------------------------------------------------------------------------- (e) state
def test_transcribe_after_a_call_is_a_fresh_engines(golden_dir):
    eng = engine("tiny_soft", "tiny_lm")
    g = np.load(os.path.join(golden_dir, "model_tiny_soft__tiny_lm.npz"))
    pcm = synth.synth_pcm(3, 16000 * 3, seed=1234)
    cands = candidates()
    with open_slots(eng, 3) as slots:
        eng.lm_score(slots, [cands[3], cands[4], cands[2]], start=2)
        eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
        for i, s in enumerate(slots):
            assert eng.fetch(s)[0] == list(g[f"off_tokens_{i}"]), i
        eng.lm_score(slots[:2], [cands[4], cands[3]])
        eng.transcribe_pcm(slots, [pcm[i] for i in range(3)])
        for i, s in enumerate(slots):
            assert eng.fetch(s)[0] == list(g[f"off_tokens_{i}"]), i


def stream_run(eng, slot, chunks, hooks):
    """the synchronous streaming protocol on one slot from fresh state; hooks {chunk index: callable} run in front of that chunk's
    push.  -> (tokens, per-step counts, tokens emitted before each hook)"""
    eng.reset(slot, 15)
    toks, counts, seen = [], [], {}
    for k, ch in enumerate(chunks):
        if k in hooks:
            seen[k] = len(toks)
            hooks[k]()
        eng.push([slot], ch[None])
        if eng.step([slot]):
            t = eng.fetch(slot)[0]
            toks += t
            counts.append(len(t))
    return toks, counts, seen


@pytest.mark.parametrize("int8", [False, True])
def test_streaming_slot_keeps_its_lm_state(int8):
    """slot A mid-utterance, LM attached: lm_score on two OTHER slots between two of its steps changes nothing for A (the rows that
    do not take part are carried, the h ping-pong parity is stored back: an odd and an even number of passes); with A itself listed
    the call is, for A, reset(A, 4) at that point"""
    eng = engine("tiny_soft", "tiny_lm", int8=int8)
    cands = candidates()
    pcm = synth.synth_pcm(1, 16000 * 3, seed=1234)[0]
    chunks = synth.stream_chunks(pcm, 1280, lead=1, tail=10)
    # in front of chunk 6 A has emitted 3 tokens and what its LM state holds there decides a later re-pick: losing it (reset(A, 4))
    # changes the transcript (found with the numpy oracle, which the engine's tokens equal); so the hooks below act where A's LM
    # state is live
    k1 = 6
    with open_slots(eng, 3) as (A, B, Cc):
        base = stream_run(eng, A, chunks, {})
        odd = lambda: eng.lm_score([B, Cc], [cands[3], cands[2]], start=2)           # 17 passes
        even = lambda: eng.lm_score([Cc, B], [cands[4], cands[6]], start=2)          # 40 passes
        for hook in (odd, even):
            other = stream_run(eng, A, chunks, {k1: hook})
            assert other[2][k1] == 3
            assert other[0] == base[0] and other[1] == base[1]
        both = stream_run(eng, A, chunks, {k1: odd, k1 + 7: even})
        assert both[0] == base[0] and both[1] == base[1]
        listed = stream_run(eng, A, chunks, {k1: lambda: eng.lm_score([B, A], [cands[3], cands[2]], start=2)})
        reset4 = stream_run(eng, A, chunks, {k1: lambda: eng.reset(A, 4)})
        assert listed[0] == reset4[0] and listed[1] == reset4[1]
        assert reset4[0] != base[0]                                                  # (the LM state at the hook matters)


# ------------------------------------------------------------------------------- (f) errors
def raw_call(eng, slots, toks, n=None, start=2, total=True):
    """lasr_lm_score itself -> its return code"""
    a = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    ts = [np.asarray(t, dtype=np.int32).reshape(-1) for t in toks]
    nt = np.ascontiguousarray(np.array([t.size for t in ts], dtype=np.int32))
    tok = np.ascontiguousarray(np.concatenate(ts + [np.zeros(1, np.int32)]))
    tot = np.zeros(max(len(ts), 1), np.float64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    return eng.lib.lasr_lm_score(eng.ctx, p(a), len(ts) if n is None else n, p(tok), p(nt), start, p(tot) if total else None, None)


def test_errors_leave_everything_as_it_was(golden_dir):
    from libreasr_amd.engine import Engine
    eng = engine("tiny_soft", "tiny_lm")
    g = np.load(os.path.join(golden_dir, "model_tiny_soft__tiny_lm.npz"))
    pcm = synth.synth_pcm(3, 16000 * 3, seed=1234)

    def unchanged(slots):
        eng.transcribe_pcm(slots[:3], [pcm[i] for i in range(3)])
        for i in range(3):
            assert eng.fetch(slots[i])[0] == list(g[f"off_tokens_{i}"]), i

    V = 64
    with open_slots(eng, 7) as slots:                     # slot 7 stays closed
        unchanged(slots)
        cases = [
            ("label = blank", dict(slots=[0, 1], toks=[[5, 0, 6], [7]])),
            ("label = V", dict(slots=[0, 1], toks=[[5, 6], [V]])),
            ("start = V", dict(slots=[0], toks=[[5, 6]], start=V)),
            ("start = -2", dict(slots=[0], toks=[[5, 6]], start=-2)),
            ("a slot listed twice", dict(slots=[2, 2], toks=[[5], [6]])),
            ("a closed slot", dict(slots=[0, 7], toks=[[5], [6]])),
            ("n = 9 on 8 slots", dict(slots=list(range(9)), toks=[[5]] * 9)),
            ("U = 1536", dict(slots=[0], toks=[[5] * 1536])),
            ("null total", dict(slots=[0], toks=[[5, 6]], total=False)),
        ]
        for what, kw in cases:
            assert raw_call(eng, **kw) == N.LASR_EINVAL, what
            unchanged(slots)
        assert raw_call(eng, [0], [[5] * 1535]) == N.LASR_OK          # (the limit itself is served)
        # a submitted, uncollected step
        eng.reset_many(slots[:3], 15)
        chunk = synth.stream_chunks(pcm[0], 1280, lead=1, tail=0)
        for ch in chunk:                                   # (the first chunks of a stream complete no model step)
            eng.push([slots[0]], ch[None])
            eng.submit([slots[0]])
            if eng.pending():
                break
        assert eng.pending() > 0
        assert raw_call(eng, [1], [[5, 6]]) == N.LASR_ESTATE
        while eng.pending():
            eng.wait()
        unchanged(slots)
    # no LM attached; a beam context (on "tiny": the beam's best hypothesis of this utterance is not empty there)
    for name, kw, want in (("tiny_soft", dict(), N.LASR_ESTATE), ("tiny", dict(beam=2), N.LASR_EINVAL)):
        cfg = synth.model_cfg(name)
        sd = synth.synth_state_dict(cfg, seed=0)
        e2 = Engine(sd, cfg, max_streams=8, **kw)
        if kw:
            e2.attach_lm(synth.synth_lm_state_dict("tiny_lm"))
        s = e2.open()
        e2.transcribe_pcm([s], [pcm[0]])
        before = e2.fetch(s)[0]
        assert raw_call(e2, [s], [[5, 6]]) == want, kw
        with pytest.raises(N.LasrError) as ei:
            e2.lm_score([s], [[5, 6]], start=2)
        assert ei.value.code == want
        e2.transcribe_pcm([s], [pcm[0]])
        assert e2.fetch(s)[0] == before and len(before) > 0
        e2.close()


# ------------------------------------------------------------------------------- (g) the facade
def test_facade_lm_score_and_rescore_lm():
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", synthetic="tiny_soft", synthetic_lm="tiny_lm", max_streams=4)
    eng = asr.engine
    cands = candidates()[:6]                               # two groups on 4 slots
    pcm = synth.synth_pcm(1, 16000 * 2, seed=1234)[0]
    try:
        want = []
        for i in range(0, 6, 4):
            part = cands[i:i + 4]
            slots = [eng.open() for _ in part]
            want += [r["total"] for r in eng.lm_score(slots, part, start=2)]
            for s in slots:
                eng.close_slot(s)
        lm = asr.lm_score(cands, start=2)
        assert lm == want
        am = asr.rescore(pcm, cands)
        r = asr.rescore_lm(pcm, cands, lm_weight=0.35, length_bonus=0.2, start=2)
        assert r["am"] == am and r["lm"] == lm
        score = [float(np.float64(a) + np.float64(0.35) * np.float64(l) + np.float64(0.2) * np.float64(len(y))) for a, l, y in zip(am, lm, cands)]
        assert r["score"] == score
        assert r["best"] == int(np.argmax(score)) and r["order"] == sorted(range(6), key=lambda j: (-score[j], j))
        r0 = asr.rescore_lm(pcm, cands, lm_weight=0.0, length_bonus=0.0, start=2)
        assert r0["best"] == int(np.argmax(am)) and r0["score"] == am
        assert asr.lm_score(cands) == [x["total"] for i in range(0, 6, 4) for x in _engine_group(eng, cands[i:i + 4])]
    finally:
        eng.close()


def _engine_group(eng, part):
    slots = [eng.open() for _ in part]
    try:
        return eng.lm_score(slots, part)
    finally:
        for s in slots:
            eng.close_slot(s)
