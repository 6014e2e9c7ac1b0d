"""The front-end kernels, stage by stage, against float64 of the same stage (tests/frontend_ref.py, docs/frontend_bound.md) on
every launch path and geometry: k_logmel offline / per chunk / by-value windows, k_fe_mel with the chunk from the ring, from the
caller's buffer (`src`) and with the deferred chunk (`src2`), frames computed early (materialize_pending), k_stack,
k_stack_ln<20,10> / <32,0>, k_ln_tile, k_push_pcm.

A stage behind the first is fed with what the engine produced: x0 is compared with the float64 LayerNorm of the `pend` read back
from the device, so the FFT's rounding does not widen the LayerNorm check.  The PCM ring is compared exactly, and the fused
kernels are compared bit for bit with the per-chunk kernels (LASR_FE_LEGACY) on the same chunks.  `tiny` weights everywhere; every
test prints its worst error / bound (run with -s; docs/frontend_bound.md keeps the table)."""
import os

import numpy as np
import pytest
import torch

import frontend_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
FE_KEYS = ("win", "hop", "n_mels", "n_stack", "stride", "n_buffer", "n_window", "chunk")
MAX_STREAMS = 20
ROWS = (0, 15, 16, 19)            # both m-tiles of k_ln_tile, the last slot; slot 16 is driven one chunk late
LATE = (16,)
_ENGINES = {}


class Eng:
    def __init__(self, name, legacy, dtype):
        import __graft_entry__ as graft
        from libreasr_amd.engine import Engine
        graft.build()
        self.g = g = R.STREAM_GEOMETRIES[name] if name in R.STREAM_GEOMETRIES else R.OFFLINE_GEOMETRIES[name]
        cfg, sd = R.tiny_model(g)
        old = os.environ.pop("LASR_FE_LEGACY", None)
        if legacy:
            os.environ["LASR_FE_LEGACY"] = "1"
        try:
            self.eng = Engine(sd, cfg, max_streams=MAX_STREAMS, dtype=dtype, **{k: g[k] for k in FE_KEYS})
        finally:
            os.environ.pop("LASR_FE_LEGACY", None)
            if old is not None:
                os.environ["LASR_FE_LEGACY"] = old
        self.legacy, self.bf = legacy, dtype == "bf16"
        self.fused = R.fused(g, legacy)
        self.w = np.asarray(sd["encoder.input_norm.weight"], F32)
        self.b = np.asarray(sd["encoder.input_norm.bias"], F32)
        assert [self.eng.open() for _ in range(MAX_STREAMS)] == list(range(MAX_STREAMS))


def engine(name, legacy=False, dtype="f32"):
    key = (name, legacy, dtype)
    if key not in _ENGINES:
        _ENGINES[key] = Eng(name, legacy, dtype)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.eng.close()
    _ENGINES.clear()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------ offline: k_logmel, k_stack
@pytest.mark.parametrize("name", sorted(R.OFFLINE_GEOMETRIES))
def test_offline_logmel_against_float64(name):
    """Engine.logmel: 3 different rows, five signals, lengths with T % 4 in {0, 1, 2, 3} (a wave without a frame recomputes the last
    one and must not store: the words behind the last frame keep their sentinel) down to 513 samples, where one frame reflects on
    both sides.  Engine.stack of the result is the reference stacking, bit for bit."""
    from libreasr_amd.engine import _ptr
    E = engine(name)
    g, eng = E.g, E.eng
    worst = {}
    if g["hop"] == 160:
        assert sorted({(1 + n // 160) % 4 for n in R.OFFLINE_LENGTHS}) == [0, 1, 2, 3]
    for sig in R.SIGNALS:
        r_sig = 0.0
        for n in R.OFFLINE_LENGTHS:
            x = R.signal(sig, 3, n)
            T = 1 + n // g["hop"]
            words = 3 * T * g["n_mels"]
            buf = torch.full((words + 4 * g["n_mels"],), -777.0, device="cuda", dtype=torch.float32)
            eng._chk(eng.lib.lasr_logmel(eng.ctx, _ptr(dev(x)), 3, n, _ptr(buf)))
            out = buf.cpu().numpy()
            assert np.all(out[words:] == -777.0), (name, sig, n, "stored behind the last frame")
            out = out[:words].reshape(3, T, g["n_mels"])
            for r in range(3):
                v, b = R.logmel64(x[r], **g)
                ratio = R.ratio(out[r], v, b)
                assert ratio <= 1.0, (name, sig, n, r, ratio)
                r_sig = max(r_sig, ratio)
            if T >= g["n_stack"]:
                st = eng.stack(dev(out)).cpu().numpy()
                for r in range(3):
                    assert np.array_equal(st[r], R.stack(out[r], g["n_stack"], g["stride"])), (name, sig, n, r)
        worst[sig] = round(r_sig, 3)
    print(f"\noffline {name}: worst error / bound {worst}")


def test_offline_logmel_refuses_a_signal_no_longer_than_the_padding():
    from libreasr_amd._native import LASR_EINVAL, LasrError
    eng = engine("default").eng
    with pytest.raises(LasrError) as e:
        eng.logmel(torch.zeros(1, 512, device="cuda"))
    assert e.value.code == LASR_EINVAL
    assert eng.logmel(torch.zeros(1, 513, device="cuda")).shape == (1, 4, 128)


# ------------------------------------------------------------------------------------------------ streaming
class Tracker:
    """What the engine should hold for the rows of a scenario: the float64 stream per row, the PCM ring and its position"""

    def __init__(self, E, rows, whole_pend=True):
        self.E, self.rows = E, list(rows)
        g, eng = E.g, E.eng
        for s in self.rows:
            eng.reset(s, 15)
        self.ring = eng.debug_read("ring")
        self.RC = self.ring.shape[1] // g["chunk"]
        assert self.RC == R.ring_chunks(g, E.legacy), "the engine did not take the expected front-end path"
        ints = eng.debug_read("ints")
        assert np.array_equal(ints[0], ints[1])
        self.pos = {s: int(ints[1, s]) for s in self.rows}
        self.ref = {s: R.StreamRef(g) for s in self.rows}
        self.whole_pend = whole_pend and E.fused          # nothing runs on a chunk that completes no model step
        self.worst = [0.0, 0.0]
        self.worst_row = {s: [0.0, 0.0] for s in self.rows}
        self.records = []

    def push(self, s, chunk):
        ch = self.E.g["chunk"]
        self.ring[s, self.pos[s] * ch:(self.pos[s] + 1) * ch] = chunk
        self.pos[s] = (self.pos[s] + 1) % self.RC
        self.ref[s].push(chunk)

    def will_step(self, s, windowed=False):
        r, g = self.ref[s], self.E.g
        return (windowed or r.n >= g["n_window"]) and len(r.saved) == g["n_buffer"] - 1

    def read(self):
        eng, nb = self.E.eng, self.E.g["n_buffer"]
        return eng.debug_read("pend"), np.stack([eng.debug_read("x0", t) for t in range(nb)], 1)      # [M, nb * ns * nm], [M, nb, F]

    def verify(self, outs, before):
        """outs: row -> (value, bound) of the rows whose model ran in the call; before: read() in front of the call (or None when
        every row of the scenario ran)"""
        E, g = self.E, self.E.g
        ns, nm, nb = g["n_stack"], g["n_mels"], g["n_buffer"]
        pend, x0 = self.read()
        rec = {}
        for s, (v, bd) in outs.items():
            P = pend[s].reshape(nb * ns, nm)
            r = R.ratio(P, v, bd)
            assert r <= 1.0, ("pend", s, len(self.records), r)
            self.worst[0], self.worst_row[s][0] = max(self.worst[0], r), max(self.worst_row[s][0], r)
            y, yb = R.stream_x0_64(P, g, E.w, E.b)
            if E.bf:
                y, yb = R.bf16_allowance(y, yb)
            r = R.ratio(x0[s], y, yb)
            assert r <= 1.0, ("x0", s, len(self.records), r)
            self.worst[1], self.worst_row[s][1] = max(self.worst[1], r), max(self.worst_row[s][1], r)
            rec[s] = (P.copy(), x0[s].copy())
        ring, ints = E.eng.debug_read("ring"), E.eng.debug_read("ints")
        for s in self.rows:
            assert np.array_equal(ring[s], self.ring[s]), ("ring", s, len(self.records))
            assert ints[0, s] == ints[1, s] == self.pos[s], ("ring position", s, len(self.records), ints[0, s], ints[1, s], self.pos[s])
            if s in outs:
                continue
            assert before is not None
            assert np.array_equal(x0[s], before[1][s]), ("x0 of a row that did not step", s)
            keep = len(self.ref[s].saved) * ns * nm         # frames the row has collected for its next step may have been written
            lo = 0 if self.whole_pend else keep
            assert np.array_equal(pend[s, lo:], before[0][s, lo:]), ("pend of a row that did not step", s)
        self.records.append(rec)


    def by_signal(self):
        """worst error / bound (pend, x0) per signal: row i of a scenario carries STREAM_SIGNALS[i % 4]"""
        return {R.STREAM_SIGNALS[i % len(R.STREAM_SIGNALS)]: tuple(round(r, 3) for r in self.worst_row[s]) for i, s in enumerate(self.rows)}


def run_sync(E, rows, late, n_chunks, pushes_per_step=1, seed=0):
    """push + step on every call; rows in `late` start one call late, so their model steps fall on other calls.
    pushes_per_step = 2: the irregular client (two chunks between step calls: the first frame of a step is computed early)."""
    eng, g = E.eng, E.g
    tr = Tracker(E, rows, whole_pend=pushes_per_step == 1)
    pcm = R.stream_pcm(g, len(rows), n_chunks, seed=seed)
    sent = {s: 0 for s in rows}
    n_calls = n_chunks // pushes_per_step + 1
    for call in range(n_calls):
        act = [s for s in rows if (call >= 1 or s not in late) and sent[s] + pushes_per_step <= n_chunks]
        if not act:
            continue
        for _ in range(pushes_per_step):
            eng.push(act, np.stack([pcm[rows.index(s), sent[s]] for s in act]))
            for s in act:
                tr.push(s, pcm[rows.index(s), sent[s]])
                sent[s] += 1
        stepping = [s for s in act if tr.will_step(s)]
        before = tr.read() if stepping and len(stepping) < len(rows) else None
        ran = eng.step(act)
        outs = {s: o for s in act for o in [tr.ref[s].collect()] if o is not None}
        assert sorted(outs) == stepping and ran == len(stepping)
        if outs:
            eng.fetch_many(act, 256)
            tr.verify(outs, before)
    assert len(tr.records) >= 2
    return tr


def run_push_submit(E, rows, n_chunks, form, seed=0):
    """lasr_push_submit with one step in flight: form "host" (numpy chunk: staged, the chunk that completes no step is deferred and
    rides as src2), "stable" (device tensor, device_stable: deferred), "plain" (device tensor: appended at once).  The rows are in
    phase; state is read only behind wait(), so no read flushes a deferred chunk."""
    eng, g = E.eng, E.g
    tr = Tracker(E, rows)
    pcm = R.stream_pcm(g, len(rows), n_chunks, seed=seed)
    all_dev = dev(pcm.transpose(1, 0, 2))                     # [n_chunks, rows, chunk], alive until the end (device_stable)
    taken0 = eng.config("lazy_taken")
    for k in range(n_chunks):
        if form == "host":
            eng.push_submit(rows, np.ascontiguousarray(pcm[:, k]))
        else:
            eng.push_submit(rows, all_dev[k], device_stable=form == "stable")
        for i, s in enumerate(rows):
            tr.push(s, pcm[i, k])
        outs = {s: o for s in rows for o in [tr.ref[s].collect()] if o is not None}
        assert eng.pending() == (1 if outs else 0)
        if outs:
            assert eng.wait() == len(rows)
            eng.fetch_many(rows, 256)
            tr.verify(outs, None)
    steps = len(tr.records)
    assert steps >= 2
    taken = eng.config("lazy_taken") - taken0
    if E.fused and form != "plain" and g["n_buffer"] > 1:
        assert taken >= steps - 1, (form, taken, steps)         # the chunk in front of a step's rode in the step's launch (src2)
    else:
        assert taken == 0
    return tr


def same_records(a, b):
    assert len(a.records) == len(b.records) > 0
    for ra, rb in zip(a.records, b.records):
        assert sorted(ra) == sorted(rb)
        for s in ra:
            assert np.array_equal(ra[s][0], rb[s][0]), ("pend: fused against per-chunk kernels", s)
            assert np.array_equal(ra[s][1], rb[s][1]), ("x0: fused against per-chunk kernels", s)


def both(name, run):
    """the scenario on the engine as it comes and on one created with LASR_FE_LEGACY: each against float64, and, where the first
    one takes the fused kernels, the two bit for bit"""
    a, b = run(engine(name)), run(engine(name, legacy=True))
    same_records(a, b)
    print(f"\n{name}: fused={engine(name).fused}, {len(a.records)} model steps, worst error / bound (pend, x0): {a.by_signal()}"
          f" (per-chunk kernels: pend {b.worst[0]:.3f} x0 {b.worst[1]:.3f})")
    return a


@pytest.mark.parametrize("name", ["default", "nbuf1", "nbuf4", "ring17", "chunk1282"])
def test_streaming_rows_and_depths_against_float64_and_the_per_chunk_kernels(name):
    """push + step: slots 0, 15, 16 and 19 of 20, slot 16 one chunk late (one k_ln_tile m-tile then holds rows that step and rows
    that do not: those keep pend and x0 bit for bit), every ring slot the head twice.  Buffer depths 1, 2, 4; a ring of
    n_window + n_buffer - 1 = 17 chunks (more than the packed ring position of k_fe_mel holds: that geometry takes the per-chunk
    kernels); chunks of 1282 samples."""
    g = R.STREAM_GEOMETRIES[name]
    both(name, lambda E: run_sync(E, list(ROWS), LATE, R.stream_len(g)))


@pytest.mark.parametrize("form", ["host", "stable", "plain"])
def test_push_submit_forms_against_float64_and_the_per_chunk_kernels(form):
    g = R.STREAM_GEOMETRIES["default"]
    both("default", lambda E: run_push_submit(E, [0, 15, 19], R.stream_len(g) + 1, form, seed=3))


@pytest.mark.parametrize("name", ["ring17", "chunk1282", "nbuf4"])
def test_push_submit_other_geometries(name):
    """the chunk taken from the caller's buffer and the deferred one with 1282-sample chunks (rows of the source not 16-byte
    aligned: the scalar copy), with a Buffer of 4 (three chunks between steps: the older deferred ones are appended by launches of
    their own, the last rides in the step's), and on the 17-chunk geometry"""
    g = R.STREAM_GEOMETRIES[name]
    both(name, lambda E: run_push_submit(E, [0, 15, 19], R.stream_len(g) + 1, "host", seed=4))


def test_irregular_client_against_float64_and_the_per_chunk_kernels():
    """two chunks between step calls: the window of a step's first frame would leave the ring, so the frame is computed early
    (materialize_pending: k_logmel over the ring, window selected by its age) and the step's k_fe_mel launch skips it (age 15)"""
    g = R.STREAM_GEOMETRIES["default"]
    both("default", lambda E: run_sync(E, [0, 15, 16], LATE, 2 * R.stream_len(g), pushes_per_step=2, seed=5))


@pytest.mark.parametrize("name", ["mel64", "mel40"])
def test_streaming_generic_shapes_against_float64(name):
    """mel64: 64 mels x 12 frames, Buffer of 3, a 4-chunk window of 960-sample chunks, win 320 / hop 120 (the odd shape of
    test_odd_shapes_take_the_generic_paths, now on values).  mel40: 40 mels x 6 frames, feat 240 -- k_stack_ln<32, 0> with F no
    multiple of 64, so lanes run past F."""
    g = R.STREAM_GEOMETRIES[name]
    E = engine(name)
    assert not E.fused and (name != "mel40" or (g["n_mels"] * g["n_stack"]) % 64 != 0)
    tr = run_sync(E, list(ROWS), LATE, R.stream_len(g), seed=6)
    print(f"\n{name}: {len(tr.records)} model steps, worst error / bound (pend, x0): {tr.by_signal()}")


def test_bf16_engine_x0_by_the_bf16_rule():
    """dtype=bf16: pend is float32 as before; x0 is bf16(float64 LayerNorm of the device's pend) unless that value lies within the
    LayerNorm bound of a rounding midpoint -- then it may be the neighbour (the rule of tests/bf16_exact.py for x0)"""
    g = R.STREAM_GEOMETRIES["default"]
    E = engine("default", dtype="bf16")
    tr = run_sync(E, list(ROWS), LATE, R.stream_len(g), seed=7)
    same = [np.array_equal(rec[s][1], R.bf16(R.stream_x0_64(rec[s][0], g, E.w, E.b)[0])) for rec in tr.records for s in rec]
    print(f"\nbf16: {len(tr.records)} model steps, pend worst error / bound {tr.worst[0]:.3f}; x0 equal to bf16(float64) on every element "
          f"in {sum(same)} of {len(same)} (row, step) pairs, within the tie allowance in the rest")


def test_step_window_against_float64():
    """lasr_step_window at 16 kHz (the by-value window form of k_logmel + k_stack_ln): windows of 3 x 1280, 3 x 2000 and 2400
    samples (16 frames: the fewest that leave n_stack behind the cut; 2399 samples are refused), two slots out of phase"""
    from libreasr_amd._native import LASR_EINVAL, LasrError
    E = engine("default")
    eng, rows = E.eng, [1, 17]
    worst = {}
    for N in R.WINDOW_LENGTHS:
        tr = Tracker(E, rows, whole_pend=False)
        calls = 6
        wins = R.step_windows(N, 2, calls)
        for call in range(calls):
            act = rows if call >= 1 else rows[:1]
            w = {rows[0]: wins[0, call], rows[1]: wins[1, call - 1]}
            stepping = [s for s in act if tr.will_step(s, windowed=True)]
            before = tr.read() if stepping and len(stepping) < len(rows) else None
            ran = eng.step_window(act, np.stack([w[s] for s in act]))
            outs = {s: o for s in act for o in [tr.ref[s].collect_window(w[s])] if o is not None}
            assert sorted(outs) == stepping and ran == len(stepping)
            if outs:
                eng.fetch_many(act, 256)
                tr.verify(outs, before)
        assert len(tr.records) == 5
        worst[N] = (round(tr.worst[0], 3), round(tr.worst[1], 3))
    with pytest.raises(LasrError) as e:
        eng.step_window(rows[:1], np.zeros((1, 2399), F32))
    assert e.value.code == LASR_EINVAL
    for s in rows:
        eng.reset(s, 15)
    print(f"\nstep_window: worst error / bound (pend, x0) per window length {worst}")
