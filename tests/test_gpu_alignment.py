"""Per-token alignment records on the GPU (lasr_set_alignments / lasr_fetch_aligned / lasr_fetch_many_aligned): for every token
greedy decode emits, the encoder frame it was emitted on and the joint's log p of that decision.

Expected values: the numpy oracle's per-evaluation logits replayed by test_alignment_cpu.derive (pinned to the oracle there).
Tokens and frames must be equal; log p within 1e-3, the project's fp32 bound for the log-prob of the argmax
(test_gpu_parity.test_predictor_and_joint).  Shapes and seeds are those on which token parity is a merge gate already: tiny and
tiny_lstm, 3.0 s, seed 1234."""
import numpy as np
import pytest

from libreasr_amd import _native as N
from libreasr_amd import synth
from oracle import rnnt_oracle as O
from test_alignment_cpu import derive, utterances

pytestmark = pytest.mark.gpu

TOKRING = 512          # lasr_ctx::TOKRING: entries per row of the pipelined protocol's token / record rings
LOGP_TOL = 1e-3


def make(name, dtype="f32", lm=None, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    cfg = synth.model_cfg(name)
    sd = synth.synth_state_dict(cfg, seed=0)
    eng = Engine(sd, cfg, max_streams=8, dtype=dtype, **kw)
    m = O.OracleTransducer(sd, cfg)
    if lm:
        lsd = synth.synth_lm_state_dict(lm)
        eng.attach_lm(lsd)
        m.lm = O.OracleLM(lsd)
    return eng, m


_REF = {}


def offline_ref(name, lm=None):
    """per utterance of test_alignment_cpu.utterances(): (tokens, frames, logps, align, T) from the oracle (computed once)"""
    key = (name, lm)
    if key not in _REF:
        cfg = synth.model_cfg(name)
        m = O.OracleTransducer(synth.synth_state_dict(cfg, seed=0), cfg)
        if lm:
            m.lm = O.OracleLM(synth.synth_lm_state_dict(lm))
        out = []
        for p in utterances():
            feats = O.features_offline(p)
            y, _, score, _, outs = m.decode_greedy(feats, max_iters=3, return_logits=True)
            recs, t_end, _, _ = derive(outs, feats.shape[0], 3, m.blank)
            assert t_end == feats.shape[0] and len(recs) == len(y)
            out.append((y, [f for f, _ in recs], [lp for _, lp in recs], score, feats.shape[0]))
        _REF[key] = out
    return _REF[key]


_STREAM_REF = {}
SILENCE = float(np.log(np.float32(1e-6)))      # the log-mel floor: what every feature of a chunk of zeros is


class StreamRef(list):
    """per model step (tokens, frames, logps); .speech: the number of leading model steps that still see audio (see stream_ref)"""
    speech = 0


def stream_ref(name, n_sec, seed_row, reset_at=None, lm=None):
    """one stream (row `seed_row` of synth_pcm(.., seed=1234)) through the oracle's streaming front-end and decoder: per model
    step (tokens, frames counted from the first step, logps).  reset_at: the decoder is reset before that model step.

    These streams end in tail=10 chunks of zeros, so their last model steps (19 to 22 of 23) see nothing but digital silence:
    every input feature is the floor log(1e-6).  On such a frame the model's normalisations divide rounding noise by sqrt(eps),
    and the float32 oracle stops defining decisions and log p to this file's bounds: on `tiny`, row 0, step 22 the decision
    between blank and token 16 on frame 44 has a margin of 0.0028, and the emission lands on frame 44 or 45 with the rounding.
    .speech counts the leading model steps with any feature above the floor.  Those steps are compared against the oracle with
    the bounds unchanged (tokens and frames equal, log p within LOGP_TOL); the silent steps behind them, where the carried
    state may differ already, are checked for structure and for the frame count only (check_structure)."""
    key = (name, n_sec, seed_row, reset_at, lm)
    if key not in _STREAM_REF:
        cfg = synth.model_cfg(name)
        m = O.OracleTransducer(synth.synth_state_dict(cfg, seed=0), cfg)
        if lm:
            m.lm = O.OracleLM(synth.synth_lm_state_dict(lm))
        pcm = synth.synth_pcm(seed_row + 1, int(16000 * n_sec), seed=1234)[seed_row]
        fe, dec = O.StreamFrontend(), m.stream_decoder()
        steps, base, speech = StreamRef(), 0, None
        for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=10):
            o = fe.push(ch)
            if o is None:
                continue
            if reset_at is not None and len(steps) == reset_at:
                dec.reset()
            if speech is None and float(np.abs(np.asarray(o, np.float64) - SILENCE).max()) < 1e-4:
                speech = len(steps)
            y_seq, outs = dec.step(o, return_logits=True)
            recs, t_end, _, _ = derive(outs, o.shape[0], 10, m.blank)
            assert t_end == o.shape[0] and len(recs) == len(y_seq)
            steps.append((y_seq, [base + f for f, _ in recs], [lp for _, lp in recs]))
            base += o.shape[0]
        steps.speech = len(steps) if speech is None else speech
        _STREAM_REF[key] = steps
    return _STREAM_REF[key]


def check_structure(got, lo, hi, what):
    """records of a model step, whatever they are: well-formed and inside the step's frames [lo, hi)"""
    tok, fr, lp = got
    assert len(tok) == len(fr) == len(lp), what
    assert all(lo <= f < hi for f in fr) and np.all(np.diff(np.asarray(fr, np.int64)) >= 0), (what, list(fr))
    assert np.bincount(np.asarray(fr, np.int64) - lo, minlength=1).max() <= 10, what
    assert np.all(np.isfinite(lp)) and np.all(np.asarray(lp) <= 0), what


def align_from_frames(frames, T, max_iters):
    """alignment_score (models.py:445-453) from the emission frames alone: a frame with n tokens took n + 1 evaluations, or
    max_iters when the cap was hit"""
    per = np.bincount(np.asarray(frames, np.int64), minlength=T)
    it = np.where(per == max_iters, max_iters, per + 1)
    return (it.sum() - (it == 1).sum()) / (it.sum() + 1e-4)


def check_records(got, want, what):
    tok, fr, lp = got
    wt, wf, wl = want
    assert list(tok) == list(wt), (what, "tokens")
    assert list(fr) == list(wf), (what, "frames", list(fr), list(wf))
    assert np.asarray(lp).dtype == np.float32 and len(lp) == len(wl)
    if len(wl):
        err = float(np.abs(np.asarray(lp, np.float64) - np.asarray(wl, np.float64)).max())
        assert err < LOGP_TOL, (what, "log p", err)


# ------------------------------------------------------------------------------- 1. offline
@pytest.mark.parametrize("la", [1, 2, 4])
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_offline_records_match_the_oracle(name, la, monkeypatch):
    monkeypatch.setenv("LASR_LOOKAHEAD", str(la))
    eng, _ = make(name)
    try:
        assert eng.config("la_offline") == la
        eng.set_alignments(True)
        slots = [eng.open() for _ in range(6)]
        use = [slots[4], slots[0], slots[2]]                 # non-contiguous rows
        eng.transcribe_pcm(use, utterances())
        ref = offline_ref(name)
        for i, s in enumerate(use):
            tok, fr, lp, _, align = eng.fetch_aligned(s)
            y, f, l, score, T = ref[i]
            check_records((tok, fr, lp), (y, f, l), (name, la, i))
            assert abs(align_from_frames(fr, T, 3) - align) < 1e-9
            assert abs(align - score) < 1e-9
        assert len(ref[2][0]) == 0                          # the short row: empty arrays
        tok, fr, lp = eng.fetch_many_aligned(use)[2]
        assert tok == [] and fr.shape == (0,) and lp.shape == (0,)
        # batched fetch hands out the same records
        eng.transcribe_pcm(use, utterances())
        for i, got in enumerate(eng.fetch_many_aligned(use)):
            check_records(got, ref[i][:3], (name, la, i, "many"))
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 2. synchronous streaming
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_sync_stream_frames_keep_counting(name):
    eng, _ = make(name)
    try:
        eng.set_alignments(True)
        reset_at = 7
        refs = [stream_ref(name, 3.0, 0), stream_ref(name, 3.0, 1, reset_at=reset_at)]
        pcm = synth.synth_pcm(2, 48000, seed=1234)
        chunks = [synth.stream_chunks(p, 1280, lead=1, tail=10) for p in pcm]
        slots = [eng.open() for _ in range(4)]
        use = [slots[3], slots[1]]
        step, n_buffer = 0, eng.desc.n_buffer
        for k in range(len(chunks[0])):
            eng.push(use, np.stack([c[k] for c in chunks]))
            if not eng.step(use):
                continue
            for i, s in enumerate(use):
                tok, fr, lp, _, _ = eng.fetch_aligned(s)
                if step < refs[i].speech:
                    check_records((tok, fr, lp), refs[i][step], (name, "step", step, i))
                check_structure((tok, fr, lp), step * n_buffer, (step + 1) * n_buffer, (name, "step", step, i))   # step j starts at j * n_buffer
            step += 1
            if step == reset_at:
                eng.reset(use[1], 7)                       # model state only: the frame count runs on
        assert step == len(refs[0]) and step > reset_at + 2
        assert sum(len(r[0]) for r in refs[1][reset_at:refs[1].speech]) > 0           # tokens after the reset were compared
        assert all(r.speech == 19 and len(r) == 23 for r in refs)        # 3 s of audio: steps 0..18 are compared, 19..22 are silence
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 3. pipelined
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_pipelined_records_per_collected_step(name):
    eng, _ = make(name)
    try:
        eng.set_alignments(True)
        refs = [stream_ref(name, 3.0, 0), stream_ref(name, 3.0, 1)]
        pcm = synth.synth_pcm(2, 48000, seed=1234)
        chunks = [synth.stream_chunks(p, 1280, lead=1, tail=10) for p in pcm]
        slots = [eng.open() for _ in range(3)]
        use = [slots[2], slots[0]]
        done, n_buffer = [0], eng.desc.n_buffer

        def collect():
            if eng.wait():
                for i, got in enumerate(eng.fetch_many_aligned(use, 64)):
                    if done[0] < refs[i].speech:
                        check_records(got, refs[i][done[0]], (name, "pipelined step", done[0], i))
                    check_structure(got, done[0] * n_buffer, (done[0] + 1) * n_buffer, (name, "pipelined step", done[0], i))
                done[0] += 1

        depth = 0
        for k in range(len(chunks[0])):
            eng.push_submit(use, np.stack([c[k] for c in chunks]))
            depth = max(depth, eng.pending())
            if eng.pending() >= 5:
                collect()
        while eng.pending():
            collect()
        assert depth >= 5 and done[0] == len(refs[0])
        assert all(r.speech == 19 and sum(len(q[0]) for q in r[:r.speech]) >= 8 for r in refs)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_pipelined_ring_wrap_equals_synchronous(name):
    """include/lasr.h promises results identical to lasr_step_stream: a stream long enough to wrap the 512-entry rings gives bit for bit the synchronous protocol's (tokens, frames, log p) -- on the same engine, the slot closed and re-opened
    in between (the ring's frame cursor is global per row; the slot's count starts over)."""
    eng, _ = make(name)
    try:
        eng.set_alignments(True)
        pcm = synth.synth_pcm(1, 16000 * 75, seed=1234)[0]
        chunks = synth.stream_chunks(pcm, 1280, lead=1, tail=10)
        acc = {}
        for mode in ("pipelined", "sync", "pipelined"):
            slot = eng.open()
            tok, fr, lp = [], [], []

            def take():
                t, f, l = eng.fetch_many_aligned([slot], 256)[0]
                tok.extend(t); fr.append(f); lp.append(l)

            for c in chunks:
                if mode == "sync":
                    eng.push([slot], c[None])
                    if eng.step([slot]):
                        take()
                else:
                    eng.push_submit([slot], c[None])
                    if eng.pending() >= 8 and eng.wait():
                        take()
            while eng.pending():
                if eng.wait():
                    take()
            eng.close_slot(slot)
            got = (tok, np.concatenate(fr), np.concatenate(lp))
            if mode in acc:
                assert got[0] == acc[mode][0] and np.array_equal(got[1], acc[mode][1]) and np.array_equal(got[2], acc[mode][2])
            acc[mode] = got
        a, b = acc["sync"], acc["pipelined"]
        assert len(a[0]) > TOKRING, len(a[0])                  # cannot pass without wrapping
        assert a[0] == b[0]
        assert np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
        assert np.all(np.diff(a[1]) >= 0) and a[1][-1] > 500
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 4. LM attached
def test_lm_fusion_records_follow_the_joint():
    eng, m = make("tiny_soft", lm="tiny_lm")
    try:
        eng.set_alignments(True)
        ref = offline_ref("tiny_soft", "tiny_lm")
        nolm = offline_ref("tiny_soft")
        assert any(r[0] != q[0] for r, q in zip(ref, nolm))          # the fuser overrides tokens on these inputs
        slots = [eng.open() for _ in range(3)]
        eng.transcribe_pcm(slots, utterances())
        for i, got in enumerate(eng.fetch_many_aligned(slots)):
            check_records(got, ref[i][:3], ("lm offline", i))
        # streaming (synchronous steps) on a slot of its own: its frame count starts at 0
        s = eng.open()
        pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
        sref = stream_ref("tiny_soft", 3.0, 0, lm="tiny_lm")
        assert sref.speech == 19
        step, n, n_buffer = 0, 0, eng.desc.n_buffer
        for ch in synth.stream_chunks(pcm, 1280, lead=1, tail=10):
            eng.push([s], ch[None])
            if not eng.step([s]):
                continue
            tok, fr, lp, _, _ = eng.fetch_aligned(s)
            if step < sref.speech:
                check_records((tok, fr, lp), sref[step], ("lm stream", step))
            check_structure((tok, fr, lp), step * n_buffer, (step + 1) * n_buffer, ("lm stream", step))
            step += 1
            n += len(tok)
        assert step == len(sref) and sum(len(q[0]) for q in sref[:sref.speech]) >= 8
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 5. contract
def test_contract_errors_and_plain_fetch():
    eng, _ = make("tiny")
    try:
        ref = offline_ref("tiny")
        slots = [eng.open() for _ in range(3)]
        with pytest.raises(N.LasrError) as e:                # off by default
            eng.fetch_aligned(slots[0])
        assert e.value.code == N.LASR_ESTATE
        with pytest.raises(N.LasrError) as e:
            eng.fetch_many_aligned(slots)
        assert e.value.code == N.LASR_ESTATE
        eng.set_alignments(True)
        # a submitted, uncollected step: the switch is refused
        pcm = synth.synth_pcm(1, 16000, seed=1234)[0]
        for c in synth.stream_chunks(pcm, 1280, lead=1, tail=0):
            eng.push_submit([slots[2]], c[None])
            if eng.pending():
                break
        assert eng.pending() == 1
        with pytest.raises(N.LasrError) as e:
            eng.set_alignments(False)
        assert e.value.code == N.LASR_ESTATE
        assert eng.wait() == 1
        eng.fetch_aligned(slots[2])
        # unfetched tokens: the switch is refused as well (they would lose their records), a call that changes nothing is not
        eng.transcribe_pcm(slots, utterances())
        with pytest.raises(N.LasrError) as e:
            eng.set_alignments(False)
        assert e.value.code == N.LASR_ESTATE
        eng.set_alignments(True)
        check_records(eng.fetch_many_aligned(slots)[0], ref[0][:3], "after the refused switch")
        # cap too small: LASR_EFULL, nothing consumed
        eng.transcribe_pcm(slots, utterances())
        with pytest.raises(N.LasrError) as e:
            eng.fetch_aligned(slots[0], cap=1)
        assert e.value.code == N.LASR_EFULL
        with pytest.raises(N.LasrError) as e:
            eng.fetch_many_aligned(slots, cap=1)
        assert e.value.code == N.LASR_EFULL
        check_records(eng.fetch_aligned(slots[0])[:3], ref[0][:3], "after EFULL")
        # plain fetch on an enabled engine: same tokens, and no stale records behind it
        assert eng.fetch(slots[1])[0] == ref[1][0]
        tok, fr, lp, _, _ = eng.fetch_aligned(slots[1])
        assert tok == [] and len(fr) == 0 and len(lp) == 0
        eng.transcribe_pcm(slots, utterances())
        assert eng.fetch_many(slots[:1])[0] == ref[0][0]
        got = eng.fetch_many_aligned(slots)
        assert got[0][0] == [] and len(got[0][1]) == 0
        check_records(got[1], ref[1][:3], "after plain fetch")
    finally:
        eng.close()


def test_beam_engine_refuses_alignments():
    eng, _ = make("tiny", beam=4)
    try:
        with pytest.raises(N.LasrError) as e:
            eng.set_alignments(True)
        assert e.value.code == N.LASR_EINVAL
    finally:
        eng.close()


def test_toggling_between_steps_leaves_tokens_unchanged():
    """the cached decode graphs capture the record pointers by value: a toggle must not replay a stale one"""
    plain, _ = make("tiny_lstm")
    tog, _ = make("tiny_lstm")
    try:
        pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
        chunks = synth.stream_chunks(pcm, 1280, lead=1, tail=10)
        ref = stream_ref("tiny_lstm", 3.0, 0)
        for mode in ("sync", "pipelined"):
            a, b = plain.open(), tog.open()
            on, step, ta, tb = False, 0, [], []
            for c in chunks:
                ran = 0
                for eng, s in ((plain, a), (tog, b)):
                    if mode == "sync":
                        eng.push([s], c[None])
                        ran = eng.step([s])
                    else:
                        eng.push_submit([s], c[None])
                        ran = eng.wait()
                if not ran:
                    continue
                ta.append(plain.fetch(a)[0])
                if on:
                    tok, fr, lp, _, _ = tog.fetch_aligned(b)
                    if step < ref.speech:
                        check_records((tok, fr, lp), ref[step], (mode, "toggled on", step))
                    tb.append(tok)
                else:
                    tb.append(tog.fetch(b)[0])
                step += 1
                if step % 3 == 0:                          # every third model step: through several graph-cache generations
                    on = not on
                    tog.set_alignments(on)
            assert ta == tb and len(ta) == len(ref) and ta[:ref.speech] == [r[0] for r in ref[:ref.speech]], mode
            assert sum(len(t) for t in ta) > 0
            plain.close_slot(a); tog.close_slot(b)
            tog.set_alignments(False)
    finally:
        plain.close(); tog.close()


# ------------------------------------------------------------------------------- 6. bf16
def test_bf16_records_are_well_formed():
    """bf16 operands decide differently from fp32 now and then: structure only, no numeric bound against the fp32 oracle"""
    eng, _ = make("tiny", dtype="bf16")
    try:
        eng.set_alignments(True)
        slots = [eng.open() for _ in range(3)]
        eng.transcribe_pcm(slots, utterances())
        n = 0
        for i, s in enumerate(slots):
            tok, fr, lp, _, align = eng.fetch_aligned(s)
            T = O.features_offline(utterances()[i]).shape[0]
            assert len(tok) == len(fr) == len(lp)
            assert np.all(np.diff(fr) >= 0)
            assert np.all(fr >= 0) and np.all(fr < T)
            assert np.bincount(fr, minlength=T).max() <= 3
            assert abs(align_from_frames(fr, T, 3) - align) < 1e-9
            assert np.all(np.isfinite(lp)) and np.all(lp <= 0)
            n += len(tok)
        assert n > 0
    finally:
        eng.close()


# ------------------------------------------------------------------------------- facade
def test_libreasr_facade_returns_times_and_confidences():
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", synthetic="tiny", max_streams=4)
    try:
        ref = offline_ref("tiny")
        d = asr.engine.desc
        dt = d.stride * d.hop / d.sample_rate
        assert abs(dt - 0.08) < 1e-12
        out = asr.transcribe(utterances()[0], return_alignment=True)
        assert [t for t, _, _ in out] == ref[0][0]
        assert [round(ts / dt) for _, ts, _ in out] == ref[0][1]
        assert all(0.0 < cf <= 1.0 for _, _, cf in out)
        assert max(abs(np.log(cf) - l) for (_, _, cf), l in zip(out, ref[0][2])) < LOGP_TOL
        assert asr.transcribe(utterances()[0], return_ids=True) == ref[0][0]      # the plain form still works on the same engine
        steps = stream_ref("tiny", 3.0, 0)
        pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
        last = None
        for last in asr.stream(synth.stream_chunks(pcm, 1280, lead=1, tail=10), return_alignment=True):
            pass
        want_t = [t for s in steps[:steps.speech] for t in s[0]]
        want_f = [f for s in steps[:steps.speech] for f in s[1]]
        assert len(want_t) >= 8 and [t for t, _, _ in last][:len(want_t)] == want_t
        got_f = [round(ts / dt) for _, ts, _ in last]
        assert got_f[:len(want_f)] == want_f and got_f == sorted(got_f)
    finally:
        asr.engine.close()


def test_libreasr_facade_refuses_beam():
    from libreasr_amd.api import LibreASR
    asr = LibreASR.load("en", synthetic="tiny", max_streams=4, beam=2)
    try:
        with pytest.raises(NotImplementedError):
            asr.transcribe(utterances()[0], return_alignment=True)
        with pytest.raises(NotImplementedError):
            next(asr.stream([np.zeros(1280, np.float32)], return_alignment=True))
    finally:
        asr.engine.close()
