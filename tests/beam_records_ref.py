"""Expected values of the beam's per-token records (lasr_set_beam_records / lasr_fetch_nbest).

oracle/rnnt_oracle.py:_beam_frame is the spec of the beam, but it returns no frames and no per-token log p.  beam_frame_rec below
restates it line by line and appends (t, float(lp[v])) to a second list `r` wherever the spec appends v to `y` -- lp[v] is the
joint's log p of the candidate that was selected, i.e. with an LM the best non-blank token's, not the fuser's re-pick's.
tests/test_beam_records_cpu.py pins the restatement to the spec (every hypothesis: y and score equal, on every model step).

Not a test module: shared, cached references for test_beam_records_cpu.py and test_gpu_beam_records.py."""
import numpy as np

from libreasr_amd import synth
from oracle import rnnt_oracle as O

SILENCE = float(np.log(np.float32(1e-6)))      # the log-mel floor: what every feature of a chunk of zeros is
MARGIN = 1e-3                                  # the margin rule: a selection decided by less is a tie between GPU f32 and numpy f32


def beam_frame_rec(m, hyps, enc_t, t, W, max_iters, margins=None):
    """OracleTransducer._beam_frame with records: hyps carry `r` = [(frame, log p)] parallel to `y`."""
    A = [dict(h, inB=False) for h in hyps]
    for rnd in range(1, max_iters + 1):
        cands = []
        for b, h in enumerate(A):
            if h["inB"]:
                cands.append((-h["score"], b, 0, -1, h, None))
                continue
            lp, _ = m.joint_logp(h["h_pred"], enc_t[None])
            lp = lp[0]
            if m.lm is not None:
                nb = lp.copy()
                nb[m.blank] = -np.inf
                top = [m.blank, int(nb.argmax())]
            else:
                top = np.argsort(-lp, kind="stable")[:W]
            for v in top:
                cands.append((-(h["score"] + float(lp[v])), b, 1, int(v), h, lp))
        cands.sort(key=lambda c: c[:4])
        if margins is not None and len(cands) > W:
            margins.append(cands[W][0] - cands[W - 1][0])
        new = []
        for negs, b, kind, v, h, lp in cands[:W]:
            if kind == 0:
                new.append(h)
            elif v == m.blank:
                new.append(dict(h, score=-negs, inB=True))
            else:
                rec = (t, float(lp[v]))                  # the joint's term, before any re-pick
                fz = h.get("fuser")
                if fz is not None:
                    vj, v = v, fz.fuse(lp, v)
                    if v != vj:                          # (counted per hypothesis: the tests need re-picks that differ)
                        h = dict(h, repicked=h.get("repicked", 0) + 1)
                    nf = O.LMFuser(m.lm)
                    nf.lm_logits, nf.lm_state = fz.lm_logits, fz.lm_state
                    nf.advance(v)
                hp, ps = m.predictor([v], h["pstate"])
                nh = dict(score=-negs, y=h["y"] + [v], r=h["r"] + [rec], h_pred=hp, pstate=ps, inB=(rnd == max_iters),
                          repicked=h.get("repicked", 0))
                if fz is not None:
                    nh["fuser"] = nf
                new.append(nh)
        A = new
        if all(h["inB"] for h in A):
            break
    keys = ("score", "y", "r", "h_pred", "pstate") + (("fuser",) if m.lm is not None else ())
    return [dict({k: h[k] for k in keys}, repicked=h.get("repicked", 0)) for h in A]


def beam_init_rec(m):
    h = m.beam_init()
    h[0]["r"] = []
    return h


def ranked(hyps, prefix=None):
    """the whole beam as lasr_fetch_nbest hands it out: best first (score descending, then slot ascending);
    -> [(tokens, frames, logps, score)].  prefix = (tokens, frames, logps, score) frozen by a predictor reset."""
    p = prefix or ([], [], [], 0.0)
    order = sorted(range(len(hyps)), key=lambda i: (-hyps[i]["score"], i))
    return [(p[0] + list(hyps[i]["y"]), p[1] + [f for f, _ in hyps[i]["r"]], p[2] + [lp for _, lp in hyps[i]["r"]],
             p[3] + hyps[i]["score"]) for i in order]


def hyp_gap(hyps):
    sc = sorted((h["score"] for h in hyps), reverse=True)
    return min((a - b for a, b in zip(sc, sc[1:])), default=float("inf"))


class StreamBeamRec:
    """O.StreamBeamDecoder with records and the whole beam: .step(chunk) -> ranked beam after that model step.  The frame index
    runs on across .reset() (the slot's count); .reset() freezes the best hypothesis as the engine's predictor reset does."""

    def __init__(self, m, W, max_iters=10):
        self.m, self.W, self.max_iters = m, W, max_iters
        self.enc_state = None
        self.hyps = beam_init_rec(m)
        self.t = 0
        self.prefix = ([], [], [], 0.0)
        self.step_margin = []          # per model step: min(selection-boundary gaps of its rounds, gap between two kept hypotheses)

    def step(self, chunk):
        enc, self.enc_state = self.m.encoder(chunk[None], self.enc_state)
        margins = []
        for k in range(enc.shape[1]):
            self.hyps = beam_frame_rec(self.m, self.hyps, enc[0, k], self.t, self.W, self.max_iters, margins)
            self.t += 1
        margins.append(hyp_gap(self.hyps))
        self.step_margin.append(min(margins))
        return self.beam()

    def beam(self):
        return ranked(self.hyps, self.prefix)

    def clone(self):
        """an independent decoder in the same state (hypotheses and states are never modified in place)"""
        d = StreamBeamRec(self.m, self.W, self.max_iters)
        d.enc_state, d.hyps, d.t, d.prefix, d.step_margin = self.enc_state, list(self.hyps), self.t, self.prefix, list(self.step_margin)
        return d

    def reset(self):
        self.prefix = self.beam()[0]
        self.enc_state = None
        self.hyps = beam_init_rec(self.m)


_MODELS, _OFF, _STR = {}, {}, {}
SHAPES = [("tiny", 2), ("tiny", 4), ("tiny_lstm", 4), ("tiny", 8)]
START = [0, 1, 3]          # the chunk at which stream i joins (ragged steps)


def model(name, lm=None, operand="f32"):
    key = (name, lm, operand)
    if key not in _MODELS:
        cfg = synth.model_cfg(name)
        sd = synth.synth_state_dict(cfg, seed=0)
        m = O.OracleTransducer(sd, cfg, operand=operand)
        if lm:
            m.lm = O.OracleLM(synth.synth_lm_state_dict(lm))
        _MODELS[key] = (m, sd, cfg)
    return _MODELS[key]


LM_PCM_SEED = 31           # the LM case's utterances (the streaming tests' audio, offline): on synth_pcm(seed=1234) at W = 2 the
                           # fuser's re-pick equals the joint's token everywhere; here it differs in an utterance compared in full


def offline_pcm(name, seed=1234):
    return synth.synth_pcm(3, 16000 * 3, seed=seed) if name != "cfg2" else synth.synth_pcm(1, 16000 * 2, seed=seed)


def offline_ref(name, W, lm=None, seed=1234):
    """per utterance: dict(beam = ranked whole beam at the end, T = frames, margin, repicked = per ranked hypothesis, the tokens
    for which the fuser's re-pick differs from the joint's best non-blank token)"""
    key = (name, W, lm, seed)
    if key not in _OFF:
        m = model(name, lm)[0]
        out = []
        for p in offline_pcm(name, seed):
            feats = O.features_offline(p)
            enc, _ = m.encoder(feats[None])
            hyps, margins = beam_init_rec(m), []
            for t in range(enc.shape[1]):
                hyps = beam_frame_rec(m, hyps, enc[0, t], t, W, 3, margins)
            margins.append(hyp_gap(hyps))
            order = sorted(range(len(hyps)), key=lambda i: (-hyps[i]["score"], i))
            out.append(dict(beam=ranked(hyps), T=int(enc.shape[1]), margin=min(margins), repicked=[hyps[i]["repicked"] for i in order]))
        _OFF[key] = out
    return _OFF[key]


def stream_inputs():
    pcm = synth.synth_pcm(3, 48000, seed=31)
    return [synth.stream_chunks(pcm[i], 1280, lead=1, tail=6) for i in range(3)]


def stream_ref(name, W):
    """per stream: dict(steps = [ranked whole beam after every model step], T = [frames consumed up to and incl. that step],
    margin = [per step], speech = leading model steps that still see audio, dec = the decoder (to go on after a reset))"""
    key = (name, W)
    if key not in _STR:
        m = model(name)[0]
        out = []
        for chunks in stream_inputs():
            fe, dec = O.StreamFrontend(), StreamBeamRec(m, W)
            steps, T, speech = [], [], None
            for ch in chunks:
                o = fe.push(ch)
                if o is None:
                    continue
                if speech is None and float(np.abs(np.asarray(o, np.float64) - SILENCE).max()) < 1e-4:
                    speech = len(steps)
                steps.append(dec.step(o))
                T.append(dec.t)
            out.append(dict(steps=steps, T=T, margin=list(dec.step_margin), speech=len(steps) if speech is None else speech,
                            dec=dec, fe=fe))
        _STR[key] = out
    return _STR[key]


def full_upto(ref_stream):
    """the margin rule for a stream: the number of leading model steps that are compared in full (up to the first step whose margin
    is below MARGIN, and never into the silent tail)"""
    n = ref_stream["speech"]
    for j, g in enumerate(ref_stream["margin"][:n]):
        if g < MARGIN:
            return j
    return n
