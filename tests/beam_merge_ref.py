"""Expected values of the beam with merging of equal hypotheses (lasr_set_beam_merge / DESIGN 5.9).

frame_merge below is beam_records_ref.beam_frame_rec (itself oracle/rnnt_oracle.py:_beam_frame with records) line by line for a model
without an LM, with three additions:
  * slots keep their places: the beam is a list of W entries, None = dead slot (the spec's list simply ends where the candidates do;
    without merging the dead slots are exactly the tail, so the live entries in order are the spec's list);
  * every hypothesis carries its identity `idt` = (len, hash) of `y` (the rule of include/lasr.h) and the flag `capped`: some
    alignment merged into it put max_iters tokens on one frame (OR-ed on merge);
  * the merge step after the W survivors of a round are known: survivors with equal (idt, inB) are merged into the lowest slot, whose
    score becomes the fold of lae over the group in ascending slot order; the others become None.
tests/test_beam_merge_cpu.py pins it: with the merge step skipped it equals beam_frame_rec; identity equality coincides with list
equality; against enumeration it is exact.

The margin bookkeeping is beam_records_ref's (smallest selection-boundary gap of a round, smallest gap between two kept hypotheses)
plus one term the merge adds: in a merged group the LOWEST slot keeps its frames and log p, so the gap between the group's two best
scores decides something too.

Not a test module: shared, cached references for test_beam_merge_cpu.py and test_gpu_beam_merge.py."""
import math

import numpy as np

import beam_records_ref as R
from oracle import rnnt_oracle as O

MASK = (1 << 64) - 1
SEED = 0x9E3779B97F4A7C15
EMPTY = (0, SEED)
MARGIN = R.MARGIN
SHAPES = R.SHAPES


def mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def ident_append(idt, v):
    return (idt[0] + 1, mix(idt[1] ^ ((v + 1) & MASK)))


def ident_of(y):
    idt = EMPTY
    for v in y:
        idt = ident_append(idt, int(v))
    return idt


def lae(a, b):
    hi, lo = (a, b) if a > b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


def beam_init(m):
    h = R.beam_init_rec(m)
    h[0]["idt"] = EMPTY
    h[0]["capped"] = False
    return h


def live(hyps):
    return [h for h in hyps if h is not None]


def frame_merge(m, hyps, enc_t, t, W, max_iters, margins=None, merge=True, on_round=None, stats=None):
    """one encoder frame.  hyps: list of dict | None (slot order) -> list of W entries, dict | None.
    on_round(survivors): called with the round's survivors BEFORE the merge step (dicts with inB).  stats["merges"] counts the
    hypotheses merged away."""
    A = [None if h is None else dict(h, inB=False) for h in hyps]
    for rnd in range(1, max_iters + 1):
        cands = []
        for b, h in enumerate(A):
            if h is None:
                continue
            if h["inB"]:
                cands.append((-h["score"], b, 0, -1, h, None))
                continue
            lp, _ = m.joint_logp(h["h_pred"], enc_t[None])
            lp = lp[0]
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
                hp, ps = m.predictor([v], h["pstate"])
                new.append(dict(score=-negs, y=h["y"] + [v], r=h["r"] + [(t, float(lp[v]))], h_pred=hp, pstate=ps,
                                inB=(rnd == max_iters), idt=ident_append(h["idt"], v), capped=h["capped"] or rnd == max_iters))
        new += [None] * (W - len(new))
        if on_round is not None:
            on_round(live(new))
        if merge:                                           # ---- the merge step
            for j in range(W):
                if new[j] is None:
                    continue
                acc, cap, second = new[j]["score"], new[j]["capped"], -math.inf
                for i in range(j + 1, W):
                    o = new[i]
                    if o is not None and o["idt"] == new[j]["idt"] and o["inB"] == new[j]["inB"]:
                        acc = lae(acc, o["score"])
                        cap = cap or o["capped"]
                        second = max(second, o["score"])
                        new[i] = None
                        if stats is not None:
                            stats["merges"] = stats.get("merges", 0) + 1
                if second > -math.inf:
                    if margins is not None:
                        margins.append(new[j]["score"] - second)
                    new[j] = dict(new[j], score=acc, capped=cap)
        A = new
        if all(h["inB"] for h in live(A)):
            break
    keys = ("score", "y", "r", "h_pred", "pstate", "idt", "capped")
    return [None if h is None else {k: h[k] for k in keys} for h in A]


def ranked(hyps, prefix=None):
    """the whole beam as lasr_fetch_nbest hands it out: the live slots, best first (score descending, then slot ascending);
    -> [(tokens, frames, logps, score)].  prefix = (tokens, frames, logps, score) frozen by a predictor reset."""
    p = prefix or ([], [], [], 0.0)
    return [(p[0] + list(hyps[i]["y"]), p[1] + [f for f, _ in hyps[i]["r"]], p[2] + [lp for _, lp in hyps[i]["r"]],
             p[3] + hyps[i]["score"]) for i in order(hyps)]


def order(hyps):
    return sorted((i for i, h in enumerate(hyps) if h is not None), key=lambda i: (-hyps[i]["score"], i))


def hyp_gap(hyps):
    return R.hyp_gap(live(hyps))


class StreamBeamMerge:
    """beam_records_ref.StreamBeamRec over frame_merge.  .merge may be set between model steps (lasr_set_beam_merge in mid-stream:
    the identities are a function of `y`, so there is nothing to upload here); .reset() restarts the identities with the beam."""

    def __init__(self, m, W, max_iters=10, merge=True):
        self.m, self.W, self.max_iters, self.merge = m, W, max_iters, merge
        self.enc_state = None
        self.hyps = beam_init(m)
        self.t = 0
        self.prefix = ([], [], [], 0.0)
        self.step_margin = []
        self.on_round = None
        self.on_frame = None
        self.stats = {}

    def step(self, chunk):
        enc, self.enc_state = self.m.encoder(chunk[None], self.enc_state)
        margins = []
        for k in range(enc.shape[1]):
            self.hyps = frame_merge(self.m, self.hyps, enc[0, k], self.t, self.W, self.max_iters, margins, self.merge, self.on_round,
                                    self.stats)
            if self.on_frame is not None:
                self.on_frame(self.hyps)
            self.t += 1
        margins.append(hyp_gap(self.hyps))
        self.step_margin.append(min(margins))
        return self.beam()

    def beam(self):
        return ranked(self.hyps, self.prefix)

    def clone(self):
        d = StreamBeamMerge(self.m, self.W, self.max_iters, self.merge)
        d.enc_state, d.hyps, d.t, d.prefix, d.step_margin = self.enc_state, list(self.hyps), self.t, self.prefix, list(self.step_margin)
        return d

    def reset(self):
        self.prefix = self.beam()[0]
        self.enc_state = None
        self.hyps = beam_init(self.m)


_OFF, _STR = {}, {}


def offline_ref(name, W, max_iters=3, merge=True, seed=1234):
    """per utterance: dict(beam = ranked whole beam at the end, capped = per ranked hypothesis, T, margin, merges)"""
    key = (name, W, max_iters, merge, seed)
    if key not in _OFF:
        m = R.model(name)[0]
        out = []
        for p in R.offline_pcm(name, seed):
            enc, _ = m.encoder(O.features_offline(p)[None])
            hyps, margins, stats = beam_init(m), [], {}
            for t in range(enc.shape[1]):
                hyps = frame_merge(m, hyps, enc[0, t], t, W, max_iters, margins, merge, None, stats)
            margins.append(hyp_gap(hyps))
            out.append(dict(beam=ranked(hyps), capped=[hyps[i]["capped"] for i in order(hyps)], T=int(enc.shape[1]),
                            margin=min(margins), merges=stats.get("merges", 0)))
        _OFF[key] = out
    return _OFF[key]


def stream_run(name, W, merge_at=None):
    """the streams of beam_records_ref.stream_inputs through StreamBeamMerge.  merge_at(stream, step index) -> bool: the switch
    during that model step (default: on throughout).  per stream: dict(steps, T, margin, speech, dec, fe, on = the switch per step)"""
    m = R.model(name)[0]
    out = []
    for i, chunks in enumerate(R.stream_inputs()):
        fe, dec = O.StreamFrontend(), StreamBeamMerge(m, W)
        steps, T, on, speech = [], [], [], None
        for ch in chunks:
            o = fe.push(ch)
            if o is None:
                continue
            if speech is None and float(np.abs(np.asarray(o, np.float64) - R.SILENCE).max()) < 1e-4:
                speech = len(steps)
            dec.merge = True if merge_at is None else bool(merge_at(i, len(steps)))
            on.append(dec.merge)
            steps.append(dec.step(o))
            T.append(dec.t)
        out.append(dict(steps=steps, T=T, margin=list(dec.step_margin), speech=len(steps) if speech is None else speech, dec=dec, fe=fe,
                        on=on))
    return out


def stream_ref(name, W):
    key = (name, W)
    if key not in _STR:
        _STR[key] = stream_run(name, W)
    return _STR[key]


full_upto = R.full_upto
