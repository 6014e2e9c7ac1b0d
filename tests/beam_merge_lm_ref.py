"""Expected values of the beam with merging of equal hypotheses UNDER LM SHALLOW FUSION (lasr_set_beam_merge(c, LASR_BEAM_MERGE_LM) /
DESIGN 5.10).

frame_merge_lm below is beam_records_ref.beam_frame_rec -- with and without an LM on the model -- line by line, with the additions of
beam_merge_ref.frame_merge (slots keep their places, None = dead slot; identity `idt`; flag `capped`; the merge step) and ONE change
to that rule: the identity is chained from the token the slot actually carries after the round, i.e. the fuser's re-pick where the
parent's fuser holds LM logits and the joint's token otherwise, and the merge step runs on the round's W survivors after the re-pick.
The kept (lowest) slot keeps its fuser: LM state and LM output.
tests/test_beam_merge_lm_cpu.py pins it: with the merge step skipped it equals beam_frame_rec with the LM; without an LM it equals
beam_merge_ref.frame_merge; identity equality coincides with list equality.

For the tests that tell a correct build from a plausible wrong one every hypothesis also carries
  * `jidt`: the identity chained from the JOINT's token along the same slots -- what a merge inside the selection round, in front of
    the re-pick, would compute;
  * `rp_now`: the slot was extended in THIS round and the fuser's re-pick differs from the joint's token.
trace() counts, per utterance, the rounds whose grouping by (jidt, inB) differs from the grouping by (idt, inB), and the merged groups
that hold a member with rp_now.

The margin bookkeeping is beam_merge_ref's.

Not a test module: shared, cached references for test_beam_merge_lm_cpu.py and test_gpu_beam_merge_lm.py."""
import itertools
import math

import numpy as np

import beam_merge_ref as M
import beam_records_ref as R
from libreasr_amd import synth
from oracle import rnnt_oracle as O

MARGIN = R.MARGIN
SHAPES = R.SHAPES
LM = "tiny_lm"
EMPTY, ident_append, ident_of, lae, live, ranked, order, hyp_gap = (M.EMPTY, M.ident_append, M.ident_of, M.lae, M.live, M.ranked, M.order,
                                                                    M.hyp_gap)


def beam_init(m):
    h = R.beam_init_rec(m)
    h[0].update(idt=EMPTY, jidt=EMPTY, capped=False, repicked=0)
    return h


def frame_merge_lm(m, hyps, enc_t, t, W, max_iters, margins=None, merge=True, on_round=None, stats=None):
    """one encoder frame.  hyps: list of dict | None (slot order) -> list of W entries, dict | None.
    on_round(survivors): called with the round's live survivors in slot order, after the re-pick and BEFORE the merge step (dicts with
    inB, rp_now).  stats["merges"] counts the hypotheses merged away."""
    A = [None if h is None else dict(h, inB=False, rp_now=False) for h in hyps]
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
                new.append(dict(h, rp_now=False))
            elif v == m.blank:
                new.append(dict(h, score=-negs, inB=True, rp_now=False))
            else:
                rec = (t, float(lp[v]))                  # the joint's term, before any re-pick
                vj = v
                fz = h.get("fuser")
                if fz is not None:
                    v = fz.fuse(lp, vj)
                    nf = O.LMFuser(m.lm)
                    nf.lm_logits, nf.lm_state = fz.lm_logits, fz.lm_state
                    nf.advance(v)
                hp, ps = m.predictor([v], h["pstate"])
                nh = dict(score=-negs, y=h["y"] + [v], r=h["r"] + [rec], h_pred=hp, pstate=ps, inB=(rnd == max_iters),
                          idt=ident_append(h["idt"], v), jidt=ident_append(h["jidt"], vj), capped=h["capped"] or rnd == max_iters,
                          repicked=h["repicked"] + (v != vj), rp_now=(v != vj))
                if fz is not None:
                    nh["fuser"] = nf
                new.append(nh)
        new += [None] * (W - len(new))
        if on_round is not None:
            on_round(live(new))
        if merge:                                           # ---- the merge step, after the re-pick
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
                    new[j] = dict(new[j], score=acc, capped=cap)     # (the kept slot's fuser stays)
        A = new
        if all(h["inB"] for h in live(A)):
            break
    keys = ("score", "y", "r", "h_pred", "pstate", "idt", "jidt", "capped", "repicked") + (("fuser",) if m.lm is not None else ())
    return [None if h is None else {k: h[k] for k in keys} for h in A]


class Watch:
    """on_round / on_frame hooks: the per-round facts the CPU tests assert, counted"""

    def __init__(self):
        self.rounds = self.frames = 0
        self.collisions = 0        # pairs of same-inB survivors whose identity equality differs from their list equality
        self.dup_frames = 0        # frame ends at which two live hypotheses hold the same list
        self.jdiff_rounds = 0      # rounds in which grouping by (jidt, inB) differs from grouping by (idt, inB)
        self.groups = 0            # groups of >= 2 survivors with equal (idt, inB): the merges
        self.rp_groups = 0         # ... with a member re-picked, differing from the joint's token, in this very round
        self.lm_unequal = 0        # ... whose members' LM outputs (fuser.lm_logits) are not bit-equal

    @staticmethod
    def _partition(surv, key):
        g = {}
        for i, h in enumerate(surv):
            g.setdefault((h[key], h["inB"]), []).append(i)
        return sorted(tuple(v) for v in g.values())

    def on_round(self, surv):
        self.rounds += 1
        for a, b in itertools.combinations(surv, 2):
            if a["inB"] == b["inB"] and (a["idt"] == b["idt"]) != (a["y"] == b["y"]):
                self.collisions += 1
        true = self._partition(surv, "idt")
        if true != self._partition(surv, "jidt"):
            self.jdiff_rounds += 1
        for g in true:
            if len(g) < 2:
                continue
            self.groups += 1
            self.rp_groups += any(surv[i]["rp_now"] for i in g)
            lz = [surv[i]["fuser"].lm_logits if "fuser" in surv[i] else None for i in g]
            if not all((a is None and lz[0] is None) or (a is not None and lz[0] is not None and np.array_equal(a, lz[0])) for a in lz):
                self.lm_unequal += 1

    def on_frame(self, hyps):
        self.frames += 1
        ys = [tuple(h["y"]) for h in live(hyps)]
        self.dup_frames += len(set(ys)) != len(ys)

    def counts(self):
        return {k: v for k, v in vars(self).items()}


class StreamBeamMergeLM:
    """beam_records_ref.StreamBeamRec over frame_merge_lm.  .merge may be set between model steps (the identities are a function of
    `y`: nothing to upload here); .reset() restarts identities, predictor and LM with the beam (reset bits 1 | 2 | 4)."""

    def __init__(self, m, W, max_iters=10, merge=True):
        self.m, self.W, self.max_iters, self.merge = m, W, max_iters, merge
        self.enc_state = None
        self.hyps = beam_init(m)
        self.t = 0
        self.prefix = ([], [], [], 0.0)
        self.step_margin = []
        self.watch = Watch()
        self.stats = {}

    def step(self, chunk):
        enc, self.enc_state = self.m.encoder(chunk[None], self.enc_state)
        margins = []
        for k in range(enc.shape[1]):
            self.hyps = frame_merge_lm(self.m, self.hyps, enc[0, k], self.t, self.W, self.max_iters, margins, self.merge,
                                       self.watch.on_round, self.stats)
            if self.merge:
                self.watch.on_frame(self.hyps)
            self.t += 1
        margins.append(hyp_gap(self.hyps))
        self.step_margin.append(min(margins))
        return self.beam()

    def beam(self):
        return ranked(self.hyps, self.prefix)

    def clone(self):
        d = StreamBeamMergeLM(self.m, self.W, self.max_iters, self.merge)
        d.enc_state, d.hyps, d.t, d.prefix, d.step_margin = self.enc_state, list(self.hyps), self.t, self.prefix, list(self.step_margin)
        return d

    def reset(self):
        self.prefix = self.beam()[0]
        self.enc_state = None
        self.hyps = beam_init(self.m)


_OFF, _STR = {}, {}


def model(name, lm=LM):
    return R.model(name, lm)


def offline_ref(name, W, max_iters=3, merge=True, seed=R.LM_PCM_SEED, lm=LM):
    """per utterance: dict(beam = ranked whole beam at the end, T, margin, merges, distinct = distinct token lists in the final beam,
    n = its live hypotheses, watch = Watch.counts())"""
    key = (name, W, max_iters, merge, seed, lm)
    if key not in _OFF:
        m = model(name, lm)[0]
        out = []
        for p in R.offline_pcm(name, seed):
            enc, _ = m.encoder(O.features_offline(p)[None])
            hyps, margins, stats, w = beam_init(m), [], {}, Watch()
            for t in range(enc.shape[1]):
                hyps = frame_merge_lm(m, hyps, enc[0, t], t, W, max_iters, margins, merge, w.on_round, stats)
                w.on_frame(hyps)
            margins.append(hyp_gap(hyps))
            ys = [tuple(h["y"]) for h in live(hyps)]
            out.append(dict(beam=ranked(hyps), T=int(enc.shape[1]), margin=min(margins), merges=stats.get("merges", 0),
                            distinct=len(set(ys)), n=len(ys), watch=w.counts()))
        _OFF[key] = out
    return _OFF[key]


STREAM_SEED = 1234         # (not beam_records_ref.stream_inputs()' 31: under the LM two of its three W = 8 streams fall below the margin
                           #  within 8 model steps; test_beam_merge_lm_cpu.py asserts what this seed gives)


def stream_inputs(seed=STREAM_SEED):
    pcm = synth.synth_pcm(3, 48000, seed=seed)
    return [synth.stream_chunks(pcm[i], 1280, lead=1, tail=6) for i in range(3)]


def stream_run(name, W, merge_at=None, seed=STREAM_SEED, lm=LM):
    """the streams of stream_inputs(seed) through StreamBeamMergeLM.  merge_at(stream, step index) -> bool: the switch during that
    model step (default: on throughout).  per stream: dict(steps, T, margin, speech, dec, fe, on = the switch per step)"""
    m = model(name, lm)[0]
    out = []
    for i, chunks in enumerate(stream_inputs(seed)):
        fe, dec = O.StreamFrontend(), StreamBeamMergeLM(m, W)
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


def stream_ref(name, W, seed=STREAM_SEED):
    key = (name, W, seed)
    if key not in _STR:
        _STR[key] = stream_run(name, W, seed=seed)
    return _STR[key]


full_upto = R.full_upto
