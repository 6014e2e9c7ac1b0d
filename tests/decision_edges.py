"""Crafted models for the decision side of the decoder (no GPU): a nonzero blank id, a BOS other than 2, vocabularies on every
path of k_select / k_lat_pick* (KEEP 8 and 16, the re-read tail above 4096, the two logits tilings of the lattice) and exact ties
between logits.  test_decision_edges_cpu.py asserts on the numpy oracle alone that the edges really occur on these inputs;
test_gpu_decision_edges.py compares the engine with the oracle on them.

A model starts from synth.synth_state_dict of `tiny` / `tiny_lstm` with cfg["vocab"] = V; only the joint's output layer
(joint.joint.2.weight / .bias) changes:

  blank      rows 0 and `blank` are swapped, so the zero-weight constant-bias row sits at `blank`.
  tie groups the first member of a group gets a bias bonus; its weight row and bias are copied to the other members.  Each output
             column is its own dot product over the same K order, so the copies are bit-equal to their source in the oracle and on
             the GPU (both asserted).  The correct decision for a winning group is its lowest index (first maximum, as argmax).
  blank bias the median of the oracle's best non-blank logit over the utterances below (offline, cap 2), iterated until the
             decode with that bias sees a blank share of 0.4 to 0.65 (8 passes at most).
  tie rows   "plus": a zero-weight row at blank + 1 with the blank's bias -- never emitted (the blank is the first maximum);
             "minus": the same row at blank - 1 -- emitted wherever the blank would have won, up to the cap.

The members of the groups straddle every boundary of k_select's layout (thread j % 256, register slot j / 256, wave tid / 64; the
beam's layout for V = 2048 is v = lane + 64 vw + 512 k).  Where `blank` itself is a member (blank = V - 1 closes the last group of
every V) the member is moved to V - 2: a blank cannot be a copy of a token row."""
import numpy as np

from libreasr_amd import synth
from oracle import rnnt_oracle as O
from test_alignment_cpu import derive

F32 = np.float32
BOS = 1
BONUS = 12.0
MIN_MARGIN = 5e-3          # 2.5 x the 2e-3 by which two logits that are each within the project's 1e-3 can move their difference

GROUPS = {
    4112: [(5, 261), (200, 266), (2047, 2048, 3000), (4095, 4096), (1023, 4100, 4111)],
    2064: [(5, 261), (200, 266), (2047, 2048), (1023, 2063)],
    4096: [(5, 261), (200, 266), (2047, 2048), (3000, 4095)],
    2048: [(5, 517), (70, 576), (1023, 1024), (1500, 2047)],
}

# (cell, V, blank) -> seed of synth_state_dict.  The conditions of test_decision_edges_cpu.py are tight (every tie group wins twice in
# every run, no decision closer than MIN_MARGIN), so few seeds meet them and a change to synth.py or to the oracle's arithmetic
# invalidates them all.  tests/decision_edges_search.py finds them again: per model it walks the seeds in order and runs that
# model's checks of the CPU test.  These are the first seed that passed for each model; for the beam, the seed with the largest
# smallest gap among the first two or three that passed.
SEEDS = {
    ("tiny", 4112, 300): 1677, ("tiny_lstm", 4112, 4111): 2366, ("tiny", 2064, 2063): 4, ("tiny_lstm", 2064, 300): 10,
    ("tiny", 4096, 4095): 5, ("tiny_lstm", 4096, 300): 404,
    ("tiny_lstm", 4112, 300): 350,     # the blank-tie variants (and their plain model): offline and streamed at cap 2
}
# the beam model per width and run: the conditions of test_beam_conditions (at W = 8 about one seed in 200 meets them for one run,
# so each run has a model of its own).  Smallest non-tie gaps: 0.0028 / 0.0020 (W = 4), 0.0019 / 0.0014 (W = 8).
BEAM_SEEDS = {(4, "offline"): 50, (4, "streams"): 50, (8, "offline"): 221, (8, "streams"): 315}


# the models of test_gpu_decision_edges.py and what each one decodes there: offline caps, (streaming cap, row, reset_at)
MODELS = [("tiny", 4112, 300), ("tiny_lstm", 4112, 4111), ("tiny", 2064, 2063), ("tiny_lstm", 2064, 300), ("tiny", 4096, 4095),
          ("tiny_lstm", 4096, 300)]
OFFLINE_CAPS = (1, 2, 3)
STREAM_MODELS = MODELS[:2]
# a streaming run is both utterances as two streams: (cap, {row: model step before which that row's decoder is reset})
STREAM_RUNS = [(2, {1: 3}), (2, {}), (10, {})]
TIE_MODEL = ("tiny_lstm", 4112, 300)       # both blank-tie variants: offline and streaming (no reset) at cap 2


def groups(V, blank):
    out = []
    for g in GROUPS[V]:
        g = tuple(sorted({V - 2 if j == blank else j for j in g}))
        assert len(g) >= 2 and blank not in g and 0 not in g
        out.append(g)
    return out


_UTT, _FEATS = [], []


def utterances():
    """two 3 s utterances"""
    if not _UTT:
        _UTT.extend(synth.synth_pcm(2, 48000, seed=1234))
    return _UTT


def feats_all():
    if not _FEATS:
        _FEATS.extend(O.features_offline(p) for p in utterances())
    return _FEATS


def craft(name, V, blank, seed, tie=None, blank_bias=None, bonus=BONUS):
    """-> (state dict, cfg, blank bias).  blank_bias=None: calibrated here from the oracle (see the module docstring)."""
    cfg = synth.model_cfg(name)
    cfg["vocab"] = V
    sd = synth.synth_state_dict(cfg, seed=seed)
    w = sd["joint.joint.2.weight"].copy()
    b = sd["joint.joint.2.bias"].copy()
    w[[0, blank]] = w[[blank, 0]]
    b[[0, blank]] = b[[blank, 0]]
    for g in groups(V, blank):
        b[g[0]] += F32(bonus)
        for j in g[1:]:
            w[j] = w[g[0]]
            b[j] = b[g[0]]
    sd["joint.joint.2.weight"], sd["joint.joint.2.bias"] = w, b
    if blank_bias is None:
        for _ in range(8):                                   # fixed point of "bias = median of what the decode with it sees"
            m = O.OracleTransducer(sd, cfg, blank=blank, bos=BOS)
            best = []
            for f in feats_all():
                for z in m.decode_greedy(f, max_iters=2, return_logits=True)[4]:
                    z = z.copy()
                    z[blank] = -np.inf
                    best.append(float(z.max()))
            if 0.4 <= np.mean(np.asarray(best) < float(b[blank])) <= 0.65:
                break
            b[blank] = F32(np.median(best))
        blank_bias = float(b[blank])
    b[blank] = F32(blank_bias)
    if tie is not None:
        j = blank + 1 if tie == "plus" else blank - 1
        assert 0 < j < V and not any(j in g for g in groups(V, blank))
        w[j] = 0.0
        b[j] = b[blank]
    return sd, cfg, blank_bias


class Model:
    def __init__(self, name, V, blank, tie=None, seed=None):
        self.name, self.V, self.blank, self.bos, self.tie = name, V, blank, BOS, tie
        self.seed = SEEDS[name, V, blank] if seed is None else seed
        bias = None if tie is None else model(name, V, blank, None, seed).blank_bias
        self.sd, self.cfg, self.blank_bias = craft(name, V, blank, self.seed, tie, bias)
        self.groups = groups(V, blank)
        self.m = O.OracleTransducer(self.sd, self.cfg, blank=blank, bos=BOS)


_MODELS, _RUNS = {}, {}


def model(name, V, blank, tie=None, seed=None):
    key = (name, V, blank, tie, seed)
    if key not in _MODELS:
        _MODELS[key] = Model(*key)
    return _MODELS[key]


def margin(z):
    """the gap between the winning logit and the best one that is not bit-equal to it"""
    z = np.asarray(z, F32)
    top = z.max()
    return float(top) - float(z[z != top].max())


class Run:
    """one greedy decode of one utterance or stream by the oracle: tokens, frames, logps per emitted token (frames count from the
    start of the run); outs = the logits of every joint evaluation, evals = evaluations per frame, all_logps = log p of every
    decision; steps (streams) = per model step (tokens, frames, logps)."""

    def __init__(self):
        self.tokens, self.frames, self.logps, self.outs, self.evals, self.all_logps, self.steps = [], [], [], [], [], [], []
        self.neg_logp = self.score = None

    def add(self, toks, outs, T, cap, blank):
        recs, t_end, evals, logps = derive(outs, T, cap, blank)
        assert t_end == T and len(recs) == len(toks)
        base = len(self.evals)
        self.steps.append((list(toks), [base + f for f, _ in recs], [lp for _, lp in recs]))
        self.tokens += list(toks)
        self.frames += [base + f for f, _ in recs]
        self.logps += [lp for _, lp in recs]
        self.outs += outs
        self.evals += evals
        self.all_logps += logps

    @property
    def sum_iters(self):
        return int(sum(self.evals))

    @property
    def n_ones(self):
        return int(sum(1 for e in self.evals if e == 1))


def offline(mod, cap):
    """-> [Run per utterance] of Transducer.decode_greedy with max_iters = cap (computed once)"""
    key = (mod.name, mod.V, mod.blank, mod.tie, "off", cap)
    if key not in _RUNS:
        out = []
        for f in feats_all():
            y, neg_logp, score, iters, outs = mod.m.decode_greedy(f, max_iters=cap, return_logits=True)
            r = Run()
            r.add(y, outs, f.shape[0], cap, mod.blank)
            assert r.evals == list(iters)
            r.neg_logp, r.score = neg_logp, score
            out.append(r)
        _RUNS[key] = out
    return _RUNS[key]


TAIL = 2       # zero chunks behind the audio: every 3-chunk window still holds audio (on pure silence the float32 oracle stops
               # defining decisions to this file's margins, see test_gpu_alignment.stream_ref)


def chunks(row):
    return synth.stream_chunks(utterances()[row], 1280, lead=1, tail=TAIL)


def stream(mod, cap, row, reset_at=None):
    """-> Run of one stream through the oracle's streaming front-end and decoder; reset_at: decoder reset before that model step"""
    key = (mod.name, mod.V, mod.blank, mod.tie, "stream", cap, row, reset_at)
    if key not in _RUNS:
        fe, dec = O.StreamFrontend(), mod.m.stream_decoder(max_iters=cap)
        r = Run()
        for ch in chunks(row):
            o = fe.push(ch)
            if o is None:
                continue
            if reset_at is not None and len(r.steps) == reset_at:
                dec.reset()
            y_seq, outs = dec.step(o, return_logits=True)
            r.add(y_seq, outs, o.shape[0], cap, mod.blank)
        _RUNS[key] = r
    return _RUNS[key]


def stream_run(mod, cap, reset=None):
    """-> [Run per utterance]: both utterances as streams, reset = {row: model step}"""
    reset = reset or {}
    return [stream(mod, cap, row, reset.get(row)) for row in range(len(utterances()))]


def events(mod, runs, cap):
    """what happened in `runs` (a list of Run): group wins and whether every one was decided for the lowest index, copies bit-equal,
    blank share, frames at the cap, emitting frames below it, capped frames that are not the first of a lookahead window of 2,
    the smallest margin"""
    wins = {g: 0 for g in mod.groups}
    member = {j: g for g in mod.groups for j in g}
    ev = dict(wins=wins, lowest=True, copies_equal=True, n=0, blank=0, capped=0, uncapped_emitting=0, emitting=0, capped_odd=0,
              frames=0, min_margin=np.inf)
    for r in runs:
        for z in r.outs:
            a = int(np.argmax(z))
            ev["n"] += 1
            ev["blank"] += a == mod.blank
            ev["min_margin"] = min(ev["min_margin"], margin(z))
            for g in mod.groups:
                ev["copies_equal"] &= bool(np.all(z[list(g)].view(np.int32) == z[g[0]:g[0] + 1].view(np.int32)))
            g = member.get(a)
            if g is None and float(z[a]) in [float(z[q[0]]) for q in mod.groups]:
                ev["lowest"] = False                    # (a winner bit-equal to a group but outside it cannot happen)
            if g is not None:
                wins[g] += 1
                ev["lowest"] &= a == g[0]
        for t, e in enumerate(r.evals):
            ev["frames"] += 1
            ntok = r.frames.count(t)
            if ntok:
                ev["emitting"] += 1
                if ntok == cap:
                    ev["capped"] += 1
                    ev["capped_odd"] += t % 2 == 1
                else:
                    ev["uncapped_emitting"] += 1
    ev["blank_share"] = ev["blank"] / max(ev["n"], 1)
    return ev


def states(mod, cap, n_rows=64):
    """(h_pred, h_enc, logits) [n_rows, ..] of joint evaluations of the offline decodes (those a tie group wins first), replayed with the oracle's own
    encoder and predictor (pinned to offline(mod, cap).outs in the CPU test)"""
    m = mod.m
    hp, he, zs = [], [], []
    for f in feats_all():
        enc = m.encoder(f[None])[0][0]
        h_pred, ps = m.predictor([m.bos])
        for t in range(enc.shape[0]):
            for _ in range(cap):
                lp, z = m.joint_logp(h_pred, enc[t][None])
                hp.append(h_pred[0].copy()); he.append(enc[t].copy()); zs.append(z[0].copy())
                a = int(lp[0].argmax())
                if a == m.blank:
                    break
                h_pred, ps = m.predictor([a], ps)
    member = {j for g in mod.groups for j in g}
    won = [i for i, z in enumerate(zs) if int(np.argmax(z)) in member]         # rows on which a group wins come first
    rows = (won + [i for i in range(len(zs)) if i not in set(won)])[:n_rows]
    return np.stack([hp[i] for i in rows]), np.stack([he[i] for i in rows]), np.stack([zs[i] for i in rows])


def rand_labels(mod, n, seed):
    """n labels drawn from [0, V) without the blank"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, mod.V - 1, n)
    return [int(x) + (int(x) >= mod.blank) for x in v]


# ------------------------------------------------------------------------------- LM shallow fusion at a nonzero blank
LM_MODEL = ("tiny_lstm", 4096, 300)
LM_CFG = dict(vocab=4096, embed=32, hidden=32, layers=2, emb_scale=4.0)      # synth.LM_CONFIGS["tiny_lm"] at V = 4096
LM_SEED = 100
LM_MIN_MARGIN = 1e-3       # of the fused score alpha * lm + theta * joint (both standardised: O(1) values, float32 on both sides)


def lm_state_dict():
    return synth.synth_lm_state_dict(LM_CFG, seed=LM_SEED)


def lm_model(int8):
    """the oracle of LM_MODEL with the LM attached (a second OracleTransducer: model(*LM_MODEL).m stays unfused)"""
    key = ("lm model", int8)
    if key not in _RUNS:
        mod = model(*LM_MODEL)
        m = O.OracleTransducer(mod.sd, mod.cfg, blank=mod.blank, bos=BOS)
        m.lm = O.OracleLM(lm_state_dict(), quantized=int8)
        _RUNS[key] = m
    return _RUNS[key]


def lm_picks(m, run):
    """the fused decisions of one Run, replayed from its logits and tokens with a fuser of our own: [(joint's pick, fused pick,
    fused margin)].  The replay is pinned to the decode: the fuser's pick must be the token the decode emitted."""
    fz, picks, k = O.LMFuser(m.lm), [], 0
    for z in run.outs:
        a = int(np.argmax(z))
        if a == m.blank:
            continue
        top = z.max()
        lp = (z - (top + np.log(np.exp(z - top).sum(dtype=F32)))).astype(F32)          # joint_logp's log-softmax of these logits
        out = fz.fuse(lp, a)
        assert out == run.tokens[k], (k, out, run.tokens[k])
        if fz.lm_logits is not None:
            jo = O.standardize(lp)
            jo[0] = O.LM_MIN_VAL
            fused = (O.LM_ALPHA * fz.lm_logits).astype(F32) + (O.LM_THETA * jo).astype(F32)
            assert out == int(fused.argmax())
            two = np.sort(fused)[-2:]
            picks.append((a, out, float(two[1]) - float(two[0])))
        fz.advance(out)
        k += 1
    assert k == len(run.tokens)
    return picks


def lm_offline(int8, cap=3):
    """-> (runs with the LM attached, per run the (joint's pick, fused pick, fused margin) of every fused decision)"""
    key = ("lm", int8, cap)
    if key not in _RUNS:
        mod, m = model(*LM_MODEL), lm_model(int8)
        runs = []
        for f in feats_all():
            y, neg_logp, score, iters, outs = m.decode_greedy(f, max_iters=cap, return_logits=True)
            r = Run()
            r.add(y, outs, f.shape[0], cap, mod.blank)
            r.neg_logp, r.score = neg_logp, score
            runs.append(r)
        _RUNS[key] = (runs, [lm_picks(m, r) for r in runs])
    return _RUNS[key]


def lm_stream(int8, cap=3):
    """the same through the oracle's streaming front-end and stream decoder (its own LMFuser): -> (runs, picks), both utterances"""
    key = ("lm stream", int8, cap)
    if key not in _RUNS:
        mod, m = model(*LM_MODEL), lm_model(int8)
        runs = []
        for row in range(len(utterances())):
            fe, dec = O.StreamFrontend(), m.stream_decoder(max_iters=cap)
            r = Run()
            for ch in chunks(row):
                o = fe.push(ch)
                if o is not None:
                    y_seq, outs = dec.step(o, return_logits=True)
                    r.add(y_seq, outs, o.shape[0], cap, mod.blank)
            runs.append(r)
        _RUNS[key] = (runs, [lm_picks(m, r) for r in runs])
    return _RUNS[key]


# ------------------------------------------------------------------------------- beam search at a nonzero blank, with ties
BEAM_MODEL = ("tiny", 2048, 7)             # one seed per width and run (BEAM_SEEDS)
BEAM_WIDTHS = (4, 8)
BEAM_CAP = 2
BEAM_MARGIN = 1e-3         # beam_records_ref.MARGIN: a selection the oracle decides by less is a tie between GPU f32 and numpy f32


class BeamTrack:
    """one beam decode of the oracle, frame by frame: gaps = every selection-boundary gap and every gap between two kept hypotheses,
    pairs = frames after which two hypotheses survive that differ only in their last token, both of one tie group and emitted on
    that frame: both members survived a round; ties = those whose scores are still bit-equal at the end of the frame"""

    def __init__(self, mod, W):
        import beam_records_ref as B
        self.B, self.mod, self.W = B, mod, W
        self.member = {j: g for g in mod.groups for j in g}
        self.hyps, self.gaps, self.pairs, self.ties, self.t = B.beam_init_rec(mod.m), [], 0, 0, 0

    def frame(self, enc_t):
        member, t = self.member, self.t
        self.hyps = hyps = self.B.beam_frame_rec(self.mod.m, self.hyps, enc_t, t, self.W, BEAM_CAP, self.gaps)
        sc = sorted((h["score"] for h in hyps), reverse=True)
        self.gaps += [a - b for a, b in zip(sc, sc[1:])]
        for i, a in enumerate(hyps):
            for b in hyps[i + 1:]:
                if (a["y"] and len(a["y"]) == len(b["y"]) and a["y"][:-1] == b["y"][:-1] and a["y"][-1] != b["y"][-1]
                        and member.get(a["y"][-1]) is not None and member.get(a["y"][-1]) == member.get(b["y"][-1])
                        and a["r"][:-1] == b["r"][:-1] and a["r"][-1][0] == b["r"][-1][0] == t):      # ... of one parent, in a round of this frame
                    self.pairs += 1
                    if a["score"] == b["score"]:                         # emitted in the frame's last round: still bit-equal,
                        assert a["y"][-1] < b["y"][-1]                   # and the lower token holds the lower slot
                        self.ties += 1
        self.t += 1

    def ranked(self):
        return self.B.ranked(self.hyps)


def beam_model(W, kind):
    """kind: "offline" or "streams" (one model per run)"""
    return model(*BEAM_MODEL, seed=BEAM_SEEDS[W, kind])


def beam_offline(W):
    """per utterance dict(beam = the ranked whole beam at the end (beam_records_ref.ranked), T, gaps, pairs, ties: see BeamTrack)"""
    key = ("beam", W)
    if key not in _RUNS:
        mod = beam_model(W, "offline")
        out = []
        for f in feats_all():
            enc, _ = mod.m.encoder(f[None])
            bt = BeamTrack(mod, W)
            for t in range(enc.shape[1]):
                bt.frame(enc[0, t])
            out.append(dict(beam=bt.ranked(), T=bt.t, gaps=bt.gaps, pairs=bt.pairs, ties=bt.ties))
        _RUNS[key] = out
    return _RUNS[key]


def beam_stream(W):
    """per utterance, as a stream through the oracle's streaming front-end and encoder: dict(steps = [the ranked whole beam after
    every model step], T = [frames consumed up to and including that step], gaps, pairs, ties)"""
    key = ("beam stream", W)
    if key not in _RUNS:
        mod = beam_model(W, "streams")
        out = []
        for row in range(len(utterances())):
            fe, bt, state, steps, T = O.StreamFrontend(), BeamTrack(mod, W), None, [], []
            for ch in chunks(row):
                o = fe.push(ch)
                if o is None:
                    continue
                enc, state = mod.m.encoder(o[None], state)
                for k in range(enc.shape[1]):
                    bt.frame(enc[0, k])
                steps.append(bt.ranked())
                T.append(bt.t)
            out.append(dict(steps=steps, T=T, gaps=bt.gaps, pairs=bt.pairs, ties=bt.ties))
        _RUNS[key] = out
    return _RUNS[key]
