"""The language model of both decode loops in float64, with a per-element bound on what a correct engine may differ by (helper, not
a test): the LM case of tests/f32_exact.py and tests/bf16_exact.py, on their Stage / Trace / _tol and on lm_score_ref.LmRef.

A case is (LM config, rows B, passes per row, seeded tokens per row and pass).  Its stages are h and c of every layer after a row's
last pass, `raw` (the output layer's logits of that pass) and `lmz` (what k_lm_post makes of them: log-softmax, mean subtracted,
divided by the unbiased std + 1e-5, entry 0 = min_val).  A row that has fewer passes than the batch carries its state.

  f32    the rule of docs/f32_bound.md: the value is the float64 chain, Y the largest |float32 chain - float64 chain| of the stage over
         the batch (the float32 chain being OracleLM.step / standardize, restated row by row by StandInLM), tol = 8 Y floored at 4
         f32 ulps of the stage's largest magnitude.  Y comes from the CPU alone.
  bf16   the rule of docs/bf16_bound.md: the float64 chain rounds where the contract rounds (W_hh, W_ih of layers > 0 and the output
         weights are bf16, the layer-0 table is exact f32, h -- which is also the y the next layer and the output layer read -- is
         stored as bf16, c stays f32), with the per-element flip term and the caps of that document.
  int8   derived, no measurement: the integer part is exact on both sides (quantise / raw_int8 / tab_int8 below).
  terms  lasr_lm_score's log-probabilities with the bound they inherit from `raw` (term_bounds; tests/test_gpu_lm_score.py).

docs/lm_bound.md has the rule, the configs, the schedule each case reaches and the measured ratios."""
import numpy as np

import bf16_exact as X
from bf16_exact import F32, F64, FLOOR_ULPS, MARGIN, Stage, Trace, _tol
from lm_score_ref import LmRef
from oracle import rnnt_oracle as O

MIN_VAL = float(O.LM_MIN_VAL)
EPS = 1e-5
START = 2                     # the start token of every lm_score case

# hidden 32 tied and untied (synth.LM_CONFIGS), 96 (6 K chunks of 16: a tail in the 8-wave split; 3 chunks of 32 with bf16) and
# 1024 (64 chunks: gemm_body's (8, 8) entry on 8 waves with f32 operands)
LM_CONFIGS = {
    "h32": dict(vocab=64, embed=32, hidden=32, layers=2, emb_scale=1.0),
    "h32u": dict(vocab=64, embed=16, hidden=32, layers=2, emb_scale=1.0),
    "h96": dict(vocab=64, embed=32, hidden=96, layers=2, emb_scale=1.0),
    "h1024": dict(vocab=64, embed=32, hidden=1024, layers=2, emb_scale=1.0),
}
# weight seeds: of seeds 100..123 the one that leaves the bf16 chain the most token rows inside the caps (with most seeds the start
# token's own pass, which every row shares, already holds a tie-sensitive element)
LM_SEED = {"h32": 118, "h32u": 102, "h96": 103}
VOCABS = (64, 272, 2048, 2064, 4096)      # k_lm_post: < 256 columns, a ragged last slot, KEEP 8 full, the first KEEP 16 shape, the maximum
FLAT_TOKEN, FLAT_ENTRY = START, 7      # (the start token: a row that is fed nothing else stays at zero state)


def lm_cfg(name):
    """LM_CONFIGS, a name of synth.LM_CONFIGS, "v<V>" / "c<V>" (h32u at vocabulary V with the flat row of flat_lm, jittered / exactly
    constant), or a dict as it is"""
    from libreasr_amd import synth
    if isinstance(name, dict):
        return dict(name)
    if name in synth.LM_CONFIGS:
        return dict(synth.LM_CONFIGS[name])
    if name[0] in "vc" and name[1:].isdigit():
        return dict(LM_CONFIGS["h32u"], vocab=int(name[1:]))
    return dict(LM_CONFIGS[name])


def flat_lm(sd, V, jitter=True):
    """One token whose LM row has raw = the output bias exactly, and an output bias that is constant to within 2^-13 apart from one
    entry: the embedding row of FLAT_TOKEN and the g-gate biases of every layer are zero, so that token's g gates are tanh(0), c and h stay 0
    from zero state however often it is fed, and raw = b.  The token is the start token, so the first pass of EVERY row is flat; a
    row of other labels is an ordinary row from its second pass on (from zero state).  b = 0.5 with entry FLAT_ENTRY raised by sqrt(V) / 1024: the row's
    log-softmax has an unbiased std of about 1e-3, against which the + 1e-5 is one per cent.
    The other entries carry a seeded jitter of at most 2^-13 (an eighth of that std).  With V - 1 identical logits every rounding
    error of the row is the same one V - 1 times over, in numpy and in the kernel alike: the error of the mean no longer averages
    out, it depends on the summation order alone, and the float32 chain's distance from float64 -- the yardstick -- swings by a
    factor of 25 between vocabularies (3.8e-5 at V = 2064, 9.7e-4 at 4096, for values of 45 and 63) while the kernel's own stays
    near |log p| / std x 2^-24 = 5e-4, as it must (docs/lm_bound.md has the figures of that run).  The jitter makes the yardstick
    a fair sample of the noise of a row this badly conditioned; the condition itself, and with it the sensitivity to the + 1e-5,
    is the same."""
    sd = {k: np.array(v, F32) for k, v in sd.items()}
    sd["embed.weight"][FLAT_TOKEN] = 0.0
    l = 0
    while f"rnn.bias_ih_l{l}" in sd:
        H = sd[f"rnn.bias_ih_l{l}"].size // 4
        sd[f"rnn.bias_ih_l{l}"][2 * H:3 * H] = 0.0
        sd[f"rnn.bias_hh_l{l}"][2 * H:3 * H] = 0.0
        l += 1
    b = (0.5 + np.random.default_rng(V).uniform(-1.0, 1.0, V) / (8192.0 if jitter else np.inf)).astype(F32)
    b[FLAT_ENTRY] = F32(0.5 + np.sqrt(V) / 1024.0)
    sd["linear.bias"] = b
    return sd


_SD = {}


def state_dict(name):
    from libreasr_amd import synth
    key = name if isinstance(name, str) else tuple(sorted(name.items()))
    if key not in _SD:
        cfg = lm_cfg(name)
        sd = synth.synth_lm_state_dict(cfg, seed=LM_SEED.get(name, 100) if isinstance(name, str) else 100)
        flat = isinstance(name, str) and name[0] in "vc" and name[1:].isdigit()
        _SD[key] = flat_lm(sd, cfg["vocab"], jitter=name[0] == "v") if flat else sd
    return _SD[key]


def bf16_operands(sd):
    """the state dict as the dtype=bf16 engine holds it: W_hh, W_ih of layers > 0 and the output weights rounded, the rest as it is
    (a tied output layer is the rounded copy of the embedding; the table is made from the unrounded one)"""
    out = {k: np.asarray(v, F32) for k, v in sd.items()}
    out["linear.weight"] = O.bf16_round(out["linear.weight"] if "linear.weight" in out else out["embed.weight"])
    for k in sd:
        if k.startswith("rnn.weight_hh") or (k.startswith("rnn.weight_ih") and not k.endswith("_l0")):
            out[k] = O.bf16_round(out[k])
    return out


# ----------------------------------------------------------------------------- the last stage: k_lm_post
def post64(z, min_val=MIN_VAL):
    """raw [B, V] float64 -> lmz"""
    m = z.max(-1, keepdims=True)
    lp = (z - m) - np.log(np.exp(z - m).sum(-1, keepdims=True))
    t = lp - lp.mean(-1, keepdims=True)
    out = t / (t.std(-1, ddof=1, keepdims=True) + EPS)
    out[:, 0] = min_val
    return out


def post32(z, fault=None):
    """raw [V] float32 -> lmz as OracleLM.step's log_softmax and LMFuser.advance make it (fault: one of POST_FAULTS)"""
    z = np.asarray(z, F32)
    m = z.max()
    lp = ((z - m) - np.log(np.exp(z - m).sum(dtype=F32))).astype(F32)
    if fault is None:
        out = O.standardize(lp)
    else:
        # "mean_once": of the two subtractions of utils.py:162-164 (t -= t.mean(); then torch.std centres again) only std's own is
        # made -- the other way round (the values centred, the std taken about zero) moves nothing beyond rounding and no bound can see it
        t = lp if fault == "mean_once" else (lp - lp.mean(dtype=F32)).astype(F32)
        sd = t.std(ddof=0 if fault == "biased_std" else 1, dtype=F32)
        out = (t / (sd + F32(0.0 if fault == "no_eps" else EPS))).astype(F32)
    if fault != "entry0_standardised":
        out[0] = O.LM_MIN_VAL
    return out


def _post_flip(z, ez, out):
    """bound on the move of post64(z) when z moves by at most ez per element: log-sum-exp is 1-Lipschitz in the largest norm, so is
    the mean, the unbiased std moves by at most ||dt||_2 / sqrt(V - 1) <= sqrt(V / (V - 1)) max |dt|, and
    |t'/d' - t/d| <= (|dt| + |t/d| |dd|) / d' with d' >= d - |dd|"""
    V = z.shape[-1]
    e_lp = ez + ez.max(-1, keepdims=True)
    e_t = e_lp + e_lp.mean(-1, keepdims=True)
    m = z.max(-1, keepdims=True)
    lp = (z - m) - np.log(np.exp(z - m).sum(-1, keepdims=True))
    t = lp - lp.mean(-1, keepdims=True)
    den = t.std(-1, ddof=1, keepdims=True) + EPS
    e_den = np.sqrt(V / (V - 1.0)) * e_t.max(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):       # (no bound where the std itself may vanish: such a row is not checked)
        e = np.where(e_den < den, (e_t + np.abs(t / den) * e_den) / (den - e_den), np.inf)
    e[:, 0] = 0.0
    return np.where(ez.max(-1, keepdims=True) > 0, e, 0.0)


def post_conditioning(raw):
    """k_lm_post on a row whose logits are EXACTLY constant apart from one entry (the "c<V>" LMs): the float64 value and a bound
    from the conditioning alone.  With V - 1 identical logits every rounding error of the row is the same one V - 1 times over, so
    the float32 chain's distance from float64 is one draw of the summation order and no yardstick (3.8e-5 at V = 2064, 9.7e-4 at
    4096); what any f32 evaluation owes is the rounding of log p -- the subtraction of lse and of the mean, each at the magnitude
    of |log p| -- amplified by 1 / (std + 1e-5): FLOOR_ULPS f32 ulps of the row's largest |log p|, divided by that.
    -> (value [B, V], bound [B, 1])"""
    z = np.asarray(raw, F32).astype(F64)
    m = z.max(-1, keepdims=True)
    lp = (z - m) - np.log(np.exp(z - m).sum(-1, keepdims=True))
    t = lp - lp.mean(-1, keepdims=True)
    den = t.std(-1, ddof=1, keepdims=True) + EPS
    return post64(z), FLOOR_ULPS * ulp32(np.abs(lp).max(-1, keepdims=True)) / den


def post_stage(raw):
    """k_lm_post alone: the float64 standardisation of the engine's own raw [B, V] (float32) with the f32 rule, Y being numpy f32
    standardize against float64 on that same input"""
    raw = np.asarray(raw, F32)
    v = post64(raw.astype(F64))
    r32 = np.stack([post32(z) for z in raw])
    tol, Y = _tol(r32, v, np.zeros(v.shape))
    return Stage("lmz|raw", v, tol, np.zeros(v.shape), Y, r32)


# ----------------------------------------------------------------------------- float32: OracleLM's arithmetic, every stage visible
WEIGHT_FAULTS = ("bias_dropped", "gates_f_g_swapped", "h_k_tail_dropped")
RUN_FAULTS = ("row16_takes_row0", "idle_row_stepped", "parent_plus_one")
POST_FAULTS = ("mean_once", "biased_std", "no_eps", "entry0_standardised")
FAULT_UNIT = 5


def faulty_weights(sd, kind):
    """a copy of the state dict with one weight fault: the bias of gate f of unit 5 of layer 0 dropped; the rows of gates f and g of
    that unit swapped (weights and biases: the two pre-activations change places); the last 16-wide K chunk of every layer's W_hh
    left out"""
    sd = {k: np.array(v, F32) for k, v in sd.items()}
    H = sd["rnn.weight_hh_l0"].shape[1]
    f, g = H + FAULT_UNIT, 2 * H + FAULT_UNIT
    if kind == "bias_dropped":
        sd["rnn.bias_ih_l0"][f] = 0.0
        sd["rnn.bias_hh_l0"][f] = 0.0
    elif kind == "gates_f_g_swapped":
        for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            sd[f"rnn.{k}_l0"][[f, g]] = sd[f"rnn.{k}_l0"][[g, f]]
    elif kind == "h_k_tail_dropped":
        l = 0
        while f"rnn.weight_hh_l{l}" in sd:
            sd[f"rnn.weight_hh_l{l}"][:, -16:] = 0.0
            l += 1
    else:
        raise KeyError(kind)
    return sd


class StandInLM:
    """OracleLM.step + LMFuser.advance over a batch, row by row on the oracle's own functions (one row per call, as the oracle runs,
    so the two agree bit for bit) -- the float32 evaluation of the yardstick, and with a fault switched on the subtly wrong kernel
    of the sensitivity tests.  q: the rounding of the stored h (identity for f32, O.bf16_round for bf16)."""

    def __init__(self, sd, operand="f32", fault=None, W=1):
        self.sd0, self.operand, self.fault, self.W = sd, operand, fault, W
        if fault in WEIGHT_FAULTS:
            sd = faulty_weights(sd, fault)
        self.lm = O.OracleLM(bf16_operands(sd) if operand == "bf16" else sd)
        if operand == "bf16":                   # the table side stays exact: embedding and W_ih of layer 0 are not rounded
            assert np.array_equal(self.lm.embed, np.asarray(sd["embed.weight"], F32))
        self.q = O.bf16_round if operand == "bf16" else (lambda x: x)

    def run(self, toks, n=None, parent=None):
        """toks [B, U]; n [B] passes per row (default U); parent [B, U] (beam): the row whose state row r continues at pass u
        -> dict of [B, ..] float32 arrays: l{l}.u{u}.h.pre / .h / .c, u{u}.raw / .lmz, and l{l}.h / l{l}.c / raw / lmz / valid
        after the last pass (rows that were never stepped: zeros, valid 0)"""
        lm, q = self.lm, self.q
        toks = np.asarray(toks)
        B, U = toks.shape
        n = np.full(B, U) if n is None else np.asarray(n)
        L, H, V = len(lm.layers), lm.H, lm.w.shape[0]
        h = [np.zeros((B, H), F32) for _ in range(L)]
        hp = [np.zeros((B, H), F32) for _ in range(L)]
        c = [np.zeros((B, H), F32) for _ in range(L)]
        raw, lmz, valid = np.zeros((B, V), F32), np.zeros((B, V), F32), np.zeros(B, np.int32)
        s = {}
        for u in range(U):
            if parent is not None:
                src = np.asarray(parent)[:, u]
                if self.fault == "parent_plus_one":
                    src = (src // self.W) * self.W + (src % self.W + 1) % self.W
                h, hp, c = [x[src] for x in h], [x[src] for x in hp], [x[src] for x in c]
                raw, lmz, valid = raw[src], lmz[src], valid[src]
            elif self.fault == "row16_takes_row0" and u >= 1 and B > 16:
                for x in h + hp + c:
                    x[16] = x[0]
            h, hp, c = [x.copy() for x in h], [x.copy() for x in hp], [x.copy() for x in c]
            raw, lmz, valid = raw.copy(), lmz.copy(), valid.copy()
            for r in range(B):
                if u >= n[r] and self.fault != "idle_row_stepped":
                    continue
                x = lm.embed[toks[r, u]][None]
                for l, p in enumerate(lm.layers):
                    h2, c2 = O.lstm_step(x, h[l][r][None], c[l][r][None], p)
                    hp[l][r], c[l][r] = h2[0], c2[0]
                    x = q(h2)
                    h[l][r] = x[0]
                raw[r] = (x @ lm.w.T + lm.b).astype(F32)[0]
                lmz[r] = post32(raw[r], self.fault if self.fault in POST_FAULTS else None)
                valid[r] = 1
            for l in range(L):
                s[f"l{l}.u{u}.h.pre"], s[f"l{l}.u{u}.h"], s[f"l{l}.u{u}.c"] = hp[l], h[l], c[l]
            s[f"u{u}.raw"], s[f"u{u}.lmz"] = raw, lmz
        for l in range(L):
            s[f"l{l}.h.pre"], s[f"l{l}.h"], s[f"l{l}.c"] = hp[l], h[l], c[l]
        s["raw"], s["lmz"], s["valid"] = raw, lmz, valid
        return s


def mutated(ref, kind, W=1):
    """the stand-in `ref` with one of WEIGHT_FAULTS / RUN_FAULTS / POST_FAULTS (after bf16_exact.mutated)"""
    return StandInLM(ref.sd0, ref.operand, fault=kind, W=W)


# ----------------------------------------------------------------------------- float64 with the flip allowance
def _no_nan(e):
    """an allowance that has grown past every value (inf, and nan where inf met a zero): no bound"""
    return np.where(np.isnan(e), np.inf, e)


class Lm64(LmRef):
    """LmRef with the operands the engine holds (operand="bf16": bf16_operands) and a batched step that carries a flip allowance
    beside every value (bf16_exact.Exact._lstm); f32: the allowances are zero throughout"""

    def __init__(self, sd, operand="f32"):
        super().__init__(bf16_operands(sd) if operand == "bf16" else sd)
        self.operand = operand
        if operand == "bf16":                   # (LmRef ties the output layer to the embedding: here it is the rounded copy)
            self.w = np.asarray(bf16_operands(sd)["linear.weight"], F64)
        self.p = [dict(weight_ih_l0=wi, weight_hh_l0=wh, bias_ih_l0=bi, bias_hh_l0=bh) for wi, wh, bi, bh in self.layers]
        self.V = self.w.shape[0]

    def run(self, toks, ref32, n=None, parent=None):
        """-> Trace: l{l}.u{u}.c, l{l}.u{u}.h (bf16: + .h.pre, the unrounded value), u{u}.raw, u{u}.lmz for every pass over all B
        rows (a row without that pass carries), and the same names without u{u}. for the state after the last pass"""
        toks = np.asarray(toks)
        B, U = toks.shape
        n = np.full(B, U) if n is None else np.asarray(n)
        L, H, V, bf = len(self.p), self.H, self.V, self.operand == "bf16"
        tr = Trace()
        z = lambda *s: np.zeros(s)
        h, eh, c, ec = [z(B, H) for _ in range(L)], [z(B, H) for _ in range(L)], [z(B, H) for _ in range(L)], [z(B, H) for _ in range(L)]
        raw, eraw, lmz, elmz, valid = z(B, V), z(B, V), z(B, V), z(B, V), np.zeros(B, bool)
        hpre, ehpre = [z(B, H) for _ in range(L)], [z(B, H) for _ in range(L)]
        ramp = np.arange(V)[None] * 1.0         # stands in for the logits of a row that has none (its lmz is 0, valid 0)
        for u in range(U):
            if parent is not None:
                src = np.asarray(parent)[:, u]
                h, eh, c, ec, hpre, ehpre = ([a[src] for a in v] for v in (h, eh, c, ec, hpre, ehpre))
                raw, eraw, lmz, elmz, valid = raw[src], eraw[src], lmz[src], elmz[src], valid[src]
            act = (u < n)[:, None]
            valid = valid | act[:, 0]
            x, ex = self.embed[toks[:, u]], z(B, self.embed.shape[1])
            for l in range(L):
                hp, ehp, c2, ec2 = X.Exact._lstm(x, ex, h[l], eh[l], c[l], ec[l], self.p[l])
                ehp, ec2 = _no_nan(ehp), _no_nan(ec2)
                c[l], ec[l] = np.where(act, c2, c[l]), np.where(act, ec2, ec[l])
                tr.cont(f"l{l}.u{u}.c", c[l], ec[l], ref32)
                hpre[l], ehpre[l] = np.where(act, hp, hpre[l]), np.where(act, ehp, ehpre[l])
                name = f"l{l}.u{u}.h"
                if bf:
                    hq, fl = tr.rnd(name, hpre[l], ehpre[l], ref32)
                    # (a carried row keeps the value and the allowance it was stored with)
                    h[l], eh[l] = np.where(act, hq, h[l]), np.where(act, fl, eh[l])
                    tr[name] = Stage(name, h[l], 0.0, eh[l], 0.0, ref32[name], eh[l] > 0)
                else:
                    h[l] = hpre[l]
                    tr.cont(name, h[l], eh[l], ref32)
                x, ex = h[l], eh[l]
            r2, er2 = x @ self.w.T + self.b, _no_nan(ex @ np.abs(self.w).T)
            raw, eraw = np.where(act, r2, raw), np.where(act, er2, eraw)
            tr.cont(f"u{u}.raw", raw, eraw, ref32)
            safe = np.where(valid[:, None], raw, ramp)
            lz = post64(safe)
            lmz = np.where(act, lz, lmz)
            elmz = np.where(act, _post_flip(safe, eraw, lz), elmz)
            tr.cont(f"u{u}.lmz", lmz, elmz, ref32)
        last = U - 1
        for l in range(L):
            tr[f"l{l}.h"], tr[f"l{l}.c"] = tr[f"l{l}.u{last}.h"], tr[f"l{l}.u{last}.c"]
        tr["raw"], tr["lmz"] = tr[f"u{last}.raw"], tr[f"u{last}.lmz"]
        tr.final = [f"l{l}.{k}" for l in range(L) for k in ("h", "c")] + ["raw", "lmz"]
        return tr


class Chain:
    """the float64 model and the float32 stand-in of one LM and operand type"""

    def __init__(self, name, operand="f32"):
        self.name, self.operand, self.sd, self.cfg = name, operand, state_dict(name), lm_cfg(name)
        self.m, self.ref = Lm64(self.sd, operand), StandInLM(self.sd, operand)

    def run(self, toks, n=None, parent=None):
        with np.errstate(over="ignore", invalid="ignore"):      # (an allowance that outgrows every value becomes inf: no bound)
            return self.m.run(toks, self.ref.run(toks, n, parent), n, parent)


_CHAINS, _CASES = {}, {}


def chain(name, operand="f32"):
    key = (name if isinstance(name, str) else tuple(sorted(name.items())), operand)
    if key not in _CHAINS:
        _CHAINS[key] = Chain(name, operand)
    return _CHAINS[key]


UMAX = 3


def seeded_tokens(V, B, seed, avoid=None):
    """labels [B, UMAX] from [1, V): no blank; row 16 never starts like row 0 (the m-tile mix-up has to show)"""
    rng = np.random.default_rng([seed, B, V])
    toks = rng.integers(1, V, (B, UMAX)).astype(np.int32)
    if avoid is not None:
        toks[toks == avoid] = avoid + 1
    if B > 16 and toks[16, 0] == toks[0, 0]:
        toks[16, 0] = 3 + (toks[0, 0] + 1) % (V - 3)
    return toks


def lm_inputs(labels):
    """what the LM reads for a row's labels y_1 .. y_U under lasr_lm_score with start = START: (START, y_1, .., y_{U-1})"""
    labels = np.asarray(labels)
    return np.concatenate([np.full((len(labels), 1), START, labels.dtype), labels[:, :-1]], 1)


def case(name, operand, B, seed=0, ragged=False):
    """-> (labels [B, UMAX], n [B], Trace) of one lm_score case, computed once and left unchanged.  Scoring the first U labels of
    every row makes U passes, behind which the engine holds the stages u{U-1}.raw / u{U-1}.lmz (the LM reads lm_inputs(labels): the
    labels of a shorter call are a prefix, so one chain serves U = 1, 2, 3).  ragged: row r is scored on its first n[r] labels (1 ..
    UMAX by row) and the stages are `raw` / `lmz`, every row's own last pass.  A "v<V>" LM gives its last row FLAT_TOKEN throughout
    (flat_lm) and no other row that token.  bf16: the rows are picked from a seeded pool by the reference alone so that the caps of
    docs/bf16_bound.md hold (bf16_exact._rows), except where no such batch exists (capped()): those cases are held to tol + flip
    outside the caps, like the encoder's deeper stages there."""
    key = (name, operand, B, seed, ragged)
    if key in _CASES:
        return _CASES[key]
    ch = chain(name, operand)
    V = ch.cfg["vocab"]
    n = (1 + (np.arange(B) * 2 + seed) % UMAX) if ragged else np.full(B, UMAX)
    flat = isinstance(name, str) and name.startswith("v")

    def fix(labels):
        labels = np.array(labels)
        if flat:
            labels[-1, :] = FLAT_TOKEN
        return labels

    if operand == "f32" or not capped(name):
        labels = fix(seeded_tokens(V, B, seed, FLAT_TOKEN if flat else None))
        out = (labels, n, ch.run(lm_inputs(labels), n))
    else:
        pool = seeded_tokens(V, X.POOL * B + 256, seed)
        order = X._pick_within_caps(ch.run(lm_inputs(pool)))       # (all UMAX passes: a row that is clean there is clean when cut short)
        idx, tr = X._rows(lambda i: ch.run(lm_inputs(pool[i]), n), order, B)
        out = (pool[idx], n, tr)
    _CASES[key] = out
    return out


def capped(name):
    """bf16: can a batch be picked inside the caps?  Not at hidden 1024 (a row has 2 x 1024 rounded elements per pass: every row of
    the pool holds tie-sensitive ones), and not with a flat row (its h is exactly 0, where the bf16 grid is finer than any tol:
    the tie rule flags every element of it)"""
    return lm_cfg(name)["hidden"] < 1024 and not (isinstance(name, str) and name.startswith("v"))


# ----------------------------------------------------------------------------- the int8-served form
QUANT_FAULTS = ("zero_point_unclamped", "scale_zero_kept", "truncated", "padding_nonzero")


def quantise(x, Kp, fault=None, nxt=None):
    """One row of h as k_lm_cell_q / k_lm_quant store it: (q - zp as float32 [Kp], scale float32), ChooseQuantizationParams(min(x, 0),
    max(x, 0), 0, 127) as oracle.rnnt_oracle.dq_linear states it, columns [len(x), Kp) zero.  fault: one of QUANT_FAULTS
    (padding_nonzero: the padding columns hold the quantised start of the row `nxt`)."""
    x = np.asarray(x, F32).reshape(-1)
    mn, mx = min(float(x.min()), 0.0), max(float(x.max()), 0.0)
    if fault in ("zero_point_unclamped", "scale_zero_kept"):
        scale = (np.float64(mx) - np.float64(mn)) / 127.0
        if (scale == 0.0 or np.isinf(1.0 / scale)) and fault != "scale_zero_kept":
            scale = 0.1
        if scale == 0.0:
            return np.zeros(Kp, F32), F32(0.0)
        zmin, zmax = 0.0 - mn / scale, 127.0 - mx / scale
        izp = zmin if abs(mn / scale) < 127.0 + abs(mx / scale) else zmax
        zp = int(np.rint(izp)) if fault == "zero_point_unclamped" else int(min(max(np.rint(izp), 0), 127))
        s = F32(scale)
    else:
        s, zp = O.dq_choose_qparams(x.min(), x.max())
    v = x * (F32(1.0) / s)
    qx = np.clip((np.trunc(v) if fault == "truncated" else np.rint(v)) + zp, 0, 127)
    out = np.zeros(Kp, F32)
    out[:x.size] = qx - zp
    if fault == "padding_nonzero":
        out[x.size:] = quantise(nxt, Kp)[0][:Kp - x.size]
    return out, F32(s)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def dequant64(acc, sx, sw, b):
    """acc (integers) * (sx * sw) + b in float64 on the float32 operands, and the int8 rule's bound: three f32 roundings of at most
    half an ulp each (the product of the scales, the scaled sum, the sum with the bias), of which contraction may remove one --
    2 ulps of the largest intermediate magnitude"""
    acc, sx, sw, b = np.asarray(acc, F64), np.asarray(sx, F32).astype(F64), float(F32(sw)), np.asarray(b, F32).astype(F64)
    prod = acc * (sx * sw)
    v = prod + b
    return v, 2.0 * ulp32(np.maximum(np.abs(prod), np.abs(v)))


def raw_int8(qh, sxh, sd):
    """lm_raw of the int8-served form from the engine's own quantised h of the last layer (qh [B, Kp], sxh [B]) and the host-side
    quantised output weights -> (value [B, V] float64, bound [B, V])"""
    w = np.asarray(sd["linear.weight"] if "linear.weight" in sd else sd["embed.weight"], F32)
    qw, sw = O.dq_weight(w)
    acc = np.asarray(qh, F64)[:, :w.shape[1]] @ qw.astype(F64).T
    assert np.abs(acc).max() < 2 ** 24
    return dequant64(acc, np.asarray(sxh)[:, None], sw, np.asarray(sd["linear.bias"], F32)[None])


def tab_int8(sd):
    """lm_tab of the int8-served form: linear_dynamic(embed[v]; W_ih of layer 0) + b_ih of layer 0 -> (value [V, 4H], bound, integer sums)"""
    emb, w = np.asarray(sd["embed.weight"], F32), np.asarray(sd["rnn.weight_ih_l0"], F32)
    qw, sw = O.dq_weight(w)
    q = [quantise(e, emb.shape[1]) for e in emb]
    acc = np.stack([a for a, _ in q]).astype(F64) @ qw.astype(F64).T
    v, bound = dequant64(acc, np.array([s for _, s in q], F32)[:, None], sw, np.asarray(sd["rnn.bias_ih_l0"], F32)[None])
    return v, bound, acc


SAT_CFG = dict(vocab=64, embed=1024, hidden=32, layers=1)
SAT_SUM = -16646144        # 1024 x 127 x (-128): the largest magnitude an integer sum of the int8-served form can reach, below 2^24


def saturating_lm(c=0.75, a=0.05):
    """E = 1024, every embedding row the positive constant c, every W_ih entry of layer 0 equal to -a: every quantised activation is
    127 (range [0, c], zero point 0), every quantised weight -128 (scale a / 127.5, rint(-127.5) is even; a is one for which the
    float32 product -a * (1 / scale) is -127.5 itself and not the float below it in magnitude), every integer sum SAT_SUM"""
    from libreasr_amd import synth
    sd = {k: np.array(v, F32) for k, v in synth.synth_lm_state_dict(SAT_CFG).items()}
    sd["embed.weight"][:] = c
    sd["rnn.weight_ih_l0"][:] = -a
    return sd


def replay_int8(sd, seqs):
    """OracleLM(quantized=True) over each token sequence from zero state -> h, c [L][B, H] float32, raw [B, V] (zeros for an empty one)"""
    lm = O.OracleLM(sd, quantized=True)
    L, H = len(lm.layers), lm.H
    h, c = np.zeros((L, len(seqs), H), F32), np.zeros((L, len(seqs), H), F32)
    for r, seq in enumerate(seqs):
        st = None
        for tok in seq:
            _, st = lm.step(int(tok), st)
        if st is not None:
            for l in range(L):
                h[l, r], c[l, r] = st[l][0][0], st[l][1][0]
    return h, c


# ----------------------------------------------------------------------------- replays of decoded tokens
def replay(name, operand, seqs, parent=None):
    """The LM from zero state over each row's own emitted tokens (padded to the longest; a row carries behind its last) -> Trace
    whose final stages hold every row's state after its last token.  The tolerance comes from the whole-chain Y of this replay."""
    ch = chain(name, operand)
    U = max(1, max(len(s) for s in seqs))
    toks = np.zeros((len(seqs), U), np.int32)
    for r, s in enumerate(seqs):
        toks[r, :len(s)] = s
    n = np.array([len(s) for s in seqs])
    return ch.run(toks, n), n


def _lse(z):
    m = z.max(-1, keepdims=True)
    return m + np.log(np.exp(z - m).sum(-1, keepdims=True))


def term_bounds(name, operand, cands, start):
    """lasr_lm_score's terms with their bound (tests/test_gpu_lm_score.py) -> [(lp float64 [U], bound [U])] per candidate.  A term
    is raw[y] - lse(raw) of the pass that reads the label's predecessor: it moves by at most the bound of raw[y] plus the row's
    largest (log-sum-exp is 1-Lipschitz in the largest norm), plus the reduction's own tol -- 8 Y, Y being the float32
    log-softmax of the float32 chain's raw against the float64 one of the same raw, floored at 4 f32 ulps (as for lp in
    bf16_exact.Exact.joint).  start = None: the first label has no term (0, bound 0)."""
    shift = 1 if start is None else 0
    xs = [([] if not len(y) else list(y[:-1]) if shift else [start] + list(y[:-1])) for y in cands]
    tr, n = replay(name, operand, xs)
    out = [(np.zeros(len(y)), np.zeros(len(y))) for y in cands]
    for u in range(int(n.max())):
        s = tr[f"u{u}.raw"]
        rows = np.nonzero(n > u)[0]
        tgt = np.array([cands[r][u + shift] for r in rows])
        z, b, z32 = s.value[rows], s.bound()[rows], s.ref32[rows]
        lp = (z - _lse(z))[np.arange(len(rows)), tgt]
        m32 = z32.max(-1, keepdims=True)
        lp32 = ((z32 - m32) - np.log(np.exp(z32 - m32).sum(-1, keepdims=True, dtype=F32))).astype(F32)
        lp32_64 = z32.astype(F64) - _lse(z32.astype(F64))
        Y = float(np.abs(lp32.astype(F64) - lp32_64)[np.arange(len(rows)), tgt].max())
        tol = max(MARGIN * Y, FLOOR_ULPS * float(np.spacing(F32(np.abs(lp).max() + np.abs(z).max()))))
        bound = b[np.arange(len(rows)), tgt] + b.max(-1) + tol
        for i, r in enumerate(rows):
            out[r][0][u + shift], out[r][1][u + shift] = lp[i], bound[i]
    return out


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_lm_exact.py
ROWS64, ROWS128 = (1, 16, 17, 33, 64), (80,)
PASSES = (1, 2, 3)
SCORE_LMS = {"f32": ("h32", "h32u", "h96", "h1024"), "bf16": ("h32", "h32u", "h96", "h1024")}
POST_ROWS = 17
# (LM, waves, entries of the layers' cell launches, entry of the output layer): launch_lm_t at this commit -- every cell in the
# four-unit tiling on 8 waves (layer 0's x phase is the token table: absent), the output layer launch_linear_ops on 8 waves
LM_SCHEDULES = [("h32", 8, [None, None], [None]), ("h32u", 8, [None, None], [None]), ("h96", 8, [None, None], [None]),
                ("h1024", 8, [(8, 8), (8, 8)], [(8, 8)])]

