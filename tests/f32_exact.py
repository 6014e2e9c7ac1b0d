"""The dtype=f32 kernels' yardstick: every stage in float64, with a per-element bound on what a correct engine may differ by (helper,
not a test).  The f32 case of tests/bf16_exact.py, on its Stage / Trace / _tol / StandIn.

f32 weights and activations are exact in float64 and nothing is rounded between stages, so the float64 evaluation of the whole
chain on the values as they are is the value, there is no flip term (flip = 0 everywhere), no tie cap, and no input is picked:

  tol   one number per stage: 8 x Y, floored at 4 f32 ulps of the stage's largest magnitude (bf16_exact._tol, unchanged).  Y is
        the largest |float32 numpy oracle - float64| over the stage, on the same inputs, for the same batch: the oracle's own
        arithmetic (OracleTransducer(operand="f32"), restated stage by stage by bf16_exact.StandIn, whose activation rounding is
        the identity here).  Y comes from the CPU alone, never from the engine.
  deep  layer 1, the second frame and the second token take Y from the whole float32 chain against the whole float64 chain: that
        difference contains the propagation of the f32 noise of every earlier stage, so no extra term is propagated.

An engine value passes when |engine - value| <= tol, element by element.  docs/f32_bound.md has the rule, the K schedule every
(launcher, model, wave count) takes, the sensitivity table and the measured ratios."""
import copy

import numpy as np

import bf16_exact as X
from bf16_exact import F32, F64, FLOOR_ULPS, MARGIN, Stage, StandIn, Trace, sig
from oracle import rnnt_oracle as O


# ----------------------------------------------------------------------------- float64
def _lstm(x, h, c, p):
    H = h.shape[-1]
    g = x @ p["weight_ih_l0"].T + p["bias_ih_l0"] + h @ p["weight_hh_l0"].T + p["bias_hh_l0"]
    c2 = sig(g[:, H:2 * H]) * c + sig(g[:, :H]) * np.tanh(g[:, 2 * H:3 * H])
    return sig(g[:, 3 * H:]) * np.tanh(c2), c2


def _nbrc(x, h, p):
    H = h.shape[-1]
    Wx, Rh = x @ p["kernel"] + p["bias"], h @ p["recurrent_kernel"] + p["recurrent_bias"]
    z, r = sig(Wx[:, :H] + Rh[:, :H]), sig(Wx[:, H:2 * H] + Rh[:, H:2 * H])
    return z * h + (1.0 - z) * np.tanh(Wx[:, 2 * H:] + r * Rh[:, 2 * H:])


class Exact:
    """The float64 model of the f32 engine: .encoder / .predictor / .joint -> Trace of continuous stages (flip = 0, tie = None),
    named as StandIn names them without ".pre" (the value before rounding and the rounded one coincide: one is kept)."""

    def __init__(self, sd, cfg):
        self.cfg = cfg
        self.o = O.OracleTransducer(sd, cfg, operand="f32")
        self.ref = StandIn(self.o)
        self.H, self.lstm = cfg["hidden"], cfg["pred_cell"] == "LSTM"
        d = lambda v: np.asarray(v, F64)
        self.ln_w, self.ln_b = d(self.o.ln_w), d(self.o.ln_b)

        def stack(cells):
            out = []
            for L in cells:
                bn = {k: d(v) for k, v in L["bn"].items()}
                s = bn["weight"] / np.sqrt(bn["running_var"] + 1e-5)
                out.append(dict(rnn={k: d(v) for k, v in L["rnn"].items()}, hs=d(L["hs"]), bn_s=s, bn_t=bn["bias"] - bn["running_mean"] * s))
            return out

        self.enc, self.pred = stack(self.o.enc), stack(self.o.pred)
        self.embed = d(self.o.embed)
        self.ffn = None if self.o.ffn_w is None else (d(self.o.ffn_w), d(self.o.ffn_b))
        self.j0_w, self.j0_b, self.j2_w, self.j2_b = d(self.o.j0_w), d(self.o.j0_b), d(self.o.j2_w), d(self.o.j2_b)

    @staticmethod
    def _cont(tr, name, x64, ref):
        tr.cont(name, x64, np.zeros(x64.shape), ref)

    def encoder(self, x):
        """x [B, T, F] float32 -> Trace: x0 [B, T, F], enc{l}.t{t}.c / .h [B, H], enc{l}.y (BN(h), [B, T, H])"""
        ref, tr = self.ref.encoder(x), Trace()
        B, T, _ = x.shape
        x = X._ln64(self, x)[0]
        self._cont(tr, "x0", x, ref)
        for l, L in enumerate(self.enc):
            h, c = np.repeat(L["hs"][0, 0], B, 0), np.repeat(L["hs"][1, 0], B, 0)
            ys = np.empty((B, T, self.H))
            for t in range(T):
                h, c = _lstm(x[:, t], h, c, L["rnn"])
                ys[:, t] = h
                self._cont(tr, f"enc{l}.t{t}.c", c, ref)
                self._cont(tr, f"enc{l}.t{t}.h", h, ref)
            x = ys * L["bn_s"] + L["bn_t"]
            self._cont(tr, f"enc{l}.y", x, ref)
        return tr

    def predictor(self, toks):
        """toks [B, U] -> Trace: pred{l}.u{u}.h, .y (BN(h)), .c (LSTM)"""
        toks = np.asarray(toks)
        ref, tr = self.ref.predictor(toks), Trace()
        B, U = toks.shape
        st = [(np.repeat(L["hs"][0, 0], B, 0), np.repeat(L["hs"][1, 0], B, 0) if self.lstm else None) for L in self.pred]
        for u in range(U):
            x = self.embed[toks[:, u]]
            if self.ffn is not None:
                x = x @ self.ffn[0].T + self.ffn[1]
            for l, L in enumerate(self.pred):
                if self.lstm:
                    h, c = _lstm(x, st[l][0], st[l][1], L["rnn"])
                    self._cont(tr, f"pred{l}.u{u}.c", c, ref)
                else:
                    h, c = _nbrc(x, st[l][0], L["rnn"]), None
                self._cont(tr, f"pred{l}.u{u}.h", h, ref)
                st[l] = (h, c)
                x = h * L["bn_s"] + L["bn_t"]
                self._cont(tr, f"pred{l}.u{u}.y", x, ref)
        return tr

    def joint(self, a, b):
        """a = h_pred, b = h_enc [B, H] float32 -> Trace: pp, pe, act, logits, lp (the largest log-softmax of the row)"""
        ref, tr = self.ref.joint(a, b), Trace()
        H = self.H
        a, b = np.asarray(a, F64), np.asarray(b, F64)
        pp, pe = a @ self.j0_w[:, :H].T + self.j0_b, b @ self.j0_w[:, H:].T
        self._cont(tr, "pp", pp, ref)
        self._cont(tr, "pe", pe, ref)
        act = np.tanh(pp + pe)
        self._cont(tr, "act", act, ref)
        z = act @ self.j2_w.T + self.j2_b
        self._cont(tr, "logits", z, ref)
        # lp: within the logits' bound plus the reduction's own yardstick -- the float32 log-softmax of the float32 logits against
        # the float64 one of the same logits (as in bf16_exact.Exact.joint)
        lp = lambda v: (v - v.max(-1, keepdims=True) - np.log(np.exp(v - v.max(-1, keepdims=True)).sum(-1, keepdims=True))).max(-1)
        Y = float(np.abs(ref["lp"].astype(F64) - lp(ref["logits"].astype(F64))).max())
        tol = max(MARGIN * Y, FLOOR_ULPS * float(np.spacing(F32(np.abs(lp(z)).max() + np.abs(z).max()))))
        tr["lp"] = Stage("lp", lp(z), tr["logits"].tol + tol, np.zeros(len(z)), Y, ref["lp"])
        tr.tol_reduction = tol
        return tr


# ----------------------------------------------------------------------------- models
def wide_cfg(hidden, pred_cell, feat=1280):
    """tiny's depth (2 + 2 layers), embedding and vocabulary at a width whose K meets a static schedule of gemm_body"""
    from libreasr_amd import synth
    return dict(synth.model_cfg("tiny"), feat=feat, hidden=hidden, joint=hidden, pred_cell=pred_cell)


WIDE = {"s1024": (1024, "NBRC"), "s1024_lstm": (1024, "LSTM"), "s1536_lstm": (1536, "LSTM"),
        "s256": (256, "NBRC", 320)}           # 64 mels x 5 stacked frames: K = 320 / 256, the 4- and 5-chunk schedules on 4 waves
MODELS = ["tiny", "tiny_lstm", "d96", "d96_lstm", "d96_v80", "g768", "s256", "s1024", "s1024_lstm", "s1536_lstm"]
FRONTEND = dict(X.FRONTEND, s256=dict(n_mels=64, n_stack=5))        # Engine keywords of a model whose feat is not 128 x 10


def model_cfg(name):
    return wide_cfg(*WIDE[name]) if name in WIDE else X.model_cfg(name)


_MODELS = {}


def model(name):
    """-> (Exact, state dict, cfg); the weights of the models bf16_exact has are the same ones (same seeds)"""
    from libreasr_amd import synth
    if name not in _MODELS:
        cfg = model_cfg(name)
        sd = synth.synth_state_dict(cfg, seed=X.MODEL_SEED.get(name, 0))
        _MODELS[name] = (Exact(sd, cfg), sd, cfg)
    return _MODELS[name]


_CASES = {}


def case(kind, name, B, n=1, seed=0):
    """-> (inputs, Trace) of one case, computed once and left unchanged.  kind "enc": n = T', inputs [B, T', feat] seeded normal
    with a per-row scale and offset; "pred": n = U, seeded tokens [B, U] (no blank); "joint": (h_pred, h_enc) [B, hidden] seeded
    normal.  Nothing is picked: no f32 stage is tie-sensitive."""
    key = (kind, name, B, n, seed)
    if key not in _CASES:
        m, _, cfg = model(name)
        rng = np.random.default_rng([seed, B, n, {"enc": 1, "pred": 2, "joint": 3}[kind]])
        if kind == "enc":
            x = (rng.standard_normal((B, n, cfg["feat"])) * rng.uniform(0.5, 2.0, (B, 1, 1)) + rng.uniform(-1, 1, (B, 1, 1))).astype(F32)
            _CASES[key] = (x, m.encoder(x))
        elif kind == "pred":
            toks = rng.integers(1, cfg["vocab"], (B, n)).astype(np.int32)
            _CASES[key] = (toks, m.predictor(toks))
        else:
            a, b = rng.standard_normal((B, cfg["hidden"])).astype(F32), rng.standard_normal((B, cfg["hidden"])).astype(F32)
            _CASES[key] = ((a, b), m.joint(a, b))
    return _CASES[key]


# ----------------------------------------------------------------------------- sensitivity: the subtly wrong kernels
def tf32(x):
    """f32 with the low 13 mantissa bits cleared: what a reduced-precision matrix instruction would read"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return (u & np.uint32(0xFFFFE000)).view(F32)


CHUNK = slice(16, 32)       # K chunk 1 of Ops::KCH = 16 elements: one wave's share of a K split


def mutated(o, kind):
    """a copy of the f32 oracle `o` with one weight fault: bf16_exact.mutated's "k_tail" and "bias_twice"; "chunk_dropped" /
    "chunk_twice": K chunk 1 of the recurrent GEMM of every cell and of the vocabulary GEMM left out / added twice; "tf32": the
    weight operand of encoder layer 0's input GEMM with its low 13 mantissa bits cleared"""
    if kind in ("k_tail", "bias_twice"):
        return X.mutated(o, kind)
    m = copy.copy(o)
    m.enc = [dict(L, rnn=dict(L["rnn"])) for L in o.enc]
    m.pred = [dict(L, rnn=dict(L["rnn"])) for L in o.pred]
    if kind in ("chunk_dropped", "chunk_twice"):
        f = F32(0.0 if kind == "chunk_dropped" else 2.0)
        for L in m.enc + m.pred:
            k = "weight_hh_l0" if "weight_hh_l0" in L["rnn"] else "recurrent_kernel"
            w = L["rnn"][k].copy()
            if k == "weight_hh_l0":
                w[:, CHUNK] *= f                     # torch layout [4H, K]
            else:
                w[CHUNK, :] *= f                     # haste layout [K, 3H]
            L["rnn"][k] = w
        m.j2_w = o.j2_w.copy()
        m.j2_w[:, CHUNK] *= f
    elif kind == "tf32":
        m.enc[0]["rnn"]["weight_ih_l0"] = tf32(o.enc[0]["rnn"]["weight_ih_l0"])
    else:
        raise KeyError(kind)
    return m


# ----------------------------------------------------------------------------- the K schedule a launch takes
# gemm_body (lasr_gemm.hip.h) runs the fully unrolled gemm_static when, for an entry (N0, N1) of its f32 list, every phase the
# epilogue has satisfies KC == N x waves (KC = K / 16 chunks), the first entry that fits; otherwise the dynamic gemm_phase loop.
# Nothing in the engine reports which: this restates the list and the launchers at this commit (docs/f32_bound.md).
F32_TRY = [(4, 4), (5, 4), (16, 16), (20, 16), (8, 8), (10, 8), (12, 12), (10, 12)]
KCH = 16


def static_entry(k0, k1, nw):
    """the list entry a launch with k0 / k1 chunks (None: the epilogue has no such phase) on nw waves takes, or None (dynamic loop)"""
    for n0, n1 in F32_TRY:
        if (k0 is None or k0 == n0 * nw) and (k1 is None or k1 == n1 * nw):
            return (n0, n1)
    return None


def launches(launcher, cfg):
    """[(k0, k1)] of the GEMM launches of one pass: "enc_cell" one per layer (x phase K = feat or hidden, h phase K = hidden);
    "pred_cell" one per layer (layer 0's x phase is the token table: absent); "joint_half" pp and pe (one phase, K = hidden);
    "logits" (one phase, K = joint); of an LM step (cfg: an LM config; launch_lm_t): "lm_cell" one per layer (layer 0's x phase is
    the token table: absent), "lm_out" the output layer (one phase, K = hidden)"""
    if launcher in ("lm_cell", "lm_out"):
        H = cfg["hidden"] // KCH
        return [(None if l == 0 else H, H) for l in range(cfg["layers"])] if launcher == "lm_cell" else [(H, None)]
    F, H, J = cfg["feat"] // KCH, cfg["hidden"] // KCH, cfg["joint"] // KCH
    if launcher == "enc_cell":
        return [(F if l == 0 else H, H) for l in range(cfg["enc_layers"])]
    if launcher == "pred_cell":
        return [(None if l == 0 else H, H) for l in range(cfg["pred_layers"])]
    return {"joint_half": [(H, None), (H, None)], "logits": [(J, None)]}[launcher]


def schedule(launcher, name, nw):
    """the static entries (None: dynamic) of the launches of `launcher` for model `name` (a config dict is taken as it is: the LM
    kinds) on nw waves"""
    return [static_entry(k0, k1, nw) for k0, k1 in launches(launcher, name if isinstance(name, dict) else model_cfg(name))]


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_f32_exact.py
# encoder tilings: (environment, what Engine.config reports, waves of the K split).  launch_enc_cell_t / launch_enc_wave_t: tiling C
# on cell_nw waves (f32 default 4); tiling D on 8 waves unless LASR_CELL_NW is 4 (it tests the switch, not the f32 default: config
# reports cell_nw 4 either way)
ENC_TILINGS = {
    "default": ({}, dict(enc_wave=0, cell_nw=4, enc_u12=0), 4),
    "eight_waves": ({"LASR_CELL_NW": "8"}, dict(enc_wave=0, cell_nw=8, enc_u12=0), 8),
    "wavefront": ({"LASR_ENC_WAVE": "1"}, dict(enc_wave=1, cell_nw=4, enc_u12=0), 4),
    "tiling_d": ({"LASR_ENC_U12": "1"}, dict(enc_wave=0, cell_nw=4, enc_u12=1), 8),
    "tiling_d_four_waves": ({"LASR_ENC_U12": "1", "LASR_CELL_NW": "4"}, dict(enc_wave=0, cell_nw=4, enc_u12=1), 4),
}
TILING_C, TILING_D = ("default", "eight_waves", "wavefront"), ("tiling_d", "tiling_d_four_waves")
DYNAMIC_ROWS, STATIC_ROWS = (1, 16, 17, 33, 64), (17, 64)
# (model, tiling, rows, the static entry of each layer's launch): tiling D needs hidden % 12 == 0 -- d96 and s1536_lstm
ENC_PARAMS = (
    [("tiny", t, DYNAMIC_ROWS, [None, None]) for t in TILING_C]
    + [("d96", t, DYNAMIC_ROWS, [None, None]) for t in TILING_C + TILING_D]
    + [("g768", "default", (17,), [None, None])]
    + [("s256", "default", STATIC_ROWS, [(5, 4), (4, 4)])]
    + [("s1024", "default", STATIC_ROWS, [(20, 16), (16, 16)]), ("s1024", "eight_waves", STATIC_ROWS, [(10, 8), (8, 8)]),
       ("s1024", "wavefront", STATIC_ROWS, [(20, 16), (16, 16)])]
    + [("s1536_lstm", "eight_waves", STATIC_ROWS, [(10, 12), (12, 12)]), ("s1536_lstm", "tiling_d", STATIC_ROWS, [(10, 12), (12, 12)]),
       ("s1536_lstm", "tiling_d_four_waves", STATIC_ROWS, [None, None])]       # (24 chunks per wave: no entry)
)
ENC_FRAMES = (1, 2)
ENC_GROUP2 = ("d96", 128, 80, ("default", "tiling_d"))      # max_streams 128, 80 rows: a second m-group behind both grids

# predictor: the tiling follows Md = M x beam (launch_predictor_t): < 512 four units per workgroup on 8 waves, >= 512 the 16-unit
# tiling on 4 waves; wide8 (256 <= Md < 512) is bf16 only
PRED_TILINGS = {"units4": (dict(max_streams=64), 64, 8, (5, 17, 33, 64)), "wide16": (dict(max_streams=64, beam=8), 512, 4, (64,))}
PRED_MODELS = ["tiny", "tiny_lstm", "d96", "d96_lstm", "s1024", "s1024_lstm"]
PRED_TOKENS = (1, 2)

# joint: (model, max_streams, rows, waves of the logits launch at each row count, tiling).  pp and pe: launch_linear_ops<true, 3> on
# 8 waves.  logits (launch_logits_ops, logits_mt = 2): 32 x 16 below 512 rows and 64 x 16 from 512, both on 8 waves; 64 x 64 on 4
# waves from 512 rows where vocab % 64 == 0
JOINT_ENGINES = [
    ("tiny", 64, (5, 16, 17, 64), 8, "32 rows x 16 columns"),
    ("d96", 64, (5, 16, 17, 64), 8, "32 rows x 16 columns"),
    ("s1024", 64, (5, 16, 17, 64), 8, "32 rows x 16 columns"),
    ("d96", 512, (512,), 4, "64 x 64 (rows >= 512, vocab % 64 == 0)"),
    ("s1024", 512, (512,), 4, "64 x 64 (rows >= 512, vocab % 64 == 0)"),
    ("d96_v80", 512, (17, 512), 8, "32 x 16 below 512 rows, 64 x 16 from 512 (vocab 80)"),
]


def gpu_schedules():
    """[(what, launcher, model, waves, entries)] of every GEMM launch kind the GPU cases run"""
    out = [(f"encoder {n} {t}", "enc_cell", n, ENC_TILINGS[t][2], want) for n, t, _, want in ENC_PARAMS]
    out += [(f"encoder {ENC_GROUP2[0]} {t} second row group", "enc_cell", ENC_GROUP2[0], ENC_TILINGS[t][2], [None, None]) for t in ENC_GROUP2[3]]
    for t, (_, _, nw, _) in PRED_TILINGS.items():
        out += [(f"predictor {n} {t}", "pred_cell", n, nw, schedule("pred_cell", n, nw)) for n in PRED_MODELS]
    for n, M, _, nw, _ in JOINT_ENGINES:
        out += [(f"joint {n} M {M} pp / pe", "joint_half", n, 8, schedule("joint_half", n, 8)),
                (f"joint {n} M {M} logits", "logits", n, nw, schedule("logits", n, nw))]
    return out
