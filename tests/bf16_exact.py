"""The dtype=bf16 contract in float64, with a per-element bound on what a correct engine may differ by (helper, not a test).

bf16 operands are exact in float64 and so are their products: a float64 evaluation on the operands the engine rounds (the contract of
OracleTransducer.__init__: GEMM weights, LayerNorm output, h, BN(h), the joint activation; cell state, biases, the predictor's
layer-0 table, pe / pp and logits stay f32) is the value, and every stage returns (value, tol, flip):

  tol   one number per stage: 8 x Y, floored at 4 f32 ulps of the stage's largest magnitude.  The yardstick Y is the largest
        |float32 evaluation - float64 evaluation| of the stage, the float32 evaluation being the numpy oracle's own arithmetic
        (operand="bf16"; StandIn below restates its loops so that every stage is visible, and test_bf16_exact_cpu pins the
        restatement to OracleTransducer bit for bit).  Y comes from the CPU alone, never from the engine.  It is taken over the
        elements whose flip allowance is zero: the float32 evaluation rounds too, and where it may round the other way its
        distance is a flip, not accumulation noise (all the operations here act row by row, so the other rows are untouched).
        Behind the encoder's first GEMM no element is free of one: there Y comes from the oracle's cell evaluated on the model's
        own bf16 operands ("forced"), over every element.
  flip  per element, the room for discrete rounding flips.  A value that is rounded to bf16 and fed onward may round the other
        way in the engine when its unrounded value lies within d = tol + flip_in of a rounding midpoint; the engine's rounded value
        then lies between bf16(x - d) and bf16(x + d), so the allowance is max |bf16(x +- d) - bf16(x)|: zero for an element that
        is not tie-sensitive, one bf16 ulp of the element for one that is (more only where flip_in itself exceeds an ulp).  A rounded
        stage has tol = 0: away from a tie the engine's bf16 value IS the reference's.  Onward the allowance propagates as a
        first-order bound: |W| . flip through a GEMM, 1/4 through sigmoid, 1 through tanh, the product rule through the cell
        update, |scale| through BatchNorm.  Only the flip part is propagated through depth; the continuous part of a deep stage
        comes from its own yardstick, which contains the propagation of the float32 evaluation's noise.

An engine value passes when |engine - value| <= tol + flip, element by element.

Caps (check_caps): at most 2 % of the elements of any rounded tensor may be tie-sensitive and at most 10 % of the elements of any
stage may carry a nonzero flip; a budget that covers many elements hides failures.  The cases below were picked on the CPU so that
the reference alone meets both."""
import copy
import itertools

import numpy as np

from oracle import rnnt_oracle as O

F32, F64 = np.float32, np.float64
MARGIN, FLOOR_ULPS = 8.0, 4.0
TIE_CAP, FLIP_CAP = 0.02, 0.10


def r64(x):
    """float64 -> nearest-even bf16 (through f32, as the engine's values are) -> float64"""
    return O.bf16_round(np.asarray(x, F64).astype(F32)).astype(F64)


def bf16_trunc(x):
    """f32 -> bf16 by dropping the low 16 bits (the wrong conversion of mutation (a))"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(F32)


def bf16_ulp(x):
    """distance from |x| to the next bf16 number above it (x bf16-representable)"""
    return np.spacing(np.abs(np.asarray(x, F32))).astype(F64) * 65536.0


def sig(x):
    return 1.0 / (1.0 + np.exp(-x))


class Stage:
    """value float64; tol float; flip float64 array; Y the yardstick; ref32 the float32 evaluation; tie = tie-sensitive mask (rounded stages)"""

    def __init__(self, name, value, tol, flip, Y, ref32, tie=None):
        self.name, self.value, self.tol, self.flip, self.Y, self.ref32, self.tie = name, value, float(tol), flip, float(Y), ref32, tie

    def bound(self):
        return self.tol + self.flip

    def ratio(self, got, sl=Ellipsis):
        """largest |got - value| / (tol + flip) over the elements of `sl`; inf where a difference meets a zero bound"""
        d = np.abs(np.asarray(got, F64) - self.value[sl])
        b = self.bound()[sl]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, d / b, np.where(d > 0, np.inf, 0.0))
        return float(r.max()) if r.size else 0.0

    def sub(self, sl):
        return Stage(self.name, self.value[sl], self.tol, self.flip[sl], self.Y, self.ref32[sl], None if self.tie is None else self.tie[sl])


def _tol(x32, x64, e, forced=False):
    """forced: x32 was evaluated on the float64 model's own (bf16-exact) operands, so it never rounded another way than the model
    and every element counts"""
    free, d = (e >= 0) if forced else (e == 0), np.abs(x32.astype(F64) - x64)
    # (no element without an allowance -- never so in a case inside the caps: what the allowance does not explain)
    Y = float(d[free].max()) if free.any() else float(np.maximum(d - e, 0.0).max())
    floor = FLOOR_ULPS * float(np.spacing(F32(np.abs(x64).max())))
    return max(MARGIN * Y, floor), Y


class Trace(dict):
    """name -> Stage, in evaluation order; .rounded = the names of the activations that were rounded"""

    def __init__(self):
        super().__init__()
        self.rounded = []
        self.capped = None                  # names of the stages the caps are asserted for (None: all)

    def cont(self, name, x64, e, ref32, forced=None):
        """a continuous (f32 in the engine) stage; forced: the stage's float32 evaluation on the model's own operands (the yardstick
        is then taken from it, over every element: behind the encoder's first GEMM no element is free of an inherited flip)"""
        tol, Y = _tol(ref32[name], x64, e) if forced is None else _tol(forced, x64, e, True)
        self[name] = Stage(name, x64, tol, e, Y, ref32[name])
        return tol

    def rnd(self, name, x64, e, ref32, forced=None):
        """x64 (+- e inherited) is rounded to bf16 and fed onward -> (rounded value, its flip allowance)"""
        tol = self.cont(name + ".pre", x64, e, ref32, forced)
        d = tol + e
        q = r64(x64)
        fl = np.maximum(np.abs(r64(x64 + d) - q), np.abs(r64(x64 - d) - q))
        self[name] = Stage(name, q, 0.0, fl, 0.0, ref32[name], fl > 0)
        self.rounded.append(name)
        return q, fl


def check_caps(trace):
    """the two caps of the module docstring; -> (largest tie fraction, largest flip fraction)"""
    stages = [s for k, s in trace.items() if trace.capped is None or k in trace.capped]
    tie = max([float(s.tie.mean()) for s in stages if s.tie is not None] + [0.0])
    flip = max(float((s.flip > 0).mean()) for s in stages)
    for s in stages:
        if s.tie is not None:
            assert s.tie.mean() <= TIE_CAP, f"{s.name}: {s.tie.mean():.4f} of the elements are tie-sensitive (cap {TIE_CAP})"
        assert (s.flip > 0).mean() <= FLIP_CAP, f"{s.name}: {(s.flip > 0).mean():.4f} of the elements carry a flip (cap {FLIP_CAP})"
    return tie, flip


# ----------------------------------------------------------------------------- float32: the oracle's loops, every stage visible
class StandIn:
    """OracleTransducer.encoder / .predictor / .joint_logp restated on the oracle's own functions and weights so that every stage
    can be read -- the float32 evaluation of the yardstick, and with a mutation switched on the subtly wrong kernel of the
    sensitivity tests: q = the activation rounding, raw_h_t = time step that is fed an unrounded h, raw_act = the vocabulary GEMM is
    fed the unrounded joint activation, stale_c_t = time step whose LSTM cells read the learned initial cell state instead of the
    previous step's (weight mutations are made on a copy of the oracle: mutated())."""

    def __init__(self, o, q=None, raw_h_t=None, raw_act=False, stale_c_t=None):
        self.o, self.q, self.raw_h_t, self.raw_act, self.stale_c_t = o, (q or o.q), raw_h_t, raw_act, stale_c_t

    def encoder(self, x):
        o, q, s = self.o, self.q, {}
        B, T, _ = x.shape
        s["x0.pre"] = O.layer_norm(x.reshape(B, T, -1), o.ln_w, o.ln_b)
        x = s["x0"] = q(s["x0.pre"])
        for l, L in enumerate(o.enc):
            h, c = q(np.repeat(L["hs"][0, 0], B, 0).copy()), np.repeat(L["hs"][1, 0], B, 0).copy()
            ys, c_init = np.empty((B, T, o.H), F32), c
            for t in range(T):
                h, c = O.lstm_step(x[:, t], h, c_init if self.stale_c_t == t else c, L["rnn"])
                ys[:, t] = h
                s[f"enc{l}.t{t}.c"], s[f"enc{l}.t{t}.h.pre"] = c, h
                h = s[f"enc{l}.t{t}.h"] = q(h)
                if self.raw_h_t == t + 1:
                    h = s[f"enc{l}.t{t}.h.pre"]
            s[f"enc{l}.y.pre"] = O.bn_eval(ys, L["bn"])
            x = s[f"enc{l}.y"] = q(s[f"enc{l}.y.pre"])
        return s

    def predictor(self, toks):
        """toks [B, U], from the learned initial state (Engine.predictor)"""
        o, q, s = self.o, self.q, {}
        B, U = toks.shape
        st = [(q(np.repeat(L["hs"][0, 0], B, 0).copy()), np.repeat(L["hs"][1, 0], B, 0).copy() if o.pred_lstm else None) for L in o.pred]
        c_init = [c for _, c in st]
        for u in range(U):
            x = o.embed[toks[:, u]]
            if o.ffn_w is not None:
                x = (x @ o.ffn_w.T + o.ffn_b).astype(F32)
            for l, L in enumerate(o.pred):
                h0, c0 = st[l]
                if o.pred_lstm:
                    h, c = O.lstm_step(x, h0, c_init[l] if self.stale_c_t == u else c0, L["rnn"])
                    s[f"pred{l}.u{u}.c"] = c
                else:
                    h, c = O.nbrc_step(x, h0, L["rnn"]), None
                s[f"pred{l}.u{u}.h.pre"] = h
                s[f"pred{l}.u{u}.h"] = q(h)
                st[l] = (h if self.raw_h_t == u + 1 else s[f"pred{l}.u{u}.h"], c)
                s[f"pred{l}.u{u}.y.pre"] = O.bn_eval(h, L["bn"])
                x = s[f"pred{l}.u{u}.y"] = q(s[f"pred{l}.u{u}.y.pre"])
        return s

    def joint(self, a, b):
        o, q, s = self.o, self.q, {}
        H = o.H
        a, b = q(a), q(b)
        s["pp"] = (a @ o.j0_w[:, :H].T + o.j0_b).astype(F32)
        s["pe"] = (b @ o.j0_w[:, H:].T).astype(F32)
        # (the oracle's own order: one GEMM over the concatenation)
        s["act.pre"] = np.tanh(np.concatenate([a, b], axis=-1) @ o.j0_w.T + o.j0_b).astype(F32)
        s["act"] = q(s["act.pre"])
        z = s["logits"] = ((s["act.pre"] if self.raw_act else s["act"]) @ o.j2_w.T + o.j2_b).astype(F32)
        m = z.max(-1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(-1, keepdims=True, dtype=F32))
        s["lp"] = (z - lse).astype(F32).max(-1)
        return s


def mutated(o, kind):
    """a copy of the bf16 oracle `o` with one of the weight mutations: "k_tail" the last K element of every recurrent GEMM (encoder
    and predictor) dropped; "w_ulp" one row (the K elements of output column 5) of the recurrent weights of encoder layer 0 and of predictor
    layer 0 and of both joint weights off by one bf16 ulp; "bias_twice" the joint bias added twice in pp"""
    m = copy.copy(o)
    m.enc = [dict(L, rnn=dict(L["rnn"])) for L in o.enc]
    m.pred = [dict(L, rnn=dict(L["rnn"])) for L in o.pred]
    rk = "weight_hh_l0" if o.pred_lstm else "recurrent_kernel"
    if kind == "k_tail":
        for L in m.enc:
            L["rnn"]["weight_hh_l0"] = L["rnn"]["weight_hh_l0"].copy()
            L["rnn"]["weight_hh_l0"][:, -1] = 0                      # torch layout [4H, K]
        for L in m.pred:
            L["rnn"][rk] = L["rnn"][rk].copy()
            if o.pred_lstm:
                L["rnn"][rk][:, -1] = 0
            else:
                L["rnn"][rk][-1, :] = 0                              # haste layout [K, 3H]
    elif kind == "w_ulp":
        for attr in ("j0_w", "j2_w"):                                # output column 5 of both joint GEMMs
            w = getattr(o, attr).copy()
            w[5] = (w[5].astype(F64) + bf16_ulp(w[5])).astype(F32)
            setattr(m, attr, w)
        for L, k in ((m.enc[0], "weight_hh_l0"), (m.pred[0], rk)):
            w = L["rnn"][k].copy()
            row = w[5] if k == "weight_hh_l0" else w[:, 5]           # the K elements of output column 5
            row[...] = (row.astype(F64) + bf16_ulp(row)).astype(F32)
            assert np.array_equal(O.bf16_round(w), w)
            L["rnn"][k] = w
    elif kind == "bias_twice":
        m.j0_b = (o.j0_b * F32(2)).astype(F32)
    else:
        raise KeyError(kind)
    return m


# ----------------------------------------------------------------------------- float64 with the flip allowance
def _prod(u, eu, v, ev):
    """bound on |u' v' - u v| for |u' - u| <= eu, |v' - v| <= ev"""
    return np.abs(u) * ev + np.abs(v) * eu + eu * ev


class Exact:
    def __init__(self, sd, cfg):
        self.cfg = cfg
        self.o = O.OracleTransducer(sd, cfg, operand="bf16")
        self.ref = StandIn(self.o)
        self.H, self.lstm = cfg["hidden"], cfg["pred_cell"] == "LSTM"
        d = lambda k: np.asarray(sd[k], F64)                                   # kept as it is
        r = lambda k: r64(np.asarray(sd[k], F32))                              # a bf16 GEMM operand
        self.ln_w, self.ln_b = d("encoder.input_norm.weight"), d("encoder.input_norm.bias")
        self.rounded_weights = []

        def stack(prefix, n, lstm, table0):
            out = []
            for i in range(n):
                bn = {k: d(f"{prefix}.rnn_stack.bns.{i}.{k}") for k in ("weight", "bias", "running_mean", "running_var")}
                keys = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0") if lstm else ("kernel", "recurrent_kernel", "bias", "recurrent_bias")
                rnn = {}
                for j, k in enumerate(keys):
                    full = f"{prefix}.rnn_stack.rnns.{i}.{k}"
                    rounded = j == 1 or (j == 0 and not (table0 and i == 0))
                    rnn[k] = r(full) if rounded else d(full)
                    if rounded:
                        self.rounded_weights.append(full)
                L = dict(rnn=rnn, hs=d(f"{prefix}.rnn_stack.hs.{i}"), bn_s=bn["weight"] / np.sqrt(bn["running_var"] + 1e-5))
                L["bn_t"] = bn["bias"] - bn["running_mean"] * L["bn_s"]
                out.append(L)
            return out

        self.enc = stack("encoder", cfg["enc_layers"], True, False)
        self.pred = stack("predictor", cfg["pred_layers"], self.lstm, True)
        self.embed = d("predictor.embed.weight")
        self.ffn = (d("predictor.ffn.weight"), d("predictor.ffn.bias")) if "predictor.ffn.weight" in sd else None
        self.j0_w, self.j0_b = r("joint.joint.0.weight"), d("joint.joint.0.bias")
        self.j2_w, self.j2_b = r("joint.joint.2.weight"), d("joint.joint.2.bias")
        self.rounded_weights += ["joint.joint.0.weight", "joint.joint.2.weight"]

    # -- cells: (value, allowance) pairs
    @staticmethod
    def _lstm(x, ex, h, eh, c, ec, p):
        H = h.shape[-1]
        g = x @ p["weight_ih_l0"].T + p["bias_ih_l0"] + h @ p["weight_hh_l0"].T + p["bias_hh_l0"]
        eg = ex @ np.abs(p["weight_ih_l0"]).T + eh @ np.abs(p["weight_hh_l0"]).T
        i, f, gg, o = sig(g[:, :H]), sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), sig(g[:, 3 * H:])
        ei, ef, egg, eo = eg[:, :H] / 4, eg[:, H:2 * H] / 4, eg[:, 2 * H:3 * H], eg[:, 3 * H:] / 4
        c2 = f * c + i * gg
        ec2 = _prod(f, ef, c, ec) + _prod(i, ei, gg, egg)
        h2 = o * np.tanh(c2)
        return h2, _prod(o, eo, np.tanh(c2), ec2), c2, ec2

    @staticmethod
    def _nbrc(x, ex, h, eh, p):
        H = h.shape[-1]
        Wx, eWx = x @ p["kernel"] + p["bias"], ex @ np.abs(p["kernel"])
        Rh, eRh = h @ p["recurrent_kernel"] + p["recurrent_bias"], eh @ np.abs(p["recurrent_kernel"])
        z, ez = sig(Wx[:, :H] + Rh[:, :H]), (eWx[:, :H] + eRh[:, :H]) / 4
        r, er = sig(Wx[:, H:2 * H] + Rh[:, H:2 * H]), (eWx[:, H:2 * H] + eRh[:, H:2 * H]) / 4
        g = np.tanh(Wx[:, 2 * H:] + r * Rh[:, 2 * H:])
        eg = eWx[:, 2 * H:] + _prod(r, er, Rh[:, 2 * H:], eRh[:, 2 * H:])
        return z * h + (1.0 - z) * g, _prod(z, ez, h, eh) + _prod(1.0 - z, ez, g, eg)

    # -- stages
    def encoder(self, x):
        """x [B, T, F] float32 -> Trace: x0, enc{l}.t{t}.c / .h (rounded), enc{l}.y (BN, rounded, [B, T, H])"""
        ref, tr = self.ref.encoder(x), Trace()
        B, T, _ = x.shape
        x, ex = tr.rnd("x0", _ln64(self, x)[0], np.zeros(x.shape), ref)
        for l, L in enumerate(self.enc):
            h, eh = r64(np.repeat(L["hs"][0, 0], B, 0)), np.zeros((B, self.H))       # (rounded once at load: no allowance)
            c, ec = np.repeat(L["hs"][1, 0], B, 0), np.zeros((B, self.H))
            ys, eys = np.empty((B, T, self.H)), np.empty((B, T, self.H))
            ys32 = np.empty((B, T, self.H), F32)
            for t in range(T):
                # the oracle's cell on the model's own operands (bf16 values and the f32 image of c): the float32 evaluation of
                # this stage on the same operands, whatever was rounded the other way upstream
                h32, c32 = O.lstm_step(x[:, t].astype(F32), h.astype(F32), c.astype(F32), self.o.enc[l]["rnn"])
                hp, ehp, c, ec = self._lstm(x[:, t], ex[:, t], h, eh, c, ec, L["rnn"])
                tr.cont(f"enc{l}.t{t}.c", c, ec, ref, c32)
                ys[:, t], eys[:, t], ys32[:, t] = hp, ehp, h32
                h, eh = tr.rnd(f"enc{l}.t{t}.h", hp, ehp, ref, h32)
            x, ex = tr.rnd(f"enc{l}.y", ys * L["bn_s"] + L["bn_t"], eys * np.abs(L["bn_s"]), ref, O.bn_eval(ys32, self.o.enc[l]["bn"]))
        return tr

    def predictor(self, toks):
        """toks [B, U] -> Trace: pred{l}.u{u}.h (rounded), .y (BN, rounded), .c (LSTM)"""
        toks = np.asarray(toks)
        ref, tr = self.ref.predictor(toks), Trace()
        B, U = toks.shape
        z = np.zeros((B, self.H))
        st = [(r64(np.repeat(L["hs"][0, 0], B, 0)), z, np.repeat(L["hs"][1, 0], B, 0) if self.lstm else None, z) for L in self.pred]
        for u in range(U):
            x, ex = self.embed[toks[:, u]], z
            if self.ffn is not None:
                x = x @ self.ffn[0].T + self.ffn[1]
            for l, L in enumerate(self.pred):
                h0, eh0, c0, ec0 = st[l]
                if self.lstm:
                    hp, ehp, c, ec = self._lstm(x, ex, h0, eh0, c0, ec0, L["rnn"])
                    tr.cont(f"pred{l}.u{u}.c", c, ec, ref)
                else:
                    (hp, ehp), c, ec = self._nbrc(x, ex, h0, eh0, L["rnn"]), None, z
                h, eh = tr.rnd(f"pred{l}.u{u}.h", hp, ehp, ref)
                st[l] = (h, eh, c, ec)
                x, ex = tr.rnd(f"pred{l}.u{u}.y", hp * L["bn_s"] + L["bn_t"], ehp * np.abs(L["bn_s"]), ref)
        return tr

    def joint(self, a, b, ea=None, eb=None):
        """a = h_pred, b = h_enc [B, H] float32 (rounded once, deterministically: no allowance unless ea / eb hand one in)
        -> Trace: pp, pe, act (rounded), logits, lp (the largest log-softmax of the row)"""
        ref, tr = self.ref.joint(a, b), Trace()
        H = self.H
        a, b = r64(a), r64(b)
        # (inputs that carry an allowance: ref was evaluated on the very values given here, so it is the forced evaluation)
        fo = (lambda k: None) if ea is None and eb is None else (lambda k: ref[k])
        ea = np.zeros(a.shape) if ea is None else ea
        eb = np.zeros(b.shape) if eb is None else eb
        pp, epp = a @ self.j0_w[:, :H].T + self.j0_b, ea @ np.abs(self.j0_w[:, :H]).T
        pe, epe = b @ self.j0_w[:, H:].T, eb @ np.abs(self.j0_w[:, H:]).T
        tr.cont("pp", pp, epp, ref, fo("pp"))
        tr.cont("pe", pe, epe, ref, fo("pe"))
        act, eact = tr.rnd("act", np.tanh(pp + pe), epp + epe, ref, fo("act.pre"))
        z, ez = act @ self.j2_w.T + self.j2_b, eact @ np.abs(self.j2_w).T
        tol_z = tr.cont("logits", z, ez, ref, None if fo("pp") is None else (act.astype(F32) @ self.o.j2_w.T + self.o.j2_b).astype(F32))
        tr.tol_reduction = None
        # lp: within the logits' bound (a row's largest) plus the reduction's own yardstick -- the float32 log-softmax of the
        # float32 logits against the float64 one of the same logits
        lp = lambda v: (v - v.max(-1, keepdims=True) - np.log(np.exp(v - v.max(-1, keepdims=True)).sum(-1, keepdims=True))).max(-1)
        z32 = ref["logits"].astype(F64)
        Y = float(np.abs(ref["lp"].astype(F64) - lp(z32)).max())
        tol = max(MARGIN * Y, FLOOR_ULPS * float(np.spacing(F32(np.abs(lp(z)).max() + np.abs(z).max()))))
        tr["lp"] = Stage("lp", lp(z), tol_z + tol, ez.max(-1), Y, ref["lp"])
        tr.tol_reduction = tol
        return tr

    def first_cell(self, feat0, labels, bos=2):
        """The lattice's first frame and first label row: log p(blank) and log p(label) of the joint on the encoder's output for
        the frame feat0 [feat] and the predictor's output after BOS from the learned initial state -> (values [1 + len(labels)]
        blank first, bounds).  The allowances of both paths go into the joint; a log-softmax term z_k - lse(z) moves by at most the
        bound of z_k plus the row's largest (lse is 1-Lipschitz in the largest norm) plus the reduction's own tol.  Every row behind
        the encoder's K = 1280 GEMM carries a flip, so this bound is outside the caps: it is what the flips allow, not a sharp one."""
        Le, Lp = self.cfg["enc_layers"], self.cfg["pred_layers"]
        ye = self.encoder(np.asarray(feat0, F32)[None, None])[f"enc{Le - 1}.y"]
        yp = self.predictor(np.array([[bos]], np.int32))[f"pred{Lp - 1}.u0.y"]
        tr = self.joint(yp.value.astype(F32), ye.value[:, 0].astype(F32), ea=yp.flip, eb=ye.flip[:, 0])
        z, bz = tr["logits"].value[0], tr["logits"].bound()[0]
        k = np.array([0] + [int(v) for v in labels])                  # (blank = 0)
        lse = z.max() + np.log(np.exp(z - z.max()).sum())
        return z[k] - lse, bz[k] + bz.max() + tr.tol_reduction


# ----------------------------------------------------------------------------- the cases both test files use
def derived_cfg(vocab=64, pred_cell="NBRC"):
    """tiny with hidden = joint = 96: the smallest width bf16 accepts (multiples of 32, valid_desc) that is neither a power of two
    nor a multiple of 64 -- three 32-wide K chunks, so a K split over 4 or 8 waves has a tail"""
    from libreasr_amd import synth
    cfg = synth.model_cfg("tiny")
    cfg.update(hidden=96, joint=96, vocab=vocab, pred_cell=pred_cell)
    return cfg


# weight seeds where 0 will not do: of seeds 0..11 one that leaves the predictor the most token sequences inside the caps
MODEL_SEED = {"tiny_lstm": 6, "d96": 10, "d96_v80": 10, "d96_lstm": 11}


def model_cfg(name):
    from libreasr_amd import synth
    if name == "d96":
        return derived_cfg()
    if name == "d96_v80":
        return derived_cfg(vocab=80)
    if name == "d96_lstm":
        return derived_cfg(pred_cell="LSTM")
    if name == "g768":                      # 64 mels x 12 stacked frames: the runtime-shaped k_stack_ln, 24 K chunks into layer 0
        return dict(synth.model_cfg("tiny"), feat=768)
    return synth.model_cfg(name)


_MODELS = {}


def model(name):
    from libreasr_amd import synth
    if name not in _MODELS:
        cfg = model_cfg(name)
        sd = synth.synth_state_dict(cfg, seed=MODEL_SEED.get(name, 0))
        _MODELS[name] = (Exact(sd, cfg), sd, cfg)
    return _MODELS[name]


def _ln64(m, x):
    x = np.asarray(x, F64)
    mu = x.mean(-1, keepdims=True)
    sd = np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + 1e-5)
    return (x - mu) / sd * m.ln_w + m.ln_b, sd


def settle_x0(m, x, rounds=48, leave=0):
    """Features next to x whose LayerNorm output is free of tie-sensitive elements.  With 1280 features a row always has some
    (about 1 %: near zero the bf16 grid is finer than any tolerance), and a tie in x0 reaches every output of the encoder.  Each
    such feature is moved so that its LayerNorm output lands on a bf16 number of magnitude >= 2^-6, to the side that keeps the sum of
    the moves small; the moves shift the row's statistics a little, so it takes a few rounds.  The reference alone decides."""
    x = np.array(x, F32)
    for _ in range(rounds):
        pre, sd = _ln64(m, x)
        tol, _ = _tol(O.layer_norm(x, m.o.ln_w, m.o.ln_b), pre, np.zeros(pre.shape))
        q = r64(pre)
        tie = (r64(pre + tol) != q) | (r64(pre - tol) != q)
        if leave:
            tie[len(x) - leave:] = False          # the last `leave` rows stay as drawn (they count in tol all the same)
        if not tie.any():
            break
        lo = np.where(np.abs(q) >= 2.0 ** -6, q, np.where(pre >= 0, 1.0, -1.0) * 2.0 ** -6)
        other = lo + np.sign(pre - lo + 1e-300) * bf16_ulp(lo)                 # the bf16 number on the far side of the midpoint
        other = np.where(np.abs(other) >= 2.0 ** -6, other, lo)
        for idx in zip(*np.nonzero(tie.any(-1))):                              # per (row, frame): alternate the sides by the running sum
            run = 0.0
            for j in np.nonzero(tie[idx])[0]:
                d = np.array([lo[idx][j], other[idx][j]]) - pre[idx][j]
                d = d * sd[idx][0] / m.ln_w[j]
                k = int(np.argmin(np.abs(run + d)))
                run += d[k]
                x[idx][j] = F32(x[idx][j] + d[k])
    return x


POOL = 24        # candidate rows per row wanted


def _no_inherited_flip(tr):
    """per row: no continuous stage carries a flip, that is, nothing that is fed onward is tie-sensitive"""
    ok = None
    for s in tr.values():
        if s.tie is None:
            r = s.flip.reshape(s.flip.shape[0], -1).max(1) == 0
            ok = r if ok is None else ok & r
    return ok


def _rows(run, order, B, dirty=()):
    """The batch of a case: B - len(dirty) rows from the pool rows `order` (repeated down the batch where they are fewer) plus the
    rows `dirty`, taken as they come so that the flip rule is exercised.  run(idx) -> Trace of the batch of pool rows idx.  The
    float32 evaluation's noise, and with it every tol, depends on the batch (BLAS blocks by shape), so a row that was clean in the
    pool is looked at again in its batch and replaced if it no longer is.  -> (idx, Trace); check_caps holds."""
    order, n = list(order), B - len(dirty)
    for _ in range(64):
        K = min(len(order), n)
        assert K >= min(4, n), f"{K} usable rows left"
        idx = [order[i % K] for i in range(n)] + list(dirty)
        tr = run(idx)
        ok = _no_inherited_flip(tr)
        bad = {idx[i] for i in range(n) if not ok[i]}
        if not bad:
            try:
                check_caps(tr)
                return idx, tr
            except AssertionError:         # over a cap: without the row that has the most tie-sensitive elements
                ties = sum(s.tie.reshape(B, -1).sum(1) for s in tr.values() if s.tie is not None)
                bad = {idx[int(np.argmax(ties[:n]))]}
        order = [i for i in order if i not in bad]
    raise AssertionError("no batch inside the caps")


def _pick_within_caps(tr):
    """the rows of the pool in which nothing tie-sensitive is fed onward, fewest tie-sensitive elements first, as long as every
    rounded tensor of the rows taken so far stays inside the 2 % cap"""
    up = _no_inherited_flip(tr)
    n = len(up)
    ties = np.stack([s.tie.reshape(n, -1).sum(1) for s in tr.values() if s.tie is not None], 1)
    width = np.array([s.tie.reshape(n, -1).shape[1] for s in tr.values() if s.tie is not None])
    chosen, tot = [], np.zeros(len(width))
    for i in np.argsort(ties.max(1), kind="stable"):
        if up[i] and np.all(tot + ties[i] <= TIE_CAP * width * (len(chosen) + 1)):
            chosen.append(int(i))
            tot += ties[i]
    return chosen


# the stages of an encoder case for which the caps hold and are asserted; everything behind the rounding of layer 0's h is held to
# tol + flip all the same, outside the caps (docs/bf16_bound.md)
ENC_STAGES = ("x0.pre", "x0", "enc0.t0.c", "enc0.t0.h.pre")      # (+ "enc0.y.pre" with one frame)
ENC_H_TIE_CAP = 0.25        # layer-0 h and BN(h) behind the K = feat GEMM: nothing inherited (tol = 0 off a tie), but 13 .. 16 % tie-sensitive
_CASES = {}


def case(kind, name, B, n=1, seed=0):
    """-> (inputs, Trace) of one case, computed once and left unchanged.  kind "enc": n = T', inputs [B, T', feat] (the caps are
    asserted for ENC_STAGES); "pred": n = U, inputs tokens [B, U]; "joint": inputs (h_pred, h_enc) [B, hidden].  The rows are picked
    from a seeded pool by the reference alone (_rows; the encoder's are settled, settle_x0, all but B // 16 of them);
    check_caps(trace) holds for every case the test files list."""
    key = (kind, name, B, n, seed)
    if key in _CASES:
        return _CASES[key]
    m, _, cfg = model(name)
    rng = np.random.default_rng([seed, B, n, {"enc": 1, "pred": 2, "joint": 3}[kind]])
    P = POOL * B + 256
    if kind == "enc":
        x = (rng.standard_normal((B, n, cfg["feat"])) * rng.uniform(0.5, 2.0, (B, 1, 1)) + rng.uniform(-1, 1, (B, 1, 1))).astype(F32)
        nd = B // 16
        x = settle_x0(m, x, leave=nd)
        tr = m.encoder(x)
        tr.capped = ENC_STAGES + (("enc0.y.pre",) if n == 1 else ())
        out = (x, tr)
    elif kind == "pred":
        # the tokens are the only input: every sequence is tried (vocab^U of them, a seeded sample beyond 4096) and the usable ones
        # repeat down the rows -- a row's place in the tiling differs even where its tokens do not
        V = cfg["vocab"]
        if (V - 1) ** n <= 4096:
            toks = np.array(list(itertools.product(range(1, V), repeat=n)), np.int32)
        else:
            toks = rng.integers(1, V, (4096, n)).astype(np.int32)
        idx, tr = _rows(lambda i: m.predictor(toks[i]), _pick_within_caps(m.predictor(toks)), B)
        out = (toks[idx], tr)
    else:
        # rows in which no element of the activation is tie-sensitive, plus B // 16 rows as they come (6 % of the logits carry a flip)
        a, b = rng.standard_normal((P, cfg["hidden"])).astype(F32), rng.standard_normal((P, cfg["hidden"])).astype(F32)
        ok = _no_inherited_flip(m.joint(a, b))
        idx, tr = _rows(lambda i: m.joint(a[i], b[i]), np.nonzero(ok)[0], B, dirty=list(np.nonzero(~ok)[0][:B // 16]))
        out = ((a[idx], b[idx]), tr)
    _CASES[key] = out
    return out


# the cases of tests/test_gpu_bf16_exact.py; tests/test_bf16_exact_cpu.py asserts the caps for each of them
ENC_CASES = [(name, B, T) for name in ("tiny", "d96") for B in (1, 16, 17, 64) for T in (1, 2)] + [("g768", 17, 1)]
FRONTEND = {"g768": dict(n_mels=64, n_stack=12)}        # Engine keywords of a model whose feat is not 128 x 10
PRED_CASES = [(name, U) for name in ("tiny", "tiny_lstm", "d96", "d96_lstm") for U in (1, 2)]
PRED_ROWS = 64      # a whole 64-row group: every m-tile of a wide workgroup
JOINT_CASES = [("tiny", B) for B in (5, 16, 17, 64)] + [("d96", B) for B in (5, 16, 17, 64, 512)] + [("d96_v80", 17), ("d96_v80", 512)]


def check_first_cell(name, feat0, blank, emits, what):
    """The lattice tests' bf16 contexts: the engine's log p(blank) and log p(label) (emits: {label: value}) on the first frame and
    the first label row against Exact.first_cell, asserted within its bound; figures printed."""
    labels = sorted(emits)
    val, bound = model(name)[0].first_cell(feat0, labels)
    got = np.array([blank] + [emits[k] for k in labels], F64)
    d = np.abs(got - val)
    print(f"{what}: first cell |d| {d.max():.3g} of a bound of {bound[int(np.argmax(d / bound))]:.3g} (ratio {float((d / bound).max()):.3g})")
    assert np.all(d <= bound), (what, d, bound)
