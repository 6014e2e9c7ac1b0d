"""Float64 restatement of lasr_lm_score's definition (include/lasr.h) in numpy: LM.forward on a whole sequence
(lm.py:31-40: Embedding -> LSTM stack from zero state -> Linear -> log_softmax at every position) and the gather of the labels.

    start >= 0:   the LM reads (start, y_1, .., y_{U-1});  lp[u-1] = log_softmax(LM(x_1..x_u))[y_u],  u = 1..U
    start = None: the LM reads y_1..y_{U-1};  lp[0] = 0;   lp[u-1] = log_softmax(LM(y_1..y_{u-1}))[y_u],  u = 2..U
    total = sum(lp)
"""
import numpy as np

F64 = np.float64


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


class LmRef:
    """sd: an lm.py LM state_dict (synth.synth_lm_state_dict).  torch.nn.LSTM gate order i, f, g, o; the output layer is tied to the
    embedding when embed == hidden (lm.py:27-29)."""

    def __init__(self, sd):
        self.embed = np.asarray(sd["embed.weight"], F64)
        self.layers = []
        l = 0
        while f"rnn.weight_ih_l{l}" in sd:
            self.layers.append(tuple(np.asarray(sd[f"rnn.{k}_l{l}"], F64) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
            l += 1
        self.H = self.layers[0][1].shape[1]
        tied = self.embed.shape[1] == self.H
        self.w = self.embed if tied else np.asarray(sd["linear.weight"], F64)
        self.b = np.asarray(sd["linear.bias"], F64)

    def log_softmax_seq(self, x):
        """x: input ids [n] -> [n, V] log_softmax of the output layer at every position, from zero state"""
        H = self.H
        state = [(np.zeros(H, F64), np.zeros(H, F64)) for _ in self.layers]
        out = np.zeros((len(x), self.w.shape[0]), F64)
        for k, tok in enumerate(x):
            v = self.embed[int(tok)]
            for l, (wi, wh, bi, bh) in enumerate(self.layers):
                h, c = state[l]
                g = wi @ v + bi + wh @ h + bh
                i, f, gg, o = _sigmoid(g[:H]), _sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sigmoid(g[3 * H:])
                c = f * c + i * gg
                h = o * np.tanh(c)
                state[l] = (h, c)
                v = h
            z = self.w @ v + self.b
            m = z.max()
            out[k] = (z - m) - np.log(np.exp(z - m).sum())
        return out

    def score(self, y, start=None):
        """-> (total, lp float64 [U])"""
        y = [int(t) for t in y]
        U = len(y)
        lp = np.zeros(U, F64)
        if U == 0:
            return 0.0, lp
        if start is None:
            if U > 1:
                ls = self.log_softmax_seq(y[:-1])
                lp[1:] = ls[np.arange(U - 1), y[1:]]
        else:
            ls = self.log_softmax_seq([int(start)] + y[:-1])
            lp[:] = ls[np.arange(U), y]
        return float(lp.sum()), lp
