"""LM sequence scoring without a GPU: the float64 reference the GPU tests take their expected values from
(tests/lm_score_ref.py) against torch.nn's Embedding / LSTM / Linear / log_softmax in double on the whole sequence, and the host
logic of LibreASR.lm_score / rescore_lm (grouping, the score formula, ties, order) against a fake engine object."""
import numpy as np
import pytest
import torch

import lm_score_ref as LR
from libreasr_amd import _native as N
from libreasr_amd import synth

LENGTHS = (0, 1, 2, 17, 40)


def torch_lm(sd):
    """lm.py:20-29 in double from a state dict: (embed, rnn, linear), the output layer tied when embed == hidden"""
    V, E = sd["embed.weight"].shape
    H = sd["rnn.weight_hh_l0"].shape[1]
    L = sum(1 for k in sd if k.startswith("rnn.weight_hh_l"))
    embed = torch.nn.Embedding(V, E, padding_idx=0).double()
    rnn = torch.nn.LSTM(E, H, batch_first=True, num_layers=L).double()
    linear = torch.nn.Linear(H, V).double()
    with torch.no_grad():
        embed.weight.copy_(torch.as_tensor(np.asarray(sd["embed.weight"], np.float64)))
        for l in range(L):
            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(rnn, f"{k}_l{l}").copy_(torch.as_tensor(np.asarray(sd[f"rnn.{k}_l{l}"], np.float64)))
        linear.bias.copy_(torch.as_tensor(np.asarray(sd["linear.bias"], np.float64)))
        if E == H:
            linear.weight = embed.weight
        else:
            linear.weight.copy_(torch.as_tensor(np.asarray(sd["linear.weight"], np.float64)))
    return embed, rnn, linear


def torch_terms(mods, y, start):
    """LM.forward on the whole input sequence (lm.py:31-40), then the gather of the labels"""
    embed, rnn, linear = mods
    U = len(y)
    lp = np.zeros(U, np.float64)
    x = list(y[:-1]) if start is None else [start] + list(y[:-1])
    if U == 0 or not x:
        return lp
    with torch.no_grad():
        ls = torch.log_softmax(linear(rnn(embed(torch.as_tensor([x], dtype=torch.long)))[0]), dim=-1)[0].numpy()
    tgt = y[1:] if start is None else y
    lp[U - len(tgt):] = ls[np.arange(len(tgt)), tgt]
    return lp


@pytest.mark.parametrize("lm_name", ["tiny_lm", "tiny_lm_untied"])
def test_reference_against_torch_nn(lm_name):
    sd = synth.synth_lm_state_dict(lm_name)
    ref, mods = LR.LmRef(sd), torch_lm(sd)
    rng = np.random.default_rng(5)
    worst = 0.0
    for U in LENGTHS:
        y = [int(t) for t in rng.integers(1, 64, U)]
        for start in (None, 2):
            total, lp = ref.score(y, start)
            want = torch_terms(mods, y, start)
            assert lp.shape == (U,) and total == float(lp.sum())
            if U:
                worst = max(worst, float(np.abs(lp - want).max()))
                assert np.abs(lp - want).max() <= 1e-9, (lm_name, U, start)
            if start is None and U >= 1:
                assert lp[0] == 0.0
            assert np.all(lp <= 0.0)
    print(f"{lm_name}: max |reference - torch.nn| per term {worst:.3e}")


def test_symbol_and_python_surface():
    assert ("lasr_lm_score", N.C.c_int, [N._P, N._P, N.C.c_int, N._P, N._P, N.C.c_int, N._P, N._P]) in N.SYMBOLS
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    assert callable(getattr(Engine, "lm_score", None))
    assert callable(getattr(LibreASR, "lm_score", None)) and callable(getattr(LibreASR, "rescore_lm", None))
    import __graft_entry__ as graft
    graft.build()
    assert N.lib().lasr_lm_score(None, None, 1, None, None, -1, None, None) == N.LASR_EINVAL      # no context: an error code


# ------------------------------------------------------------------------------- host logic of the facade
class FakeEngine:
    """What LibreASR.lm_score / rescore_lm use of an engine; am / lm: per candidate (keyed by its id tuple) the two scores"""

    def __init__(self, am, lm, max_streams=4):
        self.max_streams, self.am, self.lm = max_streams, am, lm
        self.open_now, self.calls = set(), []

    def open(self):
        s = min(set(range(self.max_streams)) - self.open_now)      # (KeyError-free: min() of an empty set raises ValueError = "full")
        self.open_now.add(s)
        return s

    def close_slot(self, s):
        self.open_now.remove(s)

    def score_pcm(self, slots_per_utt, pcm_list, cand_lists):
        assert len(slots_per_utt) == len(pcm_list) == len(cand_lists) == 1
        assert set(slots_per_utt[0]) <= self.open_now and len(slots_per_utt[0]) == len(cand_lists[0])
        self.calls.append(("score_pcm", tuple(slots_per_utt[0]), len(cand_lists[0])))
        return [{"loglik": np.array([self.am[tuple(c)] for c in cand_lists[0]], np.float64)}]

    def lm_score(self, slots, token_lists, start=None):
        assert set(slots) <= self.open_now and len(slots) == len(token_lists) == len(set(slots))
        self.calls.append(("lm_score", tuple(slots), len(token_lists), start))
        return [{"total": self.lm[tuple(c)], "logps": np.zeros(len(c), np.float32)} for c in token_lists]


def facade(eng):
    from libreasr_amd.api import LibreASR

    class Model:
        engine = eng
    return LibreASR(None, None, Model(), None, None)


CANDS = [[5, 6, 7], [5, 6], [9], [], [4, 4, 4, 4], [8, 1]]
AM = dict(zip(map(tuple, CANDS), [-3.0, -2.5, -7.0, -9.0, -2.5, -4.0]))
LM = dict(zip(map(tuple, CANDS), [-6.0, -5.0, -1.0, 0.0, -11.0, -3.5]))
PCM = np.zeros(16000, np.float32)


def test_rescore_lm_formula_groups_and_order():
    eng = FakeEngine(AM, LM)
    asr = facade(eng)
    r = asr.rescore_lm(PCM, CANDS, lm_weight=0.3, length_bonus=0.5, start=2)
    am, lm = [AM[tuple(c)] for c in CANDS], [LM[tuple(c)] for c in CANDS]
    assert r["am"] == am and r["lm"] == lm
    want = [np.float64(a) + np.float64(0.3) * np.float64(l) + np.float64(0.5) * np.float64(len(c)) for a, l, c in zip(am, lm, CANDS)]
    assert r["score"] == [float(w) for w in want] and all(isinstance(s, float) for s in r["score"])
    assert r["order"] == sorted(range(6), key=lambda j: (-want[j], j)) and r["best"] == r["order"][0] == int(np.argmax(want))
    # 6 candidates on 4 slots: two groups, each opens its slots once for both engine calls and closes them
    assert eng.calls == [("score_pcm", (0, 1, 2, 3), 4), ("lm_score", (0, 1, 2, 3), 4, 2),
                         ("score_pcm", (0, 1), 2), ("lm_score", (0, 1), 2, 2)]
    assert not eng.open_now


def test_rescore_lm_ties_and_zero_weights():
    eng = FakeEngine(AM, LM)
    asr = facade(eng)
    r = asr.rescore_lm(PCM, CANDS, lm_weight=0.0, length_bonus=0.0)
    am = [AM[tuple(c)] for c in CANDS]
    assert r["score"] == am
    assert r["best"] == int(np.argmax(am)) == 1                  # candidates 1 and 4 tie at -2.5: the lowest index
    assert r["order"] == [1, 4, 0, 5, 2, 3]
    assert eng.calls[1][3] is None                               # start=None reaches the engine as it is
    # a tie made by the combination itself
    eng2 = FakeEngine({(1,): -1.0, (2,): -2.0, (3,): -1.0}, {(1,): -4.0, (2,): -2.0, (3,): -4.0})
    r = facade(eng2).rescore_lm(PCM, [[1], [2], [3]], lm_weight=0.5)
    assert r["score"] == [-3.0, -3.0, -3.0] and r["best"] == 0 and r["order"] == [0, 1, 2]


def test_lm_score_groups():
    eng = FakeEngine(AM, LM)
    out = facade(eng).lm_score(CANDS, start=2)
    assert out == [LM[tuple(c)] for c in CANDS] and all(isinstance(v, float) for v in out)
    assert eng.calls == [("lm_score", (0, 1, 2, 3), 4, 2), ("lm_score", (0, 1), 2, 2)]
    assert not eng.open_now
