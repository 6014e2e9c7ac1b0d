"""The slot bookkeeping of the LibreASR facade without a GPU (beside tests/test_lm_score_cpu.py, which pins the grouping): whatever
happens inside a call, every slot it opened is closed again."""
import types

import numpy as np
import pytest

from libreasr_amd.api import LibreASR


class Full(RuntimeError):
    pass


class FakeEngine:
    """open() hands out 0, 1, .. and raises on call number `fail_at`; the engine calls raise when `broken`"""
    max_streams, beam, desc = 4, 1, types.SimpleNamespace(stride=8, hop=160, sample_rate=16000)

    def __init__(self, fail_at=None, broken=False):
        self.fail_at, self.broken, self.opens, self.open_now, self.closed = fail_at, broken, 0, set(), []

    def open(self):
        self.opens += 1
        if self.opens == self.fail_at:
            raise Full("LASR_EFULL")
        self.open_now.add(self.opens - 1)
        return self.opens - 1

    def close_slot(self, s):
        self.open_now.remove(s)
        self.closed.append(s)

    def lm_score(self, slots, token_lists, start=None):
        if self.broken:
            raise Full("engine call")
        return [{"total": -1.0, "logps": np.zeros(len(c), np.float32)} for c in token_lists]

    def score_pcm(self, slots_per_utt, pcm_list, cand_lists, viterbi=False):
        return [{"loglik": np.zeros(len(cand_lists[0])), "viterbi": np.zeros(len(cand_lists[0]))}]

    def align_pcm(self, slots, pcm_list, token_lists, **kw):
        return [{"loglik": 0.0, "viterbi": 0.0, "frames": np.zeros(len(y), np.int32), "logps": np.zeros(len(y), np.float32)} for y in token_lists]

    def transcribe_pcm(self, slots, pcm_list):
        pass

    def fetch(self, slot):
        return [1], 0.0, 0.0


def facade(eng):
    class Model:
        engine = eng
    return LibreASR(None, None, Model(), None, None)


PCM = np.zeros(16000, np.float32)
CANDS = [[5, 6], [7], [8, 9, 9]]
CALLS = {"transcribe": lambda asr: asr.transcribe([PCM] * 3, return_ids=True),
         "align": lambda asr: asr.align([PCM] * 3, CANDS),
         "score": lambda asr: asr.score(PCM, CANDS),
         "rescore": lambda asr: asr.rescore(PCM, CANDS),
         "lm_score": lambda asr: asr.lm_score(CANDS),
         "rescore_lm": lambda asr: asr.rescore_lm(PCM, CANDS, 0.5)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_failed_open_closes_the_slots_opened_before_it(name):
    """open() raises on the third call: the two opened slots are closed and the exception propagates"""
    eng = FakeEngine(fail_at=3)
    with pytest.raises(Full, match="LASR_EFULL"):
        CALLS[name](facade(eng))
    assert eng.opens == 3 and sorted(eng.closed) == [0, 1] and not eng.open_now


@pytest.mark.parametrize("name", sorted(CALLS))
def test_every_call_closes_what_it_opened(name):
    eng = FakeEngine()
    CALLS[name](facade(eng))
    assert eng.opens == 3 and sorted(eng.closed) == [0, 1, 2] and not eng.open_now


def test_failed_engine_call_closes_the_group():
    """a second group is not opened after the first one's engine call failed, and the first one's slots are closed before the
    exception leaves the facade"""
    eng = FakeEngine(broken=True)
    with pytest.raises(Full, match="engine call"):
        facade(eng).lm_score(CANDS * 2)
    assert eng.opens == 4 and sorted(eng.closed) == [0, 1, 2, 3] and not eng.open_now
