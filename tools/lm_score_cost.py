"""What does an LM sequence score cost?  (run on the GPU box; the LM-side sibling of tools/lattice_cost.py)
cfg2 + lm768 (synthetic weights), the 8 candidates of lattice_cost.py's rescoring leg: the engine's own greedy transcript y of the
20.65 s demo utterance (taken before the LM is attached, so the candidates are that leg's) and, for j = 1..7, y with the labels from
position U - 8 j onwards replaced by (id % (V - 3)) + 3.  lasr_lm_score on the 8 candidates in one call and on the first alone, start
token 2: HIP events around the call, median of 20 calls after 3 warm-up calls; the time per pass is the call's over its passes (one
pass = command block + two small copies + the LM step + k_lm_pick).
    python tools/lm_score_cost.py [f32|bf16] [int8]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from libreasr_amd import flac, synth
from libreasr_amd.engine import Engine

dtype = sys.argv[1] if len(sys.argv) > 1 else "f32"
int8 = "int8" in sys.argv[2:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pcm, sr, _ = flac.decode(os.path.join(root, "tests", "golden", "demo_3729-6852-0035.flac"))
assert sr == 16000
cfg = synth.model_cfg("cfg2")
eng = Engine(synth.synth_state_dict(cfg), cfg, max_streams=8, dtype=dtype)
slots = [eng.open() for _ in range(8)]
eng.transcribe_pcm(slots[:1], [torch.as_tensor(np.ascontiguousarray(pcm, np.float32)).to(eng.device)])
y = eng.fetch(slots[0])[0]
eng.attach_lm(synth.synth_lm_state_dict("lm768"), int8=int8)
U, V = len(y), cfg["vocab"]
cands = [list(y)] + [list(y[:max(U - 8 * j, 0)]) + [(t % (V - 3)) + 3 for t in y[max(U - 8 * j, 0):]] for j in range(1, 8)]
out = {"dtype": dtype, "lm": "int8" if int8 else dtype, "labels": U}


def timed(call):
    ms = []
    for rep in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = call()
        e1.record()
        e1.synchronize()
        if rep >= 3:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), res


for n in (8, 1):
    ms, res = timed(lambda: eng.lm_score(slots[:n], cands[:n], start=2))
    passes = max(len(c) for c in cands[:n])
    out[f"n{n}"] = {"call_ms_median": round(ms, 3), "passes": passes, "us_per_pass": round(1e3 * ms / passes, 2),
                    "total": [r["total"] for r in res]}
eng.close()
print(json.dumps(out))
