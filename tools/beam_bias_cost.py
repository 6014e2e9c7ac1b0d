"""What does contextual biasing cost in beam search?  (run on the GPU box)
cfg2 (synthetic weights), bf16 operands, beam 4, 64 streams of synthetic speech, pipelined (lasr_push_submit / lasr_step_wait, 3 model
steps in flight, every model step's best hypothesis fetched): regions of 48 chunks (24 model steps) that alternate graph OFF / ON in one
process, 4 of each after one warm-up region of each; the streams are reset before every region, so every region decodes the same audio
from the same state.  The graph: 100 random phrases of 2 to 4 tokens, boost 1.0.  Per setting: audio seconds per second (median and
range over its regions), selection rounds per model step (lasr_get_stats decode_iters) and tokens of the 64 best hypotheses at the end of a region --
biasing changes how many tokens are emitted, so the two settings do not do the same work.  A figure, no threshold.
    python tools/beam_bias_cost.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from libreasr_amd import synth
from libreasr_amd.engine import Engine

CHUNK, B, NCH, WIDTH = 1280, 64, 48, 4
cfg = synth.model_cfg("cfg2")
sd = synth.synth_state_dict(cfg)
pcm = np.stack([synth.synth_pcm(1, NCH * CHUNK, seed=1234 + s)[0] for s in range(B)]).reshape(B, NCH, CHUNK)


def graph(eng, n=100, boost=1.0, seed=7):
    rng = np.random.default_rng(seed)
    phrases = [[int(t) for t in rng.integers(3, cfg["vocab"], int(rng.integers(2, 5)))] for _ in range(n)]
    return eng.beam_bias_compile(phrases, [boost] * n)


def throughput():
    dev = torch.as_tensor(pcm).to("cuda")
    eng = Engine(sd, cfg, max_streams=B, beam=WIDTH, dtype="bf16")
    g = graph(eng)
    slots = [eng.open() for _ in range(B)]
    res = {"off": [], "on": []}
    for rep in range(10):
        on = bool(rep & 1)
        eng.set_beam_bias(g if on else None)
        for s in slots:
            eng.reset(s, 15)
        iters, steps, toks = 0, 0, 0

        def collect():
            nonlocal iters, steps, toks
            if eng.wait():
                toks = sum(len(t) for t in eng.fetch_many(slots, 8192))      # (a beam's result is the whole best hypothesis: the last one counts)
                iters += eng.stats()["decode_iters"]
                steps += 1

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(NCH):
            eng.push_submit(slots, dev[:, k])
            while eng.pending() >= 3:
                collect()
        while eng.pending():
            collect()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep >= 2:
            res["on" if on else "off"].append((B * NCH * CHUNK / 16000.0 / dt, iters / max(steps, 1), toks))
    eng.close()
    out = {"graph": {"phrases": 100, "nodes": int(g.n_nodes), "edges": int(g.n_edges)}}
    for k, v in res.items():
        a = np.array(v, dtype=np.float64)
        out[k] = {"audio_s_per_s_median": round(float(np.median(a[:, 0])), 1), "audio_s_per_s_min": round(float(a[:, 0].min()), 1),
                  "audio_s_per_s_max": round(float(a[:, 0].max()), 1), "rounds_per_model_step": round(float(a[:, 1].mean()), 2),
                  "tokens_per_region": round(float(a[:, 2].mean()), 1), "regions": len(v)}
    return out


print(json.dumps({"model": "cfg2", "dtype": "bf16", "beam": WIDTH, "streams": B, "chunks_per_region": NCH, "throughput": throughput()}))
