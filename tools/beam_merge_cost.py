"""What does merging equal beam hypotheses cost?  (run on the GPU box)
cfg2 (synthetic weights), bf16 operands, beam 4, 64 streams of synthetic speech, pipelined (lasr_push_submit / lasr_step_wait, 3 model
steps in flight, every model step's best hypothesis fetched): regions of 48 chunks (24 model steps) that alternate switch OFF / ON in
one process, 4 of each after one warm-up region of each; the streams are reset before every region, so every region decodes the same
audio from the same state.  Per setting: audio seconds per second (median and range over its regions) and selection rounds per model
step (lasr_get_stats decode_iters).
    python tools/beam_merge_cost.py            # throughput
    python tools/beam_merge_cost.py timing     # LASR_DBG_TIMING: the selection kernel's own clocks (workgroup 0, synchronous steps),
                                               # ranking done [3] -> bookkeeping done [4] and entry -> [4], switch off / on, W = 4 and 8
    python tools/beam_merge_cost.py lm [W]     # the same throughput comparison with the synthetic LM `lm768` attached:
                                               # OFF against LASR_BEAM_MERGE_LM, beam W (default 4).  Under a kernel trace
                                               # (rocprofv3 --kernel-trace --stats -- python tools/beam_merge_cost.py lm) the
                                               # OFF regions run k_beam_fuse and the ON regions k_beam_fuse_merge: their times
                                               # stand side by side in the kernel statistics of one job."""
import ctypes as C
import json
import os
import sys
import time

timing = "timing" in sys.argv[1:]
with_lm = "lm" in sys.argv[1:]
WIDTH = int(sys.argv[sys.argv.index("lm") + 1]) if with_lm and len(sys.argv) > sys.argv.index("lm") + 1 else 4
if timing:
    os.environ["LASR_DBG_TIMING"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from libreasr_amd import synth
from libreasr_amd.engine import Engine

CHUNK, B, NCH = 1280, 64, 48
cfg = synth.model_cfg("cfg2")
sd = synth.synth_state_dict(cfg)
pcm = np.stack([synth.synth_pcm(1, NCH * CHUNK, seed=1234 + s)[0] for s in range(B)]).reshape(B, NCH, CHUNK)


def phases(W):
    """mean us of the last round of every synchronous model step: (ranking done -> bookkeeping done, entry -> bookkeeping done)"""
    eng = Engine(sd, cfg, max_streams=B, beam=W, dtype="bf16")
    slots = [eng.open() for _ in range(B)]
    out = {}
    for on in (False, True, False, True):
        eng.set_beam_merge(on)
        for s in slots:
            eng.reset(s, 15)
        rows = []
        for k in range(16):
            eng.push(slots, pcm[:, k])
            if eng.step(slots):
                eng.fetch_many(slots, 8192)
                buf = np.zeros(5 * 4096 * 16, dtype=np.uint64)
                eng.lib.lasr_debug_timing(eng.ctx, buf.ctypes.data_as(C.c_void_p))
                d = buf.reshape(5, 4096, 16)[4, 0, :10].astype(np.int64)
                rows.append([(d[4] - d[3]) / 100.0, (d[4] - d[0]) / 100.0])
        r = np.array(rows[1:])
        out.setdefault("on" if on else "off", []).append({"bookkeeping_us": round(float(r[:, 0].mean()), 2),
                                                          "kernel_us": round(float(r[:, 1].mean()), 2)})
    eng.close()
    return out


def throughput():
    dev = torch.as_tensor(pcm).to("cuda")
    eng = Engine(sd, cfg, max_streams=B, beam=WIDTH, dtype="bf16")
    if with_lm:
        eng.attach_lm(synth.synth_lm_state_dict("lm768"), int8=False)
    slots = [eng.open() for _ in range(B)]
    res = {"off": [], "on": []}
    for rep in range(10):
        on = bool(rep & 1)
        eng.set_beam_merge(on, lm=with_lm)
        for s in slots:
            eng.reset(s, 15)
        iters, steps = 0, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(NCH):
            eng.push_submit(slots, dev[:, k])
            while eng.pending() >= 3:
                if eng.wait():
                    eng.fetch_many(slots, 8192)
                    iters += eng.stats()["decode_iters"]
                    steps += 1
        while eng.pending():
            if eng.wait():
                eng.fetch_many(slots, 8192)
                iters += eng.stats()["decode_iters"]
                steps += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep >= 2:
            res["on" if on else "off"].append((B * NCH * CHUNK / 16000.0 / dt, iters / max(steps, 1)))
    eng.close()
    out = {}
    for k, v in res.items():
        a = np.array(v)
        out[k] = {"audio_s_per_s_median": round(float(np.median(a[:, 0])), 1), "audio_s_per_s_min": round(float(a[:, 0].min()), 1),
                  "audio_s_per_s_max": round(float(a[:, 0].max()), 1), "rounds_per_model_step": round(float(a[:, 1].mean()), 2),
                  "regions": len(v)}
    return out


if timing:
    print(json.dumps({"selection_kernel_clocks": {f"W{W}": phases(W) for W in (4, 8)}}))
else:
    print(json.dumps({"model": "cfg2", "dtype": "bf16", "beam": WIDTH, "lm": "lm768" if with_lm else None, "streams": B, "chunks_per_region": NCH, "throughput": throughput()}))
