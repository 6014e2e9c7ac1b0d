"""What does a forced alignment cost?  (run on the GPU box)
cfg2 (synthetic weights), the 20.65 s demo utterance with the engine's own greedy transcript, lasr_align_pcm at n = 1 and n = 8:
HIP events around the call, median of 20 runs after 3 warm-up runs, and the per-stage times the engine records with profiling on
(front-end + encoder, teacher-forced predictor, lattice blocks, dynamic programme).  The lattice blocks are dominated by the logits
GEMM: cells x 2 J V flop, set against the f32 MFMA peak (157.3 TFLOP/s, MI355X data sheet).
Rescoring leg: 8 candidates -- the greedy transcript y and, for j = 1..7, y with the labels from position U - 8 j onwards
replaced by (id % (V - 3)) + 3 -- through LibreASR.score's path (lasr_align_pcm on 8 copies of the audio, no Viterbi pass) and, where
the library has it, through LibreASR.rescore's (lasr_score_pcm: one encoder pass, the candidates' prefix tree), measured the same way.
Posterior leg: the n = 1 and n = 8 calls again with posteriors=True (lasr_align_post_pcm: alpha / beta and the occupancies
behind the same stages), beside the plain legs of the same process; post_ms is the added stage, to be set against dp_ms.
Banded leg: the utterance tiled 4x (82.6 s) with the engine's own greedy transcript of that audio, n = 1:
lasr_align_pcm on the full lattice beside lasr_align_band_pcm with band = 64 at max_passes 1 and 4 -- stage times (with several
passes blocks_ms runs from the end of the predictor to the end of the last pass's blocks, dp_ms is the last pass's), cells, passes,
touch, and how far the banded viterbi score and frames are from the full lattice's.
Banded posterior leg: each banded call again through lasr_align_band_post_pcm, beside the plain banded leg of the same
process: post_ms is the added stage (alpha / beta and the occupancies over the last pass's band), to be set against dp_ms.
    python tools/lattice_cost.py [f32|bf16]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from libreasr_amd import flac, synth
from libreasr_amd.engine import Engine

PEAK_F32_MFMA = 157.3e12
dtype = sys.argv[1] if len(sys.argv) > 1 else "f32"
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pcm, sr, _ = flac.decode(os.path.join(root, "tests", "golden", "demo_3729-6852-0035.flac"))
assert sr == 16000
cfg = synth.model_cfg("cfg2")
eng = Engine(synth.synth_state_dict(cfg), cfg, max_streams=8, dtype=dtype)
slots = [eng.open() for _ in range(8)]
dev_pcm = torch.as_tensor(np.ascontiguousarray(pcm, np.float32)).to(eng.device)
eng.transcribe_pcm(slots[:1], [dev_pcm])
y = eng.fetch(slots[0])[0]
out = {"dtype": dtype, "seconds": round(len(pcm) / sr, 2), "labels": len(y), "lat_R": eng.config("lat_R")}
eng.set_profiling(True)


def timed(call):
    """20 calls after 3 warm-ups -> (median call and stage times in ms, the last result, the unrounded stage medians in us)"""
    ms, stages = [], []
    for rep in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = call()
        e1.record()
        e1.synchronize()
        if rep >= 3:
            ms.append(e0.elapsed_time(e1))
            stages.append([eng.config(k) for k in ("lat_enc_us", "lat_pred_us", "lat_blocks_us", "lat_dp_us", "lat_post_us")])
    st = np.median(np.asarray(stages, np.float64), axis=0)
    return {"call_ms_median": round(float(np.median(ms)), 3), "encoder_ms": round(st[0] / 1e3, 3), "predictor_ms": round(st[1] / 1e3, 3),
            "blocks_ms": round(st[2] / 1e3, 3), "dp_ms": round(st[3] / 1e3, 3), "post_ms": round(st[4] / 1e3, 3)}, res, st


for n in (1, 8):
    leg, res, st = timed(lambda: eng.align_pcm(slots[:n], [dev_pcm] * n, [y] * n))
    T = (1 + len(pcm) // 160 - 10) // 8 + 1
    cells = n * T * (len(y) + 1)
    flop = cells * 2.0 * cfg["joint"] * cfg["vocab"]
    leg.update(T=T, cells=cells, gemm_gflop=round(flop / 1e9, 1),
               blocks_fraction_of_f32_mfma_peak=round(flop / (st[2] * 1e-6) / PEAK_F32_MFMA, 4) if st[2] else None,
               loglik=res[0]["loglik"], viterbi=res[0]["viterbi"])
    out[f"n{n}"] = leg
    leg, res, st = timed(lambda: eng.align_pcm(slots[:n], [dev_pcm] * n, [y] * n, posteriors=True))
    leg.update(post_over_dp=round(st[4] / st[3], 3) if st[3] else None, loglik=res[0]["loglik"],
               mean_time_std_frames=round(float(np.sqrt(res[0]["tok_var"]).mean()), 4) if len(y) else None)
    out[f"n{n}_post"] = leg
# rescoring: 8 candidates that share a prefix with the greedy transcript
U, V = len(y), cfg["vocab"]
cands = [list(y)] + [list(y[:max(U - 8 * j, 0)]) + [(t % (V - 3)) + 3 for t in y[max(U - 8 * j, 0):]] for j in range(1, 8)]
leg, res, _ = timed(lambda: eng.align_pcm(slots, [dev_pcm] * 8, cands, viterbi=False))
leg.update(rows=T * sum(len(c) + 1 for c in cands), loglik=[r["loglik"] for r in res])
out["score_path"] = leg
if hasattr(eng, "score_pcm"):
    leg, res, _ = timed(lambda: eng.score_pcm([slots], [dev_pcm], [cands]))
    leg.update(nodes=int(eng.prefix_tree(cands)["parent"].size), sum_u1=sum(len(c) + 1 for c in cands),
               rows=T * int(eng.prefix_tree(cands)["parent"].size), loglik=[float(v) for v in res[0]["loglik"]])
    out["rescore_path"] = leg
# banded alignment of long audio
if hasattr(eng, "lattice_band_dp"):
    long_pcm = torch.cat([dev_pcm] * 4)
    eng.transcribe_pcm(slots[:1], [long_pcm])
    yl = eng.fetch(slots[0])[0]
    Tl = (1 + 4 * len(pcm) // 160 - 10) // 8 + 1
    out["long"] = {"seconds": round(4 * len(pcm) / sr, 2), "labels": len(yl), "T": Tl}
    full = None
    if len(yl) <= eng.config("lat_umax"):
        leg, res, _ = timed(lambda: eng.align_pcm(slots[:1], [long_pcm], [yl]))
        full = res[0]
        leg.update(cells=Tl * (len(yl) + 1), loglik=full["loglik"], viterbi=full["viterbi"])
        out["long_full"] = leg
    for mp in (1, 4):
        leg, res, _ = timed(lambda: eng.align_pcm(slots[:1], [long_pcm], [yl], band=64, max_passes=mp))
        r = res[0]
        leg.update(cells=Tl * r["width"], width=r["width"], passes=r["passes"], touch=r["touch"], loglik=r["loglik"], viterbi=r["viterbi"])
        if full is not None:
            d = np.abs(np.asarray(r["frames"], np.int64) - np.asarray(full["frames"], np.int64))
            leg.update(viterbi_minus_full=r["viterbi"] - full["viterbi"], loglik_minus_full=r["loglik"] - full["loglik"],
                       frames_differ=int((d > 0).sum()), frames_max_abs_diff=int(d.max()) if d.size else 0)
        out[f"long_band64_p{mp}"] = leg
        if hasattr(eng, "align_band_post_pcm"):
            leg, res, st = timed(lambda: eng.align_band_post_pcm(slots[:1], [long_pcm], [yl], 64, max_passes=mp))
            p = res[0]
            leg.update(cells=Tl * p["width"], passes=p["passes"], post_over_dp=round(st[4] / st[3], 3) if st[3] else None, loglik=p["loglik"],
                       same_path=bool(np.array_equal(p["frames"], r["frames"]) and p["loglik"] == r["loglik"]),
                       mean_time_std_frames=round(float(np.sqrt(p["tok_var"]).mean()), 4) if len(yl) else None,
                       min_path_posterior=float(min(p["occ_emit"][int(t), u - int(p["lo"][int(t)])] for u, t in enumerate(p["frames"]))) if len(yl) else None)
            out[f"long_band64_p{mp}_post"] = leg
eng.close()
print(json.dumps(out))
