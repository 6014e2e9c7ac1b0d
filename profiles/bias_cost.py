"""Cost of contextual biasing on: cfg2 f32, 64 streams, the pipelined protocol with 12 model steps in flight, regions
of the same audio alternately with no graph and with a 100-phrase graph attached, in one process.  A figure to report, no
threshold.  With a graph the decode runs one frame per iteration (la = 1), which alone costs launches.

  python profiles/bias_cost.py [--seconds 20 --repeat 6 --regions 3 --boost 2.0]

A region streams the same `seconds` of audio per stream `repeat` times over (64 x 20 s x 6 = 7680 audio-seconds).

Prints one JSON line: audio-seconds per second of every region, the medians, and the tokens emitted per region."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft                # noqa: E402

STREAMS, DEPTH = 64, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--repeat", type=int, default=6)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--boost", type=float, default=2.0)
    a = ap.parse_args()
    graft.build()
    import torch
    from libreasr_amd import synth
    from libreasr_amd.engine import Engine
    cfg = synth.model_cfg("cfg2")
    eng = Engine(synth.synth_state_dict(cfg, seed=0), cfg, max_streams=STREAMS)
    rng = np.random.default_rng(0)
    phrases = [[int(t) for t in rng.integers(3, cfg["vocab"], int(rng.integers(2, 5)))] for _ in range(100)]
    graph = eng.bias_compile(phrases, [a.boost] * len(phrases))
    pcm = synth.synth_pcm(STREAMS, int(16000 * a.seconds), seed=1234)
    chunks = np.stack([np.stack(synth.stream_chunks(p, 1280, lead=1, tail=4)) for p in pcm], axis=1)      # [chunk][stream][1280]
    dev = torch.as_tensor(chunks).to(eng.device)
    slots = [eng.open() for _ in range(STREAMS)]

    def region():
        eng.reset_many(slots, 15)
        n_tok = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.repeat * dev.shape[0]):
            eng.push_submit(slots, dev[k % dev.shape[0]])
            if eng.pending() >= DEPTH and eng.wait():
                n_tok += sum(len(t) for t in eng.fetch_many(slots, 256))
        while eng.pending():
            if eng.wait():
                n_tok += sum(len(t) for t in eng.fetch_many(slots, 256))
        torch.cuda.synchronize()
        return STREAMS * a.repeat * dev.shape[0] * 1280 / 16000.0 / (time.perf_counter() - t0), n_tok

    out = {"off": [], "on": [], "tokens_off": [], "tokens_on": []}
    region()                                                  # warm-up (graphs captured) with no graph ...
    eng.set_bias(graph)
    region()                                                  # ... and with one
    for _ in range(a.regions):
        for key, g in (("off", None), ("on", graph)):
            eng.set_bias(g)
            rate, n = region()
            out[key].append(round(rate, 1))
            out["tokens_" + key].append(n)
    out["median_off"], out["median_on"] = float(np.median(out["off"])), float(np.median(out["on"]))
    out["graph"] = {"phrases": len(phrases), "nodes": graph.n_nodes, "edges": graph.n_edges, "boost": a.boost}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
