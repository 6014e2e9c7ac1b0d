"""How the phrase sets of bias_ref.OFFLINE_CASES / STREAM_CASE were found (not a test; run by hand after a change to synth.py or to
the oracle's arithmetic that invalidates them).  It walks random phrase sets in seed order, runs the restatement of bias_ref on
the inputs the GPU tests use, and prints every set that meets the input conditions test_bias_cpu.py asserts -- so a set printed
here passes there.  Write the first one (or the one with the most slack) into bias_ref.py.

  python tests/bias_search.py offline tiny [--lo 0 --hi 400 --want 2]
  python tests/bias_search.py stream tiny

A phrase set: 2 to 4 phrases of 3 or 4 tokens drawn from [3, vocab), weights from {2, 3, 4, 6}."""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import bias_ref as B                           # noqa: E402
from libreasr_amd import synth                 # noqa: E402
from oracle import rnnt_oracle as O            # noqa: E402
from test_alignment_cpu import oracle, utterances      # noqa: E402

RESET_AT = B.STREAM_RESET_AT          # the model step before which test_gpu_bias.py resets the stream in its state-rules test


def phrase_set(seed, vocab):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(2, 5))
    phrases = [[int(t) for t in rng.integers(3, vocab, int(rng.integers(3, 5)))] for _ in range(k)]
    weights = [float(rng.choice([2.0, 3.0, 4.0, 6.0])) for _ in range(k)]
    return phrases, weights


def offline_figures(name, phrases, weights):
    """the conditions of the offline parity test on the restatement: (min margin, tokens differ from the unbiased run, a boosted
    token taken where the joint's argmax was blank, deepest node reached, a frame at max_iters)"""
    m = oracle(name)
    g = B.automaton(phrases, weights)
    margin, differ, beaten, deepest, capped = float("inf"), False, False, 0, False
    for p in utterances():
        feats = O.features_offline(p)
        y, _, _, iters, dec, v, args = B.decode_greedy(m, feats, g, 3)
        margin = min([margin] + [d[4] for d in dec])
        differ |= y != m.decode_greedy(feats, max_iters=3)[0]
        beaten |= any(d[0] != m.blank and a == m.blank for d, a in zip(dec, args))
        deepest = max([deepest, int(g.depth[v])] + [int(g.depth[d[3]]) for d in dec])
        capped |= any(i == 3 for i in iters)          # (iters == max_iters: the cap ended the frame, models.py:408)
    return margin, differ, beaten, deepest, capped


def stream_figures(name, phrases, weights):
    """the streaming test's conditions: the smallest margin over the .speech steps of the plain run and of the run that is reset
    before step RESET_AT, tokens emitted after the reset, the node when the reset comes, tokens differ from the unbiased run"""
    m = oracle(name)
    g = B.automaton(phrases, weights)
    pcm = synth.synth_pcm(1, 48000, seed=1234)[0]
    a = B.stream_run(m, g, pcm)
    b = B.stream_run(m, g, pcm, reset_at=RESET_AT)
    plain = B.stream_run(m, None, pcm)
    margin = min(a["margins"][:a["speech"]] + b["margins"][:b["speech"]])
    after = sum(len(s[0]) for s in b["steps"][RESET_AT:b["speech"]])
    differ = [s[0] for s in a["steps"][:a["speech"]]] != [s[0] for s in plain["steps"][:plain["speech"]]]
    deepest = max(int(g.depth[d[3]]) for d in a["decisions"])
    return margin, after, int(b["nodes"][RESET_AT - 1]), differ, deepest


def try_seed(args):
    kind, name, seed = args
    phrases, weights = phrase_set(seed, synth.model_cfg(name)["vocab"])
    if kind == "offline":
        f = offline_figures(name, phrases, weights)
        ok = f[0] >= B.MARGIN and f[1] and f[2] and f[3] >= 3 and f[4]
    else:
        f = stream_figures(name, phrases, weights)
        ok = f[0] >= B.MARGIN and f[1] > 0 and f[2] != 0 and f[3] and f[4] >= 2
    return seed, ok, f, phrases, weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["offline", "stream"])
    ap.add_argument("name")
    ap.add_argument("--lo", type=int, default=0)
    ap.add_argument("--hi", type=int, default=400)
    ap.add_argument("--want", type=int, default=2)
    a = ap.parse_args()
    found = 0
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for seed, ok, f, phrases, weights in pool.imap(try_seed, [(a.kind, a.name, s) for s in range(a.lo, a.hi)]):
            if not ok:
                continue
            print(f"seed {seed} passes: figures {f}\n  phrases = {phrases}\n  weights = {weights}", flush=True)
            found += 1
            if found >= a.want:
                pool.terminate()
                break
    print(f"{found} sets found in [{a.lo}, {a.hi})")


if __name__ == "__main__":
    main()
