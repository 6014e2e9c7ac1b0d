"""How the phrase sets of beam_bias_ref.OFFLINE_CASES / STREAM_CASE were found (not a test; run by hand after a change to synth.py
or to the oracle's arithmetic that invalidates them).  It walks random phrase sets in seed order, runs the restatement of
beam_bias_ref on the inputs the GPU tests use, and prints every set that meets the input conditions test_beam_bias_cpu.py asserts
-- so a set printed here passes there.  Write the first one (or the one with the most slack) into beam_bias_ref.py.

  python tests/beam_bias_search.py offline tiny 4 [--lo 0 --hi 200 --want 2]
  python tests/beam_bias_search.py stream tiny 4

A phrase set: 2 to 4 phrases of 2 to 4 tokens cut from the hypotheses of the unbiased beam on the same inputs (none with an
immediate repeat of a token: on these randomly initialised models a kept bonus makes such a phrase repeat up to the per-frame
cap), plus one made of a two-token prefix of such a cut followed by two random tokens -- a match that starts and fails; boosts
from 0.25 to 2.0 in steps of 0.25."""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import beam_bias_ref as BB                     # noqa: E402
import beam_records_ref as R                   # noqa: E402
from libreasr_amd import synth                 # noqa: E402

RESET_AT = BB.STREAM_RESET_AT


def sources(kind, name, W):
    """the token lists of the unbiased beam's hypotheses (at least two tokens long)"""
    if kind == "offline":
        lists = [h[0] for u in R.offline_ref(name, W) for h in u["beam"]]
    else:
        lists = [h[0] for s in R.stream_ref(name, W) for step in s["steps"][:s["speech"]] for h in step]
    return sorted({tuple(y) for y in lists if len(y) >= 2})


def phrase_set(seed, src, vocab):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(2, 5))
    phrases = []
    for _ in range(200):
        y = src[int(rng.integers(len(src)))]
        n = int(rng.integers(2, min(4, len(y)) + 1))
        o = int(rng.integers(0, len(y) - n + 1))
        p = [int(t) for t in y[o:o + n]]
        if all(a != b for a, b in zip(p, p[1:])) and p not in phrases:
            phrases.append(p)
        if len(phrases) == k:
            break
    if phrases:
        phrases.append(phrases[0][:2] + [int(t) for t in rng.integers(3, vocab, 2)])
    weights = [float(rng.integers(1, 9)) * 0.25 for _ in phrases]
    return phrases, weights


def offline_figures(name, W, phrases, weights):
    """(smallest margin, utterances whose best tokens differ from the unbiased beam's, selected extensions with a negative gain,
    phrases completed, the best hypothesis differs from the run that never revokes, share of frames at the cap)"""
    g = BB.automaton(phrases, weights)
    on, keep, plain = BB.offline_run(name, W, g), BB.offline_run(name, W, g.no_revoke()), R.offline_ref(name, W)
    margin = min(u["margin"] for u in on)
    differ = sum(u["beam"][0][0] != p["beam"][0][0] for u, p in zip(on, plain))
    neg = sum(u["stats"].get("neg", 0) for u in on)
    term = sum(u["stats"].get("term", 0) for u in on)
    decides = any(u["beam"][0][0] != q["beam"][0][0] for u, q in zip(on, keep))
    capped = sum(u["stats"]["capped"] for u in on) / max(1, sum(u["stats"]["frames"] for u in on))
    return margin, differ, neg, term, decides, capped


def stream_figures(name, W, phrases, weights):
    """(streams truncated by the margin rule before their speech ends -- the larger count of the two variants, the fewest steps
    compared behind the reset, streams whose tokens differ from the unbiased beam's, negative gains selected, phrases completed)"""
    g = BB.automaton(phrases, weights)
    a, b, plain = BB.stream_run(name, W, g), BB.stream_run(name, W, g, reset_at=RESET_AT), R.stream_ref(name, W)
    trunc = max(sum(BB.full_upto(s) < s["speech"] for s in run) for run in (a, b))
    behind = min(BB.full_upto(s) - RESET_AT for s in b)
    differ = sum(s["steps"][BB.full_upto(s) - 1][0][0] != p["steps"][BB.full_upto(s) - 1][0][0] for s, p in zip(a, plain) if BB.full_upto(s))
    neg = sum(s["dec"].stats.get("neg", 0) for s in a)
    term = sum(s["dec"].stats.get("term", 0) for s in a)
    return trunc, behind, differ, neg, term


def try_seed(args):
    kind, name, W, seed = args
    phrases, weights = phrase_set(seed, sources(kind, name, W), synth.model_cfg(name)["vocab"])
    if len(phrases) < 3:
        return seed, False, None, phrases, weights
    if kind == "offline":
        f = offline_figures(name, W, phrases, weights)
        ok = f[0] >= BB.MARGIN and f[1] >= 2 and f[2] >= 1 and f[3] >= 1
    else:
        f = stream_figures(name, W, phrases, weights)
        ok = f[0] <= 1 and f[1] >= 1 and f[2] >= 1 and f[3] >= 1 and f[4] >= 1
    return seed, ok, f, phrases, weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["offline", "stream"])
    ap.add_argument("name")
    ap.add_argument("W", type=int)
    ap.add_argument("--lo", type=int, default=0)
    ap.add_argument("--hi", type=int, default=200)
    ap.add_argument("--want", type=int, default=2)
    a = ap.parse_args()
    found = 0
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for seed, ok, f, phrases, weights in pool.imap(try_seed, [(a.kind, a.name, a.W, s) for s in range(a.lo, a.hi)]):
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
