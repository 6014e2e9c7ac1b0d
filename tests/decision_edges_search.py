"""How the seeds of decision_edges.SEEDS / BEAM_SEEDS were found (not a test; run by hand after a change to synth.py or to the oracle's
arithmetic that invalidates them).  For one model it walks the synth seeds in order and runs, per seed, exactly the checks that
test_decision_edges_cpu.py makes for that model -- so a seed printed here passes there -- and prints the figures of every seed that
passes.  Take the first one, or the one with the most slack, and write it into decision_edges.py.

  python tests/decision_edges_search.py greedy tiny 4112 300 [--lo 0 --hi 2500 --want 2]
  python tests/decision_edges_search.py beam 8 offline [--margin 1.5e-3]      (kind: offline | streams)

A greedy model passes about one seed in 20 (offline caps only) to one in 2000 (the two models that also stream); a beam run about one
seed in 50 (W = 4) to 200 (W = 8), which is why every beam run has a seed of its own.  --margin asks the beam for more than
BEAM_MARGIN, to pick a seed with slack."""
import argparse
import contextlib
import io
import os
import sys
from multiprocessing import Pool

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import decision_edges as D                     # noqa: E402
import test_decision_edges_cpu as T            # noqa: E402


def checks(job):
    kind, key, margin = job
    if kind == "beam":
        T.beam_checks(key[0], (key[1],))
        return
    mod = D.model(*key)
    if key in D.MODELS:
        T.offline_checks(mod, key)
    if key in D.MODELS[::2]:
        T.test_states_replay_the_decode(key)
    if key in D.STREAM_MODELS:
        T.stream_checks(mod, key)
    if key == D.TIE_MODEL:
        T.check_run(mod, D.offline(mod, 2), 2, f"{key} offline cap 2")
        T.check_run(mod, D.stream_run(mod, 2), 2, f"{key} streams cap 2")
        T.tie_checks(key)
    if key == D.LM_MODEL:
        T.lm_checks(False)
        T.lm_checks(True)


def try_seed(args):
    job, seed = args
    kind, key, margin = job
    (D.BEAM_SEEDS if kind == "beam" else D.SEEDS)[key] = seed
    D._MODELS.clear()
    D._RUNS.clear()
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            checks(job)
    except AssertionError:
        return seed, None
    return seed, out.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["greedy", "beam"])
    ap.add_argument("key", nargs="+", help="greedy: NAME V BLANK; beam: W offline|streams")
    ap.add_argument("--lo", type=int, default=0)
    ap.add_argument("--hi", type=int, default=2500)
    ap.add_argument("--want", type=int, default=2)
    ap.add_argument("--margin", type=float, default=None)
    a = ap.parse_args()
    key = (a.key[0], int(a.key[1]), int(a.key[2])) if a.kind == "greedy" else (int(a.key[0]), a.key[1])
    if a.margin is not None:
        D.BEAM_MARGIN = a.margin
    if a.kind == "beam":                        # give up on a seed at its first gap below the margin
        frame = D.BeamTrack.frame

        def fail_fast(self, enc_t):
            frame(self, enc_t)
            assert not any(0 != g < D.BEAM_MARGIN for g in self.gaps[-4 * self.W:])

        D.BeamTrack.frame = fail_fast
    found = 0
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for seed, figures in pool.imap(try_seed, [((a.kind, key, a.margin), s) for s in range(a.lo, a.hi)]):
            if figures is None:
                continue
            print(f"seed {seed} passes:\n{figures}", flush=True)
            found += 1
            if found >= a.want:
                pool.terminate()
                break
    print(f"{found} seeds found in [{a.lo}, {a.hi})")


if __name__ == "__main__":
    main()
