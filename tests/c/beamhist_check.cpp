// beamhist_check.cpp -- libreasr_amd/csrc/lasr_beamhist.hip.h (the host's shared-prefix tree of beam hypotheses, standard C++ only)
// against plain per-slot vectors of (token, frame, logp): random selection rounds -- carried slots, extensions, dead slots (-2),
// idle rounds (-1, skipped by the caller as the engine does) -- for W in {2, 3, 8}, with and without records, with a compaction
// threshold of 100 / 300 nodes so that the compaction (2^18 nodes in the engine, never reached by a GPU test) runs many times.
// Built with -fsanitize=address,undefined by tests/test_beam_records_cpu.py.
#include "../../libreasr_amd/csrc/lasr_beamhist.hip.h"

#include <cstdio>
#include <cstdlib>
#include <random>

struct Tok { int32_t tok, frame; float logp; };

static int fail(const char* what, int W, int round) {
    std::printf("beamhist_check: FAILED (%s) W=%d round=%d\n", what, W, round);
    return 1;
}

static int run(int W, bool with_recs, size_t compact_at, unsigned seed, long long* compactions) {
    std::mt19937 rng(seed);
    BeamHost B;
    bh_reset(B, W);
    std::vector<std::vector<Tok>> plain(W);            // the hypothesis of slot j, spelled out
    std::vector<char> alive(W, 0);
    alive[0] = 1;                                      // a fresh beam: one empty hypothesis in slot 0 (cur = -1 is the empty path)
    const long long frame_add = 1000;
    int frame = 0;
    for (int round = 0; round < 1500; ++round) {
        if (rng() % 11 == 0) continue;                 // idle round (-1): the engine does not call bh_apply
        if (rng() % 3 == 0) ++frame;
        if (rng() % 400 == 0) {                        // predictor reset: the beam restarts
            bh_reset(B, W);
            for (auto& p : plain) p.clear();
            std::fill(alive.begin(), alive.end(), 0);
            alive[0] = 1;
        }
        std::vector<int> live;
        for (int j = 0; j < W; ++j)
            if (alive[j]) live.push_back(j);
        int e[8];
        BeamRec rec[8];
        std::vector<std::vector<Tok>> next(W);
        std::vector<char> nalive(W, 0);
        for (int j = 0; j < W; ++j) {
            rec[j] = BeamRec{-77, -77.f};              // stale where the slot is not extended: must never be read
            if (rng() % 7 == 0 && j > 0) { e[j] = -2; continue; }
            const int p = live[rng() % live.size()];
            const int tok = (rng() % 5 < 2) ? 1 + (int)(rng() % 2047) : 0;
            e[j] = (p << 16) | tok;
            next[j] = plain[p];
            nalive[j] = 1;
            if (tok) {
                const float lp = -(float)(rng() % 100000) / 1000.f;
                rec[j] = BeamRec{frame, lp};
                next[j].push_back(Tok{tok - 1, (int32_t)(frame + frame_add), lp});
            }
        }
        const size_t before = B.par.size();
        size_t n_ext = 0;
        for (int j = 0; j < W; ++j) n_ext += e[j] >= 0 && (e[j] & 0xffff) != 0;
        bh_apply(B, e, W, with_recs ? rec : nullptr, frame_add, compact_at);
        if (B.par.size() != before + n_ext) ++*compactions;       // (a rebuilt tree: one chain per live slot)
        plain.swap(next);
        alive.swap(nalive);
        if (with_recs ? (B.frame.size() != B.par.size() || B.logp.size() != B.par.size()) : (!B.frame.empty() || !B.logp.empty()))
            return fail("record arrays not parallel to the nodes", W, round);
        for (int j = 0; j < W; ++j) {
            if (!alive[j]) {
                if (B.cur[j] != -1) return fail("dead slot has a path", W, round);
                continue;
            }
            std::vector<int32_t> toks;
            std::vector<BeamRec> recs;
            bh_tokens(B, B.cur[j], toks);
            if (toks.size() != plain[j].size()) return fail("length", W, round);
            if (with_recs) {
                bh_records(B, B.cur[j], recs);
                if (recs.size() != toks.size()) return fail("records length", W, round);
            }
            for (size_t i = 0; i < toks.size(); ++i) {
                if (toks[i] != plain[j][i].tok) return fail("token", W, round);
                if (with_recs && (recs[i].frame != plain[j][i].frame || recs[i].logp != plain[j][i].logp)) return fail("record", W, round);
            }
        }
    }
    return 0;
}

int main() {
    long long compactions = 0;
    unsigned seed = 1;
    for (int W : {2, 3, 8})
        for (int recs = 0; recs < 2; ++recs)
            for (size_t at : {(size_t)100, (size_t)300}) {
                long long n = 0;
                if (run(W, recs != 0, at, seed++, &n)) return 1;
                if (n < 5) { std::printf("beamhist_check: FAILED (only %lld compactions, W=%d)\n", n, W); return 1; }
                compactions += n;
            }
    // the default threshold: nothing compacts
    {
        long long n = 0;
        BeamHost B;
        bh_reset(B, 2);
        int e[2] = {(0 << 16) | 5, -2};
        BeamRec r[2] = {{3, -1.f}, {0, 0.f}};
        for (int i = 0; i < 1000; ++i) bh_apply(B, e, 2, r);
        if (B.par.size() != 1000 || B.frame.size() != 1000) return fail("default threshold", 2, 0);
        (void)n;
    }
    std::printf("beamhist_check: ok (%lld compactions)\n", compactions);
    return 0;
}
