// lasr_results.hip.h -- host results of the decode protocols: what a slot holds until it is fetched (SlotResult) and, with a beam, the
// stream's hypotheses between the kernels' selection rounds and that result (BeamSlot).  Both protocols fill them through the same
// calls: the synchronous one builds a step's result and delivers it at once, the pipelined one builds it when the step's last round
// is replayed (pump thread, under lasr_ctx::mu), queues it, and delivers it when the step is collected.
// Standard C++ only, no HIP include (named like the unit's other headers so that the build tracks it): the engine includes it through
// lasr_ctx.hip.h, tests/c/results_check.cpp on its own.
#pragma once

#include <cstring>
#include <deque>
#include <utility>

#include "lasr_beamhist.hip.h"

// tokens with their records: recs runs parallel to tokens while records are on (lasr_set_alignments / lasr_set_beam_records) and is
// EMPTY while they are off
struct TokList {
    std::vector<int32_t> tokens;
    std::vector<BeamRec> recs;
    // frames / logps may be null (each on its own): that part of the records is not handed out
    void copy_to(int32_t* t, int32_t* frames, float* logps) const {
        if (!tokens.empty()) memcpy(t, tokens.data(), sizeof(int32_t) * tokens.size());
        if (frames) for (size_t i = 0; i < recs.size(); ++i) frames[i] = recs[i].frame;
        if (logps) for (size_t i = 0; i < recs.size(); ++i) logps[i] = recs[i].logp;
    }
};
struct BeamHyp : TokList { double score = 0.0; };

// What a slot hands to the fetch calls.  Greedy: the tokens decoded since the last fetch.  Beam: the whole best hypothesis as of the
// last model step and, records on, that step's whole beam (nbest[0] is the same hypothesis WITH its records; `recs` stays empty).
struct SlotResult : TokList {
    double neg_logp = 0.0, align = 0.0;      // outlive a fetch (read after it; the beam's freeze takes its score from neg_logp)
    std::vector<BeamHyp> nbest;

    void append(int32_t tok) { tokens.push_back(tok); }
    void append(int32_t tok, BeamRec r) { tokens.push_back(tok); recs.push_back(r); }
    void set_beam(std::vector<int32_t>&& best, double score, std::vector<BeamHyp>&& beam) {
        tokens = std::move(best); recs.clear(); nbest = std::move(beam);
        neg_logp = -score; align = 0.0;      // (alignment_score is a greedy-loop metric)
    }
    void clear() { tokens.clear(); recs.clear(); nbest.clear(); }
    int need() const { return (int)tokens.size(); }
    bool unfetched() const { return !tokens.empty() || !nbest.empty(); }
    // hands out the tokens and, where asked for, their records, then clears: whatever is not asked for -- the records, the rest of
    // the beam -- is dropped with them.  *n = need() either way; false (nothing consumed): more than cap, or tokens but no array
    bool take(int32_t* t, int32_t* frames, float* logps, int cap, int* n) {
        *n = need();
        if (*n > cap || (!t && *n)) return false;
        copy_to(t, frames, logps);
        clear();
        return true;
    }
};

// the result of one finished model step of a beam stream
struct BeamStep : TokList {                  // the best hypothesis; records on and no slot alive: the frozen prefix alone
    double score = 0.0;
    std::vector<BeamHyp> nbest;              // records on: every alive slot, best first
};

struct BeamSlot {
    BeamHost tree;                           // the slots' paths since the last predictor reset
    TokList frozen;                          // the best hypothesis at the last predictor reset(s)
    double frozen_score = 0.0;
    TokList best;                            // frozen + the current best path, as of the last DELIVERED step (what a reset freezes)
    std::deque<BeamStep> steps;              // pipelined protocol: finished model steps not yet collected

    // the winner: highest score, lowest slot; -1: no slot alive
    static int best_alive(const double* sc, unsigned alive, int W) {
        int best = -1;
        for (int j = 0; j < W; ++j)
            if (((alive >> j) & 1) && (best < 0 || sc[j] > sc[best])) best = j;
        return best;
    }
    // the whole beam's order: score descending, ties by slot ascending (ord[0] is best_alive's winner); returns how many are alive
    static int order(const double* sc, unsigned alive, int W, int* ord) {
        int n = 0;
        for (int j = 0; j < W; ++j)
            if ((alive >> j) & 1) ord[n++] = j;
        std::stable_sort(ord, ord + n, [&](int a, int b) { return sc[a] > sc[b]; });
        return n;
    }
    // the step that ends with the tree as it is now: sc[W] / alive = the slots' scores and alive mask at the step's end.  Every
    // hypothesis is materialised (frozen prefix + path of the tree); scores include frozen_score.
    BeamStep build(const double* sc, unsigned alive, bool recs) const {
        const int W = (int)tree.cur.size();
        BeamStep s;
        s.tokens = frozen.tokens; s.score = frozen_score;
        const int b = best_alive(sc, alive, W);
        if (b >= 0) { bh_tokens(tree, tree.cur[b], s.tokens); s.score += sc[b]; }
        if (!recs) return s;
        int ord[8];
        const int n = order(sc, alive, W, ord);
        s.nbest.resize(n);
        for (int i = 0; i < n; ++i) {
            BeamHyp& h = s.nbest[i];
            h.tokens = frozen.tokens; h.recs = frozen.recs;
            bh_tokens(tree, tree.cur[ord[i]], h.tokens); bh_records(tree, tree.cur[ord[i]], h.recs);
            h.score = frozen_score + sc[ord[i]];
        }
        s.recs = n ? s.nbest[0].recs : frozen.recs;      // hypothesis 0's records outlive the fetch: a predictor reset freezes them
        return s;
    }
    void deliver(BeamStep&& s, SlotResult& out) {
        best.tokens = s.tokens; best.recs = std::move(s.recs);
        out.set_beam(std::move(s.tokens), s.score, std::move(s.nbest));
    }
    // host side of a predictor reset: the best hypothesis so far (score: the slot's -neg_logp) is frozen, the beam restarts
    void freeze(double score) { frozen = best; frozen_score = score; bh_reset(tree, (int)tree.cur.size()); }
    void forget() { frozen = TokList{}; best = TokList{}; frozen_score = 0.0; bh_reset(tree, (int)tree.cur.size()); }
    // the tree and the prefixes keep records parallel to the tokens exactly while records are on: tokens decoded before a switch-on
    // have none (frame -1, log p 0); a switch-off drops them all
    void set_records(bool on) {
        const size_t nodes = on ? tree.par.size() : 0;
        tree.frame.assign(nodes, -1); tree.logp.assign(nodes, 0.f);
        frozen.recs.assign(on ? frozen.tokens.size() : 0, BeamRec{-1, 0.f});
        best.recs.assign(on ? best.tokens.size() : 0, BeamRec{-1, 0.f});
    }
};
