// results_check.cpp -- libreasr_amd/csrc/lasr_results.hip.h (the per-slot host results of both decode protocols, standard C++ only)
// against a spelled-out restatement: plain vectors of (token, frame, logp) per slot, written here.  Seeded random sequences.
//   greedy   append / copy-out / clear, records on and off: the three arrays come out parallel, a capacity one short consumes
//            nothing and reports the need, a null frames or logps pointer drops the records;
//   beam     W in {2, 3, 8}: random bh_apply rounds (as beamhist_check.cpp), step results from random scores and alive masks --
//            equal scores, a single alive slot, no alive slot -- built and delivered at once (the synchronous protocol) AND built,
//            queued and delivered later while the tree moves on (the pipelined one): every field equal; freezes (twice in a row,
//            with nothing decoded), forgets, and the records switched on and off mid-stream.
// Built with -fsanitize=address,undefined by tests/test_results_cpu.py.
#include "../../libreasr_amd/csrc/lasr_results.hip.h"

#include <cstdio>
#include <cstdlib>
#include <random>

struct Tok { int32_t tok, frame; float logp; };
using Path = std::vector<Tok>;

#define CHECK(cond, what)                                                                            \
    do {                                                                                             \
        if (!(cond)) { std::printf("results_check: FAILED (%s) line %d\n", what, __LINE__); return 1; } \
    } while (0)

// a TokList against the restatement: records parallel and equal while they are on, absent while they are off
static bool same(const TokList& t, const Path& p, bool recs) {
    if (t.tokens.size() != p.size() || t.recs.size() != (recs ? p.size() : 0)) return false;
    for (size_t i = 0; i < p.size(); ++i) {
        if (t.tokens[i] != p[i].tok) return false;
        if (recs && (t.recs[i].frame != p[i].frame || t.recs[i].logp != p[i].logp)) return false;
    }
    return true;
}
static bool same(const TokList& a, const TokList& b) {
    if (a.tokens != b.tokens || a.recs.size() != b.recs.size()) return false;
    for (size_t i = 0; i < a.recs.size(); ++i)
        if (a.recs[i].frame != b.recs[i].frame || a.recs[i].logp != b.recs[i].logp) return false;
    return true;
}
static bool same(const SlotResult& a, const SlotResult& b) {
    if (!same((const TokList&)a, (const TokList&)b) || a.neg_logp != b.neg_logp || a.align != b.align || a.nbest.size() != b.nbest.size()) return false;
    for (size_t i = 0; i < a.nbest.size(); ++i)
        if (!same(a.nbest[i], b.nbest[i]) || a.nbest[i].score != b.nbest[i].score) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------- greedy
static int greedy(bool recs, unsigned seed) {
    std::mt19937 rng(seed);
    SlotResult r;
    Path plain;
    int takes = 0, shorts = 0, drops = 0;
    for (int op = 0; op < 4000; ++op) {
        const int k = rng() % 10;
        if (k < 6) {                                       // a step's tokens
            for (int n = rng() % 7; n > 0; --n) {
                const Tok t{(int32_t)(rng() % 2048), (int32_t)(rng() % 100000), -(float)(rng() % 100000) / 1000.f};
                plain.push_back(t);
                if (recs) r.append(t.tok, BeamRec{t.frame, t.logp});
                else r.append(t.tok);
            }
        } else if (k == 6) {
            r.clear(); plain.clear();
        } else {
            const int n = (int)plain.size();
            CHECK(r.need() == n && same(r, plain, recs), "greedy: content before the copy-out");
            std::vector<int32_t> tok(n + 1, -5), fr(n + 1, -5);
            std::vector<float> lp(n + 1, -5.f);
            int got = -1;
            if (n > 0 && k == 7) {                         // one short: the need is reported, nothing is consumed
                CHECK(!r.take(tok.data(), fr.data(), lp.data(), n - 1, &got) && got == n, "greedy: capacity one short");
                CHECK(!r.take(nullptr, nullptr, nullptr, n, &got) && got == n, "greedy: no array");
                CHECK(tok[0] == -5 && same(r, plain, recs), "greedy: a refused copy-out consumed something");
                ++shorts;
                continue;
            }
            const bool want_fr = recs && rng() % 3 != 0, want_lp = recs && rng() % 3 != 0;
            CHECK(r.take(tok.data(), want_fr ? fr.data() : nullptr, want_lp ? lp.data() : nullptr, n, &got) && got == n, "greedy: copy-out");
            for (int i = 0; i < n; ++i) {
                CHECK(tok[i] == plain[i].tok, "greedy: token");
                CHECK(fr[i] == (want_fr ? plain[i].frame : -5) && lp[i] == (want_lp ? plain[i].logp : -5.f), "greedy: record not parallel");
            }
            CHECK(tok[n] == -5 && fr[n] == -5 && lp[n] == -5.f, "greedy: wrote past the count");
            CHECK(r.need() == 0 && r.tokens.empty() && r.recs.empty() && !r.unfetched(), "greedy: not cleared by the copy-out");
            plain.clear();
            ++takes; drops += recs && !(want_fr && want_lp);
        }
        CHECK(r.recs.size() == (recs ? r.tokens.size() : 0), "greedy: records not parallel to the tokens");
    }
    CHECK(takes > 100 && shorts > 50 && (!recs || drops > 20), "greedy: a case was not exercised");
    return 0;
}

// --------------------------------------------------------------------------------------------------------------------- beam
struct Plain {                                             // the restatement of one stream
    int W;
    std::vector<Path> path;                                // per slot, since the last freeze
    std::vector<char> alive;
    Path frozen, best;                                     // best: as of the last delivered step
    double frozen_score = 0.0, best_score = 0.0;
    bool recs;
    void restart() { for (auto& p : path) p.clear(); std::fill(alive.begin(), alive.end(), 0); alive[0] = 1; }
};
struct Hyp { Path p; double score; };

// the expected result of a step, spelled out: alive slots of the mask by score descending, then slot ascending
static std::vector<Hyp> expected(const Plain& M, const double* sc, unsigned mask) {
    std::vector<int> left;
    for (int j = 0; j < M.W; ++j)
        if ((mask >> j) & 1) left.push_back(j);
    std::vector<Hyp> out;
    while (!left.empty()) {
        size_t at = 0;
        for (size_t i = 1; i < left.size(); ++i)
            if (sc[left[i]] > sc[left[at]]) at = i;        // (left is slot-ascending: the first of equal scores wins)
        Hyp h{M.frozen, M.frozen_score + sc[left[at]]};
        h.p.insert(h.p.end(), M.path[left[at]].begin(), M.path[left[at]].end());
        out.push_back(h);
        left.erase(left.begin() + at);
    }
    return out;
}

struct Counts { int steps = 0, ties = 0, single = 0, none = 0, freezes = 0, forgets = 0, toggles = 0, max_queued = 0, after_freeze = 0; };

static int beam(int W, bool recs0, unsigned seed, Counts& n) {
    std::mt19937 rng(seed);
    BeamSlot A, P;                                         // A: built and delivered at once; P: built, queued, delivered later
    bh_reset(A.tree, W); bh_reset(P.tree, W);
    SlotResult RA, RP;
    Plain M;
    M.W = W; M.path.assign(W, {}); M.alive.assign(W, 0); M.recs = false; M.restart();
    std::deque<std::pair<SlotResult, TokList>> snaps;       // what A delivered (the slot's result, A.best), oldest first
    int frame = 0;
    auto set_records = [&](bool on) {
        A.set_records(on); P.set_records(on);
        M.recs = on;
        for (auto* q : {&M.frozen, &M.best}) for (auto& t : *q) { t.frame = -1; t.logp = 0.f; }
        for (auto& p : M.path) for (auto& t : p) { t.frame = -1; t.logp = 0.f; }
    };
    auto invariants = [&](const BeamSlot& B) {
        const size_t nodes = M.recs ? B.tree.par.size() : 0;
        return B.tree.frame.size() == nodes && B.tree.logp.size() == nodes && B.frozen.recs.size() == (M.recs ? B.frozen.tokens.size() : 0) &&
               B.best.recs.size() == (M.recs ? B.best.tokens.size() : 0);
    };
    auto drain = [&]() -> int {                            // the pipelined protocol collects: every field as the synchronous one had it
        while (!P.steps.empty()) {
            P.deliver(std::move(P.steps.front()), RP);
            P.steps.pop_front();
            CHECK(same(RP, snaps.front().first), "queued-then-delivered differs from delivered-at-once");
            CHECK(same(P.best, snaps.front().second), "best state differs between the protocols");
            snaps.pop_front();
            if (rng() % 2) { int got; std::vector<int32_t> t(RP.need() + 1); CHECK(RP.take(t.data(), nullptr, nullptr, RP.need(), &got), "fetch"); }
        }
        CHECK(snaps.empty() && same(P.frozen, A.frozen) && P.frozen_score == A.frozen_score, "protocols out of step");
        return 0;
    };
    auto fetch_all = [&]() { int got; std::vector<int32_t> t(RA.need() + RP.need() + 1);
                             (void)RA.take(t.data(), nullptr, nullptr, RA.need(), &got); (void)RP.take(t.data(), nullptr, nullptr, RP.need(), &got); };
    if (recs0) set_records(true);
    // a freeze with nothing decoded
    A.freeze(-RA.neg_logp); P.freeze(-RP.neg_logp);
    CHECK(A.frozen.tokens.empty() && A.frozen_score == 0.0 && invariants(A), "freeze with nothing decoded");
    int since_freeze = -1;                                 // steps delivered since the last freeze (-1: none yet)
    for (int round = 0; round < 3000; ++round) {
        const unsigned op = rng() % 100;
        if (op < 70) {                                     // a selection round
            if (rng() % 3 == 0) ++frame;
            std::vector<int> live;
            for (int j = 0; j < W; ++j)
                if (M.alive[j]) live.push_back(j);
            int e[8];
            BeamRec rec[8];
            std::vector<Path> next(W);
            std::vector<char> nalive(W, 0);
            for (int j = 0; j < W; ++j) {
                rec[j] = BeamRec{-77, -77.f};              // stale where the slot is not extended
                if (rng() % 7 == 0 && j > 0) { e[j] = -2; continue; }
                const int p = live[rng() % live.size()];
                const int tok = (rng() % 5 < 2) ? 1 + (int)(rng() % 2047) : 0;
                e[j] = (p << 16) | tok;
                next[j] = M.path[p];
                nalive[j] = 1;
                if (tok) {
                    const float lp = -(float)(rng() % 100000) / 1000.f;
                    rec[j] = BeamRec{frame, lp};
                    next[j].push_back(Tok{tok - 1, frame, lp});
                }
            }
            bh_apply(A.tree, e, W, M.recs ? rec : nullptr, 0, 300);
            bh_apply(P.tree, e, W, M.recs ? rec : nullptr, 0, 300);
            M.path.swap(next); M.alive.swap(nalive);
        } else if (op < 88) {                              // the end of a model step
            unsigned all = 0, mask;
            for (int j = 0; j < W; ++j) all |= (unsigned)(M.alive[j] != 0) << j;
            const unsigned kind = rng() % 8;
            if (kind == 0) mask = 0;
            else if (kind == 1) { int j; do j = rng() % W; while (!M.alive[j]); mask = 1u << j; }
            else mask = all;
            double sc[8];
            const bool coarse = rng() % 2;                 // coarse: a few values only, so that scores are equal
            for (int j = 0; j < W; ++j) sc[j] = coarse ? -0.25 * (double)(rng() % 3) : -(double)(rng() % 1000000) / 1000.0;
            const std::vector<Hyp> exp = expected(M, sc, mask);
            n.none += exp.empty(); n.single += exp.size() == 1; n.ties += exp.size() > 1 && exp[0].score == exp[1].score;
            BeamStep st = A.build(sc, mask, M.recs);
            P.steps.push_back(P.build(sc, mask, M.recs));
            n.max_queued = std::max(n.max_queued, (int)P.steps.size());
            CHECK(st.nbest.size() == (M.recs ? exp.size() : 0), "number of hypotheses");
            for (size_t i = 0; i < st.nbest.size(); ++i) {
                CHECK(same(st.nbest[i], exp[i].p, true) && st.nbest[i].score == exp[i].score, "hypothesis (order: score descending, slot ascending)");
                CHECK(i == 0 || st.nbest[i - 1].score >= st.nbest[i].score, "scores not descending");
                CHECK(st.nbest[i].tokens.size() >= M.frozen.size() && std::equal(M.frozen.begin(), M.frozen.end(), exp[i].p.begin(),
                      [](const Tok& a, const Tok& b) { return a.tok == b.tok && a.frame == b.frame && a.logp == b.logp; }), "frozen prefix");
            }
            A.deliver(std::move(st), RA);
            const Path& best = exp.empty() ? M.frozen : exp[0].p;
            const double score = exp.empty() ? M.frozen_score : exp[0].score;
            CHECK(RA.tokens.size() == best.size() && RA.recs.empty(), "delivered queue");
            for (size_t i = 0; i < best.size(); ++i) CHECK(RA.tokens[i] == best[i].tok, "delivered queue is not hypothesis 0");
            CHECK(RA.neg_logp == -score && RA.align == 0.0, "neg_logp is not minus the score of hypothesis 0");
            CHECK(RA.nbest.size() == (M.recs ? exp.size() : 0), "delivered beam");
            if (!RA.nbest.empty()) CHECK(RA.nbest[0].tokens == RA.tokens && RA.nbest[0].score == -RA.neg_logp, "hypothesis 0 against the queue");
            if (exp.empty()) CHECK(same(A.best, M.frozen, M.recs) && RA.nbest.empty(), "no slot alive: not the frozen prefix alone");
            CHECK(same(A.best, best, M.recs), "best state after the delivery");
            M.best = best; M.best_score = score;
            snaps.emplace_back(RA, A.best);
            if (rng() % 2) fetch_all();                    // (the records of hypothesis 0 must outlive the fetch)
            ++n.steps;
            if (since_freeze >= 0) { ++since_freeze; n.after_freeze += !exp.empty(); }
        } else if (op < 94) {
            if (drain()) return 1;
        } else if (op < 97) {                              // a predictor reset freezes the best hypothesis (everything collected first)
            if (drain()) return 1;
            for (int twice = rng() % 3 == 0 ? 2 : 1; twice > 0; --twice) {
                A.freeze(-RA.neg_logp); P.freeze(-RP.neg_logp);
                M.frozen = M.best; M.frozen_score = M.best_score; M.restart();
                CHECK(same(A.frozen, M.frozen, M.recs) && A.frozen_score == M.frozen_score && same(A.best, M.best, M.recs), "freeze");
                CHECK(A.tree.par.empty() && A.tree.cur == std::vector<int>(W, -1), "freeze: the beam did not restart");
            }
            ++n.freezes; since_freeze = 0;
        } else if (op < 98) {                              // the transcript starts over
            if (drain()) return 1;
            for (auto* r : {&RA, &RP}) { r->clear(); r->neg_logp = 0.0; }
            A.forget(); P.forget();
            M.frozen.clear(); M.best.clear(); M.frozen_score = M.best_score = 0.0; M.restart();
            for (const BeamSlot* B : {&A, &P})
                CHECK(B->frozen.tokens.empty() && B->frozen.recs.empty() && B->best.tokens.empty() && B->best.recs.empty() && B->frozen_score == 0.0 &&
                      B->tree.par.empty() && B->tree.tok.empty() && B->tree.frame.empty() && B->tree.logp.empty() && B->steps.empty() &&
                      B->tree.cur == std::vector<int>(W, -1), "forget left something");
            CHECK(!RA.unfetched() && !RP.unfetched(), "forget: result not cleared");
            ++n.forgets;
        } else {                                           // the records are switched (idle engine, everything fetched)
            if (drain()) return 1;
            fetch_all();
            set_records(!M.recs);
            if (M.recs) {
                for (const BeamSlot* B : {&A, &P}) {
                    CHECK(same(B->frozen, M.frozen, true) && same(B->best, M.best, true), "switch-on: prefixes not padded with (-1, 0)");
                    for (size_t i = 0; i < B->tree.par.size(); ++i) CHECK(B->tree.frame[i] == -1 && B->tree.logp[i] == 0.f, "switch-on: nodes not padded");
                }
            } else {
                for (const BeamSlot* B : {&A, &P})
                    CHECK(B->tree.frame.empty() && B->tree.logp.empty() && B->frozen.recs.empty() && B->best.recs.empty(), "switch-off left records");
            }
            ++n.toggles;
        }
        CHECK(invariants(A) && invariants(P), "record vectors not parallel to the tokens");
    }
    return drain();
}

int main() {
    unsigned seed = 1;
    for (int recs = 0; recs < 2; ++recs)
        for (int rep = 0; rep < 3; ++rep)
            if (greedy(recs != 0, seed++)) return 1;
    Counts n;
    for (int W : {2, 3, 8})
        for (int recs = 0; recs < 2; ++recs)
            for (int rep = 0; rep < 4; ++rep) {
                Counts c;
                if (beam(W, recs != 0, seed++, c)) { std::printf("results_check: (beam W=%d records %d at the start, seed %u)\n", W, recs, seed - 1); return 1; }
                n.steps += c.steps; n.ties += c.ties; n.single += c.single; n.none += c.none; n.freezes += c.freezes; n.forgets += c.forgets;
                n.toggles += c.toggles; n.max_queued = std::max(n.max_queued, c.max_queued); n.after_freeze += c.after_freeze;
            }
    if (n.ties < 50 || n.single < 50 || n.none < 50 || n.freezes < 50 || n.forgets < 10 || n.toggles < 20 || n.max_queued < 4 || n.after_freeze < 100) {
        std::printf("results_check: FAILED (a case was not exercised: %d steps, %d ties, %d single, %d none, %d freezes, %d forgets, %d toggles, "
                    "%d queued, %d after a freeze)\n", n.steps, n.ties, n.single, n.none, n.freezes, n.forgets, n.toggles, n.max_queued, n.after_freeze);
        return 1;
    }
    std::printf("results_check: ok (%d steps: %d with equal best scores, %d with one slot alive, %d with none; %d freezes, %d forgets, %d switches, "
                "up to %d steps queued)\n", n.steps, n.ties, n.single, n.none, n.freezes, n.forgets, n.toggles, n.max_queued);
    return 0;
}
