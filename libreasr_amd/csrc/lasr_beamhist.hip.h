// lasr_beamhist.hip.h -- host side of the beam: the hypotheses of one stream as a shared-prefix tree, replayed from the words
// (and, with lasr_set_beam_records, the records) k_beam_select_rw publishes per selection round.
// Standard C++ only, no HIP include (the name follows the unit's other headers so that the build tracks it): the engine includes it
// through lasr_ctx.hip.h, tests/c/beamhist_check.cpp on its own.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// what k_beam_select_rw stores beside the trellis word of a slot it extended by a non-blank token (BeamState::rec)
struct BeamRec { int32_t frame; float logp; };

// a round re-parents W slots: copying W token vectors per round grows with the length of the stream; a node per emitted token
// does not.  frame / logp run parallel to par / tok while records are on and are EMPTY while they are off (nodes created before a
// switch-on are padded with frame -1, log p 0: lasr_set_beam_records).
struct BeamHost {
    std::vector<int> par, tok;
    std::vector<int32_t> frame;
    std::vector<float> logp;
    std::vector<int> cur;
};

constexpr size_t BH_COMPACT_AT = (size_t)1 << 18;    // nodes above which bh_apply rebuilds the tree from its live hypotheses

inline void bh_reset(BeamHost& B, int W) { B.par.clear(); B.tok.clear(); B.frame.clear(); B.logp.clear(); B.cur.assign(W, -1); }
inline void bh_tokens(const BeamHost& B, int node, std::vector<int32_t>& out) {      // appends root -> leaf
    const size_t at = out.size();
    for (int n = node; n >= 0; n = B.par[n]) out.push_back(B.tok[n]);
    std::reverse(out.begin() + at, out.end());
}
// records of the same path, parallel to bh_tokens (records on)
inline void bh_records(const BeamHost& B, int node, std::vector<BeamRec>& out) {
    const size_t at = out.size();
    for (int n = node; n >= 0; n = B.par[n]) out.push_back(BeamRec{B.frame[n], B.logp[n]});
    std::reverse(out.begin() + at, out.end());
}
// one selection round of a stream: e[j] = (parent slot << 16) | (token + 1 if extended else 0); -2 dead slot.
// rec (records on, else null): rec[j] is valid where slot j was extended; its frame is the kernel's cursor, frame_add maps it to
// the slot's own count.
inline void bh_apply(BeamHost& B, const int* e, int W, const BeamRec* rec = nullptr, long long frame_add = 0,
                     size_t compact_at = BH_COMPACT_AT) {
    int nh[8];
    for (int j = 0; j < W; ++j) {
        if (e[j] < 0) { nh[j] = -1; continue; }
        const int p = B.cur[e[j] >> 16], tok = e[j] & 0xffff;
        if (tok) {
            B.par.push_back(p); B.tok.push_back(tok - 1); nh[j] = (int)B.par.size() - 1;
            if (rec) { B.frame.push_back((int32_t)(rec[j].frame + frame_add)); B.logp.push_back(rec[j].logp); }
        } else nh[j] = p;
    }
    for (int j = 0; j < W; ++j) B.cur[j] = nh[j];
    if (B.par.size() > compact_at) {                // compaction: keep the live hypotheses only
        const bool recs = B.frame.size() == B.par.size();
        std::vector<std::vector<int32_t>> live(W);
        std::vector<std::vector<BeamRec>> lrec(W);
        for (int j = 0; j < W; ++j) {
            bh_tokens(B, B.cur[j], live[j]);
            if (recs) bh_records(B, B.cur[j], lrec[j]);
        }
        B.par.clear(); B.tok.clear(); B.frame.clear(); B.logp.clear();
        for (int j = 0; j < W; ++j) {
            int n = -1;
            for (size_t i = 0; i < live[j].size(); ++i) {
                B.par.push_back(n); B.tok.push_back(live[j][i]); n = (int)B.par.size() - 1;
                if (recs) { B.frame.push_back(lrec[j][i].frame); B.logp.push_back(lrec[j][i].logp); }
            }
            B.cur[j] = n;
        }
    }
}
