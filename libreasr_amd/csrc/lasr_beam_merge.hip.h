// lasr_beam_merge.hip.h -- beam search: hypotheses that hold the same tokens are merged (lasr_set_beam_merge).
// A hypothesis's identity is (len, hash) of its token list since the stream's last predictor reset: the empty list is
// (0, BM_SEED), appending token v gives (len + 1, bm_mix(hash ^ (v + 1))).  bm_mix is the splitmix64 finaliser, a bijection: the
// extensions of one parent by different tokens never share a hash.  The first part is plain C++ (the host computes the identities
// of a running stream at switch-on: lasr_engine.hip); the device routine below is what wave 0 of k_beam_select_rw<WT, REC, true>
// calls between the selection of a round's W survivors and their stores; beam_merge_repicked behind it is k_beam_fuse_merge's.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define BM_HD __host__ __device__ __forceinline__
#else
#define BM_HD inline
#endif

constexpr uint64_t BM_SEED = 0x9E3779B97F4A7C15ull;
BM_HD uint64_t bm_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
BM_HD uint64_t bm_append(uint64_t hash, int token) { return bm_mix(hash ^ (uint64_t)(int64_t)(token + 1)); }

#if defined(__HIPCC__)
// log(exp(a) + exp(b)) in double; both finite (scores of live slots)
__device__ __forceinline__ double bm_lae(double a, double b) {
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    return hi + log1p(exp(lo - hi));
}
__device__ __forceinline__ uint64_t bm_readlane64(uint64_t x, int l) {
    return ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(x >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l);
}
__device__ __forceinline__ double bm_readlane_f64(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// The merge step of one round, by the whole of wave 0 (every lane calls; lanes >= W hold live = false).
//   in:  lane j < W holds slot j's survivor -- live, sel (its score), sord (its ordinal: parent slot * (V + 1) + 0 carried | 1 + token)
//        -- and, in own_hash / own_len, the identity slot j had at the START of the round (loaded before anything is stored).
//   The parent's identity comes from the parent's lane (its registers still hold the round's start: nothing has been stored), the
//   new identity is derived from it, and the live survivors are grouped by (len, hash, inB).  In a group the lowest lane survives
//   with the fold of the group's scores in ascending lane order; every other member leaves as a dead slot: live = false, sel = -inf.
//   out: live / sel as above; the slot's new identity is stored (a dead slot: the empty identity).
// Each lane stores its own slot's identity only, after it has read it, so the stores need no ordering among the lanes; they sit
// in front of lane 0's publish() like every other store of the round.
template <int WT>
__device__ __forceinline__ void beam_merge_round(const int lane, const int W, const int V, const int blank, const bool at_cap,
                                                 const uint64_t own_hash, const int own_len, const int sord, bool& live, double& sel,
                                                 unsigned long long* __restrict__ hash_row, int* __restrict__ len_row) {
    const int pb = live ? sord / (V + 1) : 0, k = live ? sord - pb * (V + 1) : 0;
    const bool em = live && k > 0 && k - 1 != blank;
    const int inb = (em && !at_cap) ? 0 : 1;
    // the parent's identity: pb differs per lane -- every slot's identity is broadcast in turn, a lane keeps its parent's
    uint64_t ph = BM_SEED;
    int pl = 0;
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        const uint64_t h = bm_readlane64(own_hash, j);
        const int l = __builtin_amdgcn_readlane(own_len, j);
        if (pb == j) { ph = h; pl = l; }
    }
    uint64_t nh = BM_SEED;
    int nl = 0;
    if (live) { nh = em ? bm_append(ph, k - 1) : ph; nl = pl + (em ? 1 : 0); }
    // groups: lane j's key is broadcast in turn; a lower live lane with my key takes me in, a higher one is folded into my score
    // (ascending j: the fold's order).  lae runs only in rounds that merge something (wave-uniform test).
    const double own_sel = sel;
    double acc = sel;
    bool gone = false;
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        const uint64_t h = bm_readlane64(nh, j);
        const int l = __builtin_amdgcn_readlane(nl, j);
        const int fl = __builtin_amdgcn_readlane((live ? 2 : 0) | inb, j);
        const double sc = bm_readlane_f64(own_sel, j);
        const bool same = live && j != lane && (fl & 2) && (fl & 1) == inb && l == nl && h == nh;
        if (__ballot(same) == 0ull) continue;
        if (same && j < lane) gone = true;
        if (same && j > lane) acc = bm_lae(acc, sc);
    }
    if (gone) { live = false; nh = BM_SEED; nl = 0; }
    sel = live ? acc : -INFINITY;
    if (lane < W) { hash_row[lane] = nh; len_row[lane] = nl; }
}

// The same step for k_beam_fuse_merge (merging under LM fusion, LASR_BEAM_MERGE_LM), which runs BEHIND the selection
// kernel and the fuser's re-pick: the survivor comes as the selection kernel stored it -- pb (its parent slot), em (extended by a
// non-blank token), inb (its state on the frame after the round) -- with tok = the token the slot carries after the re-pick.
// Everything else as above.  (A routine of its own, not beam_merge_round's core: k_beam_select_rw<WT, REC, true> keeps the
// instruction stream it had.)
template <int WT>
__device__ __forceinline__ void beam_merge_repicked(const int lane, const int W, const int pb, const bool em, const int tok, const int inb,
                                                    const uint64_t own_hash, const int own_len, bool& live, double& sel,
                                                    unsigned long long* __restrict__ hash_row, int* __restrict__ len_row) {
    uint64_t ph = BM_SEED;
    int pl = 0;
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        const uint64_t h = bm_readlane64(own_hash, j);
        const int l = __builtin_amdgcn_readlane(own_len, j);
        if (pb == j) { ph = h; pl = l; }
    }
    uint64_t nh = BM_SEED;
    int nl = 0;
    if (live) { nh = em ? bm_append(ph, tok) : ph; nl = pl + (em ? 1 : 0); }
    const double own_sel = sel;
    double acc = sel;
    bool gone = false;
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        const uint64_t h = bm_readlane64(nh, j);
        const int l = __builtin_amdgcn_readlane(nl, j);
        const int fl = __builtin_amdgcn_readlane((live ? 2 : 0) | inb, j);
        const double sc = bm_readlane_f64(own_sel, j);
        const bool same = live && j != lane && (fl & 2) && (fl & 1) == inb && l == nl && h == nh;
        if (__ballot(same) == 0ull) continue;
        if (same && j < lane) gone = true;
        if (same && j > lane) acc = bm_lae(acc, sc);
    }
    if (gone) { live = false; nh = BM_SEED; nl = 0; }
    sel = live ? acc : -INFINITY;
    if (lane < W) { hash_row[lane] = nh; len_row[lane] = nl; }
}
#endif
