// lasr_lattice_tables.hip.h -- the per-call tables of the lattice family: what a call's layout is (offsets and
// sizes from its T / U / W or T / N) and how its arrays become ONE buffer of 8-byte words that goes to the device in one copy.
// Standard C++ only, no HIP include and no context (the name follows the unit's other headers so that the build tracks it): the
// engine includes it ahead of lasr_lattice.hip.h, tests/c/lattice_tables_check.cpp on its own.
//
// TabImage: every array is appended with the address of the pointer that is to view it; bind(base) then points each of them at its
// array inside a copy of the image at base.  No offset is ever written by hand.  64-bit arrays first, then 32-bit ones, keeps the
// image dense; a 64-bit array always starts on an 8-byte boundary and the image ends on one (zero padding).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace lasr {

constexpr int LAT_BP_WORDS = 4096; // back-pointer words a workgroup keeps in LDS (131 072 cells of an utterance); larger: global

struct TabImage {
    struct View { void* field; size_t at, bytes; };   // field: a const T*; at: byte offset of its array in the image
    std::vector<long long> words;
    std::vector<View> views;
    size_t end32 = 0;                                 // 4-byte units in use
    void clear() { words.clear(); views.clear(); end32 = 0; }
    // n entries from p (null: zeros), to be viewed by *field
    template <class T> void put(const T** field, const T* p, size_t n) {
        static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- and 64-bit entries");
        size_t at;
        if (sizeof(T) == 8) { at = 8 * words.size(); words.resize(words.size() + n, 0); end32 = 2 * words.size(); }
        else { at = 4 * end32; end32 += n; words.resize((end32 + 1) / 2, 0); }
        if (p && n) memcpy((char*)words.data() + at, p, sizeof(T) * n);
        views.push_back(View{(void*)field, at, sizeof(T) * n});
    }
    void bind(const void* base) const {
        for (const View& v : views) { const char* p = (const char*)base + v.at; memcpy(v.field, &p, sizeof p); }
    }
};

// ---- full and banded lattice: cell = off_i + t row_i + k, row_i = U_i + 1 (full, k = u) or W_i (band, u = lo[t] + k)
struct LatTab {                    // per-call tables (device), one entry per utterance
    const long long* off;          // [n + 1] first cell
    const long long* bp_off;       // [n] first global back-pointer word (utterances that exceed the LDS share)
    const int* T;                  // [n] frames
    const int* U;                  // [n] labels
    const int* slot;               // [n] batch row of the utterance
    const int* tok_off;            // [n] first label in tok
    const int* tok;                // [sum U]
    const int* W;                  // [n] window width                        (band only; null for the full lattice)
    const int* lo_off;             // [n] first frame in lo
    const int* lo;                 // [sum T] window starts
    int n;
};
struct LatCall {                   // host side of a call: T / U / slot (and W / lo for a band) are the caller's, the rest lat_layout's
    int n = 0;
    std::vector<int> T, U, W, slot;                   // W empty: the full lattice
    std::vector<int32_t> lo;                          // [sum T] the windows of the pass
    std::vector<int> tok_off, lo_off;
    std::vector<long long> off, bp_off;
    long long cells = 0, sumU = 0, sumT = 0, bp_words = 0;
    int Umax = 0, Wmax = 0, lds_bp_words = 0;         // Wmax: the widest row; lds_bp_words: of the utterances that fit in LDS
    LatTab tab{};                                     // device views (lat_pack + TabImage::bind)
    int row(int i) const { return W.empty() ? U[i] + 1 : W[i]; }
};
inline void lat_layout(LatCall& k) {
    const int n = k.n;
    k.off.assign(n + 1, 0); k.tok_off.assign(n, 0); k.lo_off.assign(n, 0); k.bp_off.assign(n, 0);
    k.cells = k.sumU = k.sumT = k.bp_words = 0; k.Umax = k.Wmax = k.lds_bp_words = 0;
    for (int i = 0; i < n; ++i) {
        k.off[i] = k.cells; k.tok_off[i] = (int)k.sumU; k.lo_off[i] = (int)k.sumT;
        const long long ci = (long long)k.T[i] * k.row(i), wi = (ci + 31) >> 5;
        k.bp_off[i] = k.bp_words;
        if (wi > LAT_BP_WORDS) k.bp_words += wi; else k.lds_bp_words = std::max(k.lds_bp_words, (int)wi);
        k.cells += ci; k.sumU += k.U[i]; k.sumT += k.T[i];
        k.Umax = std::max(k.Umax, k.U[i]); k.Wmax = std::max(k.Wmax, k.row(i));
    }
    k.off[n] = k.cells;
}
// tok may be null (the dynamic programmes alone read no labels)
inline void lat_pack(LatCall& k, const int32_t* tok, TabImage& img) {
    const size_t n = (size_t)k.n;
    LatTab& t = k.tab;
    t = LatTab{}; t.n = k.n;
    img.clear();
    img.put(&t.off, k.off.data(), n + 1); img.put(&t.bp_off, k.bp_off.data(), n);
    img.put(&t.T, k.T.data(), n); img.put(&t.U, k.U.data(), n); img.put(&t.slot, k.slot.data(), n);
    img.put(&t.tok_off, k.tok_off.data(), n); img.put(&t.tok, tok, (size_t)k.sumU);
    if (k.W.empty()) return;
    img.put(&t.W, k.W.data(), n); img.put(&t.lo_off, k.lo_off.data(), n); img.put(&t.lo, k.lo.data(), (size_t)k.sumT);
}

// ---- prefix tree: cell = off_i + t N_i + v
struct TreeTab {                   // per-call tables (device)
    const long long* off;          // [n + 1] first cell of the utterance
    const int* T;                  // [n] frames
    const int* N;                  // [n] nodes
    const int* node_off;           // [n] first node in the per-node arrays (and in the results)
    const int* enc_row;            // [n] batch row that holds the utterance's encoder output
    const int* ds_off;             // [n] first entry in dstart
    const int* parent;             // per node (utterance-local ids): parent, -1 at the root
    const int* label;              //   the label that enters the node
    const int* depth;              //   labels of the prefix
    const int* row;                //   batch row of the lowest candidate that passes through the node (its lat_pp column)
    const int* child_lo;           //   first child
    const int* child_n;            //   children
    const int* dstart;             // per utterance [depth_max + 2]: first node of each depth, then N
    int n;
};
struct TreeCall {
    int n = 0;
    std::vector<int> T, N, enc_row;
    std::vector<int> parent, label, depth, row;      // per node, utterances concatenated (label / row may stay empty: the DP alone)
    std::vector<long long> off;
    std::vector<int> node_off;
    long long cells = 0, nodes = 0;
    int Nmax = 0;
    TreeTab tab{};
    // full: a lasr_score_* call (every table); otherwise the DP alone on caller-supplied parents: label / row / enc_row stay zero and
    // child_lo / child_n mean nothing there (children need not be contiguous) -- k_lat_dp_tree reads none of them
    bool sizes_ok() const {
        const size_t nn = (size_t)nodes;
        const bool full = !label.empty() || !row.empty() || !enc_row.empty();
        return T.size() == (size_t)n && N.size() == (size_t)n && parent.size() == nn && depth.size() == nn &&
               (!full || (label.size() == nn && row.size() == nn && enc_row.size() == (size_t)n));
    }
};
inline void tree_layout(TreeCall& k) {
    const int n = k.n;
    k.off.assign(n + 1, 0); k.node_off.assign(n, 0);
    k.cells = 0; k.nodes = 0; k.Nmax = 0;
    for (int i = 0; i < n; ++i) {
        k.off[i] = k.cells; k.node_off[i] = (int)k.nodes;
        k.cells += (long long)k.T[i] * k.N[i]; k.nodes += k.N[i]; k.Nmax = std::max(k.Nmax, k.N[i]);
    }
    k.off[n] = k.cells;
}
// behind tree_layout, sizes_ok() holds; parent / depth are valid (lasr_prefix_tree's contract)
inline void tree_pack(TreeCall& k, TabImage& img) {
    const size_t n = (size_t)k.n, nn = (size_t)k.nodes;
    std::vector<int> ds_off(n), child_lo(nn, 0), child_n(nn, 0), dstart;
    for (size_t i = 0; i < n; ++i) {
        const int no = k.node_off[i], Ni = k.N[i];
        for (int v = 1; v < Ni; ++v) {
            const int p = no + k.parent[no + v];
            if (child_n[p]++ == 0) child_lo[p] = v;
        }
        ds_off[i] = (int)dstart.size();
        for (int v = 0; v < Ni; ++v)
            if (v == 0 || k.depth[no + v] != k.depth[no + v - 1]) dstart.push_back(v);
        dstart.push_back(Ni);
    }
    auto opt = [](const std::vector<int>& a) { return a.empty() ? nullptr : a.data(); };
    TreeTab& t = k.tab;
    t = TreeTab{}; t.n = k.n;
    img.clear();
    img.put(&t.off, k.off.data(), n + 1);
    img.put(&t.T, k.T.data(), n); img.put(&t.N, k.N.data(), n); img.put(&t.node_off, k.node_off.data(), n);
    img.put(&t.enc_row, opt(k.enc_row), n); img.put(&t.ds_off, ds_off.data(), n);
    img.put(&t.parent, k.parent.data(), nn); img.put(&t.label, opt(k.label), nn); img.put(&t.depth, k.depth.data(), nn);
    img.put(&t.row, opt(k.row), nn); img.put(&t.child_lo, child_lo.data(), nn); img.put(&t.child_n, child_n.data(), nn);
    img.put(&t.dstart, dstart.data(), dstart.size());
}

}  // namespace lasr
