// lattice_tables_check.cpp -- libreasr_amd/csrc/lasr_lattice_tables.hip.h (layout and table image of the lattice family, standard C++
// only) under AddressSanitizer + UndefinedBehaviorSanitizer.  For the full, the banded and the tree layout, over n = 1 and 3 with
// U in {0, 1, 7}, T in {1, 2, 9}, odd and even totals of 32-bit entries, a single-node tree and a chain, and an utterance whose
// back-pointer words exceed LAT_BP_WORDS beside one that fits: every view lies inside the image, no two overlap, 64-bit views are
// 8-byte aligned, each view reads back its input, and the layout equals formulas written out here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libreasr_amd/csrc/lasr_lattice_tables.hip.h"

using namespace lasr;

#define CHECK(x) do { if (!(x)) { std::printf("lattice_tables_check: FAILED %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static int n_odd = 0, n_even = 0;                     // images whose 32-bit entries were an odd / even total

// the image bound to a copy of itself at `base` (exact size: a view past the end is a heap overflow): geometry of the views
static int check_geometry(const TabImage& img, size_t n64_views) {
    const size_t bytes = 8 * img.words.size();
    size_t used = 0, used32 = 0;
    for (size_t a = 0; a < img.views.size(); ++a) {
        const TabImage::View& v = img.views[a];
        CHECK(v.at + v.bytes <= bytes);
        CHECK(v.at % 4 == 0);
        if (a < n64_views) CHECK(v.at % 8 == 0 && v.bytes % 8 == 0);
        else used32 += v.bytes / 4;
        for (size_t b = 0; b < a; ++b) {
            const TabImage::View& o = img.views[b];
            CHECK(v.bytes == 0 || o.bytes == 0 || v.at + v.bytes <= o.at || o.at + o.bytes <= v.at);
        }
        used += v.bytes;
    }
    CHECK(bytes - used == (used32 % 2 ? 4u : 0u));   // dense: nothing but the padding word is unused
    (used32 % 2 ? n_odd : n_even)++;
    return 0;
}
template <class T> static bool same(const T* view, const std::vector<T>& want) {
    return want.empty() || memcmp(view, want.data(), sizeof(T) * want.size()) == 0;
}

// T / U / W (W empty: the full lattice) of one call
static int lattice_case(const std::vector<int>& T, const std::vector<int>& U, const std::vector<int>& W) {
    const int n = (int)T.size();
    const bool band = !W.empty();
    LatCall k;
    k.n = n; k.T = T; k.U = U; k.W = W;
    for (int i = 0; i < n; ++i) k.slot.push_back(2 * i + 1);
    lat_layout(k);
    // the layout, restated
    long long cells = 0, sumU = 0, sumT = 0, bp_words = 0;
    int lds_bp = 0, Umax = 0, Wmax = 0;
    CHECK(k.off.size() == (size_t)n + 1 && k.tok_off.size() == (size_t)n && k.lo_off.size() == (size_t)n && k.bp_off.size() == (size_t)n);
    for (int i = 0; i < n; ++i) {
        const int row = band ? W[i] : U[i] + 1;
        const long long ci = (long long)T[i] * row, words = ci / 32 + (ci % 32 != 0);
        CHECK(k.off[i] == cells && k.tok_off[i] == sumU && k.lo_off[i] == sumT && k.bp_off[i] == bp_words);
        if (words > LAT_BP_WORDS) bp_words += words;
        else if (words > lds_bp) lds_bp = (int)words;
        cells += ci; sumU += U[i]; sumT += T[i];
        if (U[i] > Umax) Umax = U[i];
        if (row > Wmax) Wmax = row;
    }
    CHECK(k.off[n] == cells && k.cells == cells && k.sumU == sumU && k.sumT == sumT && k.bp_words == bp_words);
    CHECK(k.lds_bp_words == lds_bp && k.Umax == Umax && k.Wmax == Wmax);
    std::vector<int32_t> tok((size_t)sumU);
    for (size_t j = 0; j < tok.size(); ++j) tok[j] = 100 + (int32_t)j;
    if (band) for (long long j = 0; j < sumT; ++j) k.lo.push_back(1000 + (int32_t)j);
    for (int with_tok = 0; with_tok < 2; ++with_tok) {
        TabImage img;
        lat_pack(k, with_tok ? tok.data() : nullptr, img);
        CHECK(img.views.size() == (band ? 10u : 7u));
        if (check_geometry(img, 2)) return 1;
        std::vector<long long> dev(img.words);        // "the device": an exact-size copy
        img.bind(dev.data());
        const LatTab& t = k.tab;
        CHECK(t.n == n && same(t.off, k.off) && same(t.bp_off, k.bp_off));
        CHECK(same(t.T, T) && same(t.U, U) && same(t.slot, k.slot) && same(t.tok_off, k.tok_off));
        CHECK(same(t.tok, with_tok ? tok : std::vector<int32_t>((size_t)sumU, 0)));
        if (band) CHECK(same(t.W, W) && same(t.lo_off, k.lo_off) && same(t.lo, k.lo));
        else CHECK(!t.W && !t.lo_off && !t.lo);
        CHECK((const char*)t.off == (const char*)dev.data());
    }
    return 0;
}

// trees given as parent lists (utterance-local, parent[0] = -1, depth non-decreasing, children contiguous)
static int tree_case(const std::vector<int>& T, const std::vector<std::vector<int>>& parents, bool full) {
    const int n = (int)T.size();
    TreeCall k;
    k.n = n; k.T = T;
    std::vector<int> want_child_lo, want_child_n, want_dstart, want_ds_off;
    long long cells = 0, nodes = 0;
    int Nmax = 0;
    std::vector<long long> want_off;
    std::vector<int> want_node_off;
    for (int i = 0; i < n; ++i) {
        const std::vector<int>& p = parents[i];
        const int N = (int)p.size();
        k.N.push_back(N);
        want_off.push_back(cells); want_node_off.push_back((int)nodes);
        std::vector<int> depth(N, 0);
        for (int v = 1; v < N; ++v) depth[v] = depth[p[v]] + 1;
        want_ds_off.push_back((int)want_dstart.size());
        for (int v = 0; v < N; ++v) {
            k.parent.push_back(p[v]); k.depth.push_back(depth[v]);
            if (full) { k.label.push_back(50 + v); k.row.push_back(3 * i + v % 3); }
            int first = 0, count = 0;                 // the children of v, counted directly
            for (int c = N - 1; c > v; --c) if (p[c] == v) { first = c; ++count; }
            want_child_lo.push_back(first); want_child_n.push_back(count);
            int before = 0;                           // v opens a depth iff no earlier node has its depth
            for (int x = 0; x < v; ++x) before += depth[x] == depth[v];
            if (!before) want_dstart.push_back(v);
        }
        want_dstart.push_back(N);
        if (full) k.enc_row.push_back(7 * i);
        cells += (long long)T[i] * N; nodes += N;
        if (N > Nmax) Nmax = N;
    }
    want_off.push_back(cells);
    tree_layout(k);
    CHECK(k.off == want_off && k.node_off == want_node_off && k.cells == cells && k.nodes == nodes && k.Nmax == Nmax && k.sizes_ok());
    TabImage img;
    tree_pack(k, img);
    CHECK(img.views.size() == 13u);
    if (check_geometry(img, 1)) return 1;
    std::vector<long long> dev(img.words);
    img.bind(dev.data());
    const TreeTab& t = k.tab;
    const std::vector<int> zeros_n((size_t)n, 0), zeros_nn((size_t)nodes, 0);
    CHECK(t.n == n && same(t.off, want_off) && same(t.T, T) && same(t.N, k.N) && same(t.node_off, want_node_off));
    CHECK(same(t.ds_off, want_ds_off) && same(t.parent, k.parent) && same(t.depth, k.depth));
    CHECK(same(t.child_lo, want_child_lo) && same(t.child_n, want_child_n) && same(t.dstart, want_dstart));
    CHECK(same(t.enc_row, full ? k.enc_row : zeros_n) && same(t.label, full ? k.label : zeros_nn) && same(t.row, full ? k.row : zeros_nn));
    // a table of the wrong size is seen
    TreeCall bad = k;
    bad.depth.pop_back();
    CHECK(!bad.sizes_ok());
    if (full) { bad = k; bad.label.clear(); CHECK(!bad.sizes_ok()); }
    return 0;
}

int main() {
    const int Us[3] = {0, 1, 7}, Ts[3] = {1, 2, 9};
    // n = 1: every (T, U); band widths 1 .. U + 1 (T = 1: U + 1 alone)
    for (int T : Ts)
        for (int U : Us) {
            if (lattice_case({T}, {U}, {})) return 1;
            for (int w = T == 1 ? U + 1 : 1; w <= U + 1; ++w)
                if (lattice_case({T}, {U}, {w})) return 1;
        }
    // n = 3: every rotation of the U and T values against each other
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const std::vector<int> T = {Ts[a], Ts[(a + 1) % 3], Ts[(a + 2) % 3]}, U = {Us[b], Us[(b + 1) % 3], Us[(b + 2) % 3]};
            if (lattice_case(T, U, {})) return 1;
            std::vector<int> W;
            for (int i = 0; i < 3; ++i) W.push_back(T[i] == 1 ? U[i] + 1 : (U[i] + 2) / 2);
            if (lattice_case(T, U, W)) return 1;
        }
    // back-pointer words beyond the LDS share (T (U + 1) > 32 LAT_BP_WORDS) beside utterances that fit, in both orders
    const int bigT = 32 * LAT_BP_WORDS / 8 + 1;      // x 8 columns: one word more than LAT_BP_WORDS
    if (lattice_case({bigT, 9}, {7, 1}, {})) return 1;
    if (lattice_case({2, bigT, 9, bigT - 1}, {1, 7, 0, 7}, {})) return 1;
    if (lattice_case({bigT, 9}, {20, 7}, {8, 3})) return 1;
    if (lattice_case({9, bigT - 1, bigT}, {7, 20, 20}, {3, 8, 8})) return 1;
    // trees: a single node, a chain, a bush; alone and together; the DP-alone form without label / row / enc_row
    const std::vector<int> one = {-1}, chain = {-1, 0, 1, 2, 3, 4, 5}, bush = {-1, 0, 0, 0, 1, 1, 3, 4, 6, 6};
    for (int full = 0; full < 2; ++full) {
        for (int T : Ts) {
            if (tree_case({T}, {one}, full)) return 1;
            if (tree_case({T}, {chain}, full)) return 1;
            if (tree_case({T}, {bush}, full)) return 1;
        }
        if (tree_case({1, 2, 9}, {one, chain, bush}, full)) return 1;
        if (tree_case({9, 1, 2}, {chain, one, one}, full)) return 1;
        if (tree_case({2, 9, 1}, {bush, bush, chain}, full)) return 1;
    }
    CHECK(n_odd > 0 && n_even > 0);                   // the padding word was exercised both ways
    std::printf("lattice_tables_check: ok (%d images with a padding word, %d without)\n", n_odd, n_even);
    return 0;
}
