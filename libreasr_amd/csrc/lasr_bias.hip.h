// lasr_bias.hip.h -- contextual biasing (hotwords): a phrase list compiled into the Aho-Corasick automaton the selection kernels
// walk, in the greedy form (lasr_bias_compile, lasr_set_bias) and the beam form (lasr_beam_bias_compile,
// lasr_set_beam_bias), and the one device block either form is attached as.
// Standard C++ only, no HIP include and no context (the name follows the unit's other headers so that the build tracks it): the
// engine includes it behind lasr_prefix_tree.hip.h, tests/c/bias_check.cpp and tests/c/beam_bias_check.cpp on its own.
//
// Contract.  The nodes are lasr_prefix_tree's (node 0 = the empty prefix; depth ascending, then parent ascending, then first
// appearance).  w(v), v >= 1, is the largest weight of a phrase that has node v's prefix as a prefix.  delta(v, a) is the node of the
// LONGEST suffix of path(v) . a that is a prefix of some phrase, 0 if there is none.  The edge list of node v holds every token a
// with delta(v, a) != 0, ascending in a, as (tok, next = delta(v, a), bonus = w(next)); CSR over the nodes.  A token that is not
// listed has bonus 0 and leads to the root.
//
// Construction: fail(v) = the node of the longest PROPER suffix of path(v) that is a node.  delta(v, .) is delta(fail(v), .) with
// v's own children laid over it (delta(0, .) = the root's children), and fail(child of v by a) = delta(fail(v), a) (children of the
// root: 0).  fail(v) is shallower than v and the nodes are ordered by depth, so one pass in node order has every list it merges
// from.  Integer arithmetic and max only: the result is the same on every host.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "lasr_prefix_tree.hip.h"

namespace lasr_bias {

constexpr int B_OK = 0, B_EINVAL = -1, B_EFULL = -5;          // include/lasr.h: LASR_OK, LASR_EINVAL, LASR_EFULL
constexpr int MAX_NODES = 65536;
constexpr long long MAX_EDGES = 1ll << 22;

// the automaton, and per node what the beam form is derived from: the trie parent, "a phrase ends exactly here", w(v)
struct Graph {
    std::vector<int32_t> off, tok, next, depth, parent;
    std::vector<float> bonus, w;
    std::vector<char> term;
};

// a finite weight >= 0 (NaN fails both comparisons)
inline bool weight_ok(float w) { return w >= 0.0f && w <= 3.402823466e+38f; }

// a caller's phrase list, as both compilers take it
inline bool check_phrases(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank) {
    if (!tokens || !n_tokens || !weights || k < 1) return false;
    long long total = 0;
    for (int j = 0; j < k; ++j) {
        if (n_tokens[j] < 1 || !weight_ok(weights[j])) return false;
        total += n_tokens[j];
        if (total >= (1ll << 31) - 1) return false;
    }
    for (long long i = 0; i < total; ++i)
        if (tokens[i] < 0 || tokens[i] >= vocab || tokens[i] == blank) return false;
    return true;
}

// the phrases are valid (check_phrases).  false: more than MAX_NODES nodes or MAX_EDGES edges
inline bool build(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, Graph& g) {
    lasr_pt::Tree t;
    lasr_pt::build(tokens, n_tokens, k, t);
    const int n = (int)t.parent.size();
    if (n > MAX_NODES) return false;
    std::vector<float>& w = g.w;
    w.assign(n, 0.0f);
    g.term.assign(n, 0);
    for (int j = 0; j < k; ++j) { w[t.term[j]] = std::max(w[t.term[j]], weights[j]); g.term[t.term[j]] = 1; }
    for (int v = n - 1; v >= 1; --v) w[t.parent[v]] = std::max(w[t.parent[v]], w[v]);      // (parent[v] < v: every subtree is complete)
    // children per node, ascending in the label (tree order is first appearance)
    std::vector<std::vector<std::pair<int32_t, int32_t>>> kids(n);
    for (int v = 1; v < n; ++v) kids[t.parent[v]].emplace_back(t.label[v], v);
    for (auto& kv : kids) std::sort(kv.begin(), kv.end());
    g.off.assign(1, 0); g.tok.clear(); g.next.clear(); g.bonus.clear();
    g.depth = t.depth;
    g.parent = t.parent;
    std::vector<int32_t> fail(n, 0);
    for (int v = 0; v < n; ++v) {
        const int f = fail[v];
        // merge of fail(v)'s finished list (v > 0; node 0 has none below it) and v's children: a child overrides
        size_t i = v ? (size_t)g.off[f] : 0;
        const size_t ie = v ? (size_t)g.off[f + 1] : 0;
        size_t j = 0;
        const auto& kv = kids[v];
        while (i < ie || j < kv.size()) {
            const bool take_kid = j < kv.size() && (i >= ie || kv[j].first <= g.tok[i]);
            int32_t a, nx;
            if (take_kid) {
                a = kv[j].first; nx = kv[j].second;
                // the child's failure node: where fail(v) goes on a (the root's children fall back to the root)
                fail[nx] = (v && i < ie && g.tok[i] == a) ? g.next[i] : 0;
                if (i < ie && g.tok[i] == a) ++i;
                ++j;
            } else {
                a = g.tok[i]; nx = g.next[i];
                ++i;
            }
            g.tok.push_back(a); g.next.push_back(nx); g.bonus.push_back(w[nx]);
            if ((long long)g.tok.size() > MAX_EDGES) return false;
        }
        g.off.push_back((int32_t)g.tok.size());
    }
    return true;
}

// ---------------------------------------------------------------------------- the graph in beam form
// A beam ranks by score, so the bonus of a partial match is revocable: term(v) = some phrase ends exactly at v; cum(v) = the summed
// w along path(v); held(v) = the part of it collected since the last completed phrase on the path (0 at a term node).  An edge
// (v, a, n = delta(v, a)) gains w(n) where n is v's trie child, and cum(n) - held(v) on a failure transition (the held part is handed
// back, the new match is paid from its start); a non-blank token that is not listed gains back[v] = -held(v) and leads to the root.
// Sums in double in path order (parent[v] < v), every gain and back rounded once to f32.
constexpr float BEAM_GAIN_MAX = 1000.0f;      // bound on |gain| and |back| (k_beam_select_rw's pruning argument relies on it)

inline bool gain_ok(float g) { return g >= -BEAM_GAIN_MAX && g <= BEAM_GAIN_MAX; }      // (NaN fails both comparisons)

// gain per edge and back per node of a built graph.  false: one of them is beyond BEAM_GAIN_MAX
inline bool beam_gains(const Graph& g, std::vector<float>& gain, std::vector<float>& back) {
    const int n = (int)g.off.size() - 1;
    std::vector<double> cum(n, 0.0), held(n, 0.0);
    for (int v = 1; v < n; ++v) {
        cum[v] = cum[g.parent[v]] + (double)g.w[v];
        held[v] = g.term[v] ? 0.0 : held[g.parent[v]] + (double)g.w[v];
    }
    gain.resize(g.tok.size()); back.resize(n);
    for (int v = 0; v < n; ++v) {
        back[v] = (float)(-held[v]);
        if (!gain_ok(back[v])) return false;
        for (int32_t i = g.off[v]; i < g.off[v + 1]; ++i) {
            const int nx = g.next[i];
            gain[i] = g.parent[nx] == v ? g.w[nx] : (float)(cum[nx] - held[v]);
            if (!gain_ok(gain[i])) return false;
        }
    }
    return true;
}

// the body of both compilers.  beam: edge_val takes the gains and node_back is filled; else edge_val takes the bonuses
inline int compile_form(bool beam, const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank,
                        int cap_nodes, int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_val,
                        float* node_back, int32_t* depth, int* n_nodes, int* n_edges) {
    if (n_nodes) *n_nodes = 0;
    if (n_edges) *n_edges = 0;
    if (!edge_off || !edge_tok || !edge_next || !edge_val || (beam && !node_back) || !n_nodes || !n_edges) return B_EINVAL;
    if (!check_phrases(tokens, n_tokens, weights, k, vocab, blank)) return B_EINVAL;
    Graph g;
    if (!build(tokens, n_tokens, weights, k, g)) return B_EINVAL;
    std::vector<float> gain, back;
    if (beam && !beam_gains(g, gain, back)) return B_EINVAL;
    const int n = (int)g.off.size() - 1, e = (int)g.tok.size();
    *n_nodes = n; *n_edges = e;
    if (n > cap_nodes || e > cap_edges) return B_EFULL;
    const std::vector<float>& val = beam ? gain : g.bonus;
    for (int v = 0; v <= n; ++v) edge_off[v] = g.off[v];
    for (int i = 0; i < e; ++i) { edge_tok[i] = g.tok[i]; edge_next[i] = g.next[i]; edge_val[i] = val[i]; }
    if (beam) for (int v = 0; v < n; ++v) node_back[v] = back[v];
    if (depth) for (int v = 0; v < n; ++v) depth[v] = g.depth[v];
    return B_OK;
}
// the body of lasr_bias_compile (include/lasr.h)
inline int compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                   int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_bonus, int32_t* depth,
                   int* n_nodes, int* n_edges) {
    return compile_form(false, tokens, n_tokens, weights, k, vocab, blank, cap_nodes, cap_edges, edge_off, edge_tok, edge_next, edge_bonus,
                        nullptr, depth, n_nodes, n_edges);
}
// the body of lasr_beam_bias_compile (include/lasr.h)
inline int beam_compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                        int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_gain, float* node_back,
                        int32_t* depth, int* n_nodes, int* n_edges) {
    return compile_form(true, tokens, n_tokens, weights, k, vocab, blank, cap_nodes, cap_edges, edge_off, edge_tok, edge_next, edge_gain,
                        node_back, depth, n_nodes, n_edges);
}

// ---------------------------------------------------------------------------- a caller's graph
// The checks of lasr_set_bias (beam = false: edge_val is the bonus, finite and >= 0; node_back is not looked at) and of
// lasr_set_beam_bias (beam = true: edge_val is the gain, of either sign, and node_back must be there).  nullptr: fine, else what
// is wrong.  (The form is an argument, not "node_back != nullptr": a beam graph without the column is refused by name, behind the
// two checks that come before it.)
inline const char* validate_form(bool beam, int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                                 const float* edge_val, const float* node_back, int vocab, int blank) {
    if (n_nodes < 1 || n_nodes > MAX_NODES) return "n_nodes outside [1, 65536]";
    if (!edge_off) return "null edge_off";
    if (beam && !node_back) return "null node_back";
    if (edge_off[0] != 0) return "edge_off[0] != 0";
    for (int v = 0; v < n_nodes; ++v)
        if (edge_off[v + 1] < edge_off[v]) return "edge_off decreases";
    const long long e = edge_off[n_nodes];
    if (e > MAX_EDGES) return "more than 2^22 edges";
    if (e > 0 && (!edge_tok || !edge_next || !edge_val)) return "null edge array";
    if (beam && node_back[0] != 0.0f) return "node_back[0] != 0";
    for (int v = 0; v < n_nodes; ++v) {
        if (beam && (!(node_back[v] <= 0.0f) || !gain_ok(node_back[v]))) return "node_back positive, not finite or below -1000";
        for (int32_t i = edge_off[v]; i < edge_off[v + 1]; ++i) {
            if (edge_tok[i] < 0 || edge_tok[i] >= vocab) return "edge token outside the vocabulary";
            if (edge_tok[i] == blank) return "blank listed as an edge";
            if (i > edge_off[v] && edge_tok[i] <= edge_tok[i - 1]) return "edge tokens of a node not ascending";
            if (edge_next[i] < 1 || edge_next[i] >= n_nodes) return "edge target outside [1, n_nodes)";
            if (beam ? !gain_ok(edge_val[i]) : !weight_ok(edge_val[i]))
                return beam ? "edge gain not finite or beyond 1000" : "edge bonus negative or not finite";
        }
    }
    return nullptr;
}
inline const char* validate(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_bonus,
                            int vocab, int blank) {
    return validate_form(false, n_nodes, edge_off, edge_tok, edge_next, edge_bonus, nullptr, vocab, blank);
}
inline const char* validate_beam(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_gain,
                                 const float* node_back, int vocab, int blank) {
    return validate_form(true, n_nodes, edge_off, edge_tok, edge_next, edge_gain, node_back, vocab, blank);
}

// ---------------------------------------------------------------------------- the attached graph: one block of 32-bit words
// [off (n_nodes + 1) | tok (E) | next (E) | val (E) | back (n_nodes, beam form only)].  block_layout is the one place that knows it:
// pack_block writes a block through it, view_block points a kernel's view into one.
struct BlockLayout { size_t tok, next, val, back, words; };
inline BlockLayout block_layout(int n_nodes, size_t E, bool has_back) {
    const size_t n = (size_t)n_nodes;
    return BlockLayout{n + 1, n + 1 + E, n + 1 + 2 * E, n + 1 + 3 * E, n + 1 + 3 * E + (has_back ? n : 0)};
}
// a valid graph (validate_form) as a block; node_back == nullptr: no back column
inline std::vector<int32_t> pack_block(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                                       const float* edge_val, const float* node_back) {
    const size_t E = (size_t)edge_off[n_nodes];
    const BlockLayout at = block_layout(n_nodes, E, node_back != nullptr);
    std::vector<int32_t> img(at.words);
    std::copy(edge_off, edge_off + n_nodes + 1, img.begin());
    if (E) {
        std::copy(edge_tok, edge_tok + E, img.begin() + at.tok);
        std::copy(edge_next, edge_next + E, img.begin() + at.next);
        memcpy(img.data() + at.val, edge_val, sizeof(float) * E);
    }
    if (node_back) memcpy(img.data() + at.back, node_back, sizeof(float) * (size_t)n_nodes);
    return img;
}
// the edge columns of the block at `base` into e (BiasEdges of lasr_kernels.hip.h; e.node is the caller's); returns the back column
// (nullptr: the block has none)
template <class Edges>
inline const float* view_block(const int* base, int n_nodes, size_t E, bool has_back, Edges& e) {
    const BlockLayout at = block_layout(n_nodes, E, has_back);
    e.off = base; e.tok = base + at.tok; e.next = base + at.next; e.val = (const float*)(base + at.val);
    return has_back ? (const float*)(base + at.back) : nullptr;
}

// the edge of node v by token a (its index, -1: not listed): binary search in the node's ascending token list
inline int find_edge(const int32_t* edge_off, const int32_t* edge_tok, int v, int32_t a) {
    int lo = edge_off[v], hi = edge_off[v + 1];
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (edge_tok[mid] < a) lo = mid + 1; else hi = mid;
    }
    return lo < edge_off[v + 1] && edge_tok[lo] == a ? lo : -1;
}

// the body of lasr_bias_walk (include/lasr.h): tokens through a beam-form graph from `start`
inline int walk(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_gain,
                const float* node_back, int blank, const int32_t* tokens, int n, int start, int* end_node, double* total, float* gains) {
    if (n_nodes < 1 || !edge_off || !node_back || n < 0 || (n > 0 && !tokens) || start < 0 || start >= n_nodes) return B_EINVAL;
    if (edge_off[n_nodes] > 0 && (!edge_tok || !edge_next || !edge_gain)) return B_EINVAL;
    int v = start;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        float gn = 0.0f;
        if (tokens[i] < 0) return B_EINVAL;
        if (tokens[i] != blank) {
            const int e = find_edge(edge_off, edge_tok, v, tokens[i]);
            if (e >= 0) {
                if (edge_next[e] < 0 || edge_next[e] >= n_nodes) return B_EINVAL;
                gn = edge_gain[e]; v = edge_next[e];
            } else {
                gn = node_back[v]; v = 0;
            }
        }
        sum += (double)gn;
        if (gains) gains[i] = gn;
    }
    if (end_node) *end_node = v;
    if (total) *total = sum;
    return B_OK;
}

}  // namespace lasr_bias
