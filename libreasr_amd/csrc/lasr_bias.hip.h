// lasr_bias.hip.h -- contextual biasing (hotwords): a phrase list compiled into the Aho-Corasick automaton k_select walks
// (lasr_bias_compile, lasr_set_bias).
// Standard C++ only, no HIP include and no context (the name follows the unit's other headers so that the build tracks it): the
// engine includes it behind lasr_prefix_tree.hip.h, tests/c/bias_check.cpp on its own.
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
#include <cstdint>
#include <utility>
#include <vector>

#include "lasr_prefix_tree.hip.h"

namespace lasr_bias {

constexpr int B_OK = 0, B_EINVAL = -1, B_EFULL = -5;          // include/lasr.h: LASR_OK, LASR_EINVAL, LASR_EFULL
constexpr int MAX_NODES = 65536;
constexpr long long MAX_EDGES = 1ll << 22;

struct Graph {
    std::vector<int32_t> off, tok, next, depth;
    std::vector<float> bonus;
};

// a finite weight >= 0 (NaN fails both comparisons)
inline bool weight_ok(float w) { return w >= 0.0f && w <= 3.402823466e+38f; }

// the phrases are valid (checked by the caller).  false: more than MAX_NODES nodes or MAX_EDGES edges
inline bool build(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, Graph& g) {
    lasr_pt::Tree t;
    lasr_pt::build(tokens, n_tokens, k, t);
    const int n = (int)t.parent.size();
    if (n > MAX_NODES) return false;
    std::vector<float> w(n, 0.0f);
    for (int j = 0; j < k; ++j) w[t.term[j]] = std::max(w[t.term[j]], weights[j]);
    for (int v = n - 1; v >= 1; --v) w[t.parent[v]] = std::max(w[t.parent[v]], w[v]);      // (parent[v] < v: every subtree is complete)
    // children per node, ascending in the label (tree order is first appearance)
    std::vector<std::vector<std::pair<int32_t, int32_t>>> kids(n);
    for (int v = 1; v < n; ++v) kids[t.parent[v]].emplace_back(t.label[v], v);
    for (auto& kv : kids) std::sort(kv.begin(), kv.end());
    g.off.assign(1, 0); g.tok.clear(); g.next.clear(); g.bonus.clear();
    g.depth = t.depth;
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

// the body of lasr_bias_compile (include/lasr.h)
inline int compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                   int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_bonus, int32_t* depth,
                   int* n_nodes, int* n_edges) {
    if (n_nodes) *n_nodes = 0;
    if (n_edges) *n_edges = 0;
    if (!tokens || !n_tokens || !weights || !edge_off || !edge_tok || !edge_next || !edge_bonus || !n_nodes || !n_edges || k < 1)
        return B_EINVAL;
    long long total = 0;
    for (int j = 0; j < k; ++j) {
        if (n_tokens[j] < 1 || !weight_ok(weights[j])) return B_EINVAL;
        total += n_tokens[j];
        if (total >= (1ll << 31) - 1) return B_EINVAL;
    }
    for (long long i = 0; i < total; ++i)
        if (tokens[i] < 0 || tokens[i] >= vocab || tokens[i] == blank) return B_EINVAL;
    Graph g;
    if (!build(tokens, n_tokens, weights, k, g)) return B_EINVAL;
    const int n = (int)g.off.size() - 1, e = (int)g.tok.size();
    *n_nodes = n; *n_edges = e;
    if (n > cap_nodes || e > cap_edges) return B_EFULL;
    for (int v = 0; v <= n; ++v) edge_off[v] = g.off[v];
    for (int i = 0; i < e; ++i) { edge_tok[i] = g.tok[i]; edge_next[i] = g.next[i]; edge_bonus[i] = g.bonus[i]; }
    if (depth) for (int v = 0; v < n; ++v) depth[v] = g.depth[v];
    return B_OK;
}

// lasr_set_bias' checks of a caller's graph (nullptr: fine, else what is wrong)
inline const char* validate(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_bonus,
                            int vocab, int blank) {
    if (n_nodes < 1 || n_nodes > MAX_NODES) return "n_nodes outside [1, 65536]";
    if (!edge_off) return "null edge_off";
    if (edge_off[0] != 0) return "edge_off[0] != 0";
    for (int v = 0; v < n_nodes; ++v)
        if (edge_off[v + 1] < edge_off[v]) return "edge_off decreases";
    const long long e = edge_off[n_nodes];
    if (e > MAX_EDGES) return "more than 2^22 edges";
    if (e > 0 && (!edge_tok || !edge_next || !edge_bonus)) return "null edge array";
    for (int v = 0; v < n_nodes; ++v)
        for (int32_t i = edge_off[v]; i < edge_off[v + 1]; ++i) {
            if (edge_tok[i] < 0 || edge_tok[i] >= vocab) return "edge token outside the vocabulary";
            if (edge_tok[i] == blank) return "blank listed as an edge";
            if (i > edge_off[v] && edge_tok[i] <= edge_tok[i - 1]) return "edge tokens of a node not ascending";
            if (edge_next[i] < 1 || edge_next[i] >= n_nodes) return "edge target outside [1, n_nodes)";
            if (!weight_ok(edge_bonus[i])) return "edge bonus negative or not finite";
        }
    return nullptr;
}

// ---------------------------------------------------------------------------- the graph in beam form
// A beam ranks by score, so the bonus of a partial match is revocable: term(v) = some phrase ends exactly at v; cum(v) = the summed
// w along path(v); held(v) = the part of it collected since the last completed phrase on the path (0 at a term node).  An edge
// (v, a, n = delta(v, a)) gains w(n) where n is v's trie child, and cum(n) - held(v) on a failure transition (the held part is handed
// back, the new match is paid from its start); a non-blank token that is not listed gains back[v] = -held(v) and leads to the root.
// Sums in double in path order (parent[v] < v), every gain and back rounded once to f32.
constexpr float BEAM_GAIN_MAX = 1000.0f;      // bound on |gain| and |back| (k_beam_select_rw's pruning argument relies on it)

inline bool gain_ok(float g) { return g >= -BEAM_GAIN_MAX && g <= BEAM_GAIN_MAX; }      // (NaN fails both comparisons)

// the body of lasr_beam_bias_compile (include/lasr.h)
inline int beam_compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                        int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_gain, float* node_back,
                        int32_t* depth, int* n_nodes, int* n_edges) {
    if (n_nodes) *n_nodes = 0;
    if (n_edges) *n_edges = 0;
    if (!tokens || !n_tokens || !weights || !edge_off || !edge_tok || !edge_next || !edge_gain || !node_back || !n_nodes || !n_edges || k < 1)
        return B_EINVAL;
    long long total = 0;
    for (int j = 0; j < k; ++j) {
        if (n_tokens[j] < 1 || !weight_ok(weights[j])) return B_EINVAL;
        total += n_tokens[j];
        if (total >= (1ll << 31) - 1) return B_EINVAL;
    }
    for (long long i = 0; i < total; ++i)
        if (tokens[i] < 0 || tokens[i] >= vocab || tokens[i] == blank) return B_EINVAL;
    Graph g;
    if (!build(tokens, n_tokens, weights, k, g)) return B_EINVAL;
    const int n = (int)g.off.size() - 1, e = (int)g.tok.size();
    // the same tree once more for parent and term (lasr_prefix_tree's numbering is build's)
    lasr_pt::Tree t;
    lasr_pt::build(tokens, n_tokens, k, t);
    std::vector<char> term(n, 0);
    for (int j = 0; j < k; ++j) term[t.term[j]] = 1;
    std::vector<float> w(n, 0.0f);
    for (int v = 0; v < n; ++v)
        for (int32_t i = g.off[v]; i < g.off[v + 1]; ++i)
            if (t.parent[g.next[i]] == v) w[g.next[i]] = g.bonus[i];
    std::vector<double> cum(n, 0.0), held(n, 0.0);
    for (int v = 1; v < n; ++v) {
        cum[v] = cum[t.parent[v]] + (double)w[v];
        held[v] = term[v] ? 0.0 : held[t.parent[v]] + (double)w[v];
    }
    std::vector<float> gain(e), back(n);
    for (int v = 0; v < n; ++v) {
        back[v] = (float)(-held[v]);
        if (!gain_ok(back[v])) return B_EINVAL;
        for (int32_t i = g.off[v]; i < g.off[v + 1]; ++i) {
            const int nx = g.next[i];
            gain[i] = t.parent[nx] == v ? w[nx] : (float)(cum[nx] - held[v]);
            if (!gain_ok(gain[i])) return B_EINVAL;
        }
    }
    *n_nodes = n; *n_edges = e;
    if (n > cap_nodes || e > cap_edges) return B_EFULL;
    for (int v = 0; v <= n; ++v) edge_off[v] = g.off[v];
    for (int i = 0; i < e; ++i) { edge_tok[i] = g.tok[i]; edge_next[i] = g.next[i]; edge_gain[i] = gain[i]; }
    for (int v = 0; v < n; ++v) node_back[v] = back[v];
    if (depth) for (int v = 0; v < n; ++v) depth[v] = g.depth[v];
    return B_OK;
}

// lasr_set_beam_bias' checks of a caller's graph (nullptr: fine, else what is wrong): validate's, but a gain may have either sign
inline const char* validate_beam(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_gain,
                                 const float* node_back, int vocab, int blank) {
    if (n_nodes < 1 || n_nodes > MAX_NODES) return "n_nodes outside [1, 65536]";
    if (!edge_off) return "null edge_off";
    if (!node_back) return "null node_back";
    if (edge_off[0] != 0) return "edge_off[0] != 0";
    for (int v = 0; v < n_nodes; ++v)
        if (edge_off[v + 1] < edge_off[v]) return "edge_off decreases";
    const long long e = edge_off[n_nodes];
    if (e > MAX_EDGES) return "more than 2^22 edges";
    if (e > 0 && (!edge_tok || !edge_next || !edge_gain)) return "null edge array";
    if (node_back[0] != 0.0f) return "node_back[0] != 0";
    for (int v = 0; v < n_nodes; ++v) {
        if (!(node_back[v] <= 0.0f) || !gain_ok(node_back[v])) return "node_back positive, not finite or below -1000";
        for (int32_t i = edge_off[v]; i < edge_off[v + 1]; ++i) {
            if (edge_tok[i] < 0 || edge_tok[i] >= vocab) return "edge token outside the vocabulary";
            if (edge_tok[i] == blank) return "blank listed as an edge";
            if (i > edge_off[v] && edge_tok[i] <= edge_tok[i - 1]) return "edge tokens of a node not ascending";
            if (edge_next[i] < 1 || edge_next[i] >= n_nodes) return "edge target outside [1, n_nodes)";
            if (!gain_ok(edge_gain[i])) return "edge gain not finite or beyond 1000";
        }
    }
    return nullptr;
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
