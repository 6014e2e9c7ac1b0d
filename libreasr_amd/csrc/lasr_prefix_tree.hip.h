// lasr_prefix_tree.hip.h -- the candidates of an n-best list merged into a prefix tree (lasr_prefix_tree, lasr_score_*).
// Standard C++ only, no HIP include and no context (the name follows the unit's other headers so that the build tracks it): the
// engine includes it ahead of lasr_lattice_tree.hip.h, tests/c/trie_check.cpp on its own.
//
// Contract.  Node 0 is the empty prefix (parent -1, label -1, depth 0); every distinct non-empty prefix of a candidate is one node.
// Nodes are numbered by depth ascending; within a depth by parent ascending; within a parent by first appearance (lowest candidate
// index; a candidate contributes one label per depth, so the position adds nothing).  What the device side relies on follows:
//   * parent[v] < v                              a node's predecessor is computed before it in node order
//   * depth is non-decreasing                    the nodes of one depth are one contiguous range (k_lat_dp_tree's diagonal)
//   * the children of a node are contiguous      LatTreeMap's pick walks [child_lo, child_lo + child_n)
// term[j] is the node of candidate j: duplicates share a node, an empty candidate maps to node 0.
#pragma once

#include <cstdint>
#include <vector>

namespace lasr_pt {

constexpr int PT_OK = 0, PT_EINVAL = -1, PT_EFULL = -5;       // include/lasr.h: LASR_OK, LASR_EINVAL, LASR_EFULL

struct Tree {
    std::vector<int32_t> parent, label, depth, term;
    std::vector<int32_t> first;                      // lowest candidate index that passes through the node (node 0: 0)
};

// tokens: the k candidates concatenated, n_tokens[j] labels each (checked by the caller: non-null, k >= 1, no negative length)
inline void build(const int32_t* tokens, const int32_t* n_tokens, int k, Tree& t) {
    t.parent.assign(1, -1); t.label.assign(1, -1); t.depth.assign(1, 0); t.first.assign(1, 0);
    t.term.assign(k, 0);
    std::vector<long long> at(k);
    long long o = 0;
    int32_t longest = 0;
    for (int j = 0; j < k; ++j) { at[j] = o; o += n_tokens[j]; if (n_tokens[j] > longest) longest = n_tokens[j]; }
    std::vector<std::vector<int>> at_node(1);        // per node of the current depth (ascending): its candidates, ascending
    int lo = 0;                                      // first node of the current depth
    for (int j = 0; j < k; ++j) at_node[0].push_back(j);
    for (int32_t d = 0; d < longest; ++d) {
        const int next_lo = (int)t.parent.size();
        std::vector<std::vector<int>> nxt;
        for (size_t p = 0; p < at_node.size(); ++p) {                 // parents ascending
            const int first_child = (int)t.parent.size();
            for (int j : at_node[p]) {                                // first appearance = lowest candidate index
                if (n_tokens[j] <= d) continue;
                const int32_t y = tokens[at[j] + d];
                int v = -1;
                for (int c = first_child; c < (int)t.parent.size(); ++c)
                    if (t.label[c] == y) { v = c; break; }
                if (v < 0) {
                    v = (int)t.parent.size();
                    t.parent.push_back(lo + (int)p); t.label.push_back(y); t.depth.push_back(d + 1); t.first.push_back(j);
                    nxt.emplace_back();
                }
                nxt[v - next_lo].push_back(j);
                if (n_tokens[j] == d + 1) t.term[j] = v;
            }
        }
        at_node.swap(nxt);
        lo = next_lo;
    }
}

// the body of lasr_prefix_tree (include/lasr.h); *n_nodes is set whenever it is not null
inline int prefix_tree(const int32_t* tokens, const int32_t* n_tokens, int k, int cap, int32_t* parent, int32_t* label, int32_t* depth,
                       int32_t* term, int* n_nodes) {
    if (n_nodes) *n_nodes = 0;
    if (!n_tokens || !parent || !label || !depth || !term || !n_nodes || k < 1) return PT_EINVAL;
    long long total = 0;
    for (int j = 0; j < k; ++j) {
        if (n_tokens[j] < 0) return PT_EINVAL;
        total += n_tokens[j];
    }
    if (total > 0 && !tokens) return PT_EINVAL;
    if (total >= (1ll << 31) - 1) return PT_EINVAL;     // node ids are int32
    Tree t;
    build(tokens, n_tokens, k, t);
    const int n = (int)t.parent.size();
    *n_nodes = n;
    if (n > cap) return PT_EFULL;
    for (int v = 0; v < n; ++v) { parent[v] = t.parent[v]; label[v] = t.label[v]; depth[v] = t.depth[v]; }
    for (int j = 0; j < k; ++j) term[j] = t.term[j];
    return PT_OK;
}

}  // namespace lasr_pt
