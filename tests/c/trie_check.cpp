// trie_check.cpp -- libreasr_amd/csrc/lasr_prefix_tree.hip.h (the prefix tree of an n-best list, standard C++ only) under
// AddressSanitizer + UndefinedBehaviorSanitizer: random candidate lists over a small alphabet against a restatement with std::map,
// the order contract of the header, the exact-capacity and LASR_EFULL paths (guard words behind every output), the argument checks.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../libreasr_amd/csrc/lasr_prefix_tree.hip.h"

#define CHECK(x) do { if (!(x)) { std::printf("trie_check: FAILED %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static unsigned rnd_state = 12345u;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static int one_case(const std::vector<std::vector<int32_t>>& cands) {
    const int k = (int)cands.size();
    std::vector<int32_t> tok, nt;
    for (const auto& c : cands) { nt.push_back((int32_t)c.size()); tok.insert(tok.end(), c.begin(), c.end()); }
    // restatement: distinct prefixes by depth, then parent, then first appearance
    std::map<std::vector<int32_t>, int> id;
    std::vector<int32_t> parent{-1}, label{-1}, depth{0};
    id[{}] = 0;
    size_t longest = 0;
    for (const auto& c : cands) longest = c.size() > longest ? c.size() : longest;
    for (size_t d = 0; d < longest; ++d) {
        std::vector<std::pair<int, std::vector<int32_t>>> fresh;               // (parent id, prefix) in order of appearance
        std::map<std::vector<int32_t>, bool> seen;
        for (const auto& c : cands) {
            if (c.size() <= d) continue;
            std::vector<int32_t> pre(c.begin(), c.begin() + d + 1), par(c.begin(), c.begin() + d);
            if (seen.count(pre)) continue;
            seen[pre] = true;
            fresh.emplace_back(id[par], pre);
        }
        for (size_t i = 1; i < fresh.size(); ++i)                              // stable insertion sort by parent
            for (size_t j = i; j > 0 && fresh[j - 1].first > fresh[j].first; --j) std::swap(fresh[j - 1], fresh[j]);
        for (const auto& f : fresh) {
            id[f.second] = (int)parent.size();
            parent.push_back(f.first); label.push_back(f.second.back()); depth.push_back((int32_t)d + 1);
        }
    }
    const int N = (int)parent.size();
    // exact capacity, guard words behind every array
    std::vector<int32_t> p(N + 1, 777), l(N + 1, 777), dp(N + 1, 777), term(k + 1, 777);
    int n = -1;
    CHECK(lasr_pt::prefix_tree(tok.data(), nt.data(), k, N, p.data(), l.data(), dp.data(), term.data(), &n) == lasr_pt::PT_OK);
    CHECK(n == N && p[N] == 777 && l[N] == 777 && dp[N] == 777 && term[k] == 777);
    for (int v = 0; v < N; ++v) CHECK(p[v] == parent[v] && l[v] == label[v] && dp[v] == depth[v]);
    for (int j = 0; j < k; ++j) CHECK(term[j] == id[cands[j]]);
    // the order contract
    CHECK(p[0] == -1 && l[0] == -1 && dp[0] == 0);
    for (int v = 1; v < N; ++v) {
        CHECK(p[v] >= 0 && p[v] < v && dp[v] == dp[p[v]] + 1 && dp[v] >= dp[v - 1]);
        CHECK(p[v] >= p[v - 1] || dp[v] > dp[v - 1]);                          // parents ascending within a depth: children contiguous
    }
    // one short: nothing but *n_nodes is written
    if (N > 1) {
        std::vector<int32_t> q(N, 555), t2(k, 555);
        int n2 = -1;
        CHECK(lasr_pt::prefix_tree(tok.data(), nt.data(), k, N - 1, q.data(), q.data(), q.data(), t2.data(), &n2) == lasr_pt::PT_EFULL);
        CHECK(n2 == N);
        for (int v = 0; v < N; ++v) CHECK(q[v] == 555);
        for (int j = 0; j < k; ++j) CHECK(t2[j] == 555);
    }
    return 0;
}

int main() {
    if (one_case({{}})) return 1;
    if (one_case({{3, 4, 5}})) return 1;
    if (one_case({{3, 4, 5}, {3, 4, 5}, {}, {3, 4}, {3, 4, 6}, {7}, {7, 3, 4}})) return 1;
    for (int it = 0; it < 300; ++it) {
        const int k = 1 + (int)(rnd() % 9);
        std::vector<std::vector<int32_t>> cands(k);
        for (auto& c : cands) {
            const int len = (int)(rnd() % 7);
            for (int u = 0; u < len; ++u) c.push_back(1 + (int32_t)(rnd() % 4));
        }
        if (one_case(cands)) return 1;
    }
    // argument checks
    int32_t tok[2] = {1, 2}, nt[1] = {2}, bad[1] = {-1}, out[4], term[1];
    int n = -1;
    CHECK(lasr_pt::prefix_tree(tok, nt, 0, 4, out, out, out, term, &n) == lasr_pt::PT_EINVAL && n == 0);
    CHECK(lasr_pt::prefix_tree(tok, bad, 1, 4, out, out, out, term, &n) == lasr_pt::PT_EINVAL);
    CHECK(lasr_pt::prefix_tree(nullptr, nt, 1, 4, out, out, out, term, &n) == lasr_pt::PT_EINVAL);
    CHECK(lasr_pt::prefix_tree(tok, nt, 1, 4, out, out, out, nullptr, &n) == lasr_pt::PT_EINVAL);
    CHECK(lasr_pt::prefix_tree(tok, nt, 1, 4, out, out, out, term, nullptr) == lasr_pt::PT_EINVAL);
    std::printf("trie_check: ok\n");
    return 0;
}
