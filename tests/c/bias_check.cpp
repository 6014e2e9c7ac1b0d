// bias_check.cpp -- libreasr_amd/csrc/lasr_bias.hip.h (the phrase-automaton compiler of contextual biasing) against a plain
// restatement of its definition, on random inputs; built with -fsanitize=address,undefined by tests/test_bias_cpu.py.
//
// The restatement does not share the header's construction: the set of trie prefixes is a std::map from token paths to node ids
// (numbered as lasr_prefix_tree numbers them, by a breadth-first pass over the phrases), delta(v, a) tries the suffixes of
// path(v) . a from the longest to the shortest, and w(v) scans the phrases.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>

#include "../../libreasr_amd/csrc/lasr_bias.hip.h"

using Path = std::vector<int32_t>;

static int fails = 0;
#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            if (++fails < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
        }                                                              \
    } while (0)

struct Plain {
    std::vector<int32_t> off, tok, next, depth;
    std::vector<float> bonus;
};

static Plain restate(const std::vector<Path>& ph, const std::vector<float>& w, int vocab) {
    std::map<Path, int> index;
    std::vector<Path> paths(1);
    index[Path{}] = 0;
    std::vector<Path> level(1);
    while (!level.empty()) {
        std::vector<Path> nxt;
        for (const Path& p : level)
            for (const Path& q : ph) {
                if (q.size() <= p.size() || !std::equal(p.begin(), p.end(), q.begin())) continue;
                Path c(q.begin(), q.begin() + p.size() + 1);
                if (index.count(c)) continue;
                index[c] = (int)paths.size();
                paths.push_back(c);
                nxt.push_back(c);
            }
        level.swap(nxt);
    }
    Plain g;
    g.off.push_back(0);
    for (const Path& p : paths) {
        g.depth.push_back((int32_t)p.size());
        for (int a = 0; a < vocab; ++a) {
            Path s = p;
            s.push_back(a);
            for (size_t k = 0; k < s.size(); ++k) {
                Path suf(s.begin() + k, s.end());
                auto it = index.find(suf);
                if (it == index.end()) continue;
                float best = -1.0f;
                for (size_t j = 0; j < ph.size(); ++j)
                    if (ph[j].size() >= suf.size() && std::equal(suf.begin(), suf.end(), ph[j].begin())) best = std::max(best, w[j]);
                g.tok.push_back(a); g.next.push_back(it->second); g.bonus.push_back(best);
                break;
            }
        }
        g.off.push_back((int32_t)g.tok.size());
    }
    return g;
}

struct Out {
    std::vector<int32_t> off, tok, next, depth;
    std::vector<float> bonus;
    int n_nodes = -7, n_edges = -7;
};

static int run(const std::vector<Path>& ph, const std::vector<float>& w, int vocab, int blank, int cap_nodes, int cap_edges, Out& o,
               bool with_depth = true) {
    std::vector<int32_t> cat, nt;
    for (const Path& p : ph) { nt.push_back((int32_t)p.size()); cat.insert(cat.end(), p.begin(), p.end()); }
    cat.push_back(0);                                 // (never read: keeps data() non-null for a set of empty phrases)
    // exactly the capacities that were promised, so that the sanitizer sees a write past them
    o.off.assign((size_t)cap_nodes + 1, -3); o.depth.assign((size_t)cap_nodes, -3);
    o.tok.assign((size_t)cap_edges, -3); o.next.assign((size_t)cap_edges, -3); o.bonus.assign((size_t)cap_edges, -3.0f);
    std::vector<int32_t> pad(1);
    std::vector<float> padf(1);
    return lasr_bias::compile(cat.data(), nt.data(), w.data(), (int)ph.size(), vocab, blank, cap_nodes, cap_edges, o.off.data(),
                              cap_edges ? o.tok.data() : pad.data(), cap_edges ? o.next.data() : pad.data(),
                              cap_edges ? o.bonus.data() : padf.data(), with_depth ? (cap_nodes ? o.depth.data() : pad.data()) : nullptr,
                              &o.n_nodes, &o.n_edges);
}

static void compare(const std::vector<Path>& ph, const std::vector<float>& w, int vocab, int blank) {
    const Plain g = restate(ph, w, vocab);
    const int n = (int)g.off.size() - 1, e = (int)g.tok.size();
    Out o;
    CHECK(run(ph, w, vocab, blank, 0, 0, o) == lasr_bias::B_EFULL);
    CHECK(o.n_nodes == n && o.n_edges == e);
    CHECK(o.off[0] == -3);                            // nothing else is written
    if (e > 0) {
        CHECK(run(ph, w, vocab, blank, n, e - 1, o) == lasr_bias::B_EFULL);
        CHECK(o.n_nodes == n && o.n_edges == e);
    }
    CHECK(run(ph, w, vocab, blank, n - 1, e, o) == lasr_bias::B_EFULL);
    CHECK(run(ph, w, vocab, blank, n, e, o) == lasr_bias::B_OK);          // exact capacity
    CHECK(o.n_nodes == n && o.n_edges == e);
    CHECK(o.off == g.off && o.tok == g.tok && o.next == g.next && o.depth == g.depth);
    CHECK(o.bonus.size() == g.bonus.size());
    for (size_t i = 0; i < g.bonus.size() && i < o.bonus.size(); ++i) CHECK(o.bonus[i] == g.bonus[i]);
    CHECK(run(ph, w, vocab, blank, n, e, o, false) == lasr_bias::B_OK);   // depth is optional
    CHECK(lasr_bias::validate(n, o.off.data(), o.tok.data(), o.next.data(), o.bonus.data(), vocab, blank) == nullptr);
}

int main() {
    std::mt19937 rng(20240611);
    const int blank = 0;
    // random phrase sets over few symbols (overlaps, failure transitions to inner nodes, duplicates, prefixes of one another)
    for (int it = 0; it < 400; ++it) {
        const int nsym = 2 + (int)(rng() % 4), k = 1 + (int)(rng() % 6), vocab = 1 + nsym + (int)(rng() % 3);
        std::vector<Path> ph(k);
        std::vector<float> w(k);
        for (int j = 0; j < k; ++j) {
            const int len = 1 + (int)(rng() % 6);
            for (int q = 0; q < len; ++q) ph[j].push_back(1 + (int32_t)(rng() % nsym));
            w[j] = (rng() % 4 == 0) ? 0.0f : (float)(rng() % 9) * 0.25f;
        }
        compare(ph, w, vocab, blank);
    }
    // a wide root: more distinct first tokens than a workgroup has threads
    {
        std::vector<Path> ph;
        std::vector<float> w;
        for (int a = 1; a <= 300; ++a) { ph.push_back(Path{a}); w.push_back(0.5f + 0.001f * (float)a); }
        compare(ph, w, 320, blank);
    }
    // refusals: the counts are 0 and nothing is written
    {
        Out o;
        const std::vector<Path> ok{{1, 2}, {2, 3}};
        const std::vector<float> w{1.0f, 2.0f};
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        CHECK(run({{1, 2}, {}}, w, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL && o.n_nodes == 0 && o.n_edges == 0);
        CHECK(run({{1, 8}}, {1.0f}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL && o.n_nodes == 0);
        CHECK(run({{1, -1}}, {1.0f}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL);
        CHECK(run({{1, 0}}, {1.0f}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL);           // blank
        CHECK(run(ok, {1.0f, -0.5f}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL);
        CHECK(run(ok, {inf, 1.0f}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL);
        CHECK(run(ok, {1.0f, nan}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL);
        CHECK(o.off[0] == -3 && o.tok[0] == -3);
        int nn = 5, ne = 5;
        int32_t t[2] = {1, 2}, nt[1] = {2}, a[8];
        float wf[1] = {1.0f}, b[8];
        CHECK(lasr_bias::compile(t, nt, wf, 0, 8, 0, 4, 4, a, a, a, b, nullptr, &nn, &ne) == lasr_bias::B_EINVAL && nn == 0 && ne == 0);
        CHECK(lasr_bias::compile(nullptr, nt, wf, 1, 8, 0, 4, 4, a, a, a, b, nullptr, &nn, &ne) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::compile(t, nt, wf, 1, 8, 0, 4, 4, a, a, a, nullptr, nullptr, &nn, &ne) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::compile(t, nt, wf, 1, 8, 0, 4, 4, a, a, a, b, nullptr, nullptr, &ne) == lasr_bias::B_EINVAL && ne == 0);
        // more than 65536 nodes: 257 x 256 distinct two-token phrases
        std::vector<Path> big;
        for (int x = 1; x <= 257; ++x)
            for (int y = 1; y <= 256; ++y) big.push_back(Path{x, y});
        CHECK(run(big, std::vector<float>(big.size(), 1.0f), 512, blank, 8, 8, o) == lasr_bias::B_EINVAL && o.n_nodes == 0 && o.n_edges == 0);
    }
    // validate: each kind of malformed graph is named
    {
        const int32_t off[3] = {0, 2, 2}, tok[2] = {1, 3}, nxt[2] = {1, 1};
        const float bon[2] = {0.5f, 0.0f};
        CHECK(lasr_bias::validate(2, off, tok, nxt, bon, 8, 0) == nullptr);
        CHECK(lasr_bias::validate(0, off, tok, nxt, bon, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(65537, off, tok, nxt, bon, 8, 0) != nullptr);
        const int32_t off1[3] = {1, 2, 2}, off2[3] = {0, 2, 1};
        CHECK(lasr_bias::validate(2, off1, tok, nxt, bon, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off2, tok, nxt, bon, 8, 0) != nullptr);
        const int32_t tok1[2] = {3, 1}, tok2[2] = {1, 1}, tok3[2] = {1, 8}, tok4[2] = {0, 1};
        CHECK(lasr_bias::validate(2, off, tok1, nxt, bon, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off, tok2, nxt, bon, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off, tok3, nxt, bon, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off, tok4, nxt, bon, 8, 0) != nullptr);
        const int32_t nx1[2] = {0, 1}, nx2[2] = {1, 2};
        CHECK(lasr_bias::validate(2, off, tok, nx1, bon, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off, tok, nx2, bon, 8, 0) != nullptr);
        const float b1[2] = {-0.5f, 0.0f}, b2[2] = {0.5f, std::numeric_limits<float>::infinity()}, b3[2] = {std::numeric_limits<float>::quiet_NaN(), 0.f};
        CHECK(lasr_bias::validate(2, off, tok, nxt, b1, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off, tok, nxt, b2, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off, tok, nxt, b3, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, nullptr, tok, nxt, bon, 8, 0) != nullptr);
        CHECK(lasr_bias::validate(2, off, nullptr, nxt, bon, 8, 0) != nullptr);
    }
    if (fails) { printf("bias_check: %d check(s) FAILED\n", fails); return 1; }
    printf("bias_check: ok\n");
    return 0;
}
