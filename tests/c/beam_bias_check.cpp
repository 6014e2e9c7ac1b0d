// beam_bias_check.cpp -- the beam form of libreasr_amd/csrc/lasr_bias.hip.h (beam_compile, validate_beam, walk: contextual biasing
// in beam search) against a plain restatement, on random inputs; built with -fsanitize=address,undefined by
// tests/test_beam_bias_cpu.py.
//
// The restatement shares neither the header's construction nor its cum / held recurrences: trie prefixes are a std::map from token
// paths to node ids (numbered breadth-first over the phrases), delta tries the suffixes of path(v) . a from the longest to the
// shortest, and the money is kept as a ledger -- a pending part (collected since the last completed phrase of the match) and a
// banked part -- replayed token by token along a path.  gain(v, a) is what the ledger's total changes by; the walk of a random
// token string must end with exactly the ledger's total and at the ledger's path.  Weights are multiples of 0.25, so every sum is
// exact and "equal" means equal.
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

struct Book {
    const std::vector<Path>& ph;
    const std::vector<float>& w;
    std::map<Path, int> index;
    std::vector<Path> paths;
    Book(const std::vector<Path>& ph_, const std::vector<float>& w_) : ph(ph_), w(w_), paths(1) {
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
    }
    float weight(const Path& pre) const {
        float best = -1.0f;
        for (size_t j = 0; j < ph.size(); ++j)
            if (ph[j].size() >= pre.size() && std::equal(pre.begin(), pre.end(), ph[j].begin())) best = std::max(best, w[j]);
        return best;
    }
    bool whole(const Path& p) const {
        for (const Path& q : ph) if (q == p) return true;
        return false;
    }
    // the ledger after matching `p` from the root, one token at a time
    void replay(const Path& p, double& banked, double& pending) const {
        for (size_t k = 1; k <= p.size(); ++k) {
            const Path pre(p.begin(), p.begin() + k);
            pending += (double)weight(pre);
            if (whole(pre)) { banked += pending; pending = 0.0; }
        }
    }
    // the longest suffix of s that is a trie prefix (from offset `from`)
    Path longest(const Path& s, size_t from) const {
        for (size_t k = from; k < s.size(); ++k) {
            Path suf(s.begin() + k, s.end());
            if (index.count(suf)) return suf;
        }
        return Path{};
    }
};

struct Plain {
    std::vector<int32_t> off, tok, next, depth;
    std::vector<float> gain, back;
};

static Plain restate(const Book& b, int vocab) {
    Plain g;
    g.off.push_back(0);
    for (const Path& p : b.paths) {
        g.depth.push_back((int32_t)p.size());
        double bank0 = 0.0, pend0 = 0.0;
        b.replay(p, bank0, pend0);
        g.back.push_back((float)(-pend0));
        for (int a = 0; a < vocab; ++a) {
            Path s = p;
            s.push_back(a);
            if (b.index.count(s)) {
                g.tok.push_back(a); g.next.push_back(b.index.at(s)); g.gain.push_back(b.weight(s));
                continue;
            }
            const Path q = b.longest(s, 1);
            if (q.empty()) continue;
            double bank1 = 0.0, pend1 = 0.0;
            b.replay(q, bank1, pend1);                      // the new match is paid from its start, the pending part is lost
            g.tok.push_back(a); g.next.push_back(b.index.at(q)); g.gain.push_back((float)((bank1 + pend1) - pend0));
        }
        g.off.push_back((int32_t)g.tok.size());
    }
    return g;
}

struct Out {
    std::vector<int32_t> off, tok, next, depth;
    std::vector<float> gain, back;
    int n_nodes = -7, n_edges = -7;
};

static int run(const std::vector<Path>& ph, const std::vector<float>& w, int vocab, int blank, int cap_nodes, int cap_edges, Out& o,
               bool with_depth = true) {
    std::vector<int32_t> cat, nt;
    for (const Path& p : ph) { nt.push_back((int32_t)p.size()); cat.insert(cat.end(), p.begin(), p.end()); }
    cat.push_back(0);
    // exactly the capacities that were promised, so that the sanitizer sees a write past them
    o.off.assign((size_t)cap_nodes + 1, -3); o.depth.assign((size_t)cap_nodes, -3); o.back.assign((size_t)cap_nodes, -3.0f);
    o.tok.assign((size_t)cap_edges, -3); o.next.assign((size_t)cap_edges, -3); o.gain.assign((size_t)cap_edges, -3.0f);
    std::vector<int32_t> pad(1);
    std::vector<float> padf(1);
    return lasr_bias::beam_compile(cat.data(), nt.data(), w.data(), (int)ph.size(), vocab, blank, cap_nodes, cap_edges, o.off.data(),
                                   cap_edges ? o.tok.data() : pad.data(), cap_edges ? o.next.data() : pad.data(),
                                   cap_edges ? o.gain.data() : padf.data(), cap_nodes ? o.back.data() : padf.data(),
                                   with_depth ? (cap_nodes ? o.depth.data() : pad.data()) : nullptr, &o.n_nodes, &o.n_edges);
}

static void compare(const std::vector<Path>& ph, const std::vector<float>& w, int vocab, int blank, std::mt19937& rng) {
    const Book b(ph, w);
    const Plain g = restate(b, vocab);
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
    CHECK(run(ph, w, vocab, blank, n, e, o, false) == lasr_bias::B_OK);   // depth is optional
    CHECK(run(ph, w, vocab, blank, n, e, o) == lasr_bias::B_OK);          // exact capacity
    CHECK(o.n_nodes == n && o.n_edges == e);
    CHECK(o.off == g.off && o.tok == g.tok && o.next == g.next && o.depth == g.depth);
    CHECK(o.gain.size() == g.gain.size() && o.back.size() == g.back.size());
    for (size_t i = 0; i < g.gain.size() && i < o.gain.size(); ++i) CHECK(o.gain[i] == g.gain[i]);
    for (size_t i = 0; i < g.back.size() && i < o.back.size(); ++i) CHECK(o.back[i] == g.back[i]);
    CHECK(lasr_bias::validate_beam(n, o.off.data(), o.tok.data(), o.next.data(), o.gain.data(), o.back.data(), vocab, blank) == nullptr);
    // the walk of random token strings (blank among them) against the ledger kept token by token
    for (int rep = 0; rep < 4; ++rep) {
        const int len = (int)(rng() % 24);
        std::vector<int32_t> toks(len);
        for (int& t : toks) t = (int32_t)(rng() % vocab);
        Path path;
        double banked = 0.0, pending = 0.0;
        for (int32_t a : toks) {
            if (a == blank) continue;
            Path s = path;
            s.push_back(a);
            if (b.index.count(s)) {
                pending += (double)b.weight(s);
                if (b.whole(s)) { banked += pending; pending = 0.0; }
                path = s;
            } else {
                pending = 0.0;
                path = b.longest(s, 1);
                b.replay(path, banked, pending);
            }
        }
        std::vector<float> gains((size_t)len + 1, -3.0f);
        int end = -7;
        double total = -7.0;
        CHECK(lasr_bias::walk(n, o.off.data(), o.tok.data(), o.next.data(), o.gain.data(), o.back.data(), blank, toks.data(), len, 0, &end,
                              &total, gains.data()) == lasr_bias::B_OK);
        CHECK(end == b.index.at(path));
        CHECK(total == banked + pending);                 // the invariant: completed matches + held(current node)
        CHECK((double)(-o.back[end >= 0 && end < n ? end : 0]) == pending);
        CHECK(gains[len] == -3.0f);
        double sum = 0.0;
        for (int i = 0; i < len; ++i) sum += (double)gains[i];
        CHECK(sum == total);
        // optional outputs
        CHECK(lasr_bias::walk(n, o.off.data(), o.tok.data(), o.next.data(), o.gain.data(), o.back.data(), blank, toks.data(), len, 0, nullptr,
                              nullptr, nullptr) == lasr_bias::B_OK);
    }
}

int main() {
    std::mt19937 rng(20240612);
    const int blank = 0;
    for (int it = 0; it < 400; ++it) {
        const int nsym = 2 + (int)(rng() % 4), k = 1 + (int)(rng() % 6), vocab = 1 + nsym + (int)(rng() % 3);
        std::vector<Path> ph(k);
        std::vector<float> w(k);
        for (int j = 0; j < k; ++j) {
            const int len = 1 + (int)(rng() % 6);
            for (int q = 0; q < len; ++q) ph[j].push_back(1 + (int32_t)(rng() % nsym));
            w[j] = (rng() % 4 == 0) ? 0.0f : (float)(rng() % 9) * 0.25f;
        }
        compare(ph, w, vocab, blank, rng);
    }
    // a wide root: more edges at one node than a wave has lanes
    {
        std::vector<Path> ph;
        std::vector<float> w;
        for (int a = 1; a <= 300; ++a) { ph.push_back(Path{a, 1 + a % 7}); w.push_back(0.25f * (float)(1 + a % 8)); }
        compare(ph, w, 320, blank, rng);
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
        // the 1000 bound: a held bonus of 3 x 400 would have to be handed back; 2 x 400 is fine
        CHECK(run({{1, 2, 3, 4}}, {400.0f}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL && o.n_nodes == 0 && o.n_edges == 0);
        CHECK(o.off[0] == -3 && o.tok[0] == -3 && o.back[0] == -3.0f);
        CHECK(run({{1, 2, 3}}, {400.0f}, 8, blank, 16, 16, o) == lasr_bias::B_OK);
        CHECK(run({{1}}, {1000.0f}, 8, blank, 16, 16, o) == lasr_bias::B_OK);
        CHECK(run({{1}}, {1000.5f}, 8, blank, 16, 16, o) == lasr_bias::B_EINVAL);
        int nn = 5, ne = 5;
        int32_t t[2] = {1, 2}, nt[1] = {2}, a[8];
        float wf[1] = {1.0f}, g[8], bk[8];
        CHECK(lasr_bias::beam_compile(t, nt, wf, 0, 8, 0, 4, 4, a, a, a, g, bk, nullptr, &nn, &ne) == lasr_bias::B_EINVAL && nn == 0 && ne == 0);
        CHECK(lasr_bias::beam_compile(nullptr, nt, wf, 1, 8, 0, 4, 4, a, a, a, g, bk, nullptr, &nn, &ne) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::beam_compile(t, nt, wf, 1, 8, 0, 4, 4, a, a, a, nullptr, bk, nullptr, &nn, &ne) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::beam_compile(t, nt, wf, 1, 8, 0, 4, 4, a, a, a, g, nullptr, nullptr, &nn, &ne) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::beam_compile(t, nt, wf, 1, 8, 0, 4, 4, a, a, a, g, bk, nullptr, nullptr, &ne) == lasr_bias::B_EINVAL && ne == 0);
    }
    // validate_beam: each kind of malformed graph is named; walk's refusals
    {
        const int32_t off[3] = {0, 2, 2}, tok[2] = {1, 3}, nxt[2] = {1, 1};
        const float gn[2] = {0.5f, -0.5f}, bk[2] = {0.0f, -0.5f};
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, gn, bk, 8, 0) == nullptr);        // a negative gain is fine
        CHECK(lasr_bias::validate_beam(0, off, tok, nxt, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(65537, off, tok, nxt, gn, bk, 8, 0) != nullptr);
        const int32_t off1[3] = {1, 2, 2}, off2[3] = {0, 2, 1};
        CHECK(lasr_bias::validate_beam(2, off1, tok, nxt, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off2, tok, nxt, gn, bk, 8, 0) != nullptr);
        const int32_t tok1[2] = {3, 1}, tok2[2] = {1, 1}, tok3[2] = {1, 8}, tok4[2] = {0, 1};
        CHECK(lasr_bias::validate_beam(2, off, tok1, nxt, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok2, nxt, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok3, nxt, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok4, nxt, gn, bk, 8, 0) != nullptr);
        const int32_t nx1[2] = {0, 1}, nx2[2] = {1, 2};
        CHECK(lasr_bias::validate_beam(2, off, tok, nx1, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok, nx2, gn, bk, 8, 0) != nullptr);
        const float g1[2] = {1000.5f, 0.0f}, g2[2] = {0.5f, -inf}, g3[2] = {nan, 0.f};
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, g1, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, g2, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, g3, bk, 8, 0) != nullptr);
        const float k1[2] = {-0.5f, -0.5f}, k2[2] = {0.0f, 0.5f}, k3[2] = {0.0f, nan}, k4[2] = {0.0f, -1000.5f}, k5[2] = {0.0f, -inf};
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, gn, k1, 8, 0) != nullptr);        // back[0] != 0
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, gn, k2, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, gn, k3, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, gn, k4, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, gn, k5, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, nullptr, tok, nxt, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, nullptr, nxt, gn, bk, 8, 0) != nullptr);
        CHECK(lasr_bias::validate_beam(2, off, tok, nxt, gn, nullptr, 8, 0) != nullptr);
        const int32_t ts[3] = {1, 0, 5};
        int end = -7;
        double total = -7.0;
        CHECK(lasr_bias::walk(2, off, tok, nxt, gn, bk, 0, ts, 3, 0, &end, &total, nullptr) == lasr_bias::B_OK && end == 0 && total == 0.0);
        CHECK(lasr_bias::walk(2, off, tok, nxt, gn, bk, 0, ts, 0, 1, &end, &total, nullptr) == lasr_bias::B_OK && end == 1 && total == 0.0);
        CHECK(lasr_bias::walk(2, off, tok, nxt, gn, bk, 0, ts, 3, 2, &end, &total, nullptr) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::walk(2, off, tok, nxt, gn, bk, 0, ts, 3, -1, &end, &total, nullptr) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::walk(2, off, tok, nxt, gn, bk, 0, nullptr, 3, 0, &end, &total, nullptr) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::walk(2, off, tok, nxt, gn, bk, 0, ts, -1, 0, &end, &total, nullptr) == lasr_bias::B_EINVAL);
        CHECK(lasr_bias::walk(2, nullptr, tok, nxt, gn, bk, 0, ts, 3, 0, &end, &total, nullptr) == lasr_bias::B_EINVAL);
        const int32_t neg[1] = {-2};
        CHECK(lasr_bias::walk(2, off, tok, nxt, gn, bk, 0, neg, 1, 0, &end, &total, nullptr) == lasr_bias::B_EINVAL);
    }
    if (fails) { printf("beam_bias_check: %d check(s) FAILED\n", fails); return 1; }
    printf("beam_bias_check: ok\n");
    return 0;
}
