// band_windows_check.cpp -- libreasr_amd/csrc/lasr_band_windows.hip.h (the window arithmetic of the banded lattice, standard C++ only)
// under AddressSanitizer + UndefinedBehaviorSanitizer: random (T, U, band) with random monotone paths against a restatement that
// counts c(t) directly, through exact-size buffers with guard words; the result is always a valid set of windows; iterating the
// routine on its own output stays valid; the argument checks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libreasr_amd/csrc/lasr_band_windows.hip.h"

#define CHECK(x) do { if (!(x)) { std::printf("band_windows_check: FAILED %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static unsigned rnd_state = 2468u;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static int one_case(int T, int U, int band) {
    const int w = T == 1 ? U + 1 : (band < U + 1 ? band : U + 1);
    CHECK(lasr_bw::width(T, U, band) == w);
    std::vector<int32_t> lo(T + 1, 777);
    int touch = -1;
    CHECK(lasr_bw::band_windows(T, U, band, nullptr, nullptr, lo.data(), &touch) == lasr_bw::BW_OK);
    CHECK(lo[T] == 777 && touch == 0 && lasr_bw::valid(T, U, w, lo.data()));
    for (int t = 0; t < T; ++t) CHECK(lo[t] == (T == 1 ? 0 : (int32_t)((long long)t * (U + 1 - w) / (T - 1))));
    for (int round = 0; round < 3; ++round) {
        // a random monotone path (exact size: the heap buffer has no slack for a read past U)
        std::vector<int32_t> fr(U);
        for (int u = 0; u < U; ++u) fr[u] = (int32_t)(rnd() % T);
        for (int u = 1; u < U; ++u)
            for (int j = u; j > 0 && fr[j - 1] > fr[j]; --j) { const int32_t x = fr[j]; fr[j] = fr[j - 1]; fr[j - 1] = x; }
        std::vector<int32_t> cur(lo.begin(), lo.begin() + T), out(T + 1, 555);
        int tc = -1;
        CHECK(lasr_bw::band_windows(T, U, band, fr.data(), cur.data(), out.data(), &tc) == lasr_bw::BW_OK);
        CHECK(out[T] == 555 && lasr_bw::valid(T, U, w, out.data()));
        // restatement
        int want_touch = 0;
        for (int t = 0; t < T; ++t) {
            int c0 = 0, c1 = 0;
            for (int u = 0; u < U; ++u) { c0 += fr[u] < t; c1 += fr[u] < t + 1; }
            if (t == T - 1) c1 = U;
            if ((cur[t] > 0 && c0 == cur[t]) || (cur[t] + w < U + 1 && c1 == cur[t] + w - 1)) want_touch = 1;
            int x = (c0 + c1) / 2 - w / 2;
            x = x < 0 ? 0 : (x > U + 1 - w ? U + 1 - w : x);
            if (t == 0) x = 0;
            if (t == T - 1) x = U + 1 - w;
            CHECK(out[t] == x);
        }
        CHECK(tc == want_touch);
        // in place, and without the touch output
        std::vector<int32_t> same(cur);
        CHECK(lasr_bw::band_windows(T, U, band, fr.data(), same.data(), same.data(), nullptr) == lasr_bw::BW_OK);
        for (int t = 0; t < T; ++t) CHECK(same[t] == out[t]);
        for (int t = 0; t < T; ++t) lo[t] = out[t];   // the next round starts from these windows
    }
    return 0;
}

int main() {
    const int named[][3] = {{1, 0, 1}, {1, 5, 2}, {2, 0, 3}, {5, 0, 4}, {2, 7, 1}, {40, 12, 6}, {96, 64, 12}, {3, 9, 10}, {3, 9, 11}};
    for (const auto& s : named)
        if (one_case(s[0], s[1], s[2])) return 1;
    for (int it = 0; it < 400; ++it)
        if (one_case(1 + (int)(rnd() % 40), (int)(rnd() % 30), 1 + (int)(rnd() % 12))) return 1;
    // argument checks
    int32_t fr[3] = {0, 1, 1}, lo[4] = {0, 0, 1, 2}, out[4];
    int tc = -1;
    CHECK(lasr_bw::band_windows(4, 3, 2, fr, lo, out, &tc) == lasr_bw::BW_OK);
    CHECK(lasr_bw::band_windows(0, 3, 2, fr, lo, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, -1, 2, fr, lo, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 0, fr, lo, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 2, fr, lo, nullptr, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 2, fr, nullptr, out, &tc) == lasr_bw::BW_EINVAL);
    int32_t down[3] = {2, 1, 1}, far[3] = {0, 1, 4}, neg[3] = {-1, 1, 1};
    CHECK(lasr_bw::band_windows(4, 3, 2, down, lo, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 2, far, lo, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 2, neg, lo, out, &tc) == lasr_bw::BW_EINVAL);
    int32_t lo_a[4] = {1, 1, 1, 2}, lo_b[4] = {0, 1, 0, 2}, lo_c[4] = {0, 1, 2, 1}, lo_d[4] = {0, 1, 3, 2};
    CHECK(lasr_bw::band_windows(4, 3, 2, fr, lo_a, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 2, fr, lo_b, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 2, fr, lo_c, out, &tc) == lasr_bw::BW_EINVAL);
    CHECK(lasr_bw::band_windows(4, 3, 2, fr, lo_d, out, &tc) == lasr_bw::BW_EINVAL);
    std::printf("band_windows_check: ok\n");
    return 0;
}
