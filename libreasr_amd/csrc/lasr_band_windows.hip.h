// lasr_band_windows.hip.h -- the window arithmetic of the banded lattice (lasr_band_windows, lasr_align_band_*).
// Standard C++ only, no HIP include and no context (the name follows the unit's other headers so that the build tracks it): the
// engine includes it ahead of lasr_lattice_band.hip.h, tests/c/band_windows_check.cpp on its own.  Integer arithmetic only.
//
// An utterance of T >= 1 frames and U >= 0 labels with a requested width band >= 1 has the effective width
//   w = U + 1 (T == 1),  min(band, U + 1) (otherwise)
// and frame t owns the columns [lo[t], lo[t] + w).  Windows are valid when lo[0] == 0, lo[T-1] == U + 1 - w, lo is non-decreasing
// and 0 <= lo[t] <= U + 1 - w: every window cell is then a lattice cell, and (0, 0) and (T-1, U) are inside.
//   linear     lo[t] = floor(t (U + 1 - w) / (T - 1))                                       (T == 1: 0)
//   recentred  from a best path frames[0..U) found inside windows lo, with c(t) = #{u : frames[u] < t} (c(T) = U; the path occupies
//              the columns c(t)..c(t+1) on frame t):  lo'[t] = clamp(floor((c(t) + c(t+1)) / 2) - floor(w / 2), 0, U + 1 - w),
//              then lo'[0] = 0 and lo'[T-1] = U + 1 - w
//   touch      1 iff on some frame the path starts on a window's lower edge (lo[t] > 0 and c(t) == lo[t]) or ends on its upper one
//              (lo[t] + w < U + 1 and c(t+1) == lo[t] + w - 1): it ran along an edge that is not the lattice's own
#pragma once

#include <cstdint>
#include <vector>

namespace lasr_bw {

constexpr int BW_OK = 0, BW_EINVAL = -1;              // include/lasr.h: LASR_OK, LASR_EINVAL

inline int width(int T, int U, int band) { return T == 1 || band > U + 1 ? U + 1 : band; }

inline bool valid(int T, int U, int w, const int32_t* lo) {
    if (lo[0] != 0 || lo[T - 1] != U + 1 - w) return false;
    for (int t = 0; t < T; ++t)
        if (lo[t] < 0 || lo[t] > U + 1 - w || (t > 0 && lo[t] < lo[t - 1])) return false;
    return true;
}

inline void linear(int T, int U, int w, int32_t* lo) {
    for (int t = 0; t < T; ++t) lo[t] = T == 1 ? 0 : (int32_t)((long long)t * (U + 1 - w) / (T - 1));
}

// frames: non-decreasing, in [0, T); lo: valid windows of width w; lo_new [T] (must not alias lo) -> touch
inline int recentre(int T, int U, int w, const int32_t* frames, const int32_t* lo, int32_t* lo_new) {
    int touch = 0, u = 0;                             // u = c(t)
    const int top = U + 1 - w;
    for (int t = 0; t < T; ++t) {
        int v = u;                                    // -> c(t + 1)
        while (v < U && frames[v] <= t) ++v;
        if (t == T - 1) v = U;
        if (lo[t] > 0 && u == lo[t]) touch = 1;
        if (lo[t] + w < U + 1 && v == lo[t] + w - 1) touch = 1;
        int x = (u + v) / 2 - w / 2;
        x = x < 0 ? 0 : (x > top ? top : x);
        lo_new[t] = x;
        u = v;
    }
    lo_new[0] = 0; lo_new[T - 1] = top;
    return touch;
}

// the body of lasr_band_windows (include/lasr.h); lo_out may be lo_cur
inline int band_windows(int T, int U, int band, const int32_t* frames, const int32_t* lo_cur, int32_t* lo_out, int* touch) {
    if (T < 1 || U < 0 || band < 1 || !lo_out) return BW_EINVAL;
    const int w = width(T, U, band);
    if (!frames) {
        linear(T, U, w, lo_out);
        if (touch) *touch = 0;
        return BW_OK;
    }
    if (!lo_cur || !valid(T, U, w, lo_cur)) return BW_EINVAL;
    for (int u = 0; u < U; ++u)
        if (frames[u] < 0 || frames[u] >= T || (u > 0 && frames[u] < frames[u - 1])) return BW_EINVAL;
    std::vector<int32_t> nw(T);
    const int tc = recentre(T, U, w, frames, lo_cur, nw.data());
    for (int t = 0; t < T; ++t) lo_out[t] = nw[t];
    if (touch) *touch = tc;
    return BW_OK;
}

}  // namespace lasr_bw
