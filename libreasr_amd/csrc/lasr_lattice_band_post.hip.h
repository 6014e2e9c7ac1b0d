// lasr_lattice_band_post.hip.h -- edge posteriors of the banded lattice (lasr_align_band_post_pcm / lasr_align_band_post_feats /
// lasr_lattice_band_post): lasr_lattice_post.hip.h's forward-backward over the band layout of lasr_lattice_band.hip.h.
// With b / e counting -inf outside the windows, alpha and loglik as k_lat_dp_band leaves them:
//   beta[T-1,U] = b[T-1,U]; beta[t,u] = logaddexp(beta[t+1,u] + b[t,u], beta[t,u+1] + e[t,u])   on window cells
//                 (t+1,u) is inside iff t < T-1 and u >= lo[t+1];  (t,u+1) is inside iff u + 1 < lo[t] + w;  outside counts -inf
//   occ_b[t,u]  = exp(alpha[t,u] + b[t,u] + beta[t+1,u] - loglik) where (t+1,u) is inside, else 0;  occ_b[T-1,U] = 1
//   occ_e[t,u]  = exp(alpha[t,u] + e[t,u] + beta[t,u+1] - loglik) where (t,u+1) is inside, else 0
// Engine unit only (lasr_engine.hip), included at its end behind lasr_lattice_band.hip.h (DESIGN 5.6 / 5.7 have the measurements
// behind that place).
//   k_lat_ab_band   alpha and beta of one utterance, one workgroup per direction: both [cells] double, band layout
//   k_lat_occ_band  one thread per label column: the two occupancies of the column's band cells and the statistics of label u + 1
// With w = U + 1 both run k_lat_ab's / k_lat_occ's operations on the same operands in the same order: every result has their bits.
#pragma once

namespace lasr {

struct LatBandAbArgs {
    const float* b; const float* e;   // [cells] each, band layout
    const long long* off; const int* T; const int* U; const int* W; const int* lo_off; const int* lo;
    double* alpha; double* beta;      // [cells] each, band layout
    double* loglik; double* loglik_bwd;   // [n] each
    int w_max;
};
// blockIdx.y == 0: k_lat_dp_band's forward half (its slots t mod w, its ft / fs / fp registers, its double operations, so loglik has
// its bits) with alpha stored at the band cell.  blockIdx.y == 1: beta over the diagonals d = T + U - 1 .. 0.  Frame t is on the
// diagonals s[t] .. s[t] + w - 1 (s[t] = t + lo[t]); slot r starts at the largest t < T with t = r (mod w) and steps t -= w once
// d < s[t] -- s[t - w] + w - 1 < s[t], so no frame is skipped.  Cell (t, u) reads its emission successor (t, u + 1) at its own slot
// and its blank successor (t + 1, u) at slot (r + 1) mod w, both of the previous parity: an existing successor lies on diagonal
// d + 1 and was written there at exactly that slot, and whether it exists follows from lo[t + 1] (kept in fn) and k alone, so a stale
// entry is never read.  One barrier per diagonal.  LDS: two parities of w_max doubles, plain non-negative indices into lat_sh.
template <int NQ>
__global__ __launch_bounds__(256) void k_lat_ab_band(const LatBandAbArgs a) {
    extern __shared__ double lat_sh[];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int T = a.T[i], U = a.U[i], w = a.W[i], wm = a.w_max;
    const float* b = a.b + a.off[i];
    const float* e = a.e + a.off[i];
    const int* lo = a.lo + a.lo_off[i];
    const int D = T + U;                              // diagonals 0 .. T + U - 1
    if (blockIdx.y == 0) {
        double* alpha = a.alpha + a.off[i];
        int ft[NQ], fs[NQ], fp[NQ];                   // per slot: its frame t (T: none left), s[t], lo[t-1] + w
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int r = tid + 256 * q;
            ft[q] = r < w && r < T ? r : T;
            fs[q] = 0; fp[q] = 0;
            if (ft[q] < T) { fs[q] = r + lo[r]; fp[q] = r > 0 ? lo[r - 1] + w : 0; }
        }
        for (int d = 0; d < D; ++d) {
            const int cur = (d & 1) * wm, prv = wm - cur;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int r = tid + 256 * q;
                int t = ft[q];
                if (t < T && d >= fs[q] + w) {        // the frame's last diagonal is behind: the slot's next frame
                    t += w; ft[q] = t;
                    if (t < T) { fs[q] = t + lo[t]; fp[q] = lo[t - 1] + w; }
                }
                if (t >= T || d < fs[q]) continue;
                const int k = d - fs[q], u = fs[q] - t + k;
                double x = -INFINITY, z = -INFINITY;
                if (t > 0 && u < fp[q]) {             // (t - 1, u) is inside its window
                    const int rb = r > 0 ? r - 1 : w - 1;
                    x = lat_sh[prv + rb] + (double)b[(size_t)(t - 1) * w + (u - (fp[q] - w))];
                }
                if (k > 0) z = lat_sh[prv + r] + (double)e[(size_t)t * w + k - 1];
                const double v = d == 0 ? 0.0 : lat_logaddexp(x, z);
                lat_sh[cur + r] = v;
                alpha[(size_t)t * w + k] = v;
            }
            __syncthreads();
        }
        if (tid == 0) a.loglik[i] = lat_sh[((D - 1) & 1) * wm + (T - 1) % w] + (double)b[(size_t)(T - 1) * w + w - 1];
        return;
    }
    double* beta = a.beta + a.off[i];
    int ft[NQ], fs[NQ], fn[NQ];                       // per slot: its frame t (-1: none left), s[t], lo[t+1] (t < T - 1)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int r = tid + 256 * q;
        ft[q] = r < w && r < T ? r + (T - 1 - r) / w * w : -1;
        fs[q] = 0; fn[q] = 0;
        if (ft[q] >= 0) { fs[q] = ft[q] + lo[ft[q]]; fn[q] = ft[q] < T - 1 ? lo[ft[q] + 1] : 0; }
    }
    for (int d = D - 1; d >= 0; --d) {
        const int cur = (d & 1) * wm, prv = wm - cur;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int r = tid + 256 * q;
            int t = ft[q];
            if (t >= 0 && d < fs[q]) {                // the frame's first diagonal is behind: the slot's next frame down
                t -= w; ft[q] = t;
                if (t >= 0) { fs[q] = t + lo[t]; fn[q] = lo[t + 1]; }
            }
            if (t < 0 || d >= fs[q] + w) continue;
            const int k = d - fs[q], u = fs[q] - t + k;
            const size_t at = (size_t)t * w + k;
            double x = -INFINITY, z = -INFINITY;
            if (t < T - 1 && u >= fn[q]) {            // (t + 1, u) is inside its window (u < lo[t] + w <= lo[t+1] + w)
                const int rb = r + 1 < w ? r + 1 : 0;
                x = lat_sh[prv + rb] + (double)b[at];
            }
            if (k + 1 < w) z = lat_sh[prv + r] + (double)e[at];
            const double v = d == D - 1 ? (double)b[at] : lat_logaddexp(x, z);
            lat_sh[cur + r] = v;
            beta[at] = v;
        }
        __syncthreads();
    }
    if (tid == 0 && a.loglik_bwd) a.loglik_bwd[i] = lat_sh[0];   // (0, 0): diagonal 0, slot 0
}

struct LatBandOccArgs {
    const float* b; const float* e;
    const double* alpha; const double* beta; const double* loglik;
    const long long* off; const int* T; const int* U; const int* W; const int* lo_off; const int* lo; const int* tok_off;
    int n, cols;                                                 // column c belongs to the utterance i with tok_off[i] + i <= c
    float* occ_b; float* occ_e;                                  // [cells] each, band layout (optional)
    double* mean; double* var; double* peak; int* peak_frame;    // [sum U] each (optional, all or none)
};
// the first t with lo[t] + w > u, and the last t with lo[t] <= u (lo non-decreasing, lo[0] = 0, lo[T-1] + w = U + 1 > u)
__device__ __forceinline__ int lat_band_first(const int* lo, int T, int w, int u) {
    int x = 0, y = T - 1;
    while (x < y) {
        const int mid = (x + y) >> 1;
        if (lo[mid] + w > u) y = mid; else x = mid + 1;
    }
    return x;
}
__device__ __forceinline__ int lat_band_last(const int* lo, int T, int u) {
    int x = 0, y = T - 1;
    while (x < y) {
        const int mid = (x + y + 1) >> 1;
        if (lo[mid] <= u) x = mid; else y = mid - 1;
    }
    return x;
}
// One thread per label column (i, u), k_lat_occ's flat index, t ascending over the frames whose window holds the column: from the
// first t with lo[t] + w > u to the last with lo[t] <= u.  The 64 lanes of a wave hold consecutive columns; they walk t together
// over the union of their ranges -- first(lowest column) .. last(highest column), which every lane finds for itself by bisection on
// lo -- and a lane is idle on the frames outside its own range, so on one frame consecutive lanes read consecutive k.  Nothing is
// shared between threads and nothing is reduced across them.  At frame t the column's cell is k = u - lo[t]; beta[t + 1, u] is at
// (t + 1) w + u - lo[t + 1].  Frames outside the range would add exact zeros, so the statistics are those of a sum over every t: with
// w = U + 1 the operations and their order are k_lat_occ's.  loglik = -inf: every occupancy 0, mean -1, variance 0, peak 0 on frame -1.
inline __global__ __launch_bounds__(256) void k_lat_occ_band(const LatBandOccArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.cols) return;
    int x = 0, y = a.n - 1;
    while (x < y) {
        const int mid = (x + y + 1) >> 1;
        if (a.tok_off[mid] + mid <= c) x = mid; else y = mid - 1;
    }
    const int i = x, c_i = a.tok_off[i] + i, u = c - c_i;
    const int T = a.T[i], U = a.U[i], w = a.W[i];
    const long long o = a.off[i];
    const float* b = a.b + o;
    const float* e = a.e + o;
    const double* al = a.alpha + o;
    const double* be = a.beta + o;
    const int* lo = a.lo + a.lo_off[i];
    const double ll = a.loglik[i];
    const bool ok = ll != -INFINITY;
    const bool stats = a.mean != nullptr && u < U;
    // the wave's columns of this utterance, and the frames that hold any of them
    const int c0 = c & ~63, c1 = c0 + 63 < a.cols ? c0 + 63 : a.cols - 1;
    const int ua = c0 > c_i ? c0 - c_i : 0, ub = c1 - c_i < U ? c1 - c_i : U;
    const int t_lo = lat_band_first(lo, T, w, ua), t_hi = lat_band_last(lo, T, ub);
    double mean = 0.0, best = -1.0;
    int best_t = -1;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int k = u - lo[t];
        if (k < 0 || k >= w) continue;                // the frame's window does not hold the column
        const size_t at = (size_t)t * w + k;
        const double av = al[at];
        double pb = 0.0, pe = 0.0;
        if (ok) {
            if (t < T - 1) { const int kn = u - lo[t + 1]; if (kn >= 0) pb = exp(av + (double)b[at] + be[(size_t)(t + 1) * w + kn] - ll); }
            else if (u == U) pb = 1.0;
            if (k + 1 < w) pe = exp(av + (double)e[at] + be[at + 1] - ll);
        }
        if (a.occ_b) a.occ_b[o + at] = (float)pb;
        if (a.occ_e) a.occ_e[o + at] = (float)pe;
        mean += (double)t * pe;
        if (pe > best) { best = pe; best_t = t; }
    }
    if (!stats) return;
    const int ks = a.tok_off[i] + u;
    if (!ok) { a.mean[ks] = -1.0; a.var[ks] = 0.0; a.peak[ks] = 0.0; a.peak_frame[ks] = -1; return; }
    double var = 0.0;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int k = u - lo[t];
        if (k < 0 || k >= w) continue;
        const size_t at = (size_t)t * w + k;
        const double pe = k + 1 < w ? exp(al[at] + (double)e[at] + be[at + 1] - ll) : 0.0;
        const double dt = (double)t - mean;
        var += dt * dt * pe;
    }
    a.mean[ks] = mean; a.var[ks] = var; a.peak[ks] = best; a.peak_frame[ks] = best_t;
}

}  // namespace lasr

namespace {

// k_lat_ab_band and k_lat_occ_band over the band lattices b / e (device) of call k (W and lo set, tables uploaded); results stay in the
// workspace until lat_post_copy, which reads a call's sizes alone and so serves the band layout as it is
int lat_band_post_launch(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const float* b, const float* e, const LatPostOut& p) {
    const bool stats = p.tok_mean || p.tok_var || p.tok_peak_frame || p.tok_peak;
    RC(ensure_buf(c, &w.alpha, &w.alpha_n, (size_t)k.cells));
    RC(ensure_buf(c, &w.beta, &w.beta_n, (size_t)k.cells));
    RC(ensure_buf(c, &w.pres, &w.pres_n, (size_t)2 * k.n));
    if (p.occ_blank) RC(ensure_buf(c, &w.occ_b, &w.occ_b_n, (size_t)k.cells));
    if (p.occ_emit) RC(ensure_buf(c, &w.occ_e, &w.occ_e_n, (size_t)k.cells));
    const size_t su = (size_t)std::max(k.sumU, 1ll);
    if (stats) {
        RC(ensure_buf(c, &w.tstat, &w.tstat_n, 3 * su));
        RC(ensure_buf(c, &w.tpeak, &w.tpeak_n, su));
    }
    LatBandAbArgs ab{};
    ab.b = b; ab.e = e; ab.off = k.tab.off; ab.T = k.tab.T; ab.U = k.tab.U; ab.W = k.tab.W; ab.lo_off = k.tab.lo_off; ab.lo = k.tab.lo;
    ab.alpha = w.alpha; ab.beta = w.beta; ab.loglik = w.pres; ab.loglik_bwd = w.pres + k.n;
    ab.w_max = k.Wmax;
    const size_t lds = sizeof(double) * 2 * (size_t)ab.w_max;
    if (k.Wmax <= 256) hipLaunchKernelGGL(k_lat_ab_band<1>, dim3(k.n, 2), dim3(256), lds, c->stream, ab);
    else hipLaunchKernelGGL(k_lat_ab_band<LAT_BAND_WMAX / 256>, dim3(k.n, 2), dim3(256), lds, c->stream, ab);
    if (!p.occ_blank && !p.occ_emit && !stats) return LASR_OK;
    LatBandOccArgs oc{};
    oc.b = b; oc.e = e; oc.alpha = w.alpha; oc.beta = w.beta; oc.loglik = w.pres;
    oc.off = k.tab.off; oc.T = k.tab.T; oc.U = k.tab.U; oc.W = k.tab.W; oc.lo_off = k.tab.lo_off; oc.lo = k.tab.lo; oc.tok_off = k.tab.tok_off;
    oc.n = k.n; oc.cols = (int)(k.sumU + k.n);
    oc.occ_b = p.occ_blank ? w.occ_b : nullptr; oc.occ_e = p.occ_emit ? w.occ_e : nullptr;
    if (stats) { oc.mean = w.tstat; oc.var = w.tstat + su; oc.peak = w.tstat + 2 * su; oc.peak_frame = w.tpeak; }
    hipLaunchKernelGGL(k_lat_occ_band, dim3((oc.cols + 255) / 256), dim3(256), 0, c->stream, oc);
    return LASR_OK;
}

}  // namespace
