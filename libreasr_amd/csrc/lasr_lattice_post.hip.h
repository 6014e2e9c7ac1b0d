// lasr_lattice_post.hip.h -- edge posteriors (occupancies) of the teacher-forced RNN-T lattice (lasr_align_post_pcm /
// lasr_align_post_feats / lasr_lattice_post): the backward half of the forward-backward algorithm over the b / e arrays
// that lasr_lattice.hip.h leaves on the device, and per label the statistics of its emission frame.
//   beta[T-1,U] = b[T-1,U]; beta[t,u] = logaddexp(beta[t+1,u] + b[t,u], beta[t,u+1] + e[t,u])   (a missing successor counts -inf)
//   occ_b[t,u]  = exp(alpha[t,u] + b[t,u] + beta[t+1,u] - loglik) (t < T-1), occ_b[T-1,U] = 1, occ_b[T-1,u<U] = 0
//   occ_e[t,u]  = exp(alpha[t,u] + e[t,u] + beta[t,u+1] - loglik) (u < U),   occ_e[t,U] = 0
// Engine unit only (lasr_engine.hip), included after lasr_lattice.hip.h.
//   k_lat_ab   alpha and beta of one utterance, one workgroup per direction: both [cells] double, the layout of b / e
//   k_lat_occ  one thread per label column: the two occupancies of every cell of the column, and mean / variance / peak of the
//              emission frame of label u + 1 from occ_e[., u]
// Both are enqueued on the ctx stream behind whatever produced b and e: stream order is the only ordering needed.
#pragma once

namespace lasr {

constexpr long long LAT_POST_CELLS = 1ll << 24;   // alpha + beta: 16 bytes per cell of workspace (256 MB here)

struct LatAbArgs {
    const float* b; const float* e;   // [cells] each, utterance i at off[i], [T][U + 1]
    const long long* off; const int* T; const int* U;
    double* alpha; double* beta;      // [cells] each
    double* loglik; double* loglik_bwd;   // [n] each
    int u1_max;
};
// blockIdx.y == 0: k_lat_dp's forward recursion (the same double operations in the same order, so loglik has k_lat_dp's bits), every
// alpha[t,u] also stored.  blockIdx.y == 1: beta over descending diagonals; both successors of a cell of diagonal d lie on d + 1, so
// the two-parity LDS scheme and its one barrier per diagonal carry over with the direction reversed.  Which neighbours exist
// follows from (t, u) alone, so a stale entry is never read.
inline __global__ __launch_bounds__(256) void k_lat_ab(const LatAbArgs a) {
    extern __shared__ double lat_sh[];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int T = a.T[i], U = a.U[i], U1 = U + 1;
    const float* b = a.b + a.off[i];
    const float* e = a.e + a.off[i];
    // the two diagonals are addressed as lat_sh[1 + parity * u1_max + u]: plain LDS indices, so every access is a DS instruction (a table
    // of two pointers into lat_sh makes them generic, and a FLAT access picks its aperture from the base register alone: a base of
    // "LDS address 0 minus 8" plus an immediate offset of 8 lands outside the LDS aperture and faults).  One double of padding in
    // front keeps the lowest address the compiler may form for [prv + u - 1], u = 0, at zero or above.
    const int u1m = a.u1_max;
    const int D = T + U;                              // diagonals 0 .. T + U - 1
    if (blockIdx.y == 0) {
        double* alpha = a.alpha + a.off[i];
        for (int d = 0; d < D; ++d) {
            const int cur = 1 + (d & 1) * u1m, prv = 2 + u1m - cur;
            const int u_lo = d - (T - 1) > 0 ? d - (T - 1) : 0, u_hi = d < U ? d : U;
            for (int u = u_lo + tid; u <= u_hi; u += 256) {
                const int t = d - u;
                double x = -INFINITY, z = -INFINITY;
                if (t > 0) x = lat_sh[prv + u] + (double)b[(size_t)(t - 1) * U1 + u];
                if (u > 0) z = lat_sh[prv + u - 1] + (double)e[(size_t)t * U1 + u - 1];
                const double v = d == 0 ? 0.0 : lat_logaddexp(x, z);
                lat_sh[cur + u] = v;
                alpha[(size_t)t * U1 + u] = v;
            }
            __syncthreads();
        }
        if (tid == 0) a.loglik[i] = lat_sh[1 + ((D - 1) & 1) * u1m + U] + (double)b[(size_t)(T - 1) * U1 + U];
        return;
    }
    double* beta = a.beta + a.off[i];
    for (int d = D - 1; d >= 0; --d) {
        const int cur = 1 + (d & 1) * u1m, prv = 2 + u1m - cur;
        const int u_lo = d - (T - 1) > 0 ? d - (T - 1) : 0, u_hi = d < U ? d : U;
        for (int u = u_lo + tid; u <= u_hi; u += 256) {
            const int t = d - u;
            const size_t at = (size_t)t * U1 + u;
            double x = -INFINITY, z = -INFINITY;
            if (t < T - 1) x = lat_sh[prv + u] + (double)b[at];
            if (u < U) z = lat_sh[prv + u + 1] + (double)e[at];
            const double v = d == D - 1 ? (double)b[at] : lat_logaddexp(x, z);
            lat_sh[cur + u] = v;
            beta[at] = v;
        }
        __syncthreads();
    }
    if (tid == 0 && a.loglik_bwd) a.loglik_bwd[i] = lat_sh[1];
}

struct LatOccArgs {
    const float* b; const float* e;
    const double* alpha; const double* beta; const double* loglik;
    const long long* off; const int* T; const int* U; const int* tok_off;   // column c of the call belongs to the utterance i with
    int n, cols;                                                            // tok_off[i] + i <= c: cols = sum (U_i + 1)
    float* occ_b; float* occ_e;                                  // [cells] each (optional)
    double* mean; double* var; double* peak; int* peak_frame;    // [sum U] each (optional, all or none)
};
// One thread per label column (i, u), t ascending: consecutive lanes read consecutive u of every row, nothing is shared between
// threads and nothing is reduced across them, so a result does not depend on the launch.  Column u < U carries the statistics of
// label u + 1 (p(t) = occ_e[t,u]): sum t p and the first largest p in one pass, the variance about that mean in a second one over
// the double occupancies, recomputed.  loglik = -inf: every occupancy 0, mean -1, variance 0, peak 0 on frame -1.
inline __global__ __launch_bounds__(256) void k_lat_occ(const LatOccArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.cols) return;
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.tok_off[mid] + mid <= c) lo = mid; else hi = mid - 1;
    }
    const int i = lo, u = c - (a.tok_off[i] + i);
    const int T = a.T[i], U = a.U[i], U1 = U + 1;
    const long long o = a.off[i];
    const float* b = a.b + o;
    const float* e = a.e + o;
    const double* al = a.alpha + o;
    const double* be = a.beta + o;
    const double ll = a.loglik[i];
    const bool ok = ll != -INFINITY;
    const bool stats = a.mean != nullptr && u < U;
    double mean = 0.0, best = -1.0;
    int best_t = -1;
    for (int t = 0; t < T; ++t) {
        const size_t at = (size_t)t * U1 + u;
        const double av = al[at];
        double pb = 0.0, pe = 0.0;
        if (ok) {
            if (t < T - 1) pb = exp(av + (double)b[at] + be[at + U1] - ll);
            else if (u == U) pb = 1.0;
            if (u < U) pe = exp(av + (double)e[at] + be[at + 1] - ll);
        }
        if (a.occ_b) a.occ_b[o + at] = (float)pb;
        if (a.occ_e) a.occ_e[o + at] = (float)pe;
        mean += (double)t * pe;
        if (pe > best) { best = pe; best_t = t; }
    }
    if (!stats) return;
    const int k = a.tok_off[i] + u;
    if (!ok) { a.mean[k] = -1.0; a.var[k] = 0.0; a.peak[k] = 0.0; a.peak_frame[k] = -1; return; }
    double var = 0.0;
    for (int t = 0; t < T; ++t) {
        const size_t at = (size_t)t * U1 + u;
        const double pe = exp(al[at] + (double)e[at] + be[at + 1] - ll);
        const double dt = (double)t - mean;
        var += dt * dt * pe;
    }
    a.mean[k] = mean; a.var[k] = var; a.peak[k] = best; a.peak_frame[k] = best_t;
}

}  // namespace lasr

namespace {

bool lat_post_any(const LatPostOut& p) {
    return p.loglik_bwd || p.occ_blank || p.occ_emit || p.tok_mean || p.tok_var || p.tok_peak_frame || p.tok_peak;
}

// k_lat_ab and k_lat_occ over the lattices b / e (device) of call k; results stay in the workspace until lat_post_copy
int lat_post_launch(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const float* b, const float* e, const LatPostOut& p) {
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
    LatAbArgs ab{};
    ab.b = b; ab.e = e; ab.off = k.tab.off; ab.T = k.tab.T; ab.U = k.tab.U;
    ab.alpha = w.alpha; ab.beta = w.beta; ab.loglik = w.pres; ab.loglik_bwd = w.pres + k.n;
    ab.u1_max = k.Umax + 1;
    hipLaunchKernelGGL(k_lat_ab, dim3(k.n, 2), dim3(256), sizeof(double) * (2 * (size_t)ab.u1_max + 1), c->stream, ab);
    if (!p.occ_blank && !p.occ_emit && !stats) return LASR_OK;
    LatOccArgs oc{};
    oc.b = b; oc.e = e; oc.alpha = w.alpha; oc.beta = w.beta; oc.loglik = w.pres;
    oc.off = k.tab.off; oc.T = k.tab.T; oc.U = k.tab.U; oc.tok_off = k.tab.tok_off;
    oc.n = k.n; oc.cols = (int)(k.sumU + k.n);
    oc.occ_b = p.occ_blank ? w.occ_b : nullptr; oc.occ_e = p.occ_emit ? w.occ_e : nullptr;
    if (stats) { oc.mean = w.tstat; oc.var = w.tstat + su; oc.peak = w.tstat + 2 * su; oc.peak_frame = w.tpeak; }
    hipLaunchKernelGGL(k_lat_occ, dim3((oc.cols + 255) / 256), dim3(256), 0, c->stream, oc);
    return LASR_OK;
}

// the posterior results of the call to the host (stream idle)
int lat_post_copy(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const LatPostOut& p) {
    const size_t su = (size_t)std::max(k.sumU, 1ll), nu = (size_t)k.sumU, nc = (size_t)k.cells;
    if (p.loglik) HIPCHK(c, hipMemcpy(p.loglik, w.pres, sizeof(double) * k.n, hipMemcpyDeviceToHost));
    if (p.loglik_bwd) HIPCHK(c, hipMemcpy(p.loglik_bwd, w.pres + k.n, sizeof(double) * k.n, hipMemcpyDeviceToHost));
    if (p.occ_blank) HIPCHK(c, hipMemcpy(p.occ_blank, w.occ_b, sizeof(float) * nc, hipMemcpyDeviceToHost));
    if (p.occ_emit) HIPCHK(c, hipMemcpy(p.occ_emit, w.occ_e, sizeof(float) * nc, hipMemcpyDeviceToHost));
    if (!nu) return LASR_OK;
    if (p.tok_mean) HIPCHK(c, hipMemcpy(p.tok_mean, w.tstat, sizeof(double) * nu, hipMemcpyDeviceToHost));
    if (p.tok_var) HIPCHK(c, hipMemcpy(p.tok_var, w.tstat + su, sizeof(double) * nu, hipMemcpyDeviceToHost));
    if (p.tok_peak) HIPCHK(c, hipMemcpy(p.tok_peak, w.tstat + 2 * su, sizeof(double) * nu, hipMemcpyDeviceToHost));
    if (p.tok_peak_frame) HIPCHK(c, hipMemcpy(p.tok_peak_frame, w.tpeak, sizeof(int) * nu, hipMemcpyDeviceToHost));
    return LASR_OK;
}

}  // namespace
