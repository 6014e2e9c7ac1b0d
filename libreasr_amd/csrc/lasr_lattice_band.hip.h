// lasr_lattice_band.hip.h -- the teacher-forced RNN-T lattice restricted to a band of w labels per frame (lasr_align_band_pcm /
// lasr_align_band_feats / lasr_lattice_band_dp): frame t owns the columns [lo[t], lo[t] + w) (lasr_band_windows.hip.h), the
// joint is evaluated on those cells alone and both recursions of lasr_lattice.hip.h run on them, a predecessor outside its frame's
// window counting -inf.  Cost and workspace grow with T w instead of T (U + 1), and the dynamic programme's LDS with w alone.
// Engine unit only (lasr_engine.hip), included at its end, after lasr_band_windows.hip.h (DESIGN 5.6 has the measurement behind that
// place); LAT_BAND_WMAX / LAT_BAND_UMAX and the two functions align_impl calls are declared in the unit, in front of align_impl.
//
// Band layout: cell = off_i + t w_i + k with u = lo[t] + k -- the flat order of the blocks and of the two lattice arrays.
//   LatBandMap      (lasr_lattice.hip.h) that layout for k_lat_ja / k_lat_pick: the same LAT_R blocks, logits GEMM, lat_row_lse and
//                   label tail, so from the same logits a term has the bits lasr_align_* gives the same cell
//   k_lat_dp_band   both recursions of one utterance per workgroup over anti-diagonals, LDS indexed by t mod w
// The call description, its layout and its tables are lasr_lattice_tables.hip.h's LatCall with W and lo set.  The band's posteriors
// (lasr_align_band_post_*) are lasr_lattice_band_post.hip.h, included behind this header; lat_finish_band launches them.
#pragma once

namespace lasr {

struct LatBandDpArgs {
    const float* b; const float* e;   // [cells] each, band layout
    const long long* off; const int* T; const int* U; const int* W; const int* lo_off; const int* lo; const int* tok_off;
    double* loglik; double* viterbi;  // [n] (viterbi: with vit)
    int* frames; float* logps;        // [sum U] (optional, with vit)
    unsigned* bp; const long long* bp_off;   // global back-pointer words of the utterances that exceed the LDS share
    int w_max, lds_bp_words, vit;
};
// Forward algorithm and Viterbi of one utterance per workgroup, anti-diagonals d = t + u in order, k_lat_dp's operations on k_lat_dp's
// operands: with w = U + 1 every result has k_lat_dp's bits.  s[t] = t + lo[t] is strictly increasing and frame t is on the
// diagonals s[t] .. s[t] + w - 1, so the frames of one diagonal are a contiguous range of at most w: a diagonal lives in LDS at
// t mod w, two parities of alpha and two of Viterbi scores, 4 w doubles whatever T and U are.  A thread owns the slots r = tid + 256 q
// (q < NQ) and walks the frames r, r + w, r + 2 w, .. of each, keeping t, s[t] and lo[t-1] + w in registers; cell (t, u) reads
// its emission predecessor (t, u - 1) at its own slot and its blank predecessor (t - 1, u) at slot (r - 1) mod w of the previous
// parity.  Whether either exists follows from lo, so a stale entry is never read; one barrier per diagonal.  LDS is addressed by
// plain indices into lat_sh (see k_lat_ab), none of them negative.  Back-pointers: one bit per band cell.
template <int NQ>
__global__ __launch_bounds__(256) void k_lat_dp_band(const LatBandDpArgs a) {
    extern __shared__ double lat_sh[];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int T = a.T[i], U = a.U[i], w = a.W[i], wm = a.w_max;
    const float* b = a.b + a.off[i];
    const float* e = a.e + a.off[i];
    const int* lo = a.lo + a.lo_off[i];
    const long long cells = (long long)T * w;
    const long long words = (cells + 31) >> 5;
    unsigned* bp = nullptr;
    if (a.vit) {
        bp = words <= a.lds_bp_words ? (unsigned*)(lat_sh + 4 * (size_t)wm) : a.bp + a.bp_off[i];
        for (long long x = tid; x < words; x += 256) bp[x] = 0u;
        __syncthreads();
    }
    int ft[NQ], fs[NQ], fp[NQ];                       // per slot: its frame t (T: none left), s[t], lo[t-1] + w
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int r = tid + 256 * q;
        ft[q] = r < w && r < T ? r : T;
        fs[q] = 0; fp[q] = 0;
        if (ft[q] < T) { fs[q] = r + lo[r]; fp[q] = r > 0 ? lo[r - 1] + w : 0; }
    }
    const int D = T + U;                              // diagonals 0 .. T + U - 1
    for (int d = 0; d < D; ++d) {
        const int cur = (d & 1) * wm, prv = wm - cur;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int r = tid + 256 * q;
            int t = ft[q];
            if (t < T && d >= fs[q] + w) {            // the frame's last diagonal is behind: the slot's next frame (s[t + w] >= s[t] + w)
                t += w; ft[q] = t;
                if (t < T) { fs[q] = t + lo[t]; fp[q] = lo[t - 1] + w; }
            }
            if (t >= T || d < fs[q]) continue;
            const int k = d - fs[q], u = fs[q] - t + k;
            double x = -INFINITY, z = -INFINITY, vx = -INFINITY, vz = -INFINITY;
            if (t > 0 && u < fp[q]) {                 // (t - 1, u) is inside its window (u >= lo[t] >= lo[t-1])
                const int rb = r > 0 ? r - 1 : w - 1;
                const double bb = (double)b[(size_t)(t - 1) * w + (u - (fp[q] - w))];
                x = lat_sh[prv + rb] + bb;
                if (a.vit) vx = lat_sh[2 * wm + prv + rb] + bb;
            }
            if (k > 0) {
                const double ee = (double)e[(size_t)t * w + k - 1];
                z = lat_sh[prv + r] + ee;
                if (a.vit) vz = lat_sh[2 * wm + prv + r] + ee;
            }
            if (d == 0) { lat_sh[cur + r] = 0.0; if (a.vit) lat_sh[2 * wm + cur + r] = 0.0; continue; }
            lat_sh[cur + r] = lat_logaddexp(x, z);
            if (a.vit) {
                const bool emit = vz > vx;            // a tie takes the blank predecessor
                lat_sh[2 * wm + cur + r] = emit ? vz : vx;
                if (emit) {
                    const long long c = (long long)t * w + k;
                    atomicOr(&bp[c >> 5], 1u << (c & 31));
                }
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int last = ((D - 1) & 1) * wm, rl = (T - 1) % w;
    const double bl = (double)b[(size_t)(T - 1) * w + w - 1];
    a.loglik[i] = lat_sh[last + rl] + bl;
    if (!a.vit) return;
    const double best = lat_sh[2 * wm + last + rl] + bl;
    if (a.viterbi) a.viterbi[i] = best;
    if (!a.frames && !a.logps) return;
    const int o = a.tok_off[i];
    int t = T - 1, u = U;
    if (best > -INFINITY) {
        while (u > 0) {                               // (t, 0) is reached by blanks alone
            const int k = u - lo[t];
            if (k < 0 || k >= w) break;               // (a finite best path stays inside the windows: never taken)
            const long long c = (long long)t * w + k;
            if (t == 0 || ((bp[c >> 5] >> (c & 31)) & 1u)) {  // (frame 0 has no blank predecessor)
                if (k == 0) break;
                if (a.frames) a.frames[o + u - 1] = t;
                if (a.logps) a.logps[o + u - 1] = e[(size_t)t * w + k - 1];
                --u;
            } else --t;
        }
    }
    for (; u > 0; --u) {                              // no path through the windows: frames -1, logps 0
        if (a.frames) a.frames[o + u - 1] = -1;
        if (a.logps) a.logps[o + u - 1] = 0.f;
    }
}

}  // namespace lasr

namespace {

// k_lat_dp_band over the band lattices b / e (device) of call k (W set); results stay in the workspace
int lat_band_run_dp(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const float* b, const float* e, bool vit, bool want_frames,
                    bool want_logps) {
    RC(lat_dp_workspace(c, w, k, vit));
    LatBandDpArgs a{};
    a.b = b; a.e = e; a.off = k.tab.off; a.T = k.tab.T; a.U = k.tab.U; a.W = k.tab.W; a.lo_off = k.tab.lo_off; a.lo = k.tab.lo;
    a.tok_off = k.tab.tok_off;
    a.loglik = w.res; a.viterbi = vit ? w.res + k.n : nullptr;
    a.frames = vit && want_frames ? w.frames : nullptr; a.logps = vit && want_logps ? w.logps : nullptr;
    a.bp = w.bp; a.bp_off = k.tab.bp_off;
    a.w_max = k.Wmax; a.vit = vit ? 1 : 0; a.lds_bp_words = vit ? k.lds_bp_words : 0;
    const size_t lds = sizeof(double) * (vit ? 4 : 2) * (size_t)a.w_max + sizeof(unsigned) * (size_t)a.lds_bp_words;
    if (k.Wmax <= 256) hipLaunchKernelGGL(k_lat_dp_band<1>, dim3(k.n), dim3(256), lds, c->stream, a);
    else hipLaunchKernelGGL(k_lat_dp_band<LAT_BAND_WMAX / 256>, dim3(k.n), dim3(256), lds, c->stream, a);
    return LASR_OK;
}

// the banded inputs and outputs of lasr_align_band_* beside lasr_align_*'s
struct LatBandIO { int band, max_passes; const int32_t* lo_in; int32_t* lo_out; int32_t* passes; int32_t* touch; LatCall* plan; };

// a banded posterior call keeps alpha and beta of every BAND cell (lasr_lattice_band_post.hip.h): refused beyond LAT_POST_CELLS
int lat_band_post_cells(lasr_ctx* c, const LatCall& k) {
    if (k.cells > LAT_POST_CELLS) return fail(c, LASR_EINVAL, "posteriors of a band lattice of %lld cells (at most %lld)", k.cells, LAT_POST_CELLS);
    return LASR_OK;
}
int lat_band_post_launch(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const float* b, const float* e, const LatPostOut& p);

// widths and first windows of a lasr_align_band_* call from its frame counts (host only; nothing has changed when it fails).
// post: a lasr_align_band_post_* call that asks for posteriors
int lat_band_plan(lasr_ctx* c, const int* T, const int32_t* U, int n, const LatBandIO& io, bool post) {
    LatCall& k = *io.plan;
    if (io.band < 1 || io.max_passes < 1) return fail(c, LASR_EINVAL, "band = %d, max_passes = %d (both >= 1)", io.band, io.max_passes);
    k.n = n;
    k.T.assign(T, T + n); k.U.assign(U, U + n); k.W.resize(n);
    for (int i = 0; i < n; ++i) {
        k.W[i] = lasr_bw::width(T[i], U[i], io.band);
        if (k.W[i] > LAT_BAND_WMAX)
            return fail(c, LASR_EINVAL, "utterance %d: a window of %d labels (at most %d; a single frame needs U + 1)", i, k.W[i], LAT_BAND_WMAX);
    }
    RC(lat_layout_checked(c, k));
    if (post) RC(lat_band_post_cells(c, k));
    k.lo.resize((size_t)k.sumT);
    for (int i = 0; i < n; ++i) {
        int32_t* lo = k.lo.data() + k.lo_off[i];
        if (!io.lo_in) { lasr_bw::linear(T[i], U[i], k.W[i], lo); continue; }
        memcpy(lo, io.lo_in + k.lo_off[i], sizeof(int32_t) * T[i]);
        if (!lasr_bw::valid(T[i], U[i], k.W[i], lo)) return fail(c, LASR_EINVAL, "utterance %d: lo_in is not a valid set of windows of width %d", i, k.W[i]);
    }
    return LASR_OK;
}

// lat_finish over a band (io.plan: lat_band_plan's, slots not yet set): the teacher-forced predictor once, then per pass the band cells of
// every utterance through the joint and the banded dynamic programme; between passes the best paths come to the host and
// lasr_band_windows' routine recentres the windows.  The loop ends when no utterance touches, no window changed, or at max_passes.
// post (lasr_align_band_post_*): alpha / beta and the occupancies behind the loop, on the last pass's b / e, windows and tables.
int lat_finish_band(lasr_ctx* c, const int* slots, int n, const int32_t* tokens, const LatOut& o, const LatBandIO& io, const LatPostOut* post) {
    LatCall& k = *io.plan;
    lasr_ctx::Lattice& w = c->lat;
    k.slot.assign(slots, slots + n);
    lat_mark(c, w, 1);
    const int Ml = lat_rows(slots, n);
    RC(lat_workspace(c, w, k.Umax, Ml, k.cells));
    DecView v = sync_view(c, 1);
    RC(lat_teacher_force(c, w, v, slots, n, k.U, k.Umax, tokens, Ml));
    lat_mark(c, w, 2);
    const bool loop = io.max_passes > 1, path = loop || io.touch;
    const bool vit = o.viterbi || o.frames || o.logps || path;
    TabImage img;
    std::vector<int32_t> fr((size_t)std::max(k.sumU, 1ll)), lo_new((size_t)k.sumT), touch(n, 0);
    std::vector<double> res((size_t)2 * n);
    int passes = 0;
    for (;;) {
        lat_pack(k, tokens, img);                     // (the windows k.lo are the pass's)
        RC(lat_upload(c, w, img));
        lat_blocks(c, w, v, LatBandMap{k.tab}, k.cells, Ml);
        lat_mark(c, w, 3);
        RC(lat_band_run_dp(c, w, k, w.b, w.e, vit, o.frames || path, o.logps != nullptr));
        lat_mark(c, w, 4);
        ++passes;
        if (!path) break;
        // ---- the pass's best paths on the host: touch against the windows they were found in, and the recentred windows
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        c->cmd_inflight = 0;
        HIPCHK(c, hipMemcpy(res.data(), w.res, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
        if (k.sumU) HIPCHK(c, hipMemcpy(fr.data(), w.frames, sizeof(int) * (size_t)k.sumU, hipMemcpyDeviceToHost));
        bool any_touch = false, changed = false;
        for (int i = 0; i < n; ++i) {
            const int32_t* lo = k.lo.data() + k.lo_off[i];
            int32_t* nw = lo_new.data() + k.lo_off[i];
            if (res[n + i] > -INFINITY) touch[i] = lasr_bw::recentre(k.T[i], k.U[i], k.W[i], fr.data() + k.tok_off[i], lo, nw);
            else { touch[i] = 0; memcpy(nw, lo, sizeof(int32_t) * k.T[i]); }       // no path through the windows: they stay
            any_touch = any_touch || touch[i];
            changed = changed || memcmp(nw, lo, sizeof(int32_t) * k.T[i]) != 0;
        }
        if (!any_touch || !changed || passes >= io.max_passes) break;
        k.lo.swap(lo_new);
    }
    if (post) {                                       // (k.lo and k.tab are the last pass's; loglik stays the dynamic programme's)
        RC(lat_band_post_launch(c, w, k, w.b, w.e, *post));
        lat_mark(c, w, 5);
        w.ev_post = c->profiling && w.ev_ok;
    }
    RC(lat_release(c, slots, n));
    RC(lat_copy_out(c, w, k, o));
    if (post) RC(lat_post_copy(c, w, k, *post));
    if (io.lo_out) memcpy(io.lo_out, k.lo.data(), sizeof(int32_t) * (size_t)k.sumT);
    for (int i = 0; i < n; ++i) {
        if (io.passes) io.passes[i] = passes;
        if (io.touch) io.touch[i] = touch[i];
    }
    lat_times(c, w);
    return LASR_OK;
}

}  // namespace
