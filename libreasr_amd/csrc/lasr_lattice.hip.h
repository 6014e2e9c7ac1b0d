// lasr_lattice.hip.h -- the teacher-forced RNN-T lattice (lasr_align_pcm / lasr_align_feats / lasr_lattice_dp):
// for a transcript the caller already has, log_softmax(joint(g_u, f_t)) at the blank and at the next label of every cell (t, u),
// the forward algorithm over it (log P(y | x)) and the best path (forced alignment).
// Engine unit only (lasr_engine.hip), included after lasr_decode.hip.h.
//
// Cells of all utterances of a call are enumerated in one flat order -- utterance i, then t, then u: cell = off_i + t (U_i + 1) + u,
// which is also the layout of the two lattice arrays -- and go through the joint in blocks of LAT_R rows:
//   k_lat_ja    ja[row] = tanh(pe[t][slot] + lat_pp[u][slot])             fragment-major, the A operand of the logits GEMM
//   logits GEMM [LAT_R][V] f32 (launch_logits_from: the decode path's kernel over an explicit activation buffer)
//   k_lat_pick  b[cell] = z[blank] - lse, e[cell] = z[y_{u+1}] - lse       the [LAT_R][V] logits never leave the device
// and k_lat_dp runs both recursions of one utterance per workgroup.  Everything is enqueued on the ctx stream with the engine idle.
#pragma once

namespace lasr {

constexpr int LAT_R = 1024;        // lattice rows per block (>= 512: the 64 x 64 logits tiling where V % 64 == 0)
constexpr int LAT_UMAX = 1535;     // labels per transcript: four diagonals of doubles (48 KB) + 16 KB of back-pointers = 64 KB of LDS
constexpr int LAT_BP_WORDS = 4096; // back-pointer words a workgroup keeps in LDS (T (U + 1) <= 131 072 cells); larger: global

struct LatTab {                    // per-call tables (device), one entry per utterance
    const long long* off;          // [n + 1] first cell
    const int* T;                  // [n] frames
    const int* U;                  // [n] labels
    const int* slot;               // [n] batch row of the utterance
    const int* tok_off;            // [n] first label in tok
    const int* tok;                // [sum U]
    int n;
};
// utterance of a flat cell index (off is ascending, off[n] = cells)
__device__ __forceinline__ int lat_find(const LatTab& tb, long long cell) {
    int lo = 0, hi = tb.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb.off[mid] <= cell) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// joint activation of the block's rows: one workgroup per row, consecutive threads read consecutive j of both halves
inline __global__ __launch_bounds__(256) void k_lat_ja(const float* __restrict__ pe, const float* __restrict__ lat_pp, const LatTab tb,
                                                       long long cell0, int n_rows, void* __restrict__ ja, int J, int M, int Ml, int mt, int bf) {
    const int row = blockIdx.x;
    if (row >= n_rows) return;
    const long long cell = cell0 + row;
    const int i = lat_find(tb, cell);
    const int U1 = tb.U[i] + 1, rel = (int)(cell - tb.off[i]);
    const int t = rel / U1, u = rel - t * U1, s = tb.slot[i];
    const float* e = pe + ((size_t)t * M + s) * J;
    const float* p = lat_pp + ((size_t)u * Ml + s) * J;
    for (int j = threadIdx.x; j < J; j += 256) act_st(bf, ja, act_off(bf, row, j, mt), tanhf(e[j] + p[j]));
}

// log-softmax of a lattice row at two entries, one wave per row.  The f32 maximum and exp-sum are k_select's: a lane holds the
// logits of k_select's "virtual threads" lane + 64 w (w = 0..3), every virtual thread adds its terms in ascending order, the four
// virtual waves are reduced by the same butterfly and added in the same order -- so from the same logits a term is bit for bit the
// log p the decode path reports for the same predictor state and frame.
inline __global__ __launch_bounds__(256) void k_lat_pick(const float* __restrict__ logits, const LatTab tb, long long cell0, int n_rows,
                                                         int V, int blank, float* __restrict__ b_out, float* __restrict__ e_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;                       // wave-uniform
    const float* z = logits + (size_t)row * V;
    float m = -INFINITY;
    for (int j = lane; j < V; j += 64) m = fmaxf(m, z[j]);
    m = wave_max_f32(m);
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float part = 0.f;
        for (int j = lane + 64 * w; j < V; j += 256) part += expf(z[j] - m);
        sum += wave_sum_f32(part);
    }
    if (lane != 0) return;
    const float lse = logf(sum);
    const long long cell = cell0 + row;
    const int i = lat_find(tb, cell);
    const int Ui = tb.U[i], rel = (int)(cell - tb.off[i]);
    const int u = rel % (Ui + 1);
    b_out[cell] = (z[blank] - m) - lse;
    e_out[cell] = u < Ui ? (z[tb.tok[tb.tok_off[i] + u]] - m) - lse : 0.f;
}

struct LatDpArgs {
    const float* b; const float* e;   // [cells] each, utterance i at off[i], [T][U + 1]
    const long long* off; const int* T; const int* U; const int* tok_off;
    double* loglik; double* viterbi;  // [n] (viterbi: with vit)
    int* frames; float* logps;        // [sum U] (optional, with vit)
    unsigned* bp; const long long* bp_off;   // global back-pointer words of the utterances that exceed the LDS share
    int u1_max, lds_bp_words, vit;
};
__device__ __forceinline__ double lat_logaddexp(double x, double z) {
    const double m = fmax(x, z);
    // both predecessors impossible: no NaN from inf - inf.  fmax drops a NaN operand, so (NaN, -inf) arrives here too (a NaN term
    // on a cell with a single predecessor: frame 0, column 0): the sum is -inf for (-inf, -inf) and keeps that NaN, as
    // np.logaddexp does
    if (m == -INFINITY) return x + z;
    return m + log1p(exp(-fabs(x - z)));              // (one of them -inf: exp(-inf) = 0)
}
// Forward algorithm and Viterbi of one utterance per workgroup; threads run over u, anti-diagonals d = t + u in order.  Two
// diagonals of double alpha (and two of Viterbi scores) sit in LDS, indexed by u: diagonal d reads buffer (d - 1) & 1 and writes
// d & 1, one barrier per diagonal.  Which predecessors exist follows from (t, u) alone, so a stale entry is never read.
// Back-pointers: one bit per cell (1 = the emission predecessor (t, u - 1) won: strictly greater than the blank one).
inline __global__ __launch_bounds__(256) void k_lat_dp(const LatDpArgs a) {
    extern __shared__ double lat_sh[];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int T = a.T[i], U = a.U[i], U1 = U + 1;
    const float* b = a.b + a.off[i];
    const float* e = a.e + a.off[i];
    double* al[2] = {lat_sh, lat_sh + a.u1_max};
    double* vi[2] = {lat_sh + 2 * (size_t)a.u1_max, lat_sh + 3 * (size_t)a.u1_max};
    const long long cells = (long long)T * U1;
    const long long words = (cells + 31) >> 5;
    unsigned* bp = nullptr;
    bool bp_lds = false;
    if (a.vit) {
        bp_lds = words <= a.lds_bp_words;
        bp = bp_lds ? (unsigned*)(lat_sh + 4 * (size_t)a.u1_max) : a.bp + a.bp_off[i];
        for (long long w = tid; w < words; w += 256) bp[w] = 0u;
        __syncthreads();
    }
    const int D = T + U;                              // diagonals 0 .. T + U - 1
    for (int d = 0; d < D; ++d) {
        const int cur = d & 1, prv = cur ^ 1;
        const int u_lo = d - (T - 1) > 0 ? d - (T - 1) : 0, u_hi = d < U ? d : U;
        for (int u = u_lo + tid; u <= u_hi; u += 256) {
            const int t = d - u;
            double x = -INFINITY, z = -INFINITY, vx = -INFINITY, vz = -INFINITY;
            if (t > 0) {
                const double bb = (double)b[(size_t)(t - 1) * U1 + u];
                x = al[prv][u] + bb;
                if (a.vit) vx = vi[prv][u] + bb;
            }
            if (u > 0) {
                const double ee = (double)e[(size_t)t * U1 + u - 1];
                z = al[prv][u - 1] + ee;
                if (a.vit) vz = vi[prv][u - 1] + ee;
            }
            if (d == 0) { al[cur][0] = 0.0; if (a.vit) vi[cur][0] = 0.0; continue; }
            al[cur][u] = lat_logaddexp(x, z);
            if (a.vit) {
                const bool emit = vz > vx;            // a tie takes the blank predecessor
                vi[cur][u] = emit ? vz : vx;
                if (emit) {
                    const long long c = (long long)t * U1 + u;
                    atomicOr(&bp[c >> 5], 1u << (c & 31));
                }
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int last = (D - 1) & 1;
    const double bl = (double)b[(size_t)(T - 1) * U1 + U];
    a.loglik[i] = al[last][U] + bl;
    if (!a.vit) return;
    if (a.viterbi) a.viterbi[i] = vi[last][U] + bl;
    if (!a.frames && !a.logps) return;
    int t = T - 1, u = U;
    const int o = a.tok_off[i];
    while (u > 0) {                                   // (t, 0) is reached by blanks alone
        const long long c = (long long)t * U1 + u;
        if (t == 0 || ((bp[c >> 5] >> (c & 31)) & 1u)) {      // (frame 0 has no blank predecessor)
            if (a.frames) a.frames[o + u - 1] = t;
            if (a.logps) a.logps[o + u - 1] = e[(size_t)t * U1 + u - 1];
            --u;
        } else --t;
    }
}

}  // namespace lasr

namespace {

void lat_mark(lasr_ctx* c, lasr_ctx::Lattice& w, int i) {
    if (!c->profiling) return;
    if (!w.ev_ok) {
        for (hipEvent_t& ev : w.ev) if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); return; }
        w.ev_ok = true;
    }
    (void)hipEventRecord(w.ev[i], c->stream);
}

// host image of the per-call tables and their device views
struct LatCall {
    int n = 0;
    std::vector<int> T, U, slot, tok_off;
    std::vector<long long> off, bp_off;
    long long cells = 0, sumU = 0, bp_words = 0;
    int Umax = 0;
    LatTab tab{};
    const long long* d_bp_off = nullptr;
};
// tables -> device (one copy); tok may be null (lasr_lattice_dp: no labels are read)
int lat_upload(lasr_ctx* c, lasr_ctx::Lattice& w, LatCall& k, const int32_t* tok, std::vector<long long>& img) {
    const int n = k.n;
    k.off.assign(n + 1, 0); k.tok_off.assign(n, 0); k.bp_off.assign(n, 0);
    k.cells = 0; k.sumU = 0; k.bp_words = 0; k.Umax = 0;
    for (int i = 0; i < n; ++i) {
        k.off[i] = k.cells; k.tok_off[i] = (int)k.sumU;
        const long long ci = (long long)k.T[i] * (k.U[i] + 1), wi = (ci + 31) >> 5;
        k.bp_off[i] = k.bp_words;
        if (wi > LAT_BP_WORDS) k.bp_words += wi;
        k.cells += ci; k.sumU += k.U[i]; k.Umax = std::max(k.Umax, k.U[i]);
    }
    k.off[n] = k.cells;
    if (k.cells >= (1ll << 31)) return fail(c, LASR_EINVAL, "lattice of %lld cells is too large", k.cells);
    // image (8-byte units): off [n + 1], bp_off [n], then the int arrays T, U, slot, tok_off [n] each and tok [sum U]
    const size_t n_ints = 4 * (size_t)n + (size_t)k.sumU;
    img.assign((size_t)2 * n + 1 + (n_ints + 1) / 2, 0);
    memcpy(img.data(), k.off.data(), sizeof(long long) * (n + 1));
    memcpy(img.data() + n + 1, k.bp_off.data(), sizeof(long long) * n);
    int* ip = (int*)(img.data() + 2 * n + 1);
    memcpy(ip, k.T.data(), sizeof(int) * n); memcpy(ip + n, k.U.data(), sizeof(int) * n);
    memcpy(ip + 2 * n, k.slot.data(), sizeof(int) * n); memcpy(ip + 3 * n, k.tok_off.data(), sizeof(int) * n);
    if (tok && k.sumU) memcpy(ip + 4 * n, tok, sizeof(int) * (size_t)k.sumU);
    RC(ensure_buf(c, &w.tab, &w.tab_n, img.size()));
    HIPCHK(c, hipMemcpyAsync(w.tab, img.data(), sizeof(long long) * img.size(), hipMemcpyHostToDevice, c->stream));
    const long long* dl = (const long long*)w.tab;
    const int* di = (const int*)(dl + 2 * n + 1);
    k.tab = LatTab{dl, di, di + n, di + 2 * n, di + 3 * n, di + 4 * n, n};
    k.d_bp_off = dl + n + 1;
    return LASR_OK;
}

// k_lat_dp over the lattices b / e (device) of call k; results stay in the workspace
int lat_run_dp(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const float* b, const float* e, bool vit, bool want_frames, bool want_logps) {
    RC(ensure_buf(c, &w.res, &w.res_n, (size_t)2 * k.n));
    if (vit) {
        RC(ensure_buf(c, &w.frames, &w.frames_n, (size_t)std::max(k.sumU, 1ll)));
        RC(ensure_buf(c, &w.logps, &w.logps_n, (size_t)std::max(k.sumU, 1ll)));
        if (k.bp_words) RC(ensure_buf(c, &w.bp, &w.bp_n, (size_t)k.bp_words));
    }
    LatDpArgs a{};
    a.b = b; a.e = e; a.off = k.tab.off; a.T = k.tab.T; a.U = k.tab.U; a.tok_off = k.tab.tok_off;
    a.loglik = w.res; a.viterbi = vit ? w.res + k.n : nullptr;
    a.frames = vit && want_frames ? w.frames : nullptr; a.logps = vit && want_logps ? w.logps : nullptr;
    a.bp = w.bp; a.bp_off = k.d_bp_off;
    a.u1_max = k.Umax + 1; a.vit = vit ? 1 : 0;
    long long mw = 0;
    for (int i = 0; i < k.n; ++i) {
        const long long wi = ((long long)k.T[i] * (k.U[i] + 1) + 31) >> 5;
        if (wi <= LAT_BP_WORDS) mw = std::max(mw, wi);
    }
    a.lds_bp_words = vit ? (int)mw : 0;
    const size_t lds = sizeof(double) * (vit ? 4 : 2) * (size_t)a.u1_max + sizeof(unsigned) * (size_t)a.lds_bp_words;
    if (!vit) a.lds_bp_words = 0;
    hipLaunchKernelGGL(k_lat_dp, dim3(k.n), dim3(256), lds, c->stream, a);
    return LASR_OK;
}

struct LatOut { double* loglik; double* viterbi; int32_t* frames; float* logps; float* blank_lp; float* emit_lp; };
// posterior outputs (host, each optional) and the two steps that fill them: lasr_lattice_post.hip.h
struct LatPostOut {
    double* loglik; double* loglik_bwd; float* occ_blank; float* occ_emit;
    double* tok_mean; double* tok_var; int32_t* tok_peak_frame; double* tok_peak;
};
int lat_post_launch(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const float* b, const float* e, const LatPostOut& p);
int lat_post_copy(lasr_ctx* c, lasr_ctx::Lattice& w, const LatCall& k, const LatPostOut& p);

int lat_check_tokens(lasr_ctx* c, int n, const int32_t* tokens, const int32_t* n_tokens, int umax = LAT_UMAX) {
    if (!n_tokens) return fail(c, LASR_EINVAL, "null argument");
    long long at = 0;
    for (int i = 0; i < n; ++i) {
        if (n_tokens[i] < 0 || n_tokens[i] > umax) return fail(c, LASR_EINVAL, "transcript %d has %d labels (0..%d)", i, n_tokens[i], umax);
        if (n_tokens[i] > 0 && !tokens) return fail(c, LASR_EINVAL, "null argument");
        for (int u = 0; u < n_tokens[i]; ++u) {
            const int y = tokens[at + u];
            if (y < 0 || y >= c->d.vocab || y == c->d.blank) return fail(c, LASR_EINVAL, "transcript %d: label %d (id %d) is out of range or blank", i, u, y);
        }
        at += n_tokens[i];
    }
    return LASR_OK;
}

// Teacher-forced predictor of the listed rows into w.pp [Umax + 1][Ml][J]: g_0 is the BOS pass of apply_reset; g_u = the predictor
// stepped on y_u (rows whose transcript has ended: emit = 0, their state is carried and their column of lat_pp is never read).
// tokens: the n transcripts concatenated, U[i] labels each
int lat_teacher_force(lasr_ctx* c, lasr_ctx::Lattice& w, DecView& v, const int* slots, int n, const std::vector<int>& U, int Umax,
                      const int32_t* tokens, int Ml) {
    const int M = c->M, J = c->d.joint, H = c->d.hidden, L = c->d.pred_layers;
    HIPCHK(c, hipMemcpyAsync(w.pp, c->pp[0], sizeof(float) * (size_t)Ml * J, hipMemcpyDeviceToDevice, c->stream));
    long long at0 = 0;
    std::vector<long long> first(n);
    for (int i = 0; i < n; ++i) { first[i] = at0; at0 += U[i]; }
    for (int u = 1; u <= Umax; ++u) {
        RC(cmd_begin(c));
        for (int i = 0; i < n; ++i)
            if (u <= U[i]) { c->hc.token[slots[i]] = tokens[first[i] + u - 1]; c->hc.emit[slots[i]] = 1; }
        RC(cmd_commit(c));
        HIPCHK(c, hipMemcpyAsync(c->ds.token, c->dc.token, sizeof(int) * M, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ds.emit, c->dc.emit, sizeof(int) * M, hipMemcpyDeviceToDevice, c->stream));
        launch_predictor(c, v);
        c->pred_par = v.pred_par;
        GemmArgs g{};
        set_operand(g, 0, c->pred_y[0][L - 1], H, 0, 0, c->W1p); g.a_rows = Ml;
        EpiLinear::Args ea{};
        ea.bias = c->b1; ea.out = w.pp + (size_t)u * Ml * J; ea.ldo = J; ea.n_rows = Ml; ea.M = M;
        launch_linear<true, 3>(c, v, J / 16, (Ml + 15) / 16, g, H, ea);
    }
    return LASR_OK;
}
// stage times of the call from the events lat_mark recorded (stream idle)
void lat_times(lasr_ctx* c, lasr_ctx::Lattice& w) {
    if (!c->profiling || !w.ev_ok) return;
    for (int i = 0; i < 4; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, w.ev[i], w.ev[i + 1]) != hipSuccess) (void)hipGetLastError();
        w.us[i] = (int)(1e3f * ms + 0.5f);
    }
    float ms = 0.f;                                   // the posterior stage: only where this call recorded its end
    if (w.ev_post && hipEventElapsedTime(&ms, w.ev[4], w.ev[5]) != hipSuccess) (void)hipGetLastError();
    w.us[4] = (int)(1e3f * ms + 0.5f);
    w.ev_post = false;
}

// Behind the front-end and the encoder of a lasr_align_* call (pe_sync holds the joint's encoder half, the listed slots are in the
// state apply_reset left them in: predictor stepped on BOS, its joint half in pp[0]): teacher-forced predictor, lattice blocks,
// dynamic programme, results to the host, slots back to fresh state.  post (lasr_align_post_*): alpha / beta and the occupancies
// behind the dynamic programme, which then runs only for the Viterbi outputs (k_lat_ab's forward half gives loglik).
int lat_finish(lasr_ctx* c, const int* slots, int n, const int* T_row, const int32_t* tokens, const int32_t* n_tokens, const LatOut& o,
               const LatPostOut* post = nullptr) {
    const int M = c->M, J = c->d.joint, V = c->d.vocab;
    lasr_ctx::Lattice& w = c->lat;
    LatCall k;
    k.n = n;
    k.T.assign(T_row, T_row + n); k.U.assign(n_tokens, n_tokens + n); k.slot.assign(slots, slots + n);
    std::vector<long long> img;
    lat_mark(c, w, 1);
    RC(lat_upload(c, w, k, tokens, img));
    int Ml = 0;
    for (int i = 0; i < n; ++i) Ml = std::max(Ml, slots[i] + 1);
    RC(ensure_buf(c, &w.pp, &w.pp_n, (size_t)(k.Umax + 1) * Ml * J));
    RC(ensure_buf(c, &w.ja, &w.ja_n, (size_t)LAT_R * J * c->esz));
    RC(ensure_buf(c, &w.logits, &w.logits_n, (size_t)LAT_R * V));
    RC(ensure_buf(c, &w.b, &w.b_n, (size_t)k.cells));
    RC(ensure_buf(c, &w.e, &w.e_n, (size_t)k.cells));
    // ---- teacher-forced predictor
    DecView v = sync_view(c, 1);
    RC(lat_teacher_force(c, w, v, slots, n, k.U, k.Umax, tokens, Ml));
    lat_mark(c, w, 2);
    // ---- lattice blocks
    for (long long cell0 = 0; cell0 < k.cells; cell0 += LAT_R) {
        const int nr = (int)std::min<long long>(LAT_R, k.cells - cell0);
        hipLaunchKernelGGL(k_lat_ja, dim3(nr), dim3(256), 0, c->stream, (const float*)c->pe_sync, (const float*)w.pp, k.tab, cell0, nr,
                           (void*)w.ja, J, M, Ml, LAT_R / 16, c->bf);
        launch_logits_from(c, v, w.ja, LAT_R / 16, LAT_R, w.logits, nr);
        hipLaunchKernelGGL(k_lat_pick, dim3((nr + 3) / 4), dim3(256), 0, c->stream, (const float*)w.logits, k.tab, cell0, nr, V, c->d.blank,
                           w.b, w.e);
    }
    lat_mark(c, w, 3);
    const bool vit = o.viterbi || o.frames || o.logps;
    if (!post || vit) RC(lat_run_dp(c, w, k, w.b, w.e, vit, o.frames != nullptr, o.logps != nullptr));
    lat_mark(c, w, 4);
    LatPostOut po{};
    if (post) {
        po = *post;
        po.loglik = vit ? nullptr : o.loglik;
        RC(lat_post_launch(c, w, k, w.b, w.e, po));
        lat_mark(c, w, 5);
        w.ev_post = c->profiling && w.ev_ok;
    }
    // ---- the slots go back to fresh state (what lasr_stream_reset(.., 1 | 2 | 4) leaves)
    RC(cmd_begin(c));
    for (int i = 0; i < n; ++i) c->hc.what[slots[i]] = 7;
    RC(cmd_commit(c));
    RC(apply_reset(c, sync_view(c, c->la_sync), true));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    c->cmd_inflight = 0;
    if (!post || vit) HIPCHK(c, hipMemcpy(o.loglik, w.res, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (post) RC(lat_post_copy(c, w, k, po));
    if (o.viterbi) HIPCHK(c, hipMemcpy(o.viterbi, w.res + n, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (o.frames && k.sumU) HIPCHK(c, hipMemcpy(o.frames, w.frames, sizeof(int) * (size_t)k.sumU, hipMemcpyDeviceToHost));
    if (o.logps && k.sumU) HIPCHK(c, hipMemcpy(o.logps, w.logps, sizeof(float) * (size_t)k.sumU, hipMemcpyDeviceToHost));
    if (o.blank_lp) HIPCHK(c, hipMemcpy(o.blank_lp, w.b, sizeof(float) * (size_t)k.cells, hipMemcpyDeviceToHost));
    if (o.emit_lp) HIPCHK(c, hipMemcpy(o.emit_lp, w.e, sizeof(float) * (size_t)k.cells, hipMemcpyDeviceToHost));
    lat_times(c, w);
    return LASR_OK;
}

}  // namespace
