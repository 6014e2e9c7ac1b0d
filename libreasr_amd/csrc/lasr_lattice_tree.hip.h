// lasr_lattice_tree.hip.h -- the teacher-forced RNN-T lattice over a prefix tree of candidates (lasr_score_pcm / lasr_score_feats /
// lasr_lattice_tree_dp): the candidates of an n-best list share the encoder pass of their utterance and every joint row
// whose predictor state -- a function of the prefix alone -- they have in common.
// Engine unit only (lasr_engine.hip), included after lasr_lattice.hip.h and lasr_prefix_tree.hip.h.
//
// Utterance i has T_i frames and a tree of N_i nodes (lasr_prefix_tree.hip.h: parent[v] < v, depth non-decreasing, children
// contiguous).  Cells of a call in one flat order -- utterance i, then t, then node v: cell = off_i + t N_i + v, the layout of both
// lattice arrays:
//   b[cell] = lp[t, v, blank]                         lp[t, v, :] = log_softmax(joint(g_v, f_t)), g_v the predictor after v's prefix
//   e[cell] = lp[t, parent(v), label(v)]              the emission that ENTERS v is stored at v; e[t][0] = 0
// Rows go through the joint in blocks of LAT_R, as lasr_lattice.hip.h's do:
//   k_lat_ja_tree    ja[row] = tanh(pe[t][enc_row_i] + lat_pp[depth(v)][row(v)])     row(v): the batch row of the lowest candidate through v
//   logits GEMM      launch_logits_from, unchanged
//   k_lat_pick_tree  b at the row's own cell, e at the cell of every child of its node
// and k_lat_dp_tree runs both recursions of one utterance per workgroup, for every node at once.
// Who writes what: b[cell] by the row of the cell; e[cell] by the row of (t, parent(v)) -- an earlier row of the same or an earlier
// block, same stream -- and e[t][0] by the row of (t, 0).  Every cell of both arrays is written exactly once before k_lat_dp_tree
// starts behind the last block on the same stream: no flag, no fence.
#pragma once

namespace lasr {

constexpr int LAT_NMAX = 2048;     // tree nodes per utterance: two parities of alpha and of Viterbi scores in LDS, 4 x 8 x N <= 64 KB

struct TreeTab {                   // per-call tables (device)
    const long long* off;          // [n + 1] first cell of the utterance
    const int* T;                  // [n] frames
    const int* N;                  // [n] nodes
    const int* node_off;           // [n] first node in the per-node arrays (and in the results)
    const int* enc_row;            // [n] batch row that holds the utterance's encoder output
    const int* ds_off;             // [n] first entry in dstart
    const int* parent;             // per node (utterance-local ids): parent, -1 at the root
    const int* label;              //   the label that enters the node
    const int* depth;              //   labels of the prefix
    const int* row;                //   batch row of the lowest candidate that passes through the node (its lat_pp column)
    const int* child_lo;           //   first child
    const int* child_n;            //   children
    const int* dstart;             // per utterance [depth_max + 2]: first node of each depth, then N
    int n;
};
__device__ __forceinline__ int lat_find(const long long* off, int n, long long cell) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= cell) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// joint activation of the block's rows: k_lat_ja with the predictor half taken at (depth, row) of the node
inline __global__ __launch_bounds__(256) void k_lat_ja_tree(const float* __restrict__ pe, const float* __restrict__ lat_pp, const TreeTab tb,
                                                            long long cell0, int n_rows, void* __restrict__ ja, int J, int M, int Ml, int mt,
                                                            int bf) {
    const int row = blockIdx.x;
    if (row >= n_rows) return;
    const long long cell = cell0 + row;
    const int i = lat_find(tb.off, tb.n, cell);
    const int Ni = tb.N[i], rel = (int)(cell - tb.off[i]);
    const int t = rel / Ni, v = tb.node_off[i] + (rel - t * Ni);
    const float* e = pe + ((size_t)t * M + tb.enc_row[i]) * J;
    const float* p = lat_pp + ((size_t)tb.depth[v] * Ml + tb.row[v]) * J;
    for (int j = threadIdx.x; j < J; j += 256) act_st(bf, ja, act_off(bf, row, j, mt), tanhf(e[j] + p[j]));
}

// log-softmax of a lattice row at the blank and at the label of every child of the row's node, one wave per row.  Maximum and
// exp-sum are k_lat_pick's (k_select's virtual threads lane + 64 w, ascending terms, the same butterfly, the same order of the four
// sums), so from the same logits a term is bit for bit k_lat_pick's.
inline __global__ __launch_bounds__(256) void k_lat_pick_tree(const float* __restrict__ logits, const TreeTab tb, long long cell0, int n_rows,
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
    const float lse = logf(sum);                     // (the same value in every lane: wave_sum_f32 broadcasts)
    const long long cell = cell0 + row;
    const int i = lat_find(tb.off, tb.n, cell);
    const int Ni = tb.N[i], rel = (int)(cell - tb.off[i]);
    const int t = rel / Ni, vl = rel - t * Ni, v = tb.node_off[i] + vl;
    if (lane == 0) {
        b_out[cell] = (z[blank] - m) - lse;
        if (vl == 0) e_out[cell] = 0.f;              // nothing enters the root
    }
    const long long row0 = tb.off[i] + (long long)t * Ni;
    const int c_lo = tb.child_lo[v], c_n = tb.child_n[v];
    for (int k = lane; k < c_n; k += 64) {
        const int ch = c_lo + k;                     // utterance-local id of the child
        e_out[row0 + ch] = (z[tb.label[tb.node_off[i] + ch]] - m) - lse;
    }
}

struct TreeDpArgs {
    const float* b; const float* e;   // [cells] each, utterance i at off[i], [T][N]
    TreeTab tb;
    double* loglik; double* viterbi;  // per node, [sum N] (viterbi: with vit)
    int n_max, vit;
};
// Forward algorithm and Viterbi over the tree of one utterance per workgroup, every node at once: final[v] = log P(prefix_v | x).
// Anti-diagonals d = t + depth(v) in order; threads run over the contiguous node range whose depth lies in the diagonal's
// [u_lo, u_hi].  Two parities of double alpha (and two of Viterbi scores) sit in LDS, indexed by NODE: diagonal d reads parity
// (d - 1) & 1 -- (t - 1, v) and (t, parent v) both lie on diagonal d - 1 -- and writes d & 1, one barrier per diagonal; which
// predecessors exist follows from (t, v) alone, so a stale entry is never read.  A node's entry is overwritten two diagonals later,
// so the thread that computes (T - 1, v) stores the node's result itself.
inline __global__ __launch_bounds__(256) void k_lat_dp_tree(const TreeDpArgs a) {
    extern __shared__ double lat_tree_sh[];
    const int i = blockIdx.x, tid = threadIdx.x;
    const TreeTab& tb = a.tb;
    const int T = tb.T[i], N = tb.N[i], no = tb.node_off[i];
    const float* b = a.b + tb.off[i];
    const float* e = a.e + tb.off[i];
    const int* parent = tb.parent + no;
    const int* depth = tb.depth + no;
    const int* dstart = tb.dstart + tb.ds_off[i];
    double* al[2] = {lat_tree_sh, lat_tree_sh + a.n_max};
    double* vi[2] = {lat_tree_sh + 2 * (size_t)a.n_max, lat_tree_sh + 3 * (size_t)a.n_max};
    const int U = depth[N - 1];                       // the deepest node is the last
    const int D = T + U;                              // diagonals 0 .. T + U - 1
    for (int d = 0; d < D; ++d) {
        const int cur = d & 1, prv = cur ^ 1;
        const int u_lo = d - (T - 1) > 0 ? d - (T - 1) : 0, u_hi = d < U ? d : U;
        const int v_hi = dstart[u_hi + 1];
        for (int v = dstart[u_lo] + tid; v < v_hi; v += 256) {
            const int t = d - depth[v];
            double x = -INFINITY, z = -INFINITY, vx = -INFINITY, vz = -INFINITY;
            if (t > 0) {
                const double bb = (double)b[(size_t)(t - 1) * N + v];
                x = al[prv][v] + bb;
                if (a.vit) vx = vi[prv][v] + bb;
            }
            if (v > 0) {
                const double ee = (double)e[(size_t)t * N + v];
                const int p = parent[v];
                z = al[prv][p] + ee;
                if (a.vit) vz = vi[prv][p] + ee;
            }
            double av = 0.0, vv = 0.0;                // (d == 0: the root on frame 0)
            if (d > 0) {
                av = lat_logaddexp(x, z);
                vv = vz > vx ? vz : vx;               // a tie takes the blank predecessor
            }
            al[cur][v] = av;
            if (a.vit) vi[cur][v] = vv;
            if (t == T - 1) {
                const double bl = (double)b[(size_t)(T - 1) * N + v];
                a.loglik[no + v] = av + bl;
                if (a.vit) a.viterbi[no + v] = vv + bl;
            }
        }
        __syncthreads();
    }
}

}  // namespace lasr

namespace {

// host image of the per-call tables of a tree call and their device views
struct TreeCall {
    int n = 0;
    std::vector<int> T, N, enc_row;
    std::vector<int> parent, label, depth, row;      // per node, utterances concatenated (label / row may stay empty: the DP alone)
    long long cells = 0, nodes = 0;
    int Nmax = 0;
    TreeTab tab{};
};
// tables -> device (one copy, through the lattice's table buffer).  parent / depth are valid (lasr_prefix_tree's contract)
int tree_upload(lasr_ctx* c, lasr_ctx::Lattice& w, TreeCall& k, std::vector<long long>& img) {
    const int n = k.n;
    std::vector<long long> off(n + 1, 0);
    std::vector<int> node_off(n), ds_off(n), child_lo, child_n, dstart;
    k.cells = 0; k.nodes = 0; k.Nmax = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = k.cells; node_off[i] = (int)k.nodes;
        k.cells += (long long)k.T[i] * k.N[i]; k.nodes += k.N[i]; k.Nmax = std::max(k.Nmax, k.N[i]);
    }
    off[n] = k.cells;
    if (k.cells >= (1ll << 31)) return fail(c, LASR_EINVAL, "lattice of %lld cells is too large", k.cells);
    child_lo.assign((size_t)k.nodes, 0); child_n.assign((size_t)k.nodes, 0);
    for (int i = 0; i < n; ++i) {
        const int no = node_off[i], Ni = k.N[i];
        for (int v = 1; v < Ni; ++v) {
            const int p = no + k.parent[no + v];
            if (child_n[p]++ == 0) child_lo[p] = v;
        }
        ds_off[i] = (int)dstart.size();
        for (int v = 0; v < Ni; ++v)
            if (v == 0 || k.depth[no + v] != k.depth[no + v - 1]) dstart.push_back(v);
        dstart.push_back(Ni);
    }
    const size_t nn = (size_t)k.nodes;
    // full: a lasr_score_* call (every table); otherwise the DP alone on caller-supplied parents: label / row / enc_row stay zero and
    // child_lo / child_n mean nothing there (children need not be contiguous) -- k_lat_dp_tree reads none of them
    const bool full = !k.label.empty() || !k.row.empty() || !k.enc_row.empty();
    if (k.T.size() != (size_t)n || k.N.size() != (size_t)n || k.parent.size() != nn || k.depth.size() != nn ||
        (full && (k.label.size() != nn || k.row.size() != nn || k.enc_row.size() != (size_t)n)))
        return fail(c, LASR_EINVAL, "internal: tree tables of the wrong size");
    // image (8-byte units): off [n + 1], then the int arrays T, N, node_off, enc_row, ds_off [n] each, six per-node arrays, dstart
    const size_t n_ints = 5 * (size_t)n + 6 * nn + dstart.size();
    img.assign((size_t)n + 1 + (n_ints + 1) / 2, 0);
    memcpy(img.data(), off.data(), sizeof(long long) * (n + 1));
    int* ip = (int*)(img.data() + n + 1);
    auto put = [&](const std::vector<int>& a, size_t at) { if (!a.empty()) memcpy(ip + at, a.data(), sizeof(int) * a.size()); };
    put(k.T, 0); put(k.N, n); put(node_off, 2 * (size_t)n); put(ds_off, 4 * (size_t)n);
    const size_t pn = 5 * (size_t)n;
    put(k.parent, pn); put(k.depth, pn + 2 * nn); put(child_lo, pn + 4 * nn); put(child_n, pn + 5 * nn);
    if (full) { put(k.enc_row, 3 * (size_t)n); put(k.label, pn + nn); put(k.row, pn + 3 * nn); }
    put(dstart, pn + 6 * nn);
    RC(ensure_buf(c, &w.tab, &w.tab_n, img.size()));
    HIPCHK(c, hipMemcpyAsync(w.tab, img.data(), sizeof(long long) * img.size(), hipMemcpyHostToDevice, c->stream));
    const long long* dl = (const long long*)w.tab;
    const int* di = (const int*)(dl + n + 1);
    const int* dn = di + pn;
    k.tab = TreeTab{dl, di, di + n, di + 2 * n, di + 3 * n, di + 4 * n, dn, dn + nn, dn + 2 * nn, dn + 3 * nn, dn + 4 * nn, dn + 5 * nn, dn + 6 * nn, n};
    return LASR_OK;
}

// k_lat_dp_tree over the lattices b / e (device) of call k; the per-node results stay in the workspace: loglik [nodes], viterbi [nodes]
int tree_run_dp(lasr_ctx* c, lasr_ctx::Lattice& w, const TreeCall& k, const float* b, const float* e, bool vit) {
    RC(ensure_buf(c, &w.res, &w.res_n, 2 * (size_t)k.nodes));
    TreeDpArgs a{};
    a.b = b; a.e = e; a.tb = k.tab;
    a.loglik = w.res; a.viterbi = vit ? w.res + k.nodes : nullptr;
    a.n_max = k.Nmax; a.vit = vit ? 1 : 0;
    const size_t lds = sizeof(double) * (vit ? 4 : 2) * (size_t)k.Nmax;
    hipLaunchKernelGGL(k_lat_dp_tree, dim3(k.n), dim3(256), lds, c->stream, a);
    return LASR_OK;
}

struct TreeOut { double* loglik; double* viterbi; float* blank_lp; float* emit_lp; };

// Behind the front-end and the encoder of a lasr_score_* call (pe_sync holds the joint's encoder half on the row of each utterance's
// first candidate; every listed slot is in the state apply_reset left it in): teacher-forced predictor on every candidate row, tree
// blocks, tree DP, results gathered through term, slots back to fresh state.  slots / n_tokens: [sum n_cands], grouped by utterance;
// T_utt [n]; trees [n] built from the same tokens.
int tree_finish(lasr_ctx* c, const int* slots, int n, const int32_t* n_cands, const int* T_utt, const int32_t* tokens, const int32_t* n_tokens,
                const std::vector<lasr_pt::Tree>& trees, const TreeOut& o) {
    const int M = c->M, J = c->d.joint, V = c->d.vocab;
    lasr_ctx::Lattice& w = c->lat;
    TreeCall k;
    k.n = n;
    k.T.assign(T_utt, T_utt + n);
    int K = 0, Ml = 0, Umax = 0;
    for (int i = 0; i < n; ++i) {
        const lasr_pt::Tree& t = trees[i];
        k.N.push_back((int)t.parent.size()); k.enc_row.push_back(slots[K]);
        k.parent.insert(k.parent.end(), t.parent.begin(), t.parent.end());
        k.label.insert(k.label.end(), t.label.begin(), t.label.end());
        k.depth.insert(k.depth.end(), t.depth.begin(), t.depth.end());
        for (int32_t j : t.first) k.row.push_back(slots[K + j]);
        K += n_cands[i];
    }
    std::vector<int> U(n_tokens, n_tokens + K);
    for (int j = 0; j < K; ++j) { Ml = std::max(Ml, slots[j] + 1); Umax = std::max(Umax, U[j]); }
    std::vector<long long> img;
    lat_mark(c, w, 1);
    RC(tree_upload(c, w, k, img));
    RC(ensure_buf(c, &w.pp, &w.pp_n, (size_t)(Umax + 1) * Ml * J));
    RC(ensure_buf(c, &w.ja, &w.ja_n, (size_t)LAT_R * J * c->esz));
    RC(ensure_buf(c, &w.logits, &w.logits_n, (size_t)LAT_R * V));
    RC(ensure_buf(c, &w.b, &w.b_n, (size_t)k.cells));
    RC(ensure_buf(c, &w.e, &w.e_n, (size_t)k.cells));
    // ---- teacher-forced predictor: one pass per label position over all candidate rows
    DecView v = sync_view(c, 1);
    RC(lat_teacher_force(c, w, v, slots, K, U, Umax, tokens, Ml));
    lat_mark(c, w, 2);
    // ---- tree blocks
    for (long long cell0 = 0; cell0 < k.cells; cell0 += LAT_R) {
        const int nr = (int)std::min<long long>(LAT_R, k.cells - cell0);
        hipLaunchKernelGGL(k_lat_ja_tree, dim3(nr), dim3(256), 0, c->stream, (const float*)c->pe_sync, (const float*)w.pp, k.tab, cell0, nr,
                           (void*)w.ja, J, M, Ml, LAT_R / 16, c->bf);
        launch_logits_from(c, v, w.ja, LAT_R / 16, LAT_R, w.logits, nr);
        hipLaunchKernelGGL(k_lat_pick_tree, dim3((nr + 3) / 4), dim3(256), 0, c->stream, (const float*)w.logits, k.tab, cell0, nr, V,
                           c->d.blank, w.b, w.e);
    }
    lat_mark(c, w, 3);
    RC(tree_run_dp(c, w, k, w.b, w.e, o.viterbi != nullptr));
    lat_mark(c, w, 4);
    // ---- the slots go back to fresh state (what lasr_stream_reset(.., 1 | 2 | 4) leaves)
    RC(cmd_begin(c));
    for (int j = 0; j < K; ++j) c->hc.what[slots[j]] = 7;
    RC(cmd_commit(c));
    RC(apply_reset(c, sync_view(c, c->la_sync), true));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    c->cmd_inflight = 0;
    std::vector<double> res((size_t)k.nodes * (o.viterbi ? 2 : 1));
    HIPCHK(c, hipMemcpy(res.data(), w.res, sizeof(double) * res.size(), hipMemcpyDeviceToHost));
    long long no = 0;
    for (int i = 0, j = 0; i < n; ++i) {
        for (int q = 0; q < n_cands[i]; ++q, ++j) {
            o.loglik[j] = res[(size_t)(no + trees[i].term[q])];
            if (o.viterbi) o.viterbi[j] = res[(size_t)(k.nodes + no + trees[i].term[q])];
        }
        no += k.N[i];
    }
    if (o.blank_lp) HIPCHK(c, hipMemcpy(o.blank_lp, w.b, sizeof(float) * (size_t)k.cells, hipMemcpyDeviceToHost));
    if (o.emit_lp) HIPCHK(c, hipMemcpy(o.emit_lp, w.e, sizeof(float) * (size_t)k.cells, hipMemcpyDeviceToHost));
    lat_times(c, w);
    return LASR_OK;
}

}  // namespace
