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
// Rows go through the joint in lasr_lattice.hip.h's blocks (lat_blocks, k_lat_ja / k_lat_pick) with LatTreeMap:
//   ja[row] = tanh(pe[t][enc_row_i] + lat_pp[depth(v)][row(v)])     row(v): the batch row of the lowest candidate through v
//   pick: lat_row_lse, then b at the row's own cell and e at the cell of every child of its node
// and k_lat_dp_tree runs both recursions of one utterance per workgroup, for every node at once.  The call description and its
// tables (TreeCall, tree_layout, tree_pack) are lasr_lattice_tables.hip.h's.
// Who writes what: b[cell] by the row of the cell; e[cell] by the row of (t, parent(v)) -- an earlier row of the same or an earlier
// block, same stream -- and e[t][0] by the row of (t, 0).  Every cell of both arrays is written exactly once before k_lat_dp_tree
// starts behind the last block on the same stream: no flag, no fence.
#pragma once

namespace lasr {

constexpr int LAT_NMAX = 2048;     // tree nodes per utterance: two parities of alpha and of Viterbi scores in LDS, 4 x 8 x N <= 64 KB

struct LatTreeMap {                 // k: the utterance-local node
    TreeTab tb;
    __device__ __forceinline__ LatCell cell(long long c) const {
        const int i = lat_find(tb.off, tb.n, c);
        const int Ni = tb.N[i], rel = (int)(c - tb.off[i]);
        const int t = rel / Ni;
        return LatCell{i, t, rel - t * Ni};
    }
    __device__ __forceinline__ int enc_row(const LatCell& x) const { return tb.enc_row[x.i]; }
    __device__ __forceinline__ int pp_depth(const LatCell& x) const { return tb.depth[tb.node_off[x.i] + x.k]; }
    __device__ __forceinline__ int pp_row(const LatCell& x) const { return tb.row[tb.node_off[x.i] + x.k]; }
    // lane 0: b at the row's own cell (and e = 0 at the root: nothing enters it); all lanes: e at the cell of every child of the node
    // (every lane holds m and lse)
    __device__ __forceinline__ void pick(long long c, const float* __restrict__ z, float m, float lse, int lane, int blank,
                                         float* __restrict__ b_out, float* __restrict__ e_out) const {
        const LatCell x = cell(c);
        const int no = tb.node_off[x.i];
        if (lane == 0) {
            b_out[c] = (z[blank] - m) - lse;
            if (x.k == 0) e_out[c] = 0.f;
        }
        const long long row0 = c - x.k;
        const int c_lo = tb.child_lo[no + x.k], c_n = tb.child_n[no + x.k];
        for (int q = lane; q < c_n; q += 64) {
            const int ch = c_lo + q;                     // utterance-local id of the child
            e_out[row0 + ch] = (z[tb.label[no + ch]] - m) - lse;
        }
    }
};

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

// the tables of a tree call (T / N / parent / depth set; a lasr_score_* call: every table) -> device, one copy through the lattice's
// table buffer.  parent / depth are valid (lasr_prefix_tree's contract)
int tree_upload(lasr_ctx* c, lasr_ctx::Lattice& w, TreeCall& k, TabImage& img) {
    tree_layout(k);
    if (k.cells >= (1ll << 31)) return fail(c, LASR_EINVAL, "lattice of %lld cells is too large", k.cells);
    if (!k.sizes_ok()) return fail(c, LASR_EINVAL, "internal: tree tables of the wrong size");
    tree_pack(k, img);
    return lat_upload(c, w, img);
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
    lasr_ctx::Lattice& w = c->lat;
    TreeCall k;
    k.n = n;
    k.T.assign(T_utt, T_utt + n);
    int K = 0, Umax = 0;
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
    for (int j = 0; j < K; ++j) Umax = std::max(Umax, U[j]);
    const int Ml = lat_rows(slots, K);
    TabImage img;
    lat_mark(c, w, 1);
    RC(tree_upload(c, w, k, img));
    RC(lat_workspace(c, w, Umax, Ml, k.cells));
    // ---- teacher-forced predictor: one pass per label position over all candidate rows
    DecView v = sync_view(c, 1);
    RC(lat_teacher_force(c, w, v, slots, K, U, Umax, tokens, Ml));
    lat_mark(c, w, 2);
    lat_blocks(c, w, v, LatTreeMap{k.tab}, k.cells, Ml);
    lat_mark(c, w, 3);
    RC(tree_run_dp(c, w, k, w.b, w.e, o.viterbi != nullptr));
    lat_mark(c, w, 4);
    RC(lat_release(c, slots, K));
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
