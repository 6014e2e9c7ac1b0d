// lasr_lm_score.hip.h -- whole-sequence scoring by the attached LM (lasr_lm_score): log P_LM of the labels of a
// transcript the caller already has, LM.forward on the sequence (lm.py:31-40) followed by the gather of the labels' entries.
// Engine unit only (lasr_engine.hip), included after lasr_lattice.hip.h (lat_row_lse, lat_rows).
//
// Every candidate sits on one LM row (its slot).  A pass is one LM step of the decode path, driven teacher-forced: the command block
// holds the pass's input token of every row whose input sequence has one (emit = 1) and 0 for every other row, whose LM state the
// step carries; launch_lm leaves the output layer's logits in lm.raw [M][V] (f32, bf16 and the int8-served form alike):
//   k_lm_pick    lat_row_lse on the listed rows of lm.raw, then (z[y] - m) - lse at the pass's target label into lp / acc
// Everything is enqueued on the ctx stream with the engine idle.  No prefix tree: a pass costs the same for 1 row or 64 (one M-tile
// group, bound by launches and by streaming the weights), so shared prefixes would save rows and not passes.
#pragma once

namespace lasr {

// tables of a call, one upload: [n] row (slot), [n] first term of the candidate in lp, [n][passes] target label (-1: no term)
struct LmPickTab { const int* row; const int* tok_off; const int* tgt; int n, passes; };

// one wave per listed row, four rows per workgroup.  Pass `pass` of row i gives term `pass + shift` of candidate i (shift = 1
// when the sequence starts without a start token: term 0 is then 0 by definition and stays as the call's memset left it).
// lp[tok_off[i] + ..] and acc[i] have one writer, this row's lane 0, pass after pass in stream order: no atomics, no fence.
inline __global__ __launch_bounds__(256) void k_lm_pick(const float* __restrict__ raw, const LmPickTab tb, int pass, int shift, int V,
                                                        float* __restrict__ lp, double* __restrict__ acc) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= tb.n) return;                           // wave-uniform
    const int y = tb.tgt[(size_t)i * tb.passes + pass];
    if (y < 0) return;                               // wave-uniform: this row's sequence has ended
    const float* z = raw + (size_t)tb.row[i] * V;
    float m, lse;
    lat_row_lse(z, V, lane, m, lse);
    if (lane != 0) return;
    const float term = (z[y] - m) - lse;
    lp[tb.tok_off[i] + pass + shift] = term;
    acc[i] += (double)term;
}

}  // namespace lasr

namespace {

// bit 4 of the listed rows: zero LM state, no LM distribution (what lasr_stream_reset(slot, 4) does on an idle context)
int lm_score_reset(lasr_ctx* c, const int* slots, int n) {
    RC(cmd_begin(c));
    for (int i = 0; i < n; ++i) c->hc.what[slots[i]] = 4;
    RC(cmd_commit(c));
    return apply_reset(c, sync_view(c, c->la_sync), false);
}

// Teacher-forced LM over the listed rows, lat_teacher_force's pattern: pass k steps the LM on x_k of every row that has one and
// picks that row's term behind it.  x [n][passes]: input token per row and pass, -1 = none
int lm_teacher_force(lasr_ctx* c, lasr_ctx::LmScore& w, DecView& v, const int* slots, int n, const std::vector<int>& x, int passes,
                     const LmPickTab& tb, int shift) {
    const int M = c->M;
    for (int k = 0; k < passes; ++k) {
        RC(cmd_begin(c));
        for (int i = 0; i < n; ++i) {
            const int tok = x[(size_t)i * passes + k];
            if (tok >= 0) { c->hc.token[slots[i]] = tok; c->hc.emit[slots[i]] = 1; }
        }
        RC(cmd_commit(c));
        HIPCHK(c, hipMemcpyAsync(c->ds.token, c->dc.token, sizeof(int) * M, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ds.emit, c->dc.emit, sizeof(int) * M, hipMemcpyDeviceToDevice, c->stream));
        launch_lm(c, v);                              // (its k_lm_post output is dropped by the closing reset)
        c->lm.par = v.lm_par;
        hipLaunchKernelGGL(k_lm_pick, dim3((n + 3) / 4), dim3(256), 0, c->stream, (const float*)c->lm.raw, tb, k, shift, c->d.vocab, w.lp, w.acc);
    }
    return LASR_OK;
}

// the call behind its argument checks: tables, passes, results to the host, the rows' LM state reset at both ends
int lm_score_run(lasr_ctx* c, const int* slots, int n, const int32_t* tokens, const int32_t* n_tokens, int start, double* total, float* logps) {
    lasr_ctx::LmScore& w = c->lms;
    const int shift = start < 0 ? 1 : 0;
    int passes = 0;
    long long sumU = 0;
    for (int i = 0; i < n; ++i) { passes = std::max(passes, n_tokens[i] - shift); sumU += n_tokens[i]; }
    // host image of the tables and of the passes' inputs
    const size_t np = (size_t)n * passes;
    w.host.assign(2 * (size_t)n + np, -1);
    std::vector<int> x(np, -1);
    long long at = 0;
    for (int i = 0; i < n; ++i) {
        const int U = n_tokens[i];
        w.host[i] = slots[i]; w.host[n + i] = (int)at;
        for (int k = 0; k + shift < U; ++k) {        // pass k: reads x_k, its term is label k + shift
            x[(size_t)i * passes + k] = shift ? tokens[at + k] : (k == 0 ? start : tokens[at + k - 1]);
            w.host[2 * (size_t)n + (size_t)i * passes + k] = tokens[at + k + shift];
        }
        at += U;
    }
    RC(ensure_buf(c, &w.tab, &w.tab_n, w.host.size()));
    RC(ensure_buf(c, &w.lp, &w.lp_n, (size_t)std::max(sumU, 1ll)));
    RC(ensure_buf(c, &w.acc, &w.acc_n, (size_t)n));
    HIPCHK(c, hipMemcpyAsync(w.tab, w.host.data(), sizeof(int) * w.host.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w.lp, 0, sizeof(float) * (size_t)std::max(sumU, 1ll), c->stream));
    HIPCHK(c, hipMemsetAsync(w.acc, 0, sizeof(double) * (size_t)n, c->stream));
    const LmPickTab tb{w.tab, w.tab + n, w.tab + 2 * (size_t)n, n, passes};
    RC(lm_score_reset(c, slots, n));
    DecView v = sync_view(c, c->la_sync);
    RC(lm_teacher_force(c, w, v, slots, n, x, passes, tb, shift));
    RC(lm_score_reset(c, slots, n));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    c->cmd_inflight = 0;
    HIPCHK(c, hipMemcpy(total, w.acc, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (logps && sumU) HIPCHK(c, hipMemcpy(logps, w.lp, sizeof(float) * (size_t)sumU, hipMemcpyDeviceToHost));
    return LASR_OK;
}

}  // namespace
