// lasr_cmd.hip.h -- command blocks (per-step host -> device parameters), per-step tile masks, buffers that grow.
// Engine unit only (lasr_engine.hip), included after lasr_host.hip.h.
#pragma once

namespace {

// the selection kernel of one beam round (+ the LM re-pick of the extended slots' tokens)
void launch_beam_select(lasr_ctx* c, const DecView& v, BeamState& b, int iter_slot) {
    const int M = c->M, lp = par_rd(true, v.lm_par);        // (current-parity LM output of the hypothesis slots)
    b.lm_on = c->lm.on ? 1 : 0; b.done2 = c->c_done2;
    const float* lg = (const float*)c->logits;
    // one wave per hypothesis row (k_beam_select_rw; V <= 2048 is checked at lasr_create for beam > 1)
    // (b.rec: per-token records, lasr_set_beam_records -- an instantiation of their own, so "off" runs the kernel it always ran)
    // (b.seq_hash: merging of equal hypotheses, lasr_set_beam_merge -- likewise.  With an LM attached the identities are of the
    //  re-picked tokens: the selection kernel runs its MERGE = false body and k_beam_fuse_merge re-picks, merges and patches)
    const bool fuse_merge = c->lm.on && b.seq_hash;
    // (bias_on: contextual biasing, lasr_set_beam_bias -- likewise; never together with an LM)
    with_const<0, 1>(bias_on(c) ? 1 : 0, [&](auto bia) {
        with_const<0, 1>(b.seq_hash && !fuse_merge ? 1 : 0, [&](auto mrg) {
            with_const<0, 1>(b.rec ? 1 : 0, [&](auto rec) {
                with_const<2, 4, 8>(c->W, [&](auto wt) {
                    constexpr int WT = decltype(wt)::value;
                    hipLaunchKernelGGL((k_beam_select_rw<WT, decltype(rec)::value != 0, decltype(mrg)::value != 0, decltype(bia)::value != 0>),
                                       dim3(M), dim3(64 * WT), 0, v.stream, lg, b, iter_slot);
                });
            });
        });
    });
    if (fuse_merge)
        with_const<8, 16>(keep16(c->d.vocab) ? 16 : 8, [&](auto keep) {
            with_const<2, 4, 8>(c->W, [&](auto wt) {
                hipLaunchKernelGGL((k_beam_fuse_merge<decltype(wt)::value, decltype(keep)::value>), dim3(M), dim3(256), 0, v.stream, lg, b, iter_slot,
                                   (const float*)c->lm.lmz[lp], (const int*)c->lm.valid[lp], c->lm.alpha, c->lm.theta, c->lm.min_val);
            });
        });
    else if (c->lm.on)
        with_const<8, 16>(keep16(c->d.vocab) ? 16 : 8, [&](auto keep) {
            hipLaunchKernelGGL(k_beam_fuse<decltype(keep)::value>, dim3(c->Md), dim3(256), 0, v.stream, lg, b, iter_slot, (const float*)c->lm.lmz[lp],
                               (const int*)c->lm.valid[lp], c->lm.alpha, c->lm.theta, c->lm.min_val);
        });
}

// What `enqueue()` puts on stream `st`, as an instantiated graph: the one capture sequence of the library (the encoder's cell graphs,
// the decode groups of both protocols).  Once the capture has begun it is always ended, whatever enqueue() returns; callers enqueue
// through a view or a stream of their own, so a failure leaves every context member as it was (c: where the error text goes; null:
// nowhere).
template <class F>
int capture_graph(lasr_ctx* c, hipStream_t st, F&& enqueue, hipGraphExec_t* out) {
    hipGraph_t gr = nullptr;
    HIPCHK(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    hipError_t e = hipStreamEndCapture(st, &gr);
    if (rc) { if (gr) (void)hipGraphDestroy(gr); return rc; }
    if (e != hipSuccess || !gr) return fail(c, LASR_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(out, gr, nullptr, nullptr, 0);
    (void)hipGraphDestroy(gr);
    if (e != hipSuccess) return fail(c, LASR_EHIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    return LASR_OK;
}

// ---------------------------------------------------------------------------- command blocks
size_t cmd_layout(lasr_ctx::Cmd& k, char* base, int M) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += (bytes + 15) & ~size_t(15); return p; };
    k.T_row = (int*)take(sizeof(int) * M); k.what = (int*)take(sizeof(int) * M);
    k.src_idx = (int*)take(sizeof(int) * M); k.feat_sel = (int*)take(sizeof(int) * M);
    k.row_frames = (int*)take(sizeof(int) * M); k.token = (int*)take(sizeof(int) * M);
    k.emit = (int*)take(sizeof(int) * M);
    k.row_N = (long long*)take(sizeof(long long) * M); k.row_src_off = (long long*)take(sizeof(long long) * M);
    k.row_feat_off = (long long*)take(sizeof(long long) * M);
    return o;
}

// next command block: c->hc (host views) / c->dc (device views); zero-initialised
int cmd_begin(lasr_ctx* c) {
    if (c->cmd_inflight >= NCMD - 1) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->cmd_inflight = 0;
    }
    const int i = c->cmd_next;
    c->cmd_next = (i + 1) % NCMD;
    c->cmd_inflight++;
    cmd_layout(c->hc, c->cmd_host + (size_t)i * c->cmd_bytes, c->M);
    cmd_layout(c->dc, c->cmd_dev + (size_t)i * c->cmd_bytes, c->M);
    memset(c->cmd_host + (size_t)i * c->cmd_bytes, 0, c->cmd_bytes);
    return LASR_OK;
}
int cmd_commit(lasr_ctx* c) {
    HIPCHK(c, hipMemcpyAsync((char*)c->dc.T_row, (char*)c->hc.T_row, c->cmd_bytes, hipMemcpyHostToDevice, c->stream));
    return LASR_OK;
}

// device copy of the step's T_row (from the committed command block) + host-side per-step masks of
// the m-tiles that contain an active row (passed by value to the encoder cell kernels)
int commit_T_rows(lasr_ctx* c, int T_max, bool fixed_copy = true, int* fixed_home = nullptr) {
    // (fixed_home: the front-end launch wrote the counts there itself -- the pipelined protocol keeps ONE buffer on the main
    //  stream, so the cell launches of every step have the same arguments and can be replayed as a graph)
    c->T_row_dev = fixed_home ? fixed_home : c->dc.T_row;             // the command ring (NCMD blocks) outlives every step in flight
    // decode kernels of the synchronous protocols read a FIXED buffer (cached graphs replay baked-in pointers)
    if (fixed_copy) HIPCHK(c, hipMemcpyAsync(c->T_row_fix, c->T_row_dev, sizeof(int) * c->M, hipMemcpyDeviceToDevice, c->stream));
    c->tile_masks.assign(std::max(T_max, 1), 0ull);
    for (int t = 0; t < T_max; ++t) {
        unsigned long long m = 0;
        for (int r = 0; r < c->M; ++r)
            if (t < c->hc.T_row[r]) m |= 1ull << (r >> 4);
        c->tile_masks[t] = m;
    }
    return LASR_OK;
}

// ---------------------------------------------------------------------------- buffers that grow
// The step's result blocks for c->tok_cap_alloc tokens per row (stream idle).  Device: [ntok M][tokens M x tok_cap] and, with
// alignment records on, [frames M x tok_cap][log p M x tok_cap] behind them -- one contiguous block, packed by the step's own
// tok_cap (run_decode), so a group's results reach the host in one copy.  Pinned: the same block behind the flag words.
int alloc_results(lasr_ctx* c) {
    const int M = c->M;
    const size_t per_tok = c->align_on ? 3 : 1;
    dfree(c, c->ds.step_ntok);
    c->ds.step_ntok = nullptr; c->ds.step_tok = nullptr;
    RC(dalloc0(c, &c->ds.step_ntok, (size_t)M + per_tok * (size_t)M * c->tok_cap_alloc));
    c->ds.step_tok = c->ds.step_ntok + M;
    // pinned result block: [0] unfinished, then ntok[M], tokens (+ records), sum_iters[M], n_ones[M], logp[M] (double)
    if (c->res_host) (void)hipHostFree(c->res_host);
    c->res_host = nullptr;
    c->res_bytes = sizeof(int) * (8 + 3 * (size_t)M) + sizeof(double) * M + sizeof(int) * per_tok * (size_t)M * c->tok_cap_alloc + 64;
    HIPCHK(c, hipHostMalloc((void**)&c->res_host, c->res_bytes));
    memset(c->res_host, 0, c->res_bytes);
    void* dp = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dp, c->res_host, 0));
    c->res_dev = (int*)dp;
    return LASR_OK;
}

// per-token records of the beam (lasr_set_beam_records), synchronous and offline steps: [n_iter_slots][Md] beside b_trellis, and the
// pinned block they are copied to once per step (stream idle).  They exist exactly while the switch is on: switch-on allocates them
// for the trellis as it is then, ensure_T regrows them with it, switch-off frees them, so they never lag behind n_iter_slots
// (rec_slots says what they hold; run_decode_beam checks it).
void free_beam_recs(lasr_ctx* c) {
    dfree(c, c->b_rec); c->b_rec = nullptr;
    if (c->rec_host) (void)hipHostFree(c->rec_host);
    c->rec_host = nullptr;
    c->rec_slots = 0;
}
int alloc_beam_recs(lasr_ctx* c) {
    free_beam_recs(c);
    if (c->n_iter_slots <= 0) return LASR_OK;              // (nothing has run yet: ensure_T allocates with the trellis)
    RC(dalloc(c, &c->b_rec, (size_t)c->n_iter_slots * c->Md));
    HIPCHK(c, hipHostMalloc((void**)&c->rec_host, sizeof(BeamRec) * (size_t)c->n_iter_slots * c->Md));
    c->rec_slots = c->n_iter_slots;
    return LASR_OK;
}

int ensure_T(lasr_ctx* c, int T) {
    if (T <= c->Tcap) return LASR_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drop_decode_graphs(c);                                              // captured pointers become stale
    for (auto& kv : c->mgraphs) (void)hipGraphExecDestroy(kv.second);
    c->mgraphs.clear();
    const int M = c->M, H = c->d.hidden, F = c->d.feat, J = c->d.joint;
    int cap = std::max(T, std::max(2 * c->Tcap, c->d.n_buffer));
    dfree(c, c->x0); dfree(c, c->ybuf[0]); dfree(c, c->ybuf[1]); dfree(c, c->pe_sync);
    c->pe_sync = nullptr;
    dfree(c, c->ds.unfinished);
    c->x0 = c->ybuf[0] = c->ybuf[1] = nullptr; c->ds.unfinished = nullptr;
    RC(dalloc(c, (char**)&c->x0, (size_t)cap * M * F * c->esz));
    RC(dalloc(c, (char**)&c->ybuf[0], (size_t)cap * M * H * c->esz));
    RC(dalloc(c, (char**)&c->ybuf[1], (size_t)cap * M * H * c->esz));
    RC(dalloc0(c, &c->pe_sync, (size_t)cap * M * J));
    const int mi = std::max(c->d.max_iters_offline, c->d.max_iters_stream);
    c->tok_cap_alloc = cap * mi;
    RC(alloc_results(c));
    c->n_iter_slots = cap * mi + 8;
    RC(dalloc0(c, &c->ds.unfinished, (size_t)c->n_iter_slots));
    if (c->W > 1) {
        dfree(c, c->b_trellis); c->b_trellis = nullptr;
        RC(dalloc(c, &c->b_trellis, (size_t)c->n_iter_slots * c->Md));
        if (c->trellis_host) (void)hipHostFree(c->trellis_host);
        c->trellis_host_ints = (size_t)c->n_iter_slots * c->Md + 4 * (size_t)c->Md + 16;
        HIPCHK(c, hipHostMalloc((void**)&c->trellis_host, sizeof(int) * c->trellis_host_ints));
        if (c->beam_rec_on) RC(alloc_beam_recs(c));
    }
    HIPCHK(c, hipMemset(c->ybuf[0], 0, (size_t)cap * M * H * c->esz));
    HIPCHK(c, hipMemset(c->ybuf[1], 0, (size_t)cap * M * H * c->esz));
    HIPCHK(c, hipMemset(c->x0, 0, (size_t)cap * M * F * c->esz));
    c->Tcap = cap;
    return LASR_OK;
}

template <class T>
int ensure_buf(lasr_ctx* c, T** p, size_t* have, size_t need) {
    if (need <= *have) return LASR_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(c, *p);
    *p = nullptr;
    need = need + need / 4;
    RC(dalloc(c, p, need));
    *have = need;
    return LASR_OK;
}


}  // namespace
