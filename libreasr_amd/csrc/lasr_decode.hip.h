// lasr_decode.hip.h -- state reset, encoder pass, greedy and beam decode loops of the synchronous protocol
// Engine unit only (lasr_engine.hip), included after lasr_host.hip.h and lasr_cmd.hip.h.
#pragma once

namespace {

// ---------------------------------------------------------------------------- reset
// applies c->dc.what (already committed) to the state on v's stream; runs the predictor on BOS for rows with bit 2
// plain_rows: op-level entry points address predictor rows directly (row = batch index, greedy kernels)
int apply_reset(lasr_ctx* c, const DecView& v, bool any_pred, int mask = 3, bool plain_rows = false) {
    const bool beam = c->W > 1 && !plain_rows;
    ResetArgs a{};
    a.what = c->dc.what; a.mask = mask; a.M = c->M; a.MT = c->MT; a.H = c->d.hidden; a.Le = c->d.enc_layers; a.Lp = c->d.pred_layers;
    a.pred_lstm = c->d.pred_cell; a.bos = c->d.bos; a.bf = c->bf;
    a.W = beam ? c->W : 1; a.Md = c->Md; a.score = c->b_score; a.alive = c->b_alive; a.inB = c->b_inB; a.parent = c->b_parent;
    a.seq_hash = c->b_seq_hash; a.seq_len = c->b_seq_len;          // (null until lasr_set_beam_merge was first turned on)
    for (int l = 0; l < a.Le; ++l) {
        a.enc_h[l] = c->enc_h[c->enc_par][l]; a.enc_c[l] = c->enc_c[l];
        a.enc_h0[l] = c->enc[l].h0; a.enc_c0[l] = c->enc[l].c0;
    }
    for (int l = 0; l < a.Lp; ++l) {
        a.pred_h[l] = c->pred_h[v.pred_par][l];
        a.pred_c[l] = c->d.pred_cell ? c->pred_c[par_rd(beam, v.pred_par)][l] : nullptr;
        a.pred_h0[l] = c->pred[l].h0; a.pred_c0[l] = c->pred[l].c0;
    }
    a.token = c->ds.token; a.emit = c->ds.emit;
    a.bias_node = bias_on(c) && beam == (c->W > 1) ? c->bias.node : nullptr;      // (the nodes restart with the predictor; a beam's plain rows have none)
    const bool use_bos = c->bos_ready && !beam && !plain_rows && c->W == 1 && (mask & 2);
    if (use_bos) {
        for (int l = 0; l < a.Lp; ++l) { a.bos_h[l] = c->bos_h[l]; a.bos_c[l] = c->d.pred_cell ? c->bos_c[l] : nullptr; }
        a.bos_pp = c->bos_pp; a.pp = c->pp[0]; a.J = c->d.joint;
        any_pred = false;                    // the state after the BOS step is stored, not computed
    }
    hipLaunchKernelGGL(k_reset_rows, dim3(grid1((size_t)c->M * c->d.hidden)), dim3(256), 0, v.stream, a);
    if (c->lm.on && (mask & 2)) {      // LM state lives on the decode side, like the predictor's
        LmResetArgs la{};
        const bool lb = c->W > 1 && !plain_rows;         // beam: W slots per stream, current parity of every ping-pong buffer
        la.what = c->dc.what; la.M = c->M; la.H = c->lm.H; la.L = c->lm.L; la.bf = c->lm.q8 ? 0 : c->bf;
        la.W = lb ? c->W : 1; la.Md = lb ? c->Md : c->M;
        const int lp = par_rd(lb, v.lm_par);
        la.lm_valid = c->lm.valid[lp];
        for (int l = 0; l < c->lm.L; ++l) { la.h[l] = c->lm.h[v.lm_par][l]; la.c[l] = c->lm.cst[lp][l]; }
        if (c->lm.q8) { la.Kp = c->lm.Kp_h; for (int l = 0; l < c->lm.L; ++l) { la.qh[l] = c->lm.qh[l]; la.sxh[l] = c->lm.sxh[l]; } }
        hipLaunchKernelGGL(k_lm_reset, dim3(grid1((size_t)c->M * c->lm.H)), dim3(256), 0, v.stream, la);
    }
    if (any_pred) {
        // T_row = 0 for every row: EpiPPJ then only refreshes pp (models.py:489: predictor(BOS))
        DecView bos = v;
        bos.T_row = c->zero_rows;
        HIPCHK(c, hipMemsetAsync(c->ds.t_idx, 0, sizeof(int) * c->M, v.stream));
        launch_predictor(c, bos, beam);
        launch_ppj(c, bos, beam);
        c->pred_par = bos.pred_par;
    }
    return LASR_OK;
}

// ---------------------------------------------------------------------------- in-job cell timing
void cell_prof_harvest(lasr_ctx* c, bool all) {
    while (c->cp_n > 0) {
        const int i = ((c->cp_head - c->cp_n) % lasr_ctx::NCELLEV + lasr_ctx::NCELLEV) % lasr_ctx::NCELLEV;
        if (!all && c->cp_n < lasr_ctx::NCELLEV && hipEventQuery(c->cp_ev[i][1]) != hipSuccess) { (void)hipGetLastError(); break; }
        (void)hipEventSynchronize(c->cp_ev[i][1]);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->cp_ev[i][0], c->cp_ev[i][1]) == hipSuccess) {
            c->cp_us += 1e3 * (double)ms;
            c->cp_launches += c->cp_cells[i];
        } else {
            (void)hipGetLastError();
        }
        c->cp_n--;
    }
}

// ---------------------------------------------------------------------------- encoder + decode
// Encoder over T_max frames for rows with T_row > 0 (x0 already holds LayerNorm'ed features).
// st: the stream it is enqueued on; pe: where the encoder half of the joint goes; pipelined: pe is the per-row frame ring of the
// continuous loop (and the cell sequence may be replayed as a graph)
void run_encoder(lasr_ctx* c, hipStream_t st, float* pe, bool pipelined, int T_max) {
    RoctxRange roctx_range_("lasr encoder cells");
    const int L = c->d.enc_layers;
    const int mt_total = c->Tcap * c->MT;
    const int par0 = c->enc_par;
    int cp_slot = -1;
    if (c->cell_prof && c->cp_ok && c->cell_prof_events) {
        if (c->cp_n >= lasr_ctx::NCELLEV) cell_prof_harvest(c, false);
        cp_slot = c->cp_head;
        c->cp_head = (c->cp_head + 1) % lasr_ctx::NCELLEV;
        c->cp_cells[cp_slot] = L * T_max;
        (void)hipEventRecord(c->cp_ev[cp_slot][0], st);
    }
    tr_mark(c, 3, st);
    // layer wavefront: the cells (l, t) with l + t = d depend only on diagonal d - 1, so a diagonal is ONE launch
    // (k_gemm_multi, up to NPMAX cells): L + T - 1 launches instead of L * T, and the per-launch fixed costs of a cell
    // overlap its neighbours' K loops.  Cell (l, t) reads h parity par0 ^ (t & 1); all layers end on par0 ^ (T & 1).
    // Otherwise layer-major order: every layer starts from parity par0 and toggles T_max times (enc_h[par][l] is
    // indexed by the parity at launch time, so all layers end on par0 ^ (T_max & 1)).
    auto enqueue_cells = [&](hipStream_t es) {
        if (c->enc_wave && L > 1 && T_max > 1) {
            EncCellRef cells[NPMAX];
            for (int d = 0; d < L + T_max - 1; ++d) {
                int n = 0;
                for (int l = std::min(d, L - 1); l >= 0 && d - l < T_max; --l) {
                    cells[n++] = EncCellRef{l, d - l};
                    if (n == NPMAX) { launch_enc_wave(c, es, cells, n, par0, mt_total); n = 0; }
                }
                if (n) launch_enc_wave(c, es, cells, n, par0, mt_total);
            }
        } else {
            for (int l = 0; l < L; ++l) {
                c->enc_par = par0;
                const void* xsrc = (l == 0) ? c->x0 : c->ybuf[(l - 1) & 1];
                void* ydst = c->ybuf[l & 1];
                for (int t = 0; t < T_max; ++t) {
                    launch_enc_cell(c, es, l, t, xsrc, mt_total, ydst, mt_total);
                    c->enc_par ^= 1;
                }
            }
        }
        c->enc_par = par0 ^ (T_max & 1);
    };
    // Pipelined protocol: the cell sequence of a model step (launches whose arguments only depend on which m-tiles are active
    // and on the ping-pong parity) is replayed as ONE hipGraph on the caller's stream: 8 (bf16 wavefront: 5) launches -> 1 per
    // model step on the host.  The graph is recorded by capturing on an internal stream (the caller's may be the legacy NULL
    // stream, which cannot capture) and launched on the caller's.  Not with the in-kernel timers (a per-launch slot pointer) or
    // the debug stamps.
    bool replayed = false;
    if (c->main_graph && c->use_graphs && pipelined && !(c->cell_prof && c->cp_slots) && !c->dbg && T_max <= 8) {
        std::vector<unsigned long long> key{(unsigned long long)T_max, (unsigned long long)par0, (unsigned long long)(uintptr_t)c->T_row_dev,
                                            (unsigned long long)(uintptr_t)c->x0, (unsigned long long)mt_total, (unsigned long long)c->enc_wave};
        for (int t = 0; t < T_max; ++t) key.push_back(c->tile_masks.empty() ? ~0ull : c->tile_masks[t]);
        auto it = c->mgraphs.find(key);
        bool ok = true;
        if (it == c->mgraphs.end() && c->mgraphs.size() >= 64) {
            // the key holds the per-frame masks of the active m-tiles: with many slots and churning streams the combinations do
            // not repeat, and every new one costs a capture + instantiation on the submit path and memory for good.  Past 64
            // cached graphs the cache is dropped (the steady state of a full server -- all tiles active -- is one entry)
            for (auto& kv : c->mgraphs) (void)hipGraphExecDestroy(kv.second);
            c->mgraphs.clear();
        }
        if (it == c->mgraphs.end()) {
            if (!c->stream_cap && hipStreamCreateWithFlags(&c->stream_cap, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ok = false; }
            hipGraphExec_t ex = nullptr;
            // (no context for the error text: a failure here is answered by plain launches, not reported by the call)
            ok = ok && capture_graph(nullptr, c->stream_cap, [&] { enqueue_cells(c->stream_cap); return LASR_OK; }, &ex) == LASR_OK;
            c->enc_par = par0;                                                // (the capture only recorded)
            if (!ok) { (void)hipGetLastError(); c->main_graph = false; }      // (fall back to plain launches for good)
            else it = c->mgraphs.emplace(key, ex).first;
        }
        if (ok && hipGraphLaunch(it->second, st) == hipSuccess) {
            c->enc_par = par0 ^ (T_max & 1);
            replayed = true;
        }
    }
    if (!replayed) enqueue_cells(st);
    if (cp_slot >= 0) { (void)hipEventRecord(c->cp_ev[cp_slot][1], st); c->cp_n++; }
    tr_mark(c, 4, st);
    if (c->enclog && c->enclog_n < c->enclog_cap && 2 * T_max + 2 * L + 2 <= 32) {       // LASR_DBG_ENCLOG: checksums behind this step's cells
        RowSumArgs ra{};
        int e = 0;
        for (int t = 0; t < T_max; ++t) ra.s[e++] = RowSumSrc{c->x0, 0, mt_total, t * c->MT, c->d.feat};
        for (int l = 0; l < L; ++l) ra.s[e++] = RowSumSrc{c->enc_c[l], 1, 0, 0, c->d.hidden};
        for (int l = 0; l < L; ++l) ra.s[e++] = RowSumSrc{c->enc_h[c->enc_par][l], 0, c->MT, 0, c->d.hidden};
        for (int t = 0; t < T_max; ++t) ra.s[e++] = RowSumSrc{c->ybuf[(L - 1) & 1], 0, mt_total, t * c->MT, c->d.hidden};
        ra.s[e++] = RowSumSrc{c->pend, 2, 0, 0, c->d.n_buffer * c->d.n_stack * c->d.n_mels};
        ra.s[e++] = RowSumSrc{c->win, 2, 0, 0, c->ring_chunks * c->d.chunk};
        hipLaunchKernelGGL(k_dbg_rowsum, dim3(c->M, e), dim3(256), 0, st, ra, c->M, c->bf,
                           c->enclog + (size_t)c->enclog_n * 32 * c->M);
        if (c->pendlog) {
            const size_t n = (size_t)c->M * c->d.n_buffer * c->d.n_stack * c->d.n_mels;
            (void)hipMemcpyAsync(c->pendlog + (size_t)c->enclog_n * n, c->pend, sizeof(float) * n, hipMemcpyDeviceToDevice, st);
        }
        c->enclog_n++;
    }
    // encoder half of the joint for all frames: pe[t][r] = W1e * enc[t][r]
    const int H = c->d.hidden, J = c->d.joint;
    GemmArgs g{};
    set_operand(g, 0, c->ybuf[(L - 1) & 1], mt_total, 0, 0, c->W1e);
    EpiLinear::Args ea{};
    ea.bias = nullptr; ea.out = pe; ea.ldo = J; ea.n_rows = T_max * c->M; ea.t_idx = nullptr; ea.T_row = nullptr; ea.M = c->M;
    if (pipelined) { ea.ring_base = c->fe_fused ? c->c_enc_base : c->c_enc_frames; ea.ring = lasr_ctx::RING; }   // continuous mode: per-row frame ring
    DecView v{};                   // (a plain linear GEMM: launch_gemm reads the stream only)
    v.stream = st;
    launch_linear<false, 3>(c, v, J / 16, T_max * c->MT, g, H, ea);
}

// ---------------------------------------------------------------------------- one decode iteration
// LM branch of an iteration (LASR_LM_SIDE, pipelined protocol): forked onto stream_lm behind the selection kernel whose tokens it
// consumes, joined in front of the next one (which reads its scores and rewrites token / emit) or at the end of the group -- the
// predictor, the joint half and the next logits GEMM run beside it (captured: two branches of the group graph)
struct LmSide {
    bool open = false;
    void join(lasr_ctx* c, const DecView& v) {
        if (open) (void)hipStreamWaitEvent(v.stream, c->ev_lm_join, 0);
        open = false;
    }
    void fork(lasr_ctx* c, DecView& v, bool beam) {
        (void)hipEventRecord(c->ev_lm_fork, v.stream);
        (void)hipStreamWaitEvent(c->stream_lm, c->ev_lm_fork, 0);
        DecView lv = v;
        lv.stream = c->stream_lm;
        launch_lm(c, lv, beam);
        v.lm_par = lv.lm_par;
        (void)hipEventRecord(c->ev_lm_join, c->stream_lm);
        open = true;
    }
};
// logits -> selection -> predictor -> joint half -> LM step on v, once.  b: the beam's round (selection slot `it`), null: greedy
// (s, slot `it`, max_iters).  side: the LM step as a branch (see LmSide) instead of in line behind the joint half.
void decode_iteration(lasr_ctx* c, DecView& v, const DecState& s, BeamState* b, int it, int max_iters, LmSide* side = nullptr) {
    const bool beam = b != nullptr;
    launch_logits(c, v, c->logits, beam ? c->Md : v.la * c->M, true);
    if (side) side->join(c, v);
    if (beam) launch_beam_select(c, v, *b, it);
    else launch_select<false>(v.stream, c->M, c->logits, c->d.vocab, c->d.blank, max_iters, v.T_row, s, it, nullptr, nullptr, v.la, c->M, bias_on(c));
    if (side) side->fork(c, v, beam);
    launch_predictor(c, v, beam);
    launch_ppj(c, v, beam);
    if (!side) launch_lm(c, v, beam);
}
// the round protocol of the continuous loop, the same for the greedy and the beam state (host_flag: set per launch, cont_enqueue)
ContRound cont_round_state(lasr_ctx* c) { return ContRound{1, c->c_iter, c->c_done, c->c_behind, nullptr, c->c_hcur_dev}; }
// the beam's kernel state: synchronous / offline steps (trellis and records of the step), or cont = the continuous loop (rings)
BeamState beam_state(lasr_ctx* c, const DecView& v, bool cont, int max_iters) {
    BeamState b{};
    b.W = c->W; b.V = c->d.vocab; b.blank = c->d.blank; b.max_iters = max_iters; b.Md = c->Md;
    b.t_idx = v.t_idx; b.T_row = v.T_row;
    b.score = c->b_score; b.alive = c->b_alive; b.inB = c->b_inB; b.token = c->ds.token; b.emit = c->ds.emit; b.parent = c->b_parent;
    if (c->beam_merge) { b.seq_hash = c->b_seq_hash; b.seq_len = c->b_seq_len; }
    if (bias_on(c)) {                         // (lasr_set_beam_bias: the BIAS instantiations)
        b.bias.node = c->bias.node;
        b.bias_back = lasr_bias::view_block(c->bias.block, c->bias.n_nodes, c->bias.n_edges, c->bias.has_back, b.bias);
    }
    if (!cont) {
        b.iters = c->ds.iters; b.trellis = c->b_trellis; b.unfinished = c->ds.unfinished;
        b.dbg = c->dbg ? c->dbg + (size_t)4 * 4096 * 16 : nullptr;      // reuses the "logits" slot of the debug buffer
        b.rec = c->beam_rec_on ? c->b_rec : nullptr;
        return b;
    }
    static_cast<ContRound&>(b) = cont_round_state(c);
    b.iters = c->c_iters; b.trellis = c->b_tre_dev;
    b.tring = lasr_ctx::TRING; b.frame_done = c->b_fdone_dev; b.step_T = c->d.n_buffer; b.end_slots = lasr_ctx::ENDSLOTS;
    b.end_score = c->b_endsc_dev; b.end_alive = c->b_endal_dev;
    b.rec = c->beam_rec_on ? c->b_rec_ring_dev : nullptr;
    return b;
}
// wait for a pinned flag word to leave -1: a spin instead of hipStreamSynchronize (interrupt wake-up costs ~10-20 us per round
// trip, and there are 2-4 per step); a real sync of `st` if nothing arrives
int spin_flag(lasr_ctx* c, volatile int* flag, hipStream_t st) {
    unsigned long long spins = 0;
    while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == -1) {
        __builtin_ia32_pause();
        if (++spins > (1ull << 27)) { HIPCHK(c, hipStreamSynchronize(st)); break; }
    }
    return LASR_OK;
}

// Greedy decode of the current step (T_row_dev, pe ready).  Blocks until done; fills host queues.
int run_decode_beam(lasr_ctx* c, int T_max, int max_iters, bool offline, const std::vector<int>& rows);

int run_decode(lasr_ctx* c, int T_max, int max_iters, bool offline, const std::vector<int>& rows) {
    if (c->W > 1) return run_decode_beam(c, T_max, max_iters, offline, rows);
    const int M = c->M, J = c->d.joint;
    DecView v = sync_view(c, offline ? c->la_offline : c->la_sync);
    DecState s = c->ds;
    s.tok_cap = T_max * max_iters;
    // alignment records (lasr_set_alignments): two more arrays of the step's own [M][tok_cap] shape right behind the tokens, so
    // they travel in the same payload / copy; off: null pointers, the payload is what it always was
    const bool recs = c->align_on;
    if (recs) {
        s.step_frame = s.step_tok + (size_t)M * s.tok_cap;
        s.step_logp = (float*)(s.step_frame + (size_t)M * s.tok_cap);
    }
    const size_t n_tokw = (recs ? 3 : 1) * (size_t)M * s.tok_cap;     // ints behind ntok[M]
    const int total_cap = T_max * max_iters;
    int iter = 0;
    // iterations are launched in even-sized groups (the predictor ping-pong parity then returns to
    // its start); after each group the "rows still decoding" counter and the step's tokens so far
    // come back in the same round trip.  In streaming mode every group is a cached hipGraph: one
    // launch instead of 4 kernels per iteration, so the GPU is not fed at host launch speed.
    // (with lookahead a row consumes up to `la` blank frames per iteration: fewer iterations up front)
    constexpr int sync_first = 4;   // extra iterations of the first group
    constexpr int sync_next = 2;    // (swept in round 2: 4 + 2 best, +2 %)
    int group = offline ? std::min(total_cap, ((T_max + v.la - 1) / v.la + 16) & ~1) : std::min(total_cap, (T_max + sync_first) & ~1);
    const int next_group = offline ? 32 : sync_next;
    int* res = c->res_host;
    int* ntok = res + 4;
    int* toks = ntok + M;                      // contiguous with ntok, as on the device
    const int* frames = toks + (size_t)M * s.tok_cap;     // (records on)
    const float* logps = (const float*)(frames + (size_t)M * s.tok_cap);
    int* sum_iters = toks + n_tokw;
    int* n_ones = sum_iters + M;
    double* logp = (double*)(((uintptr_t)(n_ones + M) + 15) & ~uintptr_t(15));
    // (the legacy NULL stream cannot be captured: graphs then only serve the pipelined path, whose
    //  decode loop runs on the ctx-owned stream_dec)
    const bool graphs = c->use_graphs && !offline && !c->profiling && !c->dbg && v.stream != nullptr;
    const int buf_idx = 0;
    auto enqueue_group = [&](DecView& v, int first, int n) -> int {
        if (first == 0) {
            hipLaunchKernelGGL(k_step_begin, dim3(grid1(std::max(M, c->n_iter_slots))), dim3(256), 0, v.stream, s, M,
                               c->n_iter_slots, offline ? 1 : 0);
            hipLaunchKernelGGL(k_ja, dim3(grid1((size_t)M * J)), dim3(256), 0, v.stream, v.pe, c->pp[0], v.t_idx,
                               v.T_row, c->ja, J, M, c->MTj, v.ring, c->bf, 1, M, v.la);
        }
        for (int it = first; it < first + n; ++it) {
            v.dbg_gate = (it == 0);
            decode_iteration(c, v, s, nullptr, it, max_iters);
        }
        // The host spins on the "rows still decoding" word in pinned memory.  Streaming: the step's tokens so far travel with it --
        // k_publish stores them into the pinned block and releases the word last (system scope).  Offline (whole utterances,
        // large token blocks): only the word comes back per group; the results are copied once at the end, behind a real
        // synchronisation.  A word that arrives by hipMemcpyAsync carries nothing but itself: no ordering against any other
        // copy is assumed anywhere (round 3's "payload copy, then flag copy" let the flag overtake the payload: tests/soak.py).
        const int n_pay = M + (int)n_tokw;
        if (!offline) {
            const int nb = std::max(1, std::min(64, (n_pay + 1023) / 1024));
            hipLaunchKernelGGL(k_publish, dim3(nb), dim3(256), 0, v.stream, (const int*)c->ds.step_ntok, c->res_dev + 4, n_pay,
                               (const int*)(c->ds.unfinished + (first + n - 1)), c->res_dev, c->pub_arrivals);
            return LASR_OK;
        }
        HIPCHK(c, hipMemcpyAsync(res, c->ds.unfinished + (first + n - 1), sizeof(int), hipMemcpyDeviceToHost, v.stream));
        return LASR_OK;
    };
    while (iter < total_cap) {
        const int n = std::min(group, total_cap - iter);
        bool launched = false;
        __atomic_store_n(&res[0], -1, __ATOMIC_RELEASE);      // sentinel, overwritten by the last copy of the group (stored BEFORE anything
                                                              // of the group is enqueued: a fast group must not be overwritten by it)
        if (graphs && (n % 2) == 0) {
            const auto key = std::make_tuple(iter, n, buf_idx, v.pred_par + 2 * v.lm_par, T_max * 1024 + max_iters);
            auto it = c->graphs.find(key);
            if (it == c->graphs.end()) {
                hipGraphExec_t ex = nullptr;
                DecView rec_v = v;              // (an even group: the parities it ends on are the key's)
                RC(capture_graph(c, v.stream, [&] { return enqueue_group(rec_v, iter, n); }, &ex));
                it = c->graphs.emplace(key, ex).first;
            }
            HIPCHK(c, hipGraphLaunch(it->second, v.stream));
            launched = true;
        }
        if (!launched) {
            const int rc = enqueue_group(v, iter, n);
            c->pred_par = v.pred_par; c->lm.par = v.lm_par;      // (what was enqueued has advanced the buffers, whatever the group's tail returned)
            RC(rc);
        }
        iter += n;
        static const bool spin = !(getenv("LASR_SPIN") && atoi(getenv("LASR_SPIN")) == 0);      // LASR_SPIN=0: always a real sync
        if (!spin) HIPCHK(c, hipStreamSynchronize(v.stream));
        else RC(spin_flag(c, &res[0], v.stream));
        if (res[0] == 0) break;
        group = next_group;
    }
    c->stats.decode_iters = iter;
    if (offline) {
        // offline results: one copy each, read only after the stream has been synchronised
        HIPCHK(c, hipMemcpyAsync(ntok, c->ds.step_ntok, sizeof(int) * ((size_t)M + n_tokw), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(sum_iters, c->ds.sum_iters, sizeof(int) * M, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(n_ones, c->ds.n_ones, sizeof(int) * M, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(logp, c->ds.logp_sum, sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int r : rows) {
        const int n = std::min(ntok[r], s.tok_cap);
        SlotResult& out = c->results[r];
        const size_t at = (size_t)r * s.tok_cap;
        // the kernel's frame cursor starts at 0 in every step: + the frames the slot consumed before this call (offline: the
        // utterance starts the count)
        const long long base = offline ? 0 : c->slot_frames[r];
        if (!recs) for (int q = 0; q < n; ++q) out.append(toks[at + q]);
        else for (int q = 0; q < n; ++q) out.append(toks[at + q], {(int32_t)(base + frames[at + q]), logps[at + q]});
        c->slot_frames[r] = base + c->hc.T_row[r];
        if (offline) {
            out.neg_logp = -logp[r];
            // alignment_score = (sum(iters) - #frames with 1 iter) / (sum(iters) + 1e-4)  (models.py:447-453)
            out.align = ((double)sum_iters[r] - (double)n_ones[r]) / ((double)sum_iters[r] + 1e-4);
        }
    }
    return LASR_OK;
}

// Beam search over the current step (W > 1): one selection round per iteration for every stream that
// still has frames; blocks until done.  The per-round (parent, token) records come back in one copy and
// are replayed on the host into the token history of every hypothesis slot.
int run_decode_beam(lasr_ctx* c, int T_max, int max_iters, bool offline, const std::vector<int>& rows) {
    const int M = c->M, Md = c->Md, W = c->W, J = c->d.joint;
    DecView v = sync_view(c, 1);
    v.dbg_gate = c->dbg && getenv("LASR_DBG_BEAM");         // (LASR_DBG_TIMING + LASR_DBG_BEAM: phase stamps of the beam round's GEMMs)
    BeamState b = beam_state(c, v, false, max_iters);
    const bool recs = c->beam_rec_on;
    const int total_cap = T_max * max_iters;
    if (total_cap + 1 > c->n_iter_slots) return fail(c, LASR_EINVAL, "decode iteration budget exceeds the trellis");
    // the records are indexed like the trellis: they must hold as many rounds as it does
    if (recs && (!c->b_rec || !c->rec_host || c->rec_slots != c->n_iter_slots))
        return fail(c, LASR_ESTATE, "beam records are on but their buffers hold %d rounds, the trellis %d", c->rec_slots, c->n_iter_slots);
    int* res = c->res_host;
    hipLaunchKernelGGL(k_beam_begin, dim3(grid1(std::max(Md, c->n_iter_slots))), dim3(256), 0, v.stream, b, M, c->n_iter_slots);
    hipLaunchKernelGGL(k_ja, dim3(grid1((size_t)Md * J)), dim3(256), 0, v.stream, (const float*)v.pe, (const float*)cur_pp(c),
                       (const int*)v.t_idx, (const int*)v.T_row, c->ja, J, Md, c->MTj, v.ring, c->bf, W, M, 1);
    int iter = 0;
    int group = offline ? std::min(total_cap, T_max + 16) : std::min(total_cap, T_max + 4);
    const int next_group = offline ? 32 : 4;
    while (iter < total_cap) {
        const int n = std::min(group, total_cap - iter);
        for (int q = 0; q < n; ++q) decode_iteration(c, v, c->ds, &b, iter + q, max_iters);
        c->pred_par = v.pred_par; c->lm.par = v.lm_par;
        iter += n;
        __atomic_store_n(&res[0], -1, __ATOMIC_RELEASE);
        HIPCHK(c, hipMemcpyAsync(res, c->ds.unfinished + (iter - 1), sizeof(int), hipMemcpyDeviceToHost, v.stream));
        RC(spin_flag(c, &res[0], v.stream));
        if (res[0] == 0) break;
        group = next_group;
    }
    c->stats.decode_iters = iter;
    // results: the rounds' records + final scores
    int* tre = c->trellis_host;
    double* sc = (double*)(tre + (((size_t)iter * Md + 1) & ~size_t(1)));
    int* alive = (int*)(sc + Md);
    HIPCHK(c, hipMemcpyAsync(tre, c->b_trellis, sizeof(int) * (size_t)iter * Md, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sc, c->b_score, sizeof(double) * Md, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(alive, c->b_alive, sizeof(int) * Md, hipMemcpyDeviceToHost, c->stream));
    if (recs) HIPCHK(c, hipMemcpyAsync(c->rec_host, c->b_rec, sizeof(BeamRec) * (size_t)iter * Md, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r : rows) {
        BeamSlot& B = c->beams[r];
        // the kernel's frame cursor starts at 0 in every step: + the frames the slot consumed before this call (offline: the
        // utterance starts the count), as in run_decode
        const long long base = offline ? 0 : c->slot_frames[r];
        for (int it = 0; it < iter; ++it) {
            const int* e = tre + (size_t)it * Md + (size_t)r * W;
            if (e[0] == -1) continue;                          // stream idle in this round
            bh_apply(B.tree, e, W, recs ? c->rec_host + (size_t)it * Md + (size_t)r * W : nullptr, base);
        }
        c->slot_frames[r] = base + c->hc.T_row[r];
        unsigned am = 0;
        for (int j = 0; j < W; ++j) am |= (alive[(size_t)r * W + j] != 0) << j;
        B.deliver(B.build(sc + (size_t)r * W, am, recs), c->results[r]);      // beam mode: lasr_fetch hands out the whole best hypothesis
    }
    return LASR_OK;
}

// host side of a predictor reset in beam mode: the best hypothesis so far is frozen (or, with the transcript, forgotten)
void beam_host_reset(lasr_ctx* c, int slot, bool forget) {
    if (c->W <= 1) return;
    if (forget) c->beams[slot].forget();
    else c->beams[slot].freeze(-c->results[slot].neg_logp);
}

void rec(lasr_ctx* c, int i) {
    if (c->profiling && c->ev_ok) (void)hipEventRecord(c->ev[i], c->stream);
}
void collect_stats(lasr_ctx* c, int T) {
    c->stats.frames = T;
    if (!(c->profiling && c->ev_ok)) return;
    float a = 0, b = 0, d = 0;
    (void)hipEventElapsedTime(&a, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&b, c->ev[1], c->ev[2]);
    (void)hipEventElapsedTime(&d, c->ev[2], c->ev[3]);
    c->stats.frontend_ms = a; c->stats.encoder_ms = b; c->stats.decode_ms = d;
    c->stats.cell_ms = b; c->stats.cell_launches = T * c->d.enc_layers;
}

int check_slots(lasr_ctx* c, const int* slots, int n, bool need_open) {
    if (!slots || n < 0 || n > c->d.max_streams) return fail(c, LASR_EINVAL, "bad slot list (n=%d)", n);
    std::vector<char> seen(c->M, 0);
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        if (s < 0 || s >= c->d.max_streams) return fail(c, LASR_EINVAL, "slot %d out of range", s);
        if (seen[s]) return fail(c, LASR_EINVAL, "slot %d listed twice", s);
        seen[s] = 1;
        if (need_open && !c->open_[s]) return fail(c, LASR_ESTATE, "slot %d is not open", s);
    }
    return LASR_OK;
}

// c->mu held.  The ctx stream waits (on the GPU, the host does not block) for whatever the last decode group still has queued
// behind its published flag: see lasr_ctx::dec_tail_open
int order_after_decode_tail(lasr_ctx* c) {
    if (!c->dec_tail_open || !c->stream_dec || !c->ev_misc) return LASR_OK;
    HIPCHK(c, hipEventRecord(c->ev_misc, c->stream_dec));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_misc, 0));
    c->dec_tail_open = false;
    return LASR_OK;
}
int require_idle(lasr_ctx* c) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->pending.empty()) return fail(c, LASR_ESTATE, "%d submitted step(s) not collected: call lasr_step_wait first", (int)c->pending.size());
    if (c->group_inflight) {        // the last group of the pipelined protocol may still be running: the calls that need an idle engine
        HIPCHK(c, hipStreamSynchronize(c->stream_dec));      // use the same decode state on the ctx stream
        cont_poll(c);                                        // (its flag and cursors are there now)
        c->group_inflight = false;
        c->dec_tail_open = false;
    }
    return order_after_decode_tail(c);
}

bool is_device_ptr(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice;
}

// pinned (page-locked, device-mapped) host memory: returns the address the device can read it at, else nullptr
const void* pinned_host_dev_ptr(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    return at.devicePointer;
}

// HTK mel filterbank (torchaudio 0.6.0 create_fb_matrix semantics), sparse, bin-ascending
void build_fb(const lasr_model_desc& d, std::vector<int>& start, std::vector<int>& off, std::vector<float>& w) {
    const int nf = d.n_fft / 2 + 1, nm = d.n_mels;
    const double fmax = d.sample_rate / 2;
    auto mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
    std::vector<double> fpts(nm + 2);
    const double m0 = mel(0.0), m1 = mel(fmax);
    for (int i = 0; i < nm + 2; ++i) {
        const double m = m0 + (m1 - m0) * i / (nm + 1);
        fpts[i] = 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    }
    start.assign(nm, 0); off.assign(nm + 1, 0); w.clear();
    for (int m = 0; m < nm; ++m) {
        int first = -1;
        std::vector<float> vals;
        for (int k = 0; k < nf; ++k) {
            const double f = fmax * k / (nf - 1);
            const double down = (f - fpts[m]) / (fpts[m + 1] - fpts[m]);
            const double up = (fpts[m + 2] - f) / (fpts[m + 2] - fpts[m + 1]);
            const double v = std::max(0.0, std::min(down, up));
            if (v > 0.0) {
                if (first < 0) first = k;
                while ((int)vals.size() < k - first) vals.push_back(0.f);
                vals.push_back((float)v);
            }
        }
        start[m] = first < 0 ? 0 : first;
        off[m] = (int)w.size();
        w.insert(w.end(), vals.begin(), vals.end());
    }
    off[nm] = (int)w.size();
}


}  // namespace
