// lasr_launch.hip.h -- launch interface of the GEMM kernels, shared by the translation units of liblasr_hip.so.
// The library is FOUR translation units (round 6; one 3.5-minute unit before): lasr_engine.hip (C ABI, protocols, small kernels),
// lasr_launch_enc.hip (encoder cells), lasr_launch_dec_f32.hip / lasr_launch_dec_bf16.hip (predictor, joint, LM and their pair
// launches per operand type).  Every k_gemm instantiation lives in exactly one of the last three; this header declares the
// host functions that launch them (explicit instantiations per operand type) and the small inline dispatchers on c->bf.
#pragma once

// ---------------------------------------------------------------------------- launch view
// What a decode-side launch helper needs beyond the context's buffers: where it enqueues, which joint-half buffer and frame
// counters the kernels read, and which ping-pong parities the pass starts from.  Built by value, passed by reference: a caller that
// needs a variant (the BOS pass' zero_rows, the LM branch's stream, a recording `cap`) edits a copy, a capture throws its copy away,
// and whoever really enqueued work stores v.pred_par / v.lm_par back into the context.  The helpers read none of this from lasr_ctx.
// (launch_gemm itself reads `stream` and `cap` only: an encoder-side launch passes a view that holds nothing but its stream.)
struct DecView {
    hipStream_t stream;
    float* pe; int ring;            // encoder half of the joint; frame t of a row lives at slot t % ring
    int *t_idx, *T_row;             // per-row frame cursors / frames available
    int la;                         // greedy lookahead: frames evaluated per row and iteration
    bool dbg_gate;                  // LASR_DBG_TIMING: the GEMMs of this pass record their phase stamps
    lasr_ctx::Captured* cap;        // non-null: launch_gemm records into it instead of launching (pair launches)
    int pred_par, lm_par;           // advanced by the helpers
};
// synchronous / offline protocols and the op-level entry points: the caller's stream, whole-step buffers
// (a bias graph attached: one frame per iteration on every protocol; a beam's la is 1 with or without)
inline DecView sync_view(lasr_ctx* c, int la) {
    return DecView{c->stream, c->pe_sync, 1 << 30, c->ds.t_idx, c->T_row_fix, bias_on(c) ? 1 : la, true, nullptr, c->pred_par, c->lm.par};
}
// continuous loop of the pipelined protocol: the decode stream, per-row rings and cursors
inline DecView cont_view(lasr_ctx* c) {
    return DecView{c->stream_dec, c->pe_ring, lasr_ctx::RING, c->c_cur, c->c_avail, bias_on(c) ? 1 : c->la_stream, false, nullptr, c->pred_par, c->lm.par};
}
// s_setprio of a GEMM by the stream it runs on: the decode loop's two streams against everything else
inline int gemm_prio(const lasr_ctx* c, hipStream_t st) {
    return (st && (st == c->stream_dec || st == c->stream_lm)) ? c->dec_prio : c->cell_prio;
}

// ---------------------------------------------------------------------------- launch helpers
template <class Ops, class Epi, int MT, bool AROW, int D = 3, int NWV = NW>
inline void launch_gemm(lasr_ctx* c, const DecView& v, int n_groups, int m_groups, const GemmArgs& g0, const typename Epi::Args& ea) {
    GemmArgs g = g0;
    g.prio = gemm_prio(c, v.stream);
    if (v.cap) {            // recorded for a pair launch (see launch_pair)
        static_assert(sizeof(GemmArgs) <= sizeof(v.cap->g) && sizeof(typename Epi::Args) <= sizeof(v.cap->ea), "Captured too small");
        lasr_ctx::Captured& k = *v.cap;
        k.fn = (const void*)&k_gemm<Ops, Epi, MT, NWV, AROW, D>;
        k.gx = (unsigned)n_groups; k.gy = (unsigned)m_groups; k.threads = NWV * 64;
        memcpy(k.g, &g, sizeof(g)); k.g_size = sizeof(g);
        memcpy(k.ea, (const void*)&ea, sizeof(ea)); k.ea_size = sizeof(ea);
        return;
    }
    hipLaunchKernelGGL((k_gemm<Ops, Epi, MT, NWV, AROW, D>), dim3(n_groups, m_groups), dim3(NWV * 64), 0, v.stream, g, ea);
}
// a recorded launch issued on its own
inline void replay_captured(hipStream_t st, lasr_ctx::Captured& k) {
    if (!k.fn) return;
    void* args[2] = {(void*)k.g, (void*)k.ea};
    (void)hipLaunchKernel(k.fn, dim3(k.gx, k.gy), dim3(k.threads), args, 0, st);
    k.fn = nullptr;
}
inline int grid1(size_t n, int b = 256) { return (int)((n + b - 1) / b); }

// lasr_trace: a value record (no event): lasr_trace_read returns `val` in the time field
// (marks come from the API thread -- main stream -- and from the pump thread -- decode stream: slots are drawn atomically)
inline void tr_note(lasr_ctx* c, int tag, double val) {
    if (!c->tr_on) return;
    const int i = c->tr_n.fetch_add(1, std::memory_order_relaxed);
    if (i >= lasr_ctx::NTRACE) return;
    c->tr_val[i] = val;
    c->tr_tag[i] = tag;
}
// lasr_trace: one timestamped mark on stream `st` (no-op unless tracing)
inline void tr_mark(lasr_ctx* c, int tag, hipStream_t st) {
    if (!c->tr_on) return;
    const int i = c->tr_n.fetch_add(1, std::memory_order_relaxed);
    if (i >= lasr_ctx::NTRACE) return;
    (void)hipEventRecord(c->tr_ev[i], st);
    c->tr_tag[i] = tag;
}


// ---- encoder cells (lasr_launch_enc.hip)
void launch_enc_cell(lasr_ctx* c, hipStream_t st, int l, int t, const void* xsrc, int x_mt_total, void* ydst, int y_mt_total);
struct EncCellRef { int l, t; };
void launch_enc_wave(lasr_ctx* c, hipStream_t st, const EncCellRef* cells, int n, int par0, int mt_total);

// ---- decode-side GEMMs, one set per operand type (lasr_launch_dec.hip.h, instantiated in lasr_launch_dec_{f32,bf16}.hip)
// LASR_BEAM_CARRY: 0 = non-extended hypothesis slots carried inside the cell / joint kernels' epilogues (round 3), 1 = by a launch of
// their own (k_beam_carry), 2 = as extra workgroups of the joint-half GEMM's launch (k_gemm_carry)
inline int beam_carry_mode() {
    static const int v = getenv("LASR_BEAM_CARRY") ? atoi(getenv("LASR_BEAM_CARRY")) : 2;
    return v;
}
inline bool beam_carry_on() { return beam_carry_mode() != 0; }
template <class Ops> void launch_predictor_t(lasr_ctx* c, DecView& v, bool beam, int l0, int l1);
template <class Ops> void launch_ppj_t(lasr_ctx* c, DecView& v, bool beam);
template <class Ops> void launch_lm_t(lasr_ctx* c, DecView& v, bool beam, int l0, int l1, bool tail);
template <class Ops> bool launch_pair_ops(hipStream_t st, int kind, bool lm_first, lasr_ctx::Captured& A, lasr_ctx::Captured& B);
template <class Ops> void launch_logits_ops(lasr_ctx* c, const DecView& v, const void* act, int mtj, int row_cap, float* out, int n_rows, bool gated);
template <class Ops, bool AROW, int D> void launch_linear_ops(lasr_ctx* c, const DecView& v, int n_groups, int m_groups, GemmArgs g, int K, const EpiLinear::Args& ea);
void launch_lm_q8(lasr_ctx* c, DecView& v);                                // (integer-valued bf16 operands whatever the model's type: bf16 unit)
// quantise `rows` rows of src -> integer GEMV -> dequantise (+ bias) into out; also builds the int8-served LM's token table at attach
void lm_q_gemv(lasr_ctx* c, const DecView& v, const float* src, int lds, int K, int Kp, const void* Wq, float w_scale, const float* bias, float* out,
               int N, int rows, unsigned short* qa, float* sx);
void launch_table_gemm_f32(lasr_ctx* c, const DecView& v, int n_groups, int m_groups, const GemmArgs& g, const EpiLinear::Args& ea);   // f32 unit
#define LASR_DECL_OPS(X, Ops)                                                                                              \
    X template void launch_predictor_t<Ops>(lasr_ctx*, DecView&, bool, int, int);                                           \
    X template void launch_ppj_t<Ops>(lasr_ctx*, DecView&, bool);                                                           \
    X template void launch_lm_t<Ops>(lasr_ctx*, DecView&, bool, int, int, bool);                                            \
    X template bool launch_pair_ops<Ops>(hipStream_t, int, bool, lasr_ctx::Captured&, lasr_ctx::Captured&);                 \
    X template void launch_logits_ops<Ops>(lasr_ctx*, const DecView&, const void*, int, int, float*, int, bool);                \
    X template void launch_linear_ops<Ops, true, -1>(lasr_ctx*, const DecView&, int, int, GemmArgs, int, const EpiLinear::Args&);  \
    X template void launch_linear_ops<Ops, false, -1>(lasr_ctx*, const DecView&, int, int, GemmArgs, int, const EpiLinear::Args&); \
    X template void launch_linear_ops<Ops, true, 3>(lasr_ctx*, const DecView&, int, int, GemmArgs, int, const EpiLinear::Args&);   \
    X template void launch_linear_ops<Ops, false, 3>(lasr_ctx*, const DecView&, int, int, GemmArgs, int, const EpiLinear::Args&);
LASR_DECL_OPS(extern, OpsF32)
LASR_DECL_OPS(extern, OpsBF16)

// dispatchers on the context's operand type
inline void launch_predictor(lasr_ctx* c, DecView& v, bool beam = false, int l0 = 0, int l1 = -1) {
    if (c->bf) launch_predictor_t<OpsBF16>(c, v, beam, l0, l1);
    else launch_predictor_t<OpsF32>(c, v, beam, l0, l1);
}
inline void launch_ppj(lasr_ctx* c, DecView& v, bool beam = false) {
    if (c->bf) launch_ppj_t<OpsBF16>(c, v, beam);
    else launch_ppj_t<OpsF32>(c, v, beam);
}
inline float* cur_pp(lasr_ctx* c) { return c->pp[par_rd(c->W > 1, c->pred_par)]; }
inline void launch_lm(lasr_ctx* c, DecView& v, bool beam = false, int l0 = 0, int l1 = -1, bool tail = true) {
    if (!c->lm.on) return;
    if (c->lm.q8) { launch_lm_q8(c, v); return; }
    if (c->bf) launch_lm_t<OpsBF16>(c, v, beam, l0, l1, tail);
    else launch_lm_t<OpsF32>(c, v, beam, l0, l1, tail);
}
// Pair launches of the greedy loop with an fp32 / bf16 LM (cont_enqueue): stage `kind` of the predictor / joint chain (0, 1: NBRC
// layers 0, 1; 2: joint half; 3: the next iteration's logits GEMM), recorded in A, with LM layer l (0: through the token table),
// recorded in B.  The kinds the templates name are the ones configs[1] runs (2 x NBRC predictor, decode GEMMs on 8 waves);
// anything else is issued one after the other.
inline void launch_pair(lasr_ctx* c, hipStream_t st, int kind, bool lm_first, lasr_ctx::Captured& A, lasr_ctx::Captured& B) {
    const bool ok = c->bf ? launch_pair_ops<OpsBF16>(st, kind, lm_first, A, B) : launch_pair_ops<OpsF32>(st, kind, lm_first, A, B);
    if (!ok) { replay_captured(st, A); replay_captured(st, B); }
}
// plain linear over element-typed A (fragment-major, or row-major when AROW); f32 row-major output
template <bool AROW, int D>
inline void launch_linear(lasr_ctx* c, const DecView& v, int n_groups, int m_groups, GemmArgs g, int K, const EpiLinear::Args& ea) {
    if (c->bf) launch_linear_ops<OpsBF16, AROW, D>(c, v, n_groups, m_groups, g, K, ea);
    else launch_linear_ops<OpsF32, AROW, D>(c, v, n_groups, m_groups, g, K, ea);
}
inline void launch_logits(lasr_ctx* c, const DecView& v, float* out, int n_rows, bool gated) {
    if (c->bf) launch_logits_ops<OpsBF16>(c, v, c->ja, c->MTj, c->Md, out, n_rows, gated);
    else launch_logits_ops<OpsF32>(c, v, c->ja, c->MTj, c->Md, out, n_rows, gated);
}
// the same GEMM over an activation buffer of the caller's (mtj m-tiles, row_cap rows), every row < n_rows (the lattice blocks)
inline void launch_logits_from(lasr_ctx* c, const DecView& v, const void* act, int mtj, int row_cap, float* out, int n_rows) {
    if (c->bf) launch_logits_ops<OpsBF16>(c, v, act, mtj, row_cap, out, n_rows, false);
    else launch_logits_ops<OpsF32>(c, v, act, mtj, row_cap, out, n_rows, false);
}

// ---------------------------------------------------------------------------- selection family: runtime value -> template argument
// f(std::integral_constant<int, C>{}) for the first candidate C with v <= C, the last candidate if there is none: the one place
// a runtime lookahead / slot count / beam width / flag becomes a compile-time constant (f is a generic lambda that names the
// kernel and writes its argument list once)
template <int C0, int... Cs, class F>
inline void with_const(int v, F&& f) {
    if constexpr (sizeof...(Cs) == 0) f(std::integral_constant<int, C0>{});
    else if (v <= C0) f(std::integral_constant<int, C0>{});
    else with_const<Cs...>(v, f);
}
// k_lm_post / k_beam_fuse with the register slots their vocabulary needs (bit-identical either way, see k_lm_post)
inline bool keep16(int V) {
    static const int force = getenv("LASR_KEEP16") ? atoi(getenv("LASR_KEEP16")) : 0;
    return force || V > 2048;
}
// k_select with the compile-time lookahead bound that covers `la` (1, 2, 4) and 8 or 16 register slots per thread and frame
template <bool PLAIN>
inline void launch_select(hipStream_t st, int rows, const float* logits, int V, int blank, int max_iters, const int* T_row,
                          const DecState& s, int iter_slot, float* out_logp, int* out_arg, int la, int M, bool bias) {
    with_const<8, 16>(V <= 2048 && !s.lmz ? 8 : 16, [&](auto keep) {      // (the LM re-pick keeps the whole row in registers: 16 slots)
        if (bias) {                  // bias_on(c) in the decode loops (lasr_set_bias): the BIAS kernels, one frame per launch (the views say la = 1)
            hipLaunchKernelGGL((k_select<PLAIN, 1, decltype(keep)::value, true>), dim3(rows), dim3(256), 0, st, logits, V, blank, max_iters,
                               T_row, s, iter_slot, out_logp, out_arg, 1, M);
            return;
        }
        with_const<1, 2, 4>(la, [&](auto lat) {
            constexpr int LAT = decltype(lat)::value, KEEP = decltype(keep)::value;
            hipLaunchKernelGGL((k_select<PLAIN, LAT, KEEP>), dim3(rows), dim3(256), 0, st, logits, V, blank, max_iters, T_row, s, iter_slot,
                               out_logp, out_arg, LAT == 1 ? 1 : la, M);
        });
    });
}
inline void launch_lm_post(hipStream_t st, int rows, const float* raw, const int* emit, float* lmz, int* lm_valid, int V, float min_val,
                           const int* parent, int W, const float* lmz_in, const int* valid_in) {
    with_const<8, 16>(keep16(V) ? 16 : 8, [&](auto keep) {
        hipLaunchKernelGGL(k_lm_post<decltype(keep)::value>, dim3(rows), dim3(256), 0, st, raw, emit, lmz, lm_valid, V, min_val, parent, W, lmz_in, valid_in);
    });
}

