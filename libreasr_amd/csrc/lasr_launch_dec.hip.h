// lasr_launch_dec.hip.h -- decode-side GEMM launches (predictor cells, joint half, logits, LM step, pair launches), templates over
// the operand type; included by lasr_launch_dec_f32.hip and lasr_launch_dec_bf16.hip, which instantiate them (LASR_DECL_OPS).
#pragma once

// two recorded launches as ONE (k_gemm2) when they are the kinds the template names; otherwise one after the other
template <class Ops, class EpiA, int MTa, int NWa, bool AROWa, int Da, class EpiB, int MTb, int NWb, bool AROWb, int Db>
static bool launch_pair_t(hipStream_t st, lasr_ctx::Captured& A, lasr_ctx::Captured& B) {
    if (A.fn != (const void*)&k_gemm<Ops, EpiA, MTa, NWa, AROWa, Da> || B.fn != (const void*)&k_gemm<Ops, EpiB, MTb, NWb, AROWb, Db>) return false;
    GemmArgs ga, gb;
    typename EpiA::Args ea; typename EpiB::Args eb;
    memcpy(&ga, A.g, sizeof(ga)); memcpy(&gb, B.g, sizeof(gb));
    memcpy((void*)&ea, A.ea, sizeof(ea)); memcpy((void*)&eb, B.ea, sizeof(eb));
    const int na = (int)(A.gx * A.gy), nb = (int)(B.gx * B.gy);
    hipLaunchKernelGGL((k_gemm2<Ops, EpiA, MTa, NWa, AROWa, Da, EpiB, MTb, NWb, AROWb, Db>), dim3(na + nb), dim3((NWa > NWb ? NWa : NWb) * 64), 0,
                       st, ga, ea, (int)A.gx, na, gb, eb, (int)B.gx);
    A.fn = B.fn = nullptr;
    return true;
}


static void fill_beam_carry(lasr_ctx* c, const DecView& v, BeamCarryArgs& a) {      // (beam only: every buffer from parity p to p ^ 1)
    const int H = c->d.hidden, p = v.pred_par;
    a.emit = c->ds.emit; a.parent = c->b_parent; a.W = c->W; a.Md = c->Md; a.H = H; a.J = c->d.joint; a.Lp = c->d.pred_layers;
    a.bf = c->bf; a.lstm = c->d.pred_cell;
    for (int l = 0; l < a.Lp; ++l) {
        a.h_in[l] = c->pred_h[p][l]; a.h_out[l] = c->pred_h[p ^ 1][l];
        a.y_in[l] = c->pred_y[p][l]; a.y_out[l] = c->pred_y[p ^ 1][l];
        if (a.lstm) { a.c_in[l] = c->pred_c[p][l]; a.c_out[l] = c->pred_c[p ^ 1][l]; }
    }
    a.pp_in = c->pp[p]; a.pp_out = c->pp[p ^ 1];
    a.pe = v.pe; a.t_idx = v.t_idx; a.T_row = v.T_row; a.ja = c->ja; a.MTj = c->MTj; a.ring = v.ring; a.M_enc = c->M;
}
// carry blocks of a launch: Md slot blocks + (LSTM predictor) the cell-state blocks
static int beam_carry_blocks(lasr_ctx* c) {
    return c->Md + (c->d.pred_cell ? ((c->d.hidden + 15) / 16) * ((c->Md + 255) / 256) : 0);
}
// a GEMM launch whose grid carries the round's carry blocks behind its own m-groups (see k_gemm_carry)
template <class Ops, class Epi, int MT, bool AROW, int D = 3, int NWV = NW>
static void launch_gemm_carry(lasr_ctx* c, const DecView& v, int n_groups, int m_groups, const GemmArgs& g0, const typename Epi::Args& ea) {
    GemmArgs g = g0;
    g.prio = gemm_prio(c, v.stream);
    BeamCarryArgs ca{};
    fill_beam_carry(c, v, ca);
    const int extra = (beam_carry_blocks(c) + n_groups - 1) / n_groups;
    hipLaunchKernelGGL((k_gemm_carry<Ops, Epi, MT, NWV, AROW, D>), dim3(n_groups, m_groups + extra), dim3(NWV * 64), 0, v.stream, g, ea, ca, m_groups);
}


// plain linear over element-typed A (fragment-major, or row-major when AROW); f32 row-major output
template <class Ops, bool AROW, int D>
void launch_linear_ops(lasr_ctx* c, const DecView& v, int n_groups, int m_groups, GemmArgs g, int K, const EpiLinear::Args& ea) {
    g.KC[0] = K / Ops::KCH;
    launch_gemm<Ops, EpiLinear, 1, AROW, D>(c, v, n_groups, m_groups, g, ea);
}

// vocabulary projection of the joint for n_rows rows of ja.  m-tiles per workgroup (c->logits_mt): 1 = a 16-row x
// 16-column tile per workgroup (every m-tile re-reads the workgroup's 64 KB of W2 from L2); 2 / 4 = 32 / 64 rows per
// workgroup, W2 fragments fetched once per 2 / 4 m-tiles -- what a lookahead pass (la x M rows) wants
template <class Ops, int MTL>
static void launch_logits_t(lasr_ctx* c, const DecView& v, const GemmArgs& g0, int n_rows, int K, const EpiLinear::Args& ea) {
    GemmArgs g = g0;
    g.KC[0] = K / Ops::KCH;
    const int ng = c->d.vocab / 16, mg = (n_rows + 16 * MTL - 1) / (16 * MTL);
    launch_gemm<Ops, EpiLinear, MTL, false, -1>(c, v, ng, mg, g, ea);
}
// act: the fragment-major activations (mtj m-tiles, row_cap rows): c->ja / c->MTj / c->Md for the decode loops, a block buffer for the lattice
template <class Ops>
void launch_logits_ops(lasr_ctx* c, const DecView& v, const void* act, int mtj, int row_cap, float* out, int n_rows, bool gated) {
    const int J = c->d.joint, V = c->d.vocab;
    GemmArgs g{};
    set_operand(g, 0, act, mtj, 0, 0, c->W2); g.M = row_cap;
    g.dbg = (c->dbg && v.dbg_gate) ? c->dbg + (size_t)4 * 4096 * 16 : nullptr;
    EpiLinear::Args ea{};
    ea.bias = c->b2; ea.out = out; ea.ldo = V; ea.n_rows = n_rows;
    ea.t_idx = gated ? v.t_idx : nullptr; ea.T_row = v.T_row; ea.M = c->M; ea.W = c->W;
    if (n_rows >= 512 && V % 64 == 0) {      // 64 x 64 workgroups for the beam's hundreds of hypothesis rows (round 4: logits 28 -> 20 us)
        GemmArgs g4 = g;
        g4.KC[0] = J / Ops::KCH;
        launch_gemm<typename WideOps<Ops>::type, EpiLinearT<4>, 4, false, -1, 4>(c, v, V / 64, (n_rows + 63) / 64, g4, ea);
        return;
    }
    if (c->logits_mt == 4 || (c->logits_mt == 2 && n_rows >= 512)) { launch_logits_t<Ops, 4>(c, v, g, n_rows, J, ea); return; }
    if (c->logits_mt == 2) { launch_logits_t<Ops, 2>(c, v, g, n_rows, J, ea); return; }
    launch_linear_ops<Ops, false, -1>(c, v, V / 16, (n_rows + 15) / 16, g, J, ea);
}

// a predictor / LM cell in the tiling its row count asks for: 4 units per workgroup, 8 (wide8) or 16 through the wide tilings'
// operand type (wide); TABLE: the x phase is the per-token table (layer 0)
template <class Ops, bool TABLE>
static void launch_lstm_cell(lasr_ctx* c, const DecView& v, bool wide8, bool wide, int H, int mgroups, const GemmArgs& g, const LstmArgs& ea) {
    using OW = typename WideOps<Ops>::type;            // the wide tilings' matrix instruction (see OpsBF16k16)
    if (wide8) launch_gemm<Ops, EpiLSTMw<Ops, TABLE, 2>, MTA, true, -1>(c, v, H / 8, mgroups, g, ea);
    else if (wide) launch_gemm<OW, EpiLSTMw<OW, TABLE>, MTA, true, -1, 4>(c, v, H / 16, mgroups, g, ea);
    else launch_gemm<Ops, EpiLSTM<Ops, true, TABLE, 4>, MTA, true, -1>(c, v, H / 4, mgroups, g, ea);
}
template <class Ops, bool TABLE>
static void launch_nbrc_cell(lasr_ctx* c, const DecView& v, bool wide8, bool wide, int H, int mgroups, const GemmArgs& g, const NbrcArgs& ea) {
    using OW = typename WideOps<Ops>::type;
    if (wide8) launch_gemm<Ops, EpiNBRCw<Ops, TABLE, 2>, MTA, true, -1>(c, v, H / 8, mgroups, g, ea);
    else if (wide) launch_gemm<OW, EpiNBRCw<OW, TABLE>, MTA, true, -1, 4>(c, v, H / 16, mgroups, g, ea);
    else launch_gemm<Ops, EpiNBRC<Ops, TABLE>, MTA, true, -1>(c, v, H / 4, mgroups, g, ea);
}

// one predictor pass (all layers) for rows with emit != 0 (compacted inside the kernels); predictor
// state is row-major [M][H]; toggles v.pred_par
// (l0, l1: layers [l0, l1) of the pass -- the pair launches of cont_enqueue issue a pass layer by layer; the parity flips with the last one)
template <class Ops>
void launch_predictor_t(lasr_ctx* c, DecView& v, bool beam, int l0, int l1) {
    const int H = c->d.hidden;
    if (l1 < 0) l1 = c->d.pred_layers;
    const int mgroups = c->Md / (16 * MTA);
    const int p = v.pred_par, rd = par_rd(beam, p), wr = par_wr(beam, p);   // h: p -> p ^ 1; y, c: rd -> wr
    // many decoder rows (beam 8 x 64+ streams, >= 512 streams): 16-unit workgroups, a quarter of the activation traffic
    // (configs[4], 1024 rows: predictor cells 135 -> ~50 us, whole job +60 %; at 256 rows: bf16 equal, f32 -22 %; at 64: -20 %)
    const bool wide = c->Md >= 512;
    const bool wide8 = c->bf && c->Md >= 256 && c->Md < 512;   // 8 units per workgroup, 8 waves (configs[2]: 6.4 -> 7.2 k in round 2)
    const bool split_carry = beam && beam_carry_on();
    if (split_carry && beam_carry_mode() == 1 && l0 == 0) {      // the slots that are not extended: whole-row copies by their own launch (see k_beam_carry)
        BeamCarryArgs a{};
        fill_beam_carry(c, v, a);
        hipLaunchKernelGGL(k_beam_carry, dim3(std::max(c->Md, ((H + 15) / 16) * ((c->Md + 255) / 256)), 2), dim3(256), 0, v.stream, a);
    }                                                   // (mode 2: the carry rides in launch_ppj's launch of the same pass)
    for (int l = l0; l < l1; ++l) {
        const Cell& L = c->pred[l];
        GemmArgs g{};
        g.skip_idle = split_carry ? 1 : 0;
        if (l > 0) set_operand(g, 0, c->pred_y[wr][l - 1], H, 0, H / Ops::KCH, L.WxA);   // what layer l-1 just wrote
        set_operand(g, 1, c->pred_h[p][l], H, 0, H / Ops::KCH, L.WhA);
        if (beam) { g.parent = c->b_parent; g.beam_w = c->W; }
        g.compact = c->ds.emit; g.M = c->Md; g.dbg = (c->dbg && v.dbg_gate) ? c->dbg + (size_t)(1 + std::min(l, 1)) * 4096 * 16 : nullptr;
        if (c->d.pred_cell == 1) {
            LstmArgs ea{};
            ea.bias = L.bias; ea.tab = L.tab; ea.token = c->ds.token; ea.V = c->d.vocab; ea.flag = c->ds.emit; ea.t = 0;
            ea.c = c->pred_c[wr][l]; ea.h_in = c->pred_h[p][l]; ea.h_out = c->pred_h[p ^ 1][l];
            ea.y = c->pred_y[wr][l]; ea.y_mt_total = 0; ea.y_mt_off = 0;
            ea.bn_s = L.bn_s; ea.bn_t = L.bn_t; ea.H = H; ea.M = c->Md; ea.MT = c->MTd;
            if (beam) { ea.parent = c->b_parent; ea.W = c->W; ea.c_in = c->pred_c[rd][l]; ea.y_in = c->pred_y[rd][l]; }
            ea.no_carry = split_carry ? 1 : 0;
            if (l == 0) launch_lstm_cell<Ops, true>(c, v, wide8, wide, H, mgroups, g, ea);
            else launch_lstm_cell<Ops, false>(c, v, wide8, wide, H, mgroups, g, ea);
        } else {
            NbrcArgs ea{};
            ea.bias = L.bias; ea.rbias = L.rbias; ea.tab = L.tab; ea.token = c->ds.token; ea.V = c->d.vocab; ea.emit = c->ds.emit;
            ea.h_in = c->pred_h[p][l]; ea.h_out = c->pred_h[p ^ 1][l]; ea.y = c->pred_y[wr][l];
            ea.bn_s = L.bn_s; ea.bn_t = L.bn_t; ea.H = H; ea.M = c->Md;
            if (beam) { ea.parent = c->b_parent; ea.W = c->W; ea.y_in = c->pred_y[rd][l]; }
            ea.no_carry = split_carry ? 1 : 0;
            if (l == 0) launch_nbrc_cell<Ops, true>(c, v, wide8, wide, H, mgroups, g, ea);
            else launch_nbrc_cell<Ops, false>(c, v, wide8, wide, H, mgroups, g, ea);
        }
    }
    if (!beam && l1 == c->d.pred_layers) v.pred_par ^= 1;      // beam: launch_ppj (same pass, same parities) toggles
}
// pp (for emitting rows) and the joint activation ja = tanh(pe[t_idx] + pp) for all rows still decoding
template <class Ops>
void launch_ppj_t(lasr_ctx* c, DecView& v, bool beam) {
    const int H = c->d.hidden, J = c->d.joint, L = c->d.pred_layers;
    const int rd = par_rd(beam, v.pred_par), wr = par_wr(beam, v.pred_par);
    GemmArgs g{};
    set_operand(g, 0, c->pred_y[wr][L - 1], H, 0, H / Ops::KCH, c->W1p);      // what the predictor pass just wrote
    g.compact = c->ds.emit; g.M = c->Md; g.dbg = (c->dbg && v.dbg_gate) ? c->dbg + (size_t)3 * 4096 * 16 : nullptr;
    PpjArgs ea{};
    ea.b1 = c->b1; ea.pp = c->pp[wr]; ea.pe = v.pe; ea.t_idx = v.t_idx; ea.T_row = v.T_row; ea.emit = c->ds.emit;
    ea.ja = c->ja; ea.J = J; ea.M = c->Md; ea.MT = c->MTj; ea.ring = v.ring; ea.la = beam ? 1 : v.la;
    if (beam) { ea.parent = c->b_parent; ea.W = c->W; ea.M_enc = c->M; ea.pp_in = c->pp[rd]; }
    if (beam && beam_carry_on()) { ea.no_carry = 1; g.skip_idle = 1; }      // (k_beam_carry, launched with the predictor pass)
    const bool ppj_wide = c->Md >= 512 && c->MTd % 4 == 0;   // 64-row workgroups for many decoder rows (64-column ones measured slower:
                                                             // 19.9 against 14.3 us at 1024 rows, round 4)
    if (beam && beam_carry_mode() == 2) {      // the round's carry as extra workgroups of this launch
        if (ppj_wide) launch_gemm_carry<Ops, EpiPPJ<Ops>, 4, true, -1, 4>(c, v, J / 16, c->MTd / 4, g, ea);
        else launch_gemm_carry<Ops, EpiPPJ<Ops>, 1, true, -1>(c, v, J / 16, c->MTd, g, ea);
    } else
    if (ppj_wide) launch_gemm<Ops, EpiPPJ<Ops>, 4, true, -1, 4>(c, v, J / 16, c->MTd / 4, g, ea);
    else launch_gemm<Ops, EpiPPJ<Ops>, 1, true, -1>(c, v, J / 16, c->MTd, g, ea);
    if (beam) v.pred_par ^= 1;
}
// LMFuser.advance (lm.py:49-53) for the rows with emit != 0: LM step on the token just emitted, then
// log_softmax + standardise + [0] = MIN_VAL into lmz (read by the next k_select of that row)
// (l0, l1: LSTM layers [l0, l1) of the step; the output layer, k_lm_post and the parity flip come with the last one unless tail = false)
template <class Ops>
void launch_lm_t(lasr_ctx* c, DecView& v, bool beam, int l0, int l1, bool tail) {
    lasr_ctx::LM& m = c->lm;
    const int H = m.H, V = c->d.vocab, p = v.lm_par, rd = par_rd(beam, p), wr = par_wr(beam, p);   // h: p -> p ^ 1; the rest: rd -> wr
    const int R = beam ? c->Md : c->M;                   // LM rows: streams, or hypothesis slots (beam: parent-indirected)
    if (l1 < 0) l1 = m.L;
    for (int l = l0; l < l1; ++l) {
        const Cell& L = m.cells[l];
        GemmArgs g{};
        if (l > 0) set_operand(g, 0, m.y[wr][l - 1], H, 0, H / Ops::KCH, L.WxA);
        set_operand(g, 1, m.h[p][l], H, 0, H / Ops::KCH, L.WhA);
        if (beam) { g.parent = c->b_parent; g.beam_w = c->W; }
        g.compact = c->ds.emit; g.M = R;
        LstmArgs ea{};
        ea.bias = L.bias; ea.tab = L.tab; ea.token = c->ds.token; ea.V = c->d.vocab; ea.flag = c->ds.emit; ea.t = 0;
        ea.c = m.cst[wr][l]; ea.h_in = m.h[p][l]; ea.h_out = m.h[p ^ 1][l]; ea.y = m.y[wr][l];
        ea.bn_s = m.ones; ea.bn_t = m.zeros; ea.H = H; ea.M = R; ea.MT = R / 16;
        if (beam) { ea.parent = c->b_parent; ea.W = c->W; ea.c_in = m.cst[rd][l]; ea.y_in = m.y[rd][l]; }
        if (l == 0) launch_lstm_cell<Ops, true>(c, v, false, false, H, R / (16 * MTA), g, ea);      // (always the 4-unit tiling)
        else launch_lstm_cell<Ops, false>(c, v, false, false, H, R / (16 * MTA), g, ea);
    }
    if (l1 < m.L || !tail) return;
    GemmArgs g{};
    set_operand(g, 0, m.y[wr][m.L - 1], H, 0, 0, m.Wout); g.a_rows = R;
    EpiLinear::Args ea{};
    ea.bias = m.bout; ea.out = m.raw; ea.ldo = V; ea.n_rows = R; ea.t_idx = nullptr; ea.T_row = nullptr; ea.M = R;
    launch_linear_ops<Ops, true, -1>(c, v, V / 16, R / 16, g, H, ea);
    launch_lm_post(v.stream, R, m.raw, c->ds.emit, m.lmz[wr], m.valid[wr], V, m.min_val, beam ? c->b_parent : nullptr, beam ? c->W : 1,
                   m.lmz[rd], m.valid[rd]);
    v.lm_par ^= 1;
}
// the pair kinds of one operand type (see launch_pair): false = not a kind the templates name
template <class Ops>
bool launch_pair_ops(hipStream_t st, int kind, bool lm_first, lasr_ctx::Captured& A, lasr_ctx::Captured& B) {
    constexpr int NWD = NW;                         // decode GEMMs: 8 waves with either operand type (round 6: T)
    using LT = EpiLSTM<Ops, true, true, 4>; using LF = EpiLSTM<Ops, true, false, 4>;
    if (kind == 0 && lm_first) return launch_pair_t<Ops, EpiNBRC<Ops, true>, MTA, NWD, true, -1, LT, MTA, NW, true, -1>(st, A, B);
    if (kind == 1 && !lm_first) return launch_pair_t<Ops, EpiNBRC<Ops, false>, MTA, NWD, true, -1, LF, MTA, NW, true, -1>(st, A, B);
    if (kind == 2 && !lm_first) return launch_pair_t<Ops, EpiPPJ<Ops>, 1, NWD, true, -1, LF, MTA, NW, true, -1>(st, A, B);
    if (kind == 3 && !lm_first) return launch_pair_t<Ops, EpiLinear, 2, NWD, false, -1, LF, MTA, NW, true, -1>(st, A, B);
    return false;
}
