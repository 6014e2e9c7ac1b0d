// lasr_launch_enc.hip -- the encoder LSTM-cell GEMMs (tilings C and D, plain and layer-wavefront launches, both operand types):
// one of the translation units of liblasr_hip.so (see lasr_launch.hip.h).
#include "lasr_host.hip.h"

// encoder LSTM cell (layer l, step t): x from `xsrc` (fragment-major, K = I); tiling "C"
template <class Ops>
static void launch_enc_cell_t(lasr_ctx* c, hipStream_t st, int l, int t, const void* xsrc, int x_mt_total, void* ydst, int y_mt_total) {
    const Cell& L = c->enc[l];
    const int H = c->d.hidden;
    DecView v{};                   // (launch_gemm reads the stream only)
    v.stream = st;
    GemmArgs g{};
    set_operand(g, 0, xsrc, x_mt_total, t * c->MT, L.I / Ops::KCH, L.WxC);
    set_operand(g, 1, c->enc_h[c->enc_par][l], c->MT, 0, H / Ops::KCH, L.WhC);
    g.M = c->M; g.dbg = c->dbg;
    if (c->cell_prof && c->cp_slots && c->cp_slot_next < lasr_ctx::NCELLSLOT) {
        c->cp_slot_cells[c->cp_slot_next] = 1;
        g.prof = c->cp_slots + (size_t)PROF_W * c->cp_slot_next;
        g.prof_x = g.prof + (size_t)PROF_W * lasr_ctx::NCELLSLOT;
        c->cp_slot_next++;
    }
    using E = EpiLSTM<Ops, false, false, 8>;
    LstmArgs ea{};
    ea.bias = L.bias; ea.flag = c->T_row_dev; ea.t = t; ea.tile_mask = c->tile_masks.empty() ? ~0ull : c->tile_masks[t];
    ea.c = c->enc_c[l]; ea.h_in = c->enc_h[c->enc_par][l]; ea.h_out = c->enc_h[c->enc_par ^ 1][l];
    ea.y = ydst; ea.y_mt_total = y_mt_total; ea.y_mt_off = t * c->MT;
    ea.bn_s = L.bn_s; ea.bn_t = L.bn_t; ea.H = H; ea.M = c->M; ea.MT = c->MT;
    // K split over 4 waves for f32 operands (12.8 us against 17.2 us with 8: fewer requests in flight, half the
    // LDS reduction), 8 waves for bf16 (5.4 us against 6.6 us); LASR_CELL_NW overrides
    const int nw = c->cell_nw ? c->cell_nw : (Ops::BF ? 8 : 4);
    if (c->enc_u12) {
        using E12 = EpiLSTMe<Ops, 12>;
        if (c->cell_nw == 4) launch_gemm<Ops, E12, 4, false, 3, 4>(c, v, H / 12, c->M / 64, g, ea);
        else launch_gemm<Ops, E12, 4, false, 3, NW>(c, v, H / 12, c->M / 64, g, ea);
        return;
    }
    if (nw == 4) launch_gemm<Ops, E, 2, false, 3, 4>(c, v, H / 8, c->M / 32, g, ea);
    else launch_gemm<Ops, E, 2, false>(c, v, H / 8, c->M / 32, g, ea);
}
void launch_enc_cell(lasr_ctx* c, hipStream_t st, int l, int t, const void* xsrc, int x_mt_total, void* ydst, int y_mt_total) {
    if (c->bf) launch_enc_cell_t<OpsBF16>(c, st, l, t, xsrc, x_mt_total, ydst, y_mt_total);
    else launch_enc_cell_t<OpsF32>(c, st, l, t, xsrc, x_mt_total, ydst, y_mt_total);
}

// One anti-diagonal of the encoder's (layer, time) grid in ONE launch: cells (l, d - l), independent of each other.
// par0 = h ping-pong parity before the pass (cell (l, t) reads parity par0 ^ (t & 1)).
template <class Ops>
static void launch_enc_wave_t(lasr_ctx* c, hipStream_t st, const EncCellRef* cells, int n, int par0, int mt_total) {
    using E = EpiLSTM<Ops, false, false, 8>;
    const int H = c->d.hidden;
    MultiArgs<LstmArgs> m{};
    unsigned long long* prof = nullptr;
    if (c->cell_prof && c->cp_slots && c->cp_slot_next < lasr_ctx::NCELLSLOT) {
        c->cp_slot_cells[c->cp_slot_next] = (unsigned char)n;
        prof = c->cp_slots + (size_t)PROF_W * (c->cp_slot_next++);
    }
    for (int i = 0; i < n; ++i) {
        const int l = cells[i].l, t = cells[i].t, par = par0 ^ (t & 1);
        const Cell& L = c->enc[l];
        const void* xsrc = (l == 0) ? c->x0 : c->ybuf[(l - 1) & 1];
        GemmArgs& g = m.g[i];
        set_operand(g, 0, xsrc, mt_total, t * c->MT, L.I / Ops::KCH, L.WxC);
        set_operand(g, 1, c->enc_h[par][l], c->MT, 0, H / Ops::KCH, L.WhC);
        g.M = c->M; g.prof = prof; g.prof_x = prof ? prof + (size_t)PROF_W * lasr_ctx::NCELLSLOT : nullptr; g.prio = c->cell_prio;
        LstmArgs& ea = m.ea[i];
        ea.bias = L.bias; ea.flag = c->T_row_dev; ea.t = t; ea.tile_mask = c->tile_masks.empty() ? ~0ull : c->tile_masks[t];
        ea.c = c->enc_c[l]; ea.h_in = c->enc_h[par][l]; ea.h_out = c->enc_h[par ^ 1][l];
        ea.y = c->ybuf[l & 1]; ea.y_mt_total = mt_total; ea.y_mt_off = t * c->MT;
        ea.bn_s = L.bn_s; ea.bn_t = L.bn_t; ea.H = H; ea.M = c->M; ea.MT = c->MT;
    }
    const int nw = c->cell_nw ? c->cell_nw : (Ops::BF ? 8 : 4);
    if (c->enc_u12) {
        using E12 = EpiLSTMe<Ops, 12>;
        if (c->cell_nw == 4) hipLaunchKernelGGL((k_gemm_multi<Ops, E12, 4, 4, false, 3>), dim3(H / 12, c->M / 64, n), dim3(256), 0, st, m);
        else hipLaunchKernelGGL((k_gemm_multi<Ops, E12, 4, NW, false, 3>), dim3(H / 12, c->M / 64, n), dim3(NW * 64), 0, st, m);
        return;
    }
    const dim3 grid(H / 8, c->M / 32, n);
    if (nw == 4) hipLaunchKernelGGL((k_gemm_multi<Ops, E, 2, 4, false, 3>), grid, dim3(256), 0, st, m);
    else hipLaunchKernelGGL((k_gemm_multi<Ops, E, 2, NW, false, 3>), grid, dim3(NW * 64), 0, st, m);
}
void launch_enc_wave(lasr_ctx* c, hipStream_t st, const EncCellRef* cells, int n, int par0, int mt_total) {
    if (c->bf) launch_enc_wave_t<OpsBF16>(c, st, cells, n, par0, mt_total);
    else launch_enc_wave_t<OpsF32>(c, st, cells, n, par0, mt_total);
}

