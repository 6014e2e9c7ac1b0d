// lasr_fe.hip.h -- host side of the front-end kernels: every launch of k_logmel, k_fe_mel, k_stack_ln and k_ln_tile and the
// argument blocks they take (the race probe's own k_fe_mel loop in lasr_debug_fe_race excepted).
// Engine unit only (lasr_engine.hip), included after lasr_cmd.hip.h.
#pragma once

namespace {

// the constant mel fields (window, twiddles, filterbank): MelArgs and FeMelArgs carry them under the same names
template <class A>
void fill_mel_consts(const lasr_ctx* c, A& m) {
    const lasr_model_desc& d = c->d;
    m.window = c->window; m.tw512 = c->tw512; m.tw1024 = c->tw1024; m.fb_start = c->fb_start; m.fb_off = c->fb_off;
    m.fb_w = c->fb_w; m.n_mels = d.n_mels; m.hop = d.hop;
    m.win_off = (d.n_fft - d.win) / 2; m.win_len = d.win; m.fb_nnz = c->fb_nnz;
}

// window geometry of the streaming front-end (api-server.py:95-102 + TransformTime + StreamPostprocess): first frame picked
int stream_frame0(const lasr_ctx* c, int* nf_out) {
    const lasr_model_desc& d = c->d;
    const long long N = (long long)d.n_window * d.chunk;
    const int T = 1 + (int)(N / d.hop);
    const int a0 = T / 3 + 1;
    if (nf_out) *nf_out = std::min(d.n_stack, T - a0);
    return a0;
}
// can the streaming window feed a model step?  0: yes; 1: it yields fewer than n_stack frames (*nf_out of them); 2: it is not
// longer than the reflect padding
int stream_window_fault(const lasr_ctx* c, int* nf_out = nullptr) {
    int nf = 0;
    (void)stream_frame0(c, &nf);
    if (nf_out) *nf_out = nf;
    if (nf < c->d.n_stack) return 1;
    return (long long)c->d.n_window * c->d.chunk <= c->d.n_fft / 2 ? 2 : 0;
}

// ---------------------------------------------------------------------------- k_logmel
// Streaming, per chunk: the n_stack frames of the current window of every selected row, from the PCM ring into `pend`.  The
// caller states the selection: row_sel, or by value sel_v / age_v / trow_v / trow_out.
void launch_logmel_ring(lasr_ctx* c, MelArgs& m) {
    const lasr_model_desc& d = c->d;
    fill_mel_consts(c, m);
    m.pcm = c->win; m.N = (long long)d.n_window * d.chunk; m.stream = 1; m.ring_head = c->ring_pos; m.chunk = d.chunk;
    m.n_window = d.n_window; m.ring_chunks = c->ring_chunks; m.frame0 = stream_frame0(c, nullptr);
    m.frames_per_row = d.n_stack; m.out = c->pend; m.out_frames = d.n_buffer * d.n_stack;
    hipLaunchKernelGGL(k_logmel, dim3((d.n_stack + 3) / 4, c->M), dim3(256), c->logmel_lds_pad, c->stream, m);
}
// Whole client windows (lasr_step_window): launch row i reads pcm + i * N and writes n_stack frames from frame0 on into `pend`;
// the caller states dst_row_v / sel_v of its n rows.
void launch_logmel_window(lasr_ctx* c, MelArgs& m, const float* pcm, long long N, int frame0, int n) {
    const lasr_model_desc& d = c->d;
    fill_mel_consts(c, m);
    m.pcm = pcm; m.N = N; m.stream = 0; m.by_value = 1; m.frame0 = frame0; m.frames_per_row = d.n_stack;
    m.out = c->pend; m.out_frames = d.n_buffer * d.n_stack; m.chunk = d.chunk; m.n_window = d.n_window;
    hipLaunchKernelGGL(k_logmel, dim3((d.n_stack + 3) / 4, n), dim3(256), 0, c->stream, m);
}
// Offline: T frames per row of `rows` signals, [rows][N] or (row_frames set) ragged with per-row length, offset and frame count.
void launch_logmel_offline(lasr_ctx* c, const float* pcm, long long N, int rows, int T, float* out, const long long* row_N = nullptr,
                           const long long* row_src_off = nullptr, const int* row_frames = nullptr) {
    const lasr_model_desc& d = c->d;
    MelArgs m{};
    fill_mel_consts(c, m);
    m.pcm = pcm; m.N = N; m.stream = 0;
    m.ring_head = nullptr; m.chunk = d.chunk; m.n_window = d.n_window; m.row_sel = nullptr; m.frame0 = 0;
    m.frames_per_row = T; m.out = out; m.out_frames = T;
    m.row_N = row_N; m.row_src_off = row_src_off; m.row_frames = row_frames;
    hipLaunchKernelGGL(k_logmel, dim3((T + 3) / 4, rows), dim3(256), 0, c->stream, m);
}

// ---------------------------------------------------------------------------- k_fe_mel
// What every k_fe_mel launch over the resident PCM ring shares: constants, ring and geometry, the output frames, and "no row
// is pushed, no row runs" (idx -1, tp_pk / age_pk 0).  The caller adds trow_out, its rows and, fused, the sources.
void fill_fe_mel_args(const lasr_ctx* c, FeMelArgs& m, float* pend) {
    const lasr_model_desc& d = c->d;
    fill_mel_consts(c, m);
    m.pcm = c->win; m.ring_pos = c->ring_pos; m.chunk = d.chunk; m.n_window = d.n_window; m.ring_chunks = c->ring_chunks;
    m.frame0 = stream_frame0(c, nullptr);
    m.pend = pend; m.pend_frames = d.n_buffer * d.n_stack;
    for (int r = 0; r < 512; ++r) { m.idx[r] = -1; m.tp_pk[r] = 0; m.age_pk[r] = 0; }
}
// log-mel halves (+ the ring append of the newest chunk when fused) of a model step on 2 x n_buffer x rows workgroups
void launch_fe_mel(lasr_ctx* c, const FeMelArgs& m) {
    // c->fe_lds_pad bytes of unused dynamic LDS: the workgroup then shares its CU with no workgroup of the wide decode tilings
    // (see lasr_ctx::fe_lds_pad)
    hipLaunchKernelGGL((k_fe_mel<10>), dim3(2 * c->d.n_buffer, c->M), dim3(320), c->fe_lds_pad, c->stream, m);
}

// ---------------------------------------------------------------------------- k_stack_ln / k_ln_tile
// (Stack +) LayerNorm of the step's frames into x0; the reference shape (1280 = 128 mels x 10 frames) has a fully static instantiation
void launch_stack_ln(lasr_ctx* c, int mode, const float* src, int src_frames, int frame_step, const long long* row_off,
                     const int* T_row, int Tmax) {
    const lasr_model_desc& d = c->d;
    StackLnArgs a{};
    a.src = src; a.mode = mode; a.src_frames = src_frames; a.frame_step = frame_step; a.row_off = row_off;
    a.T_row = T_row; a.ln_w = c->ln_w; a.ln_b = c->ln_b; a.x0 = c->x0; a.F = d.feat; a.n_mels = d.n_mels;
    a.n_stack = d.n_stack; a.M = c->M; a.MT = c->MT; a.mt_total = c->Tcap * c->MT; a.feats_out = nullptr; a.bf = c->bf; a.Tmax = Tmax;
    const dim3 grid((Tmax + 3) / 4, c->M), block(256);
    if (a.F == 1280 && a.n_stack == 10) hipLaunchKernelGGL((k_stack_ln<20, 10>), grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL((k_stack_ln<32, 0>), grid, block, 0, c->stream, a);
}
// mode 0: log-mel frames [M][src_frames][n_mels], stacked frame t' starts at frame frame_step * t'
void stack_ln_logmel(lasr_ctx* c, const float* logmel, int src_frames, int frame_step, const int* T_row, int Tmax) {
    launch_stack_ln(c, 0, logmel, src_frames, frame_step, nullptr, T_row, Tmax);
}
// mode 1: stacked features, row r frame t' at feats[(row_off[r] + t') * feat]
void stack_ln_feats(lasr_ctx* c, const float* feats, const long long* row_off, const int* T_row, int Tmax) {
    launch_stack_ln(c, 1, feats, 0, 0, row_off, T_row, Tmax);
}

// stack + LayerNorm of the fused streaming step (reference shape: see lasr_ctx::fe_fused) from `pend`, one m-tile per workgroup
void launch_ln_tile(lasr_ctx* c, int Tm) {
    const lasr_model_desc& d = c->d;
    LnTileArgs t{};
    t.pend = c->pend; t.pend_frames = d.n_buffer * d.n_stack; t.T_row = c->T_row_dev; t.ln_w = c->ln_w; t.ln_b = c->ln_b;
    t.x0 = c->x0; t.MT = c->MT; t.mt_total = c->Tcap * c->MT; t.bf = c->bf;
    // store phase of the tile kernel on 4 z-slices (8 -> 32 workgroups; bit-identical): f32 52.5-52.7 -> 52.6-53.3 k, bf16
    // 92.8 -> 95.4 k (profiles/r04/r04_lnz_ab.txt)
    constexpr int ln_z = 4;
    // (with wide decode tilings around: 98 304 B instead of the 82 176 the tile needs -- the same CU exclusion as the log-mel
    //  launch's; this kernel reads its tile back with wide LDS reads as well and has never been seen wrong)
    hipLaunchKernelGGL(k_ln_tile, dim3(c->MT, Tm, ln_z), dim3(1024), c->fe_lds_pad ? 98304 : 16 * 1284 * 4, c->stream, t);
}

}  // namespace
