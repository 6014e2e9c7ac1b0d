// lasr_engine.hip -- host side of liblasr_hip.so: weight packing, per-stream device state, the
// per-chunk step (front-end -> encoder -> greedy decode loop) and the C ABI of include/lasr.h.
// gfx950 only.  No CPU fallback: every numeric result comes from the kernels in lasr_kernels.hip.h.
#include "lasr_host.hip.h"
#include <sys/prctl.h>
#include <time.h>

// defined further down, used before
static void cont_poll(lasr_ctx* c);       // (pipelined protocol; require_idle consumes a group that was still running)
static int cont_pump(lasr_ctx* c, int G);
static int pump_start(lasr_ctx* c);
static void pump_kick(lasr_ctx* c);
static int flush_lazy(lasr_ctx* c);       // (deferred ring append of lasr_push_submit)
struct PushSrc;
static int submit_impl(lasr_ctx* c, const int* slots, int n, const PushSrc* fused, bool* fused_done);
static int push_submit_impl(lasr_ctx* c, const int* slots, int n, const float* pcm, int flags, long long* ticket, const float* const* rows);
static int overlap_probe_impl(lasr_ctx* c, int delay_us, double* ratio, hipStream_t sa = nullptr, hipStream_t sb = nullptr);
#include "lasr_prefix_tree.hip.h"
#include "lasr_bias.hip.h"            // (ahead of lasr_decode.hip.h: beam_state() views the attached block)
#include "lasr_cmd.hip.h"
#include "lasr_fe.hip.h"
#include "lasr_decode.hip.h"
#include "lasr_lattice_tables.hip.h"
#include "lasr_lattice.hip.h"
#include "lasr_lattice_post.hip.h"
#include "lasr_lattice_tree.hip.h"
#include "lasr_lm_score.hip.h"
#include "lasr_weights.hip.h"


// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

void lasr_default_desc(lasr_model_desc* d) {
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->feat = 1280; d->hidden = 1024; d->enc_layers = 4; d->pred_layers = 2; d->pred_cell = 0;
    d->embed = 512; d->joint = 1024; d->vocab = 2048; d->blank = 0; d->bos = 2;
    d->n_fft = 1024; d->win = 400; d->hop = 160; d->n_mels = 128; d->n_stack = 10; d->stride = 8;
    d->n_buffer = 2; d->n_window = 3; d->chunk = 1280; d->sample_rate = 16000; d->dtype = 0;
    d->max_streams = 64; d->max_iters_offline = 3; d->max_iters_stream = 10; d->beam = 1;
}

size_t lasr_weight_count(const lasr_model_desc* d) {
    if (!valid_desc(d)) return 0;
    const size_t F = d->feat, H = d->hidden, E = d->embed, V = d->vocab, J = d->joint;
    size_t n = 2 * F;
    for (int l = 0; l < d->enc_layers; ++l) {
        const size_t I = l == 0 ? F : H;
        n += 2 * H + 4 * H + 4 * H * I + 4 * H * H + 8 * H;
    }
    n += V * E;
    if (E != H) n += H * E + H;
    for (int l = 0; l < d->pred_layers; ++l) {
        if (d->pred_cell == 1) n += 2 * H + 4 * H + 4 * H * H + 4 * H * H + 8 * H;
        else n += H + 4 * H + 3 * H * H + 3 * H * H + 6 * H;
    }
    n += J * 2 * H + J + V * J + V;
    return n;
}

void lasr_destroy(lasr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->pump_started) {
        { std::lock_guard<std::mutex> lk(c->mu); c->pump_stop.store(true); }
        c->cv_pump.notify_all();
        c->pump_th.join();
    }
    (void)hipStreamSynchronize(c->stream);
    if (c->stream_dec) (void)hipStreamSynchronize(c->stream_dec);
    for (void* p : c->dev_allocs) (void)hipFree(p);
    if (c->cmd_host) (void)hipHostFree(c->cmd_host);
    if (c->res_host) (void)hipHostFree(c->res_host);
    if (c->cont_host) (void)hipHostFree(c->cont_host);
    if (c->align_host) (void)hipHostFree(c->align_host);
    for (auto& e : c->tr_ev) (void)hipEventDestroy(e);
    if (c->tr_base) (void)hipEventDestroy(c->tr_base);
    if (c->trellis_host) (void)hipHostFree(c->trellis_host);
    if (c->rec_host) (void)hipHostFree(c->rec_host);
    if (c->b_rec_ring_host) (void)hipHostFree(c->b_rec_ring_host);
    if (c->push_stage_host) (void)hipHostFree(c->push_stage_host);
    if (c->stream_copy) { (void)hipStreamSynchronize(c->stream_copy); (void)hipStreamDestroy(c->stream_copy); }
    for (auto& e : c->push_copied)
        if (e) (void)hipEventDestroy(e);
    if (!c->pool.th.empty()) {
        { std::lock_guard<std::mutex> lk(c->pool.m); c->pool.stop.store(true); }
        c->pool.cv.notify_all();
        for (auto& t : c->pool.th) t.join();
    }
    for (auto& e : c->push_ev)
        if (e) (void)hipEventDestroy(e);
    for (void* p : c->host_allocs) (void)hipHostFree(p);
    if (c->ev_ok)
        for (auto& e : c->ev) (void)hipEventDestroy(e);
    for (auto& e : c->ev_enc)
        if (e) (void)hipEventDestroy(e);
    if (c->ev_misc) (void)hipEventDestroy(c->ev_misc);
    if (c->lat.ev_ok)
        for (auto& e : c->lat.ev) (void)hipEventDestroy(e);
    if (c->cp_ok)
        for (auto& p : c->cp_ev)
            for (auto& e : p) (void)hipEventDestroy(e);
    drop_decode_graphs(c);
    for (auto& kv : c->mgraphs) (void)hipGraphExecDestroy(kv.second);
    if (c->stream_cap) (void)hipStreamDestroy(c->stream_cap);
    if (c->stream_dec) { (void)hipStreamSynchronize(c->stream_dec); (void)hipStreamDestroy(c->stream_dec); }
    if (c->stream_lm) { (void)hipStreamSynchronize(c->stream_lm); (void)hipStreamDestroy(c->stream_lm); }
    if (c->stream_nb) { (void)hipStreamSynchronize(c->stream_nb); (void)hipStreamDestroy(c->stream_nb); }
    if (c->ev_lm_fork) (void)hipEventDestroy(c->ev_lm_fork);
    if (c->ev_lm_join) (void)hipEventDestroy(c->ev_lm_join);
    delete c;
}

const char* lasr_last_error(const lasr_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

static int create_impl(lasr_ctx* c, const float* weights, size_t n_weights) {
    roctx_init();
    const lasr_model_desc& d = c->d;
    const int F = d.feat, H = d.hidden, E = d.embed, V = d.vocab, J = d.joint;
    c->M = (d.max_streams + 16 * MTA - 1) / (16 * MTA) * (16 * MTA);   // whole "A"-tiling row groups
    c->MT = c->M / 16;
    const int M = c->M;
    c->W = d.beam; c->Md = M * c->W; c->MTd = c->Md / 16;
    const int Md = c->Md;
    c->MTj = std::max(c->Md, lasr_ctx::LA_MAX * M) / 16;
    {   // frames evaluated per row and iteration in the greedy loop (see k_select); measured best on configs[1]
        const char* e = getenv("LASR_LOOKAHEAD");
        if (e) c->la_stream = c->la_offline = c->la_sync = std::min(lasr_ctx::LA_MAX, std::max(1, atoi(e)));
        if (c->W > 1) c->la_stream = c->la_offline = c->la_sync = 1;
        // beam: a model step takes ~5 selection rounds per frame; with short rounds (configs[2]: 77 us) the host round trip per
        // group is worth amortising (4 rounds per group: 13.4-13.8 -> 14.3-14.5 k audio-s/s), with long ones (configs[4]: 1024
        // hypothesis rows x 1536) the rounds launched past the need cost more (10.3 -> 10.0 k): profiles/r03/r03_experiments.txt O
        if (c->W > 1 && (size_t)Md * H <= (size_t)256 * 1024) c->wait_n = 4;
    }
    // groups launched by the pump thread (see pump_main): greedy 2 iterations (f32 52.1-52.6 k at 2, 51.7-52.1 at 3, 51.8 at 4 against
    // 51.8-51.9 without the pump; bf16 96.0 / 93.4 / 93.1 against 92.6: profiles/r04/r04_pump_ab.txt); beam: the group size of
    // round 3's wait path for short rounds (configs[2]: 4; re-checked in round 6: 2 / 4 / 6 / 8 within 1 %), 2 for long ones under
    // the pump (configs[4], 5 / 6 steps in flight: G = 1 25.4 / 27.2 k, 2 26.0 / 27.6 k, 3 25.8 / 27.7 k, 4 25.2 / 26.9 k:
    // profiles/r06/r06_experiments.txt G)
    c->pump_G = c->W > 1 ? std::max(2, c->wait_n) : 2;
    if (getenv("LASR_PUMP_G")) c->pump_G = std::max(1, std::min(8, atoi(getenv("LASR_PUMP_G"))));
    {   // The pump thread spins on its group's flag by design (one host core per context).  When several engine processes share the
        // host (one rank per GPU: the launcher's LOCAL_WORLD_SIZE / WORLD_SIZE say so) it instead sleeps through 75 % of a group's
        // expected duration (moving average) before it polls: 2.04 -> 1.32 host cores per rank in the 8-rank dry run at -1.7 %
        // aggregate, -0.4 % at one rank (profiles/r05/pump_nap).  A single process keeps the spin: the headline takes the rate.
        const char* lw = getenv("LOCAL_WORLD_SIZE") ? getenv("LOCAL_WORLD_SIZE") : getenv("WORLD_SIZE");
        c->pump_nap_pct = (lw && atoi(lw) > 1) ? 75 : 0;
        if (getenv("LASR_PUMP_NAP_PCT")) c->pump_nap_pct = std::max(0, std::min(90, atoi(getenv("LASR_PUMP_NAP_PCT"))));
    }
    if (getenv("LASR_PUSH_LAZY")) c->lazy_on = atoi(getenv("LASR_PUSH_LAZY")) != 0;
    const size_t Mj = (size_t)c->MTj * 16;
    c->G_pred = d.pred_cell ? 4 : 3;
    c->bf = d.dtype == 1; c->kch = c->bf ? 32 : 16; c->esz = c->bf ? 2 : 4;
    Reader rd{weights, n_weights};
    {   // encoder cell tiling D (see EpiLSTMe): where tiling C needs more than one 32 x 32 workgroup per CU and the hidden size divides
        c->enc_u12 = c->bf && H % 12 == 0 && M % 64 == 0 && (H / 12) * (M / 64) >= 256 && (H / 8) * (M / 32) > 256
                     && F % 32 == 0 && (F / 32) % 8 == 0 && (H / 32) % 8 == 0;
        if (getenv("LASR_ENC_U12")) c->enc_u12 = atoi(getenv("LASR_ENC_U12")) != 0 && H % 12 == 0 && M % 64 == 0;
    }
    {
        if (getenv("LASR_NO_GRAPH")) c->use_graphs = false;
        if (getenv("LASR_CELL_NW")) c->cell_nw = atoi(getenv("LASR_CELL_NW")) == 4 ? 4 : 8;
        // encoder pass as a layer wavefront: bf16 cells are load-paced with idle MFMA time, two of them per CU overlap (streaming
        // +4 %, offline +14 %); f32 cells are MFMA-paced, two per CU only contend (-4 %)
        c->enc_wave = c->bf ? 1 : 0;
        // (tiling D -- one 100 KB-LDS workgroup per CU and cell -- has nothing to overlap inside a launch: plain launches.  cfg5,
        //  128 streams, greedy / beam 8: 46.8 / 14.6 k against 45.9 / 14.4 k as a wavefront, profiles/r04/r04_cell_tiling_d.txt)
        if (c->enc_u12) c->enc_wave = 0;
        if (getenv("LASR_ENC_WAVE")) c->enc_wave = atoi(getenv("LASR_ENC_WAVE"));
        if (getenv("LASR_DBG_TIMING")) {
            RC(dalloc0(c, &c->dbg, (size_t)5 * 4096 * 16));
        }
        if (getenv("LASR_DBG_ENCLOG") && atoi(getenv("LASR_DBG_ENCLOG")) > 0) {
            c->enclog_cap = atoi(getenv("LASR_DBG_ENCLOG"));
            RC(dalloc0(c, &c->enclog, (size_t)c->enclog_cap * 32 * c->M));
            if (getenv("LASR_DBG_PENDLOG") && atoi(getenv("LASR_DBG_PENDLOG")) > 0)
                RC(dalloc(c, &c->pendlog, (size_t)c->enclog_cap * c->M * d.n_buffer * d.n_stack * d.n_mels));
        }
    }

    // ---- front-end constants
    {
        std::vector<float> win(d.n_fft, 0.f);
        const int off = (d.n_fft - d.win) / 2;
        for (int i = 0; i < d.win; ++i) win[off + i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / d.win));  // periodic Hann
        RC(upload(c, &c->window, win.data(), win.size()));
        std::vector<float2> t5(512), t10(513);
        for (int i = 0; i < 512; ++i) t5[i] = float2{(float)std::cos(2.0 * M_PI * i / 512), (float)-std::sin(2.0 * M_PI * i / 512)};
        for (int i = 0; i <= 512; ++i) t10[i] = float2{(float)std::cos(2.0 * M_PI * i / 1024), (float)-std::sin(2.0 * M_PI * i / 1024)};
        RC(upload(c, &c->tw512, t5.data(), t5.size()));
        RC(upload(c, &c->tw1024, t10.data(), t10.size()));
        std::vector<int> st, of; std::vector<float> w;
        build_fb(d, st, of, w);
        RC(upload(c, &c->fb_start, st.data(), st.size()));
        RC(upload(c, &c->fb_off, of.data(), of.size()));
        RC(upload(c, &c->fb_w, w.data(), w.size()));
        c->fb_nnz = (int)w.size();
        if (c->fb_nnz > 1536 || d.n_mels > 128) return fail(c, LASR_EINVAL, "mel filterbank too large for the LDS staging (%d weights)", c->fb_nnz);
    }
    // ---- encoder
    {
        const float* lw = rd.take(F); const float* lb = rd.take(F);
        if (!lb) return fail(c, LASR_EINVAL, "weight blob too short");
        RC(upload(c, &c->ln_w, lw, F)); RC(upload(c, &c->ln_b, lb, F));
    }
    c->enc.resize(d.enc_layers);
    for (int l = 0; l < d.enc_layers; ++l) {
        Cell& L = c->enc[l];
        const float* hs = rd.take(2 * H);
        if (!hs) return fail(c, LASR_EINVAL, "weight blob too short");
        RC(upload(c, &L.h0, hs, H)); RC(upload(c, &L.c0, hs + H, H));
        RC(fold_bn(c, rd, H, &L.bn_s, &L.bn_t));
        RC(load_lstm(c, rd, L, l == 0 ? F : H, H, false, nullptr, nullptr));
    }
    // ---- predictor
    const float* embed = rd.take((size_t)V * E);
    if (!embed) return fail(c, LASR_EINVAL, "weight blob too short");
    const float *ffn_w = nullptr, *ffn_b = nullptr;
    if (E != H) {
        ffn_w = rd.take((size_t)H * E); ffn_b = rd.take(H);
        if (!ffn_b) return fail(c, LASR_EINVAL, "weight blob too short");
    }
    c->pred.resize(d.pred_layers);
    std::vector<float> in0_w;      // layer-0 input weights as [G*H][H] (n-major) for the table build
    std::vector<float> in0_b;
    for (int l = 0; l < d.pred_layers; ++l) {
        Cell& L = c->pred[l];
        L.I = H;
        const int S = d.pred_cell ? 2 : 1;
        const float* hs = rd.take((size_t)S * H);
        if (!hs) return fail(c, LASR_EINVAL, "weight blob too short");
        RC(upload(c, &L.h0, hs, H));
        if (S == 2) RC(upload(c, &L.c0, hs + H, H));
        RC(fold_bn(c, rd, H, &L.bn_s, &L.bn_t));
        if (d.pred_cell == 1) {
            RC(load_lstm(c, rd, L, H, H, true, l == 0 ? &in0_w : nullptr, l == 0 ? &in0_b : nullptr));
        } else {
            const float* kx = rd.take((size_t)H * 3 * H); const float* kh = rd.take((size_t)H * 3 * H);
            const float* b = rd.take(3 * H); const float* rb = rd.take(3 * H);
            if (!rb) return fail(c, LASR_EINVAL, "weight blob too short (nbrc)");
            Packed pk;
            // haste layout [K][3H], gates z,r,g; tiling A: tile = 4 units, live column a -> (gate a/4, unit a%4)
            pack_tiles12(pk, c->bf, H / 4, H, [&](int t, int a, int k) { return kx[(size_t)k * 3 * H + (size_t)(a >> 2) * H + 4 * t + (a & 3)]; });
            RC(upload_packed(c, &L.WxA, pk));
            pack_tiles12(pk, c->bf, H / 4, H, [&](int t, int a, int k) { return kh[(size_t)k * 3 * H + (size_t)(a >> 2) * H + 4 * t + (a & 3)]; });
            RC(upload_packed(c, &L.WhA, pk));
            RC(upload(c, &L.bias, b, 3 * H)); RC(upload(c, &L.rbias, rb, 3 * H));
            if (l == 0) {
                in0_w.resize((size_t)3 * H * H);
                for (int n = 0; n < 3 * H; ++n)
                    for (int k = 0; k < H; ++k) in0_w[(size_t)n * H + k] = kx[(size_t)k * 3 * H + n];
                in0_b.assign(b, b + 3 * H);
            }
        }
    }
    // ---- joint
    {
        const float* w0 = rd.take((size_t)J * 2 * H); const float* b0 = rd.take(J);
        const float* w2 = rd.take((size_t)V * J); const float* b2 = rd.take(V);
        if (!b2) return fail(c, LASR_EINVAL, "weight blob too short (joint)");
        if (rd.left != 0) return fail(c, LASR_EINVAL, "weight blob has %zu extra floats", rd.left);
        Packed pk;
        pack_tiles(pk, c->bf, J / 16, H, [&](int t, int ui, int k) { return w0[(size_t)(16 * t + ui) * 2 * H + k]; });          // pred half (cat order pred, enc: models.py:136)
        RC(upload_packed(c, &c->W1p, pk));
        pack_tiles(pk, c->bf, J / 16, H, [&](int t, int ui, int k) { return w0[(size_t)(16 * t + ui) * 2 * H + H + k]; });
        RC(upload_packed(c, &c->W1e, pk));
        pack_tiles(pk, c->bf, V / 16, J, [&](int t, int ui, int k) { return w2[(size_t)(16 * t + ui) * J + k]; });
        RC(upload_packed(c, &c->W2, pk));
        RC(upload(c, &c->b1, b0, J)); RC(upload(c, &c->b2, b2, V));
    }

    // ---- state + work buffers
    for (int p = 0; p < 2; ++p) { c->enc_h[p].resize(d.enc_layers); c->pred_h[p].resize(d.pred_layers); }
    c->enc_c.resize(d.enc_layers); c->pred_c[0].assign(d.pred_layers, nullptr); c->pred_y[0].resize(d.pred_layers);
    for (int l = 0; l < d.enc_layers; ++l) {
        for (int p = 0; p < 2; ++p) { RC(dalloc0(c, (char**)&c->enc_h[p][l], (size_t)M * H * c->esz)); }
        RC(dalloc0(c, &c->enc_c[l], (size_t)M * H));
    }
    for (int l = 0; l < d.pred_layers; ++l) {
        for (int p = 0; p < 2; ++p) { RC(dalloc0(c, (char**)&c->pred_h[p][l], (size_t)Md * H * c->esz)); }
        if (d.pred_cell) RC(dalloc0(c, &c->pred_c[0][l], (size_t)Md * H));
        RC(dalloc0(c, (char**)&c->pred_y[0][l], (size_t)Md * H * c->esz));
    }
    RC(dalloc0(c, &c->pp[0], (size_t)Md * J));
    if (c->W > 1) {       // second parity of every per-hypothesis buffer + the beam bookkeeping
        c->pred_c[1].assign(d.pred_layers, nullptr); c->pred_y[1].assign(d.pred_layers, nullptr);
        for (int l = 0; l < d.pred_layers; ++l) {
            if (d.pred_cell) RC(dalloc0(c, &c->pred_c[1][l], (size_t)Md * H));
            RC(dalloc0(c, (char**)&c->pred_y[1][l], (size_t)Md * H * c->esz));
        }
        RC(dalloc0(c, &c->pp[1], (size_t)Md * J));
        RC(dalloc0(c, &c->b_score, Md)); RC(dalloc0(c, &c->b_alive, Md)); RC(dalloc0(c, &c->b_inB, Md)); RC(dalloc0(c, &c->b_parent, Md));
        c->beams.assign(M, BeamSlot{});
        for (auto& b : c->beams) bh_reset(b.tree, c->W);
        c->b_frames_done.assign(M, 0); c->b_frame_off.assign(M, 0);
        {   // continuous beam loop: the rounds' records, frame marks and step-end scores in pinned host memory (zero-copy stores)
            const size_t n_tre = (size_t)lasr_ctx::TRING * Md, n_fd = (size_t)lasr_ctx::TRING * M;
            const size_t n_es = (size_t)M * lasr_ctx::ENDSLOTS * c->W, n_ea = (size_t)M * lasr_ctx::ENDSLOTS;
            char* blk = nullptr;
            const size_t bytes = sizeof(double) * n_es + sizeof(int) * (n_tre + n_fd + n_ea) + 64;
            HIPCHK(c, hipHostMalloc((void**)&blk, bytes));
            c->host_allocs.push_back(blk);
            memset(blk, 0, bytes);
            void* dp = nullptr;
            HIPCHK(c, hipHostGetDevicePointer(&dp, blk, 0));
            char* dblk = (char*)dp;
            c->b_endsc_host = (double*)blk; c->b_endsc_dev = (double*)dblk;
            size_t off = sizeof(double) * n_es;
            c->b_tre_host = (int*)(blk + off); c->b_tre_dev = (int*)(dblk + off); off += sizeof(int) * n_tre;
            c->b_fdone_host = (int*)(blk + off); c->b_fdone_dev = (int*)(dblk + off); off += sizeof(int) * n_fd;
            c->b_endal_host = (int*)(blk + off); c->b_endal_dev = (int*)(dblk + off);
        }
    }
    RC(dalloc0(c, (char**)&c->ja, Mj * J * c->esz));
    RC(dalloc0(c, (char**)&c->cvt_a, (size_t)M * H * c->esz)); RC(dalloc0(c, (char**)&c->cvt_b, (size_t)M * H * c->esz));
    RC(dalloc0(c, &c->logits, Mj * V));
    RC(dalloc0(c, &c->ds.t_idx, M)); RC(dalloc0(c, &c->ds.iters, M)); RC(dalloc0(c, &c->ds.token, Md));
    RC(dalloc0(c, &c->ds.emit, Md)); RC(dalloc0(c, &c->ds.logp_sum, M));
    RC(dalloc0(c, &c->ds.sum_iters, M)); RC(dalloc0(c, &c->ds.n_ones, M)); RC(dalloc0(c, &c->zero_rows, M));
    RC(dalloc0(c, &c->pub_arrivals, 4));
    RC(dalloc0(c, &c->T_row_fix, M));
    RC(dalloc0(c, &c->T_row_main, M));
    {   // see lasr_ctx::fe_lds_pad.  The kernels' own (static) LDS is asked of the runtime, not assumed
        hipFuncAttributes fa{}, la_{};
        HIPCHK(c, hipFuncGetAttributes(&fa, (const void*)k_fe_mel<10>));
        HIPCHK(c, hipFuncGetAttributes(&la_, (const void*)k_logmel));
        const int lds_cu = 160 * 1024, excl = 98304;             // 98 304 + 65 536 > 160 KB
        const bool wide_decode = c->Md >= 256 || lasr_ctx::LA_MAX * M >= 512;
        c->fe_lds_pad = wide_decode ? std::max(0, excl - (int)fa.sharedSizeBytes) : 0;
        if (getenv("LASR_FE_LDS_PAD")) c->fe_lds_pad = std::max(0, std::min(lds_cu - (int)fa.sharedSizeBytes, atoi(getenv("LASR_FE_LDS_PAD"))));
        c->logmel_lds_pad = c->fe_lds_pad ? std::max(0, excl - (int)la_.sharedSizeBytes) : 0;
        HIPCHK(c, hipFuncSetAttribute((const void*)k_fe_mel<10>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cu - (int)fa.sharedSizeBytes));
        HIPCHK(c, hipFuncSetAttribute((const void*)k_logmel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cu - (int)la_.sharedSizeBytes));
        HIPCHK(c, hipFuncSetAttribute((const void*)k_ln_tile, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
    }
    // measured (profiles/r03/r03_experiments.txt I): host time per model step 66 -> 45 us, but the replay starts its first cell ~6 us
    // later than a plain launch does: f32 -2 % (52.8 against 54.0 k audio-s/s), bf16 +0.5 %  =>  on for bf16, off for f32
    c->main_graph = c->bf != 0;
    if (getenv("LASR_MAIN_GRAPH")) c->main_graph = atoi(getenv("LASR_MAIN_GRAPH")) != 0;
    c->T_row_dev = c->zero_rows;
    for (int q = 0; q < lasr_ctx::NFLY; ++q) {
        RC(dalloc0(c, &c->T_row_ring[q], M));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_enc[q], hipEventDisableTiming));
    }
    // (round 3 measured CU masks for either stream, a high-priority decode stream and per-stream delay probes: every one of them
    //  lost or was a probe -- profiles/r03/r03_experiments.txt B, C; the switches are gone, the patch of the masks is in the history)
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream_dec, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_misc, hipEventDisableTiming));
    {   // The pipelined protocol needs the decode stream and the ctx stream on DIFFERENT hardware queues.  The runtime multiplexes
        // the process's streams onto a few queues (GPU_MAX_HW_QUEUES, 4 by default); in a process that already owns several
        // streams (other contexts, torch, an RCCL communicator) a new stream can land on the ctx stream's queue, and the two
        // streams then run strictly one after the other (the job at 0.73 of its rate: profiles/r04/r04_dist_ab.txt).  So the
        // stream is probed (two 0.3 ms delay kernels, one per stream) and replaced until it overlaps; the rejected ones are kept
        // alive until then, so that the next one is placed elsewhere.  LASR_DEC_STREAM_PICK=0 switches this off.
        static const int pick = getenv("LASR_DEC_STREAM_PICK") ? atoi(getenv("LASR_DEC_STREAM_PICK")) : 1;
        std::vector<hipStream_t> rejected;
        c->dec_stream_attempts = 1;
        for (int attempt = 0; pick && attempt < 8; ++attempt) {
            double ratio = 0.0;
            if (overlap_probe_impl(c, 300, &ratio) != LASR_OK) { (void)hipGetLastError(); break; }
            c->dec_stream_ratio = ratio;
            if (ratio < 1.5) break;
            rejected.push_back(c->stream_dec);
            c->stream_dec = nullptr;
            HIPCHK(c, hipStreamCreateWithFlags(&c->stream_dec, hipStreamNonBlocking));
            c->dec_stream_attempts++;
        }
        for (hipStream_t st : rejected) (void)hipStreamDestroy(st);
        if (getenv("LASR_VERBOSE"))
            fprintf(stderr, "[lasr] decode stream: %d stream(s) tried, overlap probe %.2f\n", c->dec_stream_attempts, c->dec_stream_ratio);
    }
    RC(dalloc0(c, &c->pe_ring, (size_t)lasr_ctx::RING * M * J));
    RC(dalloc0(c, &c->c_cur, M)); RC(dalloc0(c, &c->c_avail, M)); RC(dalloc0(c, &c->c_iters, M)); RC(dalloc0(c, &c->c_target, M));
    RC(dalloc0(c, &c->c_ntotal, M)); RC(dalloc0(c, &c->c_enc_frames, M)); RC(dalloc0(c, &c->c_enc_base, M)); RC(dalloc0(c, &c->c_behind, 64));
    // (c_ntok_end / c_tok_ring live in pinned host memory, written by k_select directly: see below)
    RC(dalloc0(c, &c->c_done, 64));
    RC(dalloc0(c, &c->c_done2, 64));
    RC(dalloc0(c, &c->c_iter, 4));
    HIPCHK(c, hipHostMalloc((void**)&c->cont_host, sizeof(int) * (16 + (size_t)M * (lasr_ctx::NFLY + lasr_ctx::ENDSLOTS + lasr_ctx::TOKRING))));
    memset(c->cont_host, 0, sizeof(int) * (16 + (size_t)M * (lasr_ctx::NFLY + lasr_ctx::ENDSLOTS + lasr_ctx::TOKRING)));
    {   // continuous decode: the token ring and the per-step boundary marks are written by k_select straight
        // into this pinned block (zero-copy stores over PCIe, flushed at kernel end): a finished step needs
        // no result copy at all -- the host reads them as soon as the group's "rows behind" word says 0
        void* dp = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(&dp, c->cont_host, 0));
        c->c_flag_dev = (int*)dp;
        c->c_hcur_dev = (int*)dp + 16;
        c->c_ntok_end = (int*)dp + 16 + (size_t)lasr_ctx::NFLY * M;
        c->c_tok_ring = c->c_ntok_end + (size_t)M * lasr_ctx::ENDSLOTS;
    }
    c->h_frames_sub.assign(M, 0); c->h_fetched.assign(M, 0); c->h_cur_seen.assign(M, 0); c->h_avail.assign(M, 0);
    // (the reference front-end: 10 frames of 128 mels per stacked frame; other shapes take the per-chunk kernels.  So does a window of
    //  so many chunks that the fused kernels' ring of n_window + n_buffer - 1 chunks would have more than 16 slots: the ring position
    //  travels in four bits of FeMelArgs::tp_pk)
    c->fe_fused = M <= 512 && d.n_buffer <= 4 && d.n_stack == 10 && d.n_mels <= 128 && d.feat == 1280 && d.n_window + d.n_buffer - 1 <= 16
                  && !getenv("LASR_FE_LEGACY");
    c->h_ring_pos.assign(M, 0);
    c->ring_chunks = c->fe_fused ? d.n_window + d.n_buffer - 1 : d.n_window;
    c->pend_serial.assign((size_t)M * d.n_buffer, 0); c->pend_mat.assign((size_t)M * d.n_buffer, 0);
    RC(dalloc0(c, &c->win, (size_t)M * c->ring_chunks * d.chunk));
    RC(dalloc0(c, &c->ring_pos, M));
    RC(dalloc0(c, &c->pend, (size_t)M * d.n_buffer * d.n_stack * d.n_mels));

    lasr_ctx::Cmd tmp;
    c->cmd_bytes = cmd_layout(tmp, nullptr, M);
    HIPCHK(c, hipHostMalloc((void**)&c->cmd_host, c->cmd_bytes * NCMD));
    RC(dalloc0(c, &c->cmd_dev, c->cmd_bytes * NCMD));
    RC(ensure_T(c, std::max(d.n_buffer, 4)));

    // ---- predictor input tables (one-time, on device, always exact f32: the table is f32 in both
    //      dtypes):  EF = ffn(embed);  tab = EF * Wx0^T + b
    {
        float* emb_dev = nullptr; float* EF = nullptr;
        RC(upload(c, &emb_dev, embed, (size_t)V * E));
        if (E != H) {
            Packed pk; void* wf = nullptr; float* bfn = nullptr;
            pack_tiles(pk, 0, H / 16, E, [&](int t, int ui, int k) { return ffn_w[(size_t)(16 * t + ui) * E + k]; });
            RC(upload_packed(c, &wf, pk)); RC(upload(c, &bfn, ffn_b, H));
            RC(dalloc(c, &EF, (size_t)V * H));
            GemmArgs g{}; set_operand(g, 0, emb_dev, E, 0, E / 16, wf); g.a_rows = V;
            EpiLinear::Args ea{}; ea.bias = bfn; ea.out = EF; ea.ldo = H; ea.n_rows = V; ea.t_idx = nullptr; ea.T_row = nullptr; ea.M = M;
            launch_table_gemm_f32(c, sync_view(c, c->la_sync), H / 16, V / 16, g, ea);
            HIPCHK(c, hipStreamSynchronize(c->stream));
            dfree(c, wf); dfree(c, bfn);
        } else {
            EF = emb_dev; emb_dev = nullptr;
        }
        const int G = c->G_pred;
        Packed pk; void* wt = nullptr; float* bt = nullptr;
        pack_tiles(pk, 0, G * H / 16, H, [&](int t, int ui, int k) { return in0_w[(size_t)(16 * t + ui) * H + k]; });
        RC(upload_packed(c, &wt, pk)); RC(upload(c, &bt, in0_b.data(), in0_b.size()));
        RC(dalloc(c, &c->pred[0].tab, (size_t)V * G * H));
        GemmArgs g{}; set_operand(g, 0, EF, H, 0, H / 16, wt); g.a_rows = V;
        EpiLinear::Args ea{}; ea.bias = bt; ea.out = c->pred[0].tab; ea.ldo = G * H; ea.n_rows = V; ea.t_idx = nullptr; ea.T_row = nullptr; ea.M = M;
        launch_table_gemm_f32(c, sync_view(c, c->la_sync), G * H / 16, V / 16, g, ea);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        dfree(c, wt); dfree(c, bt); dfree(c, EF); dfree(c, emb_dev);
    }

    c->open_.assign(M, 0); c->n_chunks.assign(M, 0); c->n_pend.assign(M, 0);
    c->results.assign(M, SlotResult{}); c->slot_frames.assign(M, 0);
    c->ev_ok = true;
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) c->ev_ok = false;
    // Greedy decode: what a reset leaves in a row's predictor state -- the learned initial state advanced by one step on BOS, and the
    // joint's predictor half of it (models.py:489) -- does not depend on the row: computed ONCE here, through the same kernels a
    // reset used to launch (row 0), and stored by k_reset_rows from then on.  A reset then costs the decode stream one small launch
    // instead of one + three weight-streaming GEMMs (the servicer's reset rule resets ~2 streams per model step in a replay).
    static const int bos_cache = getenv("LASR_BOS_CACHE") ? atoi(getenv("LASR_BOS_CACHE")) : 1;
    if (bos_cache && c->W == 1) {
        RC(cmd_begin(c));
        c->hc.what[0] = 2;
        RC(cmd_commit(c));
        RC(apply_reset(c, sync_view(c, c->la_sync), true));
        BosArgs b{};
        b.H = H; b.J = J; b.Lp = d.pred_layers; b.M = M; b.lstm = d.pred_cell; b.bf = c->bf;
        c->bos_h.assign(d.pred_layers, nullptr); c->bos_c.assign(d.pred_layers, nullptr);
        for (int l = 0; l < d.pred_layers; ++l) {
            RC(dalloc(c, &c->bos_h[l], H));
            if (d.pred_cell) RC(dalloc(c, &c->bos_c[l], H));
            b.pred_h[l] = c->pred_h[c->pred_par][l]; b.pred_c[l] = d.pred_cell ? c->pred_c[0][l] : nullptr;
            b.bos_h[l] = c->bos_h[l]; b.bos_c[l] = c->bos_c[l];
        }
        RC(dalloc(c, &c->bos_pp, J));
        b.pp = c->pp[0]; b.bos_pp = c->bos_pp;
        hipLaunchKernelGGL(k_bos_capture, dim3(grid1(std::max(H, J))), dim3(256), 0, c->stream, b);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        c->bos_ready = true;
    }
    return LASR_OK;
}

int lasr_create(int device, const lasr_model_desc* d, const float* weights, size_t n_weights, void* hip_stream,
                lasr_ctx** out) {
    if (!out) return LASR_EINVAL;
    *out = nullptr;
    lasr_ctx* c = new lasr_ctx();
    if (!valid_desc(d)) { int rc = fail(c, LASR_EINVAL, "invalid model description"); *out = c; return rc; }
    c->d = *d;
    c->device = device;
    *out = c;   // returned even on failure so that lasr_last_error() works; caller destroys it
    if (!weights || n_weights != lasr_weight_count(d))
        return fail(c, LASR_EINVAL, "weight blob has %zu floats, expected %zu", n_weights, lasr_weight_count(d));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(c, LASR_EHIP, "no HIP device available");
    HIPCHK(c, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(c, LASR_EHIP, "device %d is %s; liblasr_hip is built for gfx950 only", device, prop.gcnArchName);
    c->stream = (hipStream_t)hip_stream;
    return create_impl(c, weights, n_weights);
}

// ---------------------------------------------------------------------------- slots

int lasr_stream_open(lasr_ctx* c, int* slot) {
    if (!c || !slot) return LASR_EINVAL;
    for (int s = 0; s < c->d.max_streams; ++s)
        if (!c->open_[s]) {
            c->open_[s] = 1;
            c->slot_frames[s] = 0;             // the per-slot frame index of the alignment records starts here (no reset restarts it)
            *slot = s;
            return lasr_stream_reset(c, s, 1 | 2 | 4 | 8);
        }
    return fail(c, LASR_EFULL, "all %d stream slots are open", c->d.max_streams);
}

// lasr_stream_reset for n slots: all of them are checked before anything is changed (an error leaves every slot as it was), then
// ONE command block and one set of launches serve them all
static int reset_impl(lasr_ctx* c, const int* slots, int n, int what) {
    if (n <= 0) return LASR_OK;
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= c->d.max_streams || !c->open_[slots[i]]) return fail(c, LASR_ESTATE, "slot %d is not open", slots[i]);
    {
        // With LASR_RESET_IF_DECODED a slot with submitted steps can be reset once the decode loop has FINISHED them for this slot
        // (lasr_peek_slot says so), collected or not: its encoder steps are behind on the ctx stream, its frames are decoded, the tokens sit in the pinned
        // ring until lasr_step_wait hands them out.  Model state only (bits 1 | 2 | 4); greedy decode.
        const bool if_decoded = (what & LASR_RESET_IF_DECODED) != 0;
        what &= ~LASR_RESET_IF_DECODED;
        std::lock_guard<std::mutex> lk(c->mu);
        bool polled = false;
        for (int i = 0; i < n; ++i) {
            const int slot = slots[i];
            bool inflight = false, undecoded = !if_decoded;      // (without the flag: refused whenever a step of the slot is uncollected)
            for (const auto& p : c->pending)
                if (std::find(p.rows.begin(), p.rows.end(), slot) != p.rows.end()) {
                    inflight = true;
                    if (!c->pump_on && !polled) { cont_poll(c); polled = true; }
                    undecoded |= c->h_cur_seen[slot] < p.target[slot];
                }
            if (inflight && (undecoded || (what & 8) || c->W > 1))
                return fail(c, LASR_ESTATE, "slot %d has a submitted step in flight: call lasr_step_wait first", slot);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (what & 8) RC(flush_lazy(c));         // (the PCM ring of these slots starts over)
    for (int i = 0; i < n; ++i) {
        const int slot = slots[i];
        if (what & 8) { c->n_chunks[slot] = 0; c->n_pend[slot] = 0; c->results[slot].clear(); c->results[slot].neg_logp = 0.0; }
        if (what & 2) beam_host_reset(c, slot, (what & 8) != 0);
    }
    if (what & 7) {
        RC(cmd_begin(c));
        for (int i = 0; i < n; ++i) c->hc.what[slots[i]] = what & 7;
        RC(cmd_commit(c));
        std::lock_guard<std::mutex> lk(c->mu);            // (decode-side launches: the pump thread stays out)
        if (c->pending.empty() && !c->group_inflight) {
            RC(order_after_decode_tail(c));          // (the last group's predictor cells may still be running on the decode stream)
            RC(apply_reset(c, sync_view(c, c->la_sync), (what & 2) != 0));
        } else {
            // other streams have steps in flight: the encoder side of the reset is ordered on the main
            // stream, the predictor / LM side (BOS pass) on the decode stream, between two iteration groups
            if (what & 1) RC(apply_reset(c, sync_view(c, c->la_sync), false, 1));
            if (what & 6) {
                // the command block reaches the decode stream by a copy of its own: an event edge from the main stream would make
                // the decode loop wait for everything queued there (up to `steps in flight` encoder passes, ~2 ms at depth 12)
                HIPCHK(c, hipMemcpyAsync((char*)c->dc.T_row, (char*)c->hc.T_row, c->cmd_bytes, hipMemcpyHostToDevice, c->stream_dec));
                DecView v = sync_view(c, c->la_sync);
                v.stream = c->stream_dec;
                RC(apply_reset(c, v, (what & 2) != 0, 2));
            }
        }
    }
    return LASR_OK;
}
int lasr_stream_reset(lasr_ctx* c, int slot, int what) {
    if (!c) return LASR_EINVAL;
    return reset_impl(c, &slot, 1, what);
}
int lasr_stream_reset_many(lasr_ctx* c, const int* slots, int n, int what) {
    if (!c) return LASR_EINVAL;
    RC(check_slots(c, slots, n, true));
    return reset_impl(c, slots, n, what);
}

int lasr_stream_close(lasr_ctx* c, int slot) {
    if (!c) return LASR_EINVAL;
    if (slot < 0 || slot >= c->d.max_streams || !c->open_[slot]) return fail(c, LASR_ESTATE, "slot %d is not open", slot);
    for (const auto& p : c->pending)
        if (std::find(p.rows.begin(), p.rows.end(), slot) != p.rows.end())
            return fail(c, LASR_ESTATE, "slot %d has a submitted step in flight: call lasr_step_wait first", slot);
    c->open_[slot] = 0;
    c->results[slot].clear();
    return LASR_OK;
}

// ---------------------------------------------------------------------------- streaming

// Fused front-end, irregular clients: a slot that is about to be pushed again although it still has a pending frame whose
// window the ring would lose (more than one chunk pushed per lasr_step_* call) gets that frame computed NOW into `pend`
// (the per-chunk log-mel kernel, window selected by its age); the step's k_fe_mel launch then skips it (age 15).
static int materialize_pending(lasr_ctx* c, const int* slots, int n) {
    const lasr_model_desc& d = c->d;
    const int slack = c->ring_chunks - d.n_window;
    for (int j = 0; j < d.n_buffer; ++j) {
        MelArgs m{};
        bool any = false;
        for (int i = 0; i < n; ++i) {
            const int s = slots[i];
            if (j >= c->n_pend[s] || c->pend_mat[(size_t)s * d.n_buffer + j]) continue;
            const int age = c->n_chunks[s] - c->pend_serial[(size_t)s * d.n_buffer + j];
            if (age + 1 <= slack) continue;                      // still in the ring after this push
            if (!any) { for (int r = 0; r < 512; ++r) m.sel_v[r] = -1; any = true; }
            m.sel_v[s] = (short)(j * d.n_stack);
            m.age_v[s] = (unsigned char)age;
            c->pend_mat[(size_t)s * d.n_buffer + j] = 1;
        }
        if (!any) continue;
        RC(flush_lazy(c));                                       // (the kernel below reads the ring)
        m.by_value = 1; m.trow_out = nullptr;
        launch_logmel_ring(c, m);
    }
    return LASR_OK;
}

// ---- client chunks -> PCM ring.  Three kinds of caller memory:
//   device           read by the ring-append (or front-end) kernel in stream order, like any stream-ordered copy;
//   host (default)   pageable OR pinned: copied into the engine's own pinned staging ring before the call returns (the caller's
//                    buffer is free on return), DMA'd from there into a device staging entry on a copy-only stream; the kernel
//                    reads HBM;
//   pinned, no copy  LASR_PUSH_PINNED_NOCOPY: the DMA (or, zero-copy, the kernel) reads the CALLER's pinned buffer after the call
//                    has returned; the buffer must stay untouched until lasr_push_consumed(ticket) says so.
struct PushSrc { const float* src = nullptr; int ev_i = -1; long long ticket = -1; bool dma = false; };

// threaded copy into the staging ring: 328 KB per push at 64 streams is 40 us of one core when the source is cold (pageable
// client buffers), which made the single host thread the limit of the PCIe-inclusive rate.  The calling thread takes parts as
// well, so a helper that wakes up late costs nothing.
static void pool_worker(lasr_ctx::CopyPool* P) {
    long long seen = 0;
    for (;;) {
        // wait for a new job: spin briefly on the hint (pushes come every ~100 us in steady state), then sleep
        for (int spins = 0; P->gen_hint.load(std::memory_order_acquire) == seen && !P->stop.load(std::memory_order_acquire); ++spins) {
            if (spins < 20000) { __builtin_ia32_pause(); continue; }
            std::unique_lock<std::mutex> lk(P->m);
            P->cv.wait_for(lk, std::chrono::milliseconds(50), [&] { return P->gen != seen || P->stop.load(); });
            break;
        }
        if (P->stop.load(std::memory_order_acquire)) return;
        std::unique_lock<std::mutex> lk(P->m);               // parts are claimed under the lock: the job's fields cannot change under a helper
        seen = P->gen;
        while (P->next < P->parts) {
            const int i = P->next++;
            const size_t lo = (size_t)i * P->part_bytes, hi = std::min(P->bytes, lo + P->part_bytes);
            const char* s = P->src; char* d = P->dst;
            const float* const* rows = P->rows; const size_t rb = P->row_bytes;
            lk.unlock();
            if (rows) for (size_t r = lo / rb; r < hi / rb; ++r) memcpy(d + r * rb, rows[r], rb);
            else memcpy(d + lo, s + lo, hi - lo);
            lk.lock();
            if (++P->done == P->parts) P->done_hint.store(P->gen, std::memory_order_release);
        }
    }
}
// rows != nullptr: gather -- row r of the destination (row_bytes each) comes from rows[r]
static void staged_copy(lasr_ctx* c, void* dst, const void* src, size_t bytes, const float* const* rows = nullptr, size_t row_bytes = 0) {
    lasr_ctx::CopyPool& P = c->pool;
    if (!P.init) {
        P.init = true;
        int nth = 2;
        if (getenv("LASR_PUSH_THREADS")) nth = std::max(0, std::min(8, atoi(getenv("LASR_PUSH_THREADS"))));
        for (int i = 0; i < nth; ++i) P.th.emplace_back(pool_worker, &P);
    }
    if (P.th.empty() || bytes < (size_t)(96 << 10)) {
        if (rows) for (size_t r = 0; r < bytes / row_bytes; ++r) memcpy((char*)dst + r * row_bytes, rows[r], row_bytes);
        else memcpy(dst, src, bytes);
        return;
    }
    std::unique_lock<std::mutex> lk(P.m);                    // (the previous job is complete: done == parts, nobody is copying)
    P.src = (const char*)src; P.dst = (char*)dst; P.bytes = bytes; P.rows = rows; P.row_bytes = row_bytes;
    P.part_bytes = ((bytes / (4 * (P.th.size() + 1))) + 4095) & ~(size_t)4095;
    if (rows) P.part_bytes = std::max<size_t>(1, (bytes / row_bytes + 4 * (P.th.size() + 1) - 1) / (4 * (P.th.size() + 1))) * row_bytes;   // whole rows
    P.parts = (int)((bytes + P.part_bytes - 1) / P.part_bytes);
    P.next = 0; P.done = 0;
    const long long g = ++P.gen;
    P.gen_hint.store(g, std::memory_order_release);
    P.cv.notify_all();
    while (P.next < P.parts) {                               // the calling thread takes parts as well
        const int i = P.next++;
        const size_t lo = (size_t)i * P.part_bytes, hi = std::min(bytes, lo + P.part_bytes);
        lk.unlock();
        if (rows) for (size_t r = lo / row_bytes; r < hi / row_bytes; ++r) memcpy((char*)dst + r * row_bytes, rows[r], row_bytes);
        else memcpy((char*)dst + lo, (const char*)src + lo, hi - lo);
        lk.lock();
        if (++P.done == P.parts) P.done_hint.store(g, std::memory_order_release);
    }
    lk.unlock();
    while (P.done_hint.load(std::memory_order_acquire) != g) __builtin_ia32_pause();      // parts still being copied by helpers
}

static int push_prepare(lasr_ctx* c, const int* slots, int n, const float* pcm, int flags, PushSrc& ps, const float* const* rows = nullptr) {
    const int CH = c->d.chunk;
    ps.src = pcm;
    if (!rows && is_device_ptr(pcm)) {
        if (flags & LASR_PUSH_PINNED_NOCOPY) return fail(c, LASR_EINVAL, "LASR_PUSH_PINNED_NOCOPY needs pinned HOST memory");
        return LASR_OK;
    }
    if (!c->push_ev[0])
        for (auto& e : c->push_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // one event per host push: "the kernel that reads this push's source has finished" (staging entry free / ticket consumed)
    ps.ticket = c->push_serial++;
    ps.ev_i = (int)(ps.ticket % lasr_ctx::NSTAGE);
    if (c->push_used[ps.ev_i]) HIPCHK(c, hipEventSynchronize(c->push_ev[ps.ev_i]));       // 64 pushes ago: long done
    // How the bytes cross PCIe: a DMA (hipMemcpyAsync on a copy-only stream) into a device staging entry, issued NOW -- the ctx
    // stream is usually a model step behind the host, so the copy is long done when the front-end / ring-append kernel gets
    // there, and that kernel reads HBM.  (Round 2 let the kernel read the pinned memory itself, 16 bytes per lane over PCIe:
    // ~20 us of the critical stream per 328 KB chunk batch, 43 k against 51 k audio-s/s resident.)
    const float* host_src = nullptr;
    if (flags & LASR_PUSH_PINNED_NOCOPY) {
        const void* pinned = pinned_host_dev_ptr(pcm);
        if (!pinned) return fail(c, LASR_EINVAL, "LASR_PUSH_PINNED_NOCOPY: the buffer is not pinned (device-mapped) host memory");
        ps.src = (const float*)pinned;
        host_src = pcm;
    } else {
        if (!c->push_stage_host) {
            HIPCHK(c, hipHostMalloc((void**)&c->push_stage_host, sizeof(float) * (size_t)lasr_ctx::NSTAGE * c->M * CH));
            void* dp = nullptr;
            HIPCHK(c, hipHostGetDevicePointer(&dp, c->push_stage_host, 0));
            c->push_stage_host_dev = (float*)dp;
        }
        staged_copy(c, c->push_stage_host + (size_t)ps.ev_i * c->M * CH, pcm, sizeof(float) * (size_t)n * CH, rows, sizeof(float) * (size_t)CH);
        ps.src = c->push_stage_host_dev + (size_t)ps.ev_i * c->M * CH;
        host_src = c->push_stage_host + (size_t)ps.ev_i * c->M * CH;
    }
    {
        if (!c->push_stage_dev) {
            RC(dalloc(c, &c->push_stage_dev, (size_t)lasr_ctx::NSTAGE * c->M * CH));
            HIPCHK(c, hipStreamCreateWithFlags(&c->stream_copy, hipStreamNonBlocking));
            for (auto& e : c->push_copied) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        // (the device entry was last read by the kernel of push serial - NSTAGE: waited for above through push_ev)
        float* dst = c->push_stage_dev + (size_t)ps.ev_i * c->M * CH;
        HIPCHK(c, hipMemcpyAsync(dst, host_src, sizeof(float) * (size_t)n * CH, hipMemcpyHostToDevice, c->stream_copy));
        HIPCHK(c, hipEventRecord(c->push_copied[ps.ev_i], c->stream_copy));
        // (the ctx stream waits for the copy where the first kernel that reads `dst` is launched: wait_copied.  A chunk whose append is
        //  deferred is read by the NEXT call's front-end launch, behind that call's own copy on the same in-order copy stream: one
        //  cross-stream wait per model step instead of one per chunk)
        ps.src = dst;
        ps.dma = true;
    }
    return LASR_OK;
}
// the ctx stream waits until the DMA of host push `ev_i` has landed in its device staging entry
static int wait_copied(lasr_ctx* c, const PushSrc& ps) {
    if (ps.dma && ps.ev_i >= 0) HIPCHK(c, hipStreamWaitEvent(c->stream, c->push_copied[ps.ev_i], 0));
    return LASR_OK;
}
// the plain ring append (one launch)
static int push_append_launch(lasr_ctx* c, const int* slots, int n, const PushSrc& ps) {
    const int CH = c->d.chunk;
    RC(wait_copied(c, ps));
    if (c->M <= 512) {      // slot -> staging-row map by value: no command-block copy for a push
        PushIdx pi;
        for (int r = 0; r < 512; ++r) pi.idx[r] = -1;
        for (int i = 0; i < n; ++i) pi.idx[slots[i]] = (short)i;
        hipLaunchKernelGGL(k_push_pcm, dim3(c->M), dim3(256), 0, c->stream, ps.src, (const int*)nullptr, pi, c->win, c->ring_pos, CH, c->ring_chunks);
    } else {
        RC(cmd_begin(c));
        for (int r = 0; r < c->M; ++r) c->hc.src_idx[r] = -1;
        for (int i = 0; i < n; ++i) c->hc.src_idx[slots[i]] = i;
        RC(cmd_commit(c));
        PushIdx pi;
        hipLaunchKernelGGL(k_push_pcm, dim3(c->M), dim3(256), 0, c->stream, ps.src, (const int*)c->dc.src_idx, pi, c->win, c->ring_pos, CH, c->ring_chunks);
    }
    return LASR_OK;
}
// the "source consumed" event of a host push whose append was deferred: recorded behind the launch that finally read it
static int lazy_consumed(lasr_ctx* c) {
    if (c->lazy.ev_i >= 0) {
        HIPCHK(c, hipEventRecord(c->push_ev[c->lazy.ev_i], c->stream));
        c->push_used[c->lazy.ev_i] = true;
        c->push_dma[c->lazy.ev_i] = c->lazy.dma;
    }
    c->lazy = lasr_ctx::LazyPush{};
    return LASR_OK;
}
// a deferred append that the next call cannot take along: the plain append launch, now (see lasr_ctx::LazyPush)
static int flush_lazy(lasr_ctx* c) {
    if (!c->lazy.on) return LASR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    PushSrc ps;
    ps.src = c->lazy.src; ps.ev_i = c->lazy.ev_i; ps.dma = c->lazy.dma;
    const std::vector<int> slots = c->lazy.slots;
    RC(push_append_launch(c, slots.data(), (int)slots.size(), ps));
    c->lazy_flushed++;
    return lazy_consumed(c);
}
// after the launch that reads ps.src: the host mirrors and the "source consumed" event (defer_event: the append was deferred)
static int push_finish(lasr_ctx* c, const int* slots, int n, const PushSrc& ps, long long* ticket, bool counted = false, bool defer_event = false) {
    for (int i = 0; i < n; ++i) {
        if (!counted) c->n_chunks[slots[i]]++;
        c->h_ring_pos[slots[i]] = (c->h_ring_pos[slots[i]] + 1) % c->ring_chunks;
    }
    if (ps.ev_i >= 0) {
        c->push_dma[ps.ev_i] = ps.dma;
        if (!defer_event) {
            HIPCHK(c, hipEventRecord(c->push_ev[ps.ev_i], c->stream));
            c->push_used[ps.ev_i] = true;
        }
    }
    if (ticket) *ticket = ps.ticket;
    return LASR_OK;
}

int lasr_push_pcm_ex(lasr_ctx* c, const int* slots, int n, const float* pcm, int flags, long long* ticket) {
    if (!c) return LASR_EINVAL;
    if (ticket) *ticket = -1;
    RC(check_slots(c, slots, n, true));
    if (n == 0) return LASR_OK;
    if (!pcm) return fail(c, LASR_EINVAL, "pcm is null");
    HIPCHK(c, hipSetDevice(c->device));
    RC(flush_lazy(c));
    if (!c->pending.empty()) RC(cont_pump(c, c->kick_n));      // steps in flight: keep the decode loop fed
    PushSrc ps;
    RC(push_prepare(c, slots, n, pcm, flags, ps));
    tr_mark(c, 1, c->stream);
    if (c->fe_fused) RC(materialize_pending(c, slots, n));      // irregular clients only: see there
    RC(push_append_launch(c, slots, n, ps));
    return push_finish(c, slots, n, ps, ticket);
}
int lasr_push_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm) { return lasr_push_pcm_ex(c, slots, n, pcm, 0, nullptr); }

// 1: the source of the push that returned `ticket` has been read (a LASR_PUSH_PINNED_NOCOPY buffer may be reused); 0: not yet
int lasr_push_consumed(lasr_ctx* c, long long ticket) {
    if (!c) return LASR_EINVAL;
    if (ticket < 0 || ticket >= c->push_serial) return fail(c, LASR_EINVAL, "unknown push ticket %lld", ticket);
    if (c->push_serial - ticket > lasr_ctx::NSTAGE) return 1;        // its event slot has been waited for and reused since
    HIPCHK(c, hipSetDevice(c->device));
    // (DMA path: the source has been read once the copy is done; zero-copy path: once the reading kernel is)
    hipEvent_t ev = c->push_dma[ticket % lasr_ctx::NSTAGE] ? c->push_copied[ticket % lasr_ctx::NSTAGE] : c->push_ev[ticket % lasr_ctx::NSTAGE];
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return 1;
    (void)hipGetLastError();
    if (e == hipErrorNotReady) return 0;
    return fail(c, LASR_EHIP, "hipEventQuery failed: %s", hipGetErrorString(e));
}

// ---- step plumbing shared by the entry points below
// a host source is copied (stream-ordered) into the growable device buffer *buf; a device source is used where it is
static int stage_to_device(lasr_ctx* c, const float* p, size_t n, float** buf, size_t* have, const float** src) {
    *src = p;
    if (is_device_ptr(p)) return LASR_OK;
    RC(ensure_buf(c, buf, have, n));
    HIPCHK(c, hipMemcpyAsync(*buf, p, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    *src = *buf;
    return LASR_OK;
}
// a frame of slot s has been collected; Buffer.encodes: emit when n_buffer collected -- the slot then joins the model step
static void frame_collected(lasr_ctx* c, int s, std::vector<int>& model_rows) {
    if (++c->n_pend[s] != c->d.n_buffer) return;
    c->n_pend[s] = 0;
    c->hc.T_row[s] = c->d.n_buffer;
    model_rows.push_back(s);
}
static void encode_step(lasr_ctx* c, int T, bool pipelined = false) {
    rec(c, 1);
    run_encoder(c, c->stream, pipelined ? c->pe_ring : c->pe_sync, pipelined, T);
    rec(c, 2);
}
// tail of every synchronous step: decode the T encoded frames of `rows`, wait for the ctx stream, collect the statistics
static int decode_and_collect(lasr_ctx* c, int T, int max_iters, bool offline, const std::vector<int>& rows) {
    RC(run_decode(c, T, max_iters, offline, rows));
    rec(c, 3);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    collect_stats(c, T);
    return LASR_OK;
}

// front-end of one client chunk for the listed slots and, for the slots whose frame buffer filled up,
// LayerNorm + encoder + encoder half of the joint -- all enqueued on c->stream, nothing synchronises
// fused (lasr_push_submit): the listed slots' newest chunk is still in the caller's buffer `fused->src` (row i of it belongs to
// slots[i]); the front-end launch appends it to the PCM ring itself.  *fused_done tells the caller whether that happened.
// pipelined: the step belongs to the continuous loop (frame ring, its own frame counters) instead of the synchronous protocol.
static int enqueue_frontend_encoder(lasr_ctx* c, const int* slots, int n, std::vector<int>& model_rows, int& Tm, bool pipelined,
                                    const PushSrc* fused = nullptr, bool* fused_done = nullptr) {
    RoctxRange roctx_range_("lasr frontend+encoder");
    const lasr_model_desc& d = c->d;
    int nf = 0;
    const int fault = stream_window_fault(c, &nf);
    if (fault == 1) return fail(c, LASR_EINVAL, "chunk of %d samples is too short: window yields %d < n_stack frames", d.chunk, nf);
    if (fault == 2) return fail(c, LASR_EINVAL, "window shorter than the reflect padding");
    RC(cmd_begin(c));
    model_rows.clear();
    Tm = d.n_buffer;
    if (c->fe_fused) {
        // nothing runs on a chunk that does not complete a model step: the frame is only noted (chunk serial); the step's
        // single launch works through the last n_buffer windows of every model row
        for (int i = 0; i < n; ++i) {
            const int s = slots[i];
            if (c->n_chunks[s] < d.n_window) continue;          // window not full: the servicer does not call the pipeline
            const size_t q = (size_t)s * d.n_buffer + c->n_pend[s];
            c->pend_serial[q] = c->n_chunks[s]; c->pend_mat[q] = 0;
            frame_collected(c, s, model_rows);
        }
        rec(c, 0);
        if (model_rows.empty()) return LASR_OK;
        RC(ensure_T(c, Tm));
        int* enc_frames = nullptr; int* enc_base = nullptr;
        if (pipelined) { enc_frames = c->c_enc_frames; enc_base = c->c_enc_base; }
        // per (t', row): chunks pushed since the window of stacked frame t' was current; 255: the frame is already in pend
        std::vector<unsigned char> age_v((size_t)d.n_buffer * c->M, 0);
        for (int s : model_rows) {
            for (int j = 0; j < d.n_buffer; ++j) {
                const size_t q = (size_t)s * d.n_buffer + j;
                const int age = c->n_chunks[s] - c->pend_serial[q];
                if (!c->pend_mat[q] && age > c->ring_chunks - d.n_window)
                    return fail(c, LASR_ESTATE, "slot %d: the PCM ring no longer holds the window of pending frame %d", s, j);
                age_v[(size_t)j * c->M + s] = c->pend_mat[q] ? 255 : (unsigned char)age;
            }
        }
        {
            // log-mel halves (+ the ring append of the newest chunk when fused) on 2 x n_buffer x rows workgroups, then stack + LayerNorm
            FeMelArgs m{};
            fill_fe_mel_args(c, m, c->pend);
            int* trow_home = pipelined ? c->T_row_main : nullptr;      // pipelined: one fixed buffer (see commit_T_rows)
            m.trow_out = trow_home ? trow_home : c->dc.T_row; m.enc_frames = enc_frames; m.enc_base = enc_base;
            m.src = fused ? fused->src : nullptr;
            const bool with_lazy = fused && c->lazy.on;          // (push_submit_impl: the deferred chunk belongs to exactly `slots`)
            m.src2 = with_lazy ? c->lazy.src : nullptr;
            for (int r = 0; r < c->M; ++r) m.tp_pk[r] = (unsigned char)(c->h_ring_pos[r] << 4);
            if (fused)
                for (int i = 0; i < n; ++i) {
                    m.idx[slots[i]] = (short)i;
                    // (the host mirror already counts the deferred chunk; the ring on the device does not hold it yet)
                    if (with_lazy) m.tp_pk[slots[i]] = (unsigned char)(((c->h_ring_pos[slots[i]] - 1 + c->ring_chunks) % c->ring_chunks) << 4);
                }
            for (int s : model_rows) {
                m.tp_pk[s] |= (unsigned char)d.n_buffer;
                unsigned pk = 0;
                for (int j = 0; j < d.n_buffer; ++j) { const unsigned a8 = age_v[(size_t)j * c->M + s]; pk |= (a8 == 255 ? 15u : a8) << (4 * j); }
                m.age_pk[s] = (unsigned short)pk;
            }
            if (fused) {
                RC(wait_copied(c, *fused));
                if (with_lazy && c->lazy.dma && !fused->dma) { PushSrc lz; lz.ev_i = c->lazy.ev_i; lz.dma = true; RC(wait_copied(c, lz)); }
            }
            launch_fe_mel(c, m);
            if (fused_done) *fused_done = fused != nullptr;
            if (with_lazy) { c->lazy_taken++; RC(lazy_consumed(c)); }
            RC(commit_T_rows(c, Tm, /*fixed_copy=*/!pipelined, trow_home));    // the continuous loop reads its own frame counters
            launch_ln_tile(c, Tm);
        }
        encode_step(c, Tm, pipelined);
        return LASR_OK;
    }
    bool any_feat = false;
    for (int r = 0; r < c->M; ++r) c->hc.feat_sel[r] = -1;
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        if (c->n_chunks[s] < d.n_window) continue;          // window not full: the servicer does not call the pipeline
        c->hc.feat_sel[s] = c->n_pend[s] * d.n_stack;
        any_feat = true;
        frame_collected(c, s, model_rows);
    }
    // <= 512 rows: the command (frame slot + frames of this model step per row) rides in the log-mel launch's
    // arguments; otherwise it goes through the command ring (one host->device copy)
    const bool by_value = any_feat && c->M <= 512 && d.n_buffer * d.n_stack < 32768 && d.n_buffer < 256;
    if (!by_value) RC(cmd_commit(c));
    rec(c, 0);
    if (any_feat) {
        MelArgs m{};
        m.row_sel = c->dc.feat_sel;
        if (by_value) {
            m.by_value = 1;
            m.trow_out = model_rows.empty() ? nullptr : c->dc.T_row;
            for (int r = 0; r < c->M; ++r) { m.sel_v[r] = (short)c->hc.feat_sel[r]; m.trow_v[r] = (unsigned char)c->hc.T_row[r]; }
        }
        launch_logmel_ring(c, m);
    }
    if (model_rows.empty()) return LASR_OK;
    RC(ensure_T(c, Tm));
    RC(commit_T_rows(c, Tm, /*fixed_copy=*/!pipelined));    // the continuous loop reads its own frame counters
    stack_ln_logmel(c, c->pend, d.n_buffer * d.n_stack, d.n_stack, c->T_row_dev, Tm);
    encode_step(c, Tm, pipelined);
    return LASR_OK;
}

int lasr_step_stream(lasr_ctx* c, const int* slots, int n, int* n_ran) {
    if (!c) return LASR_EINVAL;
    RoctxRange roctx_range_("lasr_step_stream");
    if (n_ran) *n_ran = 0;
    RC(check_slots(c, slots, n, true));
    RC(flush_lazy(c));
    RC(require_idle(c));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int> model_rows;
    int Tm = 0;
    RC(enqueue_frontend_encoder(c, slots, n, model_rows, Tm, false));
    if (model_rows.empty()) {
        HIPCHK(c, hipGetLastError());
        return LASR_OK;
    }
    RC(decode_and_collect(c, Tm, c->d.max_iters_stream, false, model_rows));
    if (n_ran) *n_ran = (int)model_rows.size();
    return LASR_OK;
}

// Pipelined + continuous form of lasr_step_stream.  submit: front-end + encoder of this chunk on the
// main stream (the encoder half of the joint goes to a per-row frame ring).  ONE greedy loop runs on
// stream_dec across chunk boundaries, in groups of iterations (one hipGraph launch each); rows that are
// done early continue with the frames of the later, already encoded steps, so the latency-bound tail of
// a bursty stream overlaps useful work instead of idling 63 rows.  The last k_select of a group stores
// every row's frame cursor and the number of rows that still have encoded frames into pinned memory:
// the host derives "step j is decoded" for EVERY step in flight from the cursors (no per-step target on
// the device), so lasr_step_wait returns at once when the loop is ahead and the host can keep the main
// stream fed `depth` steps deep; groups are launched from push / submit / wait whenever none is in
// flight and frames are waiting (or about to be: a group may start with a stream-side wait for the next
// encoder, so decoding resumes without the host).
// Tokens are attributed to the step whose frames produced them: per-step results are identical to
// lasr_step_stream.
int lasr_step_submit(lasr_ctx* c, const int* slots, int n) {
    if (!c) return LASR_EINVAL;
    RC(check_slots(c, slots, n, true));
    RC(flush_lazy(c));
    return submit_impl(c, slots, n, nullptr, nullptr);
}

// lasr_push_pcm_ex + lasr_step_submit in one call: when the chunk completes a model step, the front-end launch reads the newest
// chunk straight from the source buffer and appends it to the PCM ring itself (one launch less per model step).
int lasr_push_submit(lasr_ctx* c, const int* slots, int n, const float* pcm, int flags, long long* ticket) {
    if (!c) return LASR_EINVAL;
    return push_submit_impl(c, slots, n, pcm, flags, ticket, nullptr);
}
// lasr_push_submit with the chunk of slots[i] at rows[i] (host memory, pageable or pinned; chunk floats each): what a server has
// when every connection's frame sits in its own receive buffer (api-server.py:88-91 tensorizes one message per stream) -- the
// gather into one batch is the copy into the staging ring that a host push makes anyway, not an extra pass on the caller's side.
int lasr_push_submit_rows(lasr_ctx* c, const int* slots, int n, const float* const* rows, long long* ticket) {
    if (!c) return LASR_EINVAL;
    if (n > 0 && !rows) return fail(c, LASR_EINVAL, "rows is null");
    for (int i = 0; i < n; ++i)
        if (!rows[i]) return fail(c, LASR_EINVAL, "rows[%d] is null", i);
    // (the runtime is asked about the first row only: a pointer query costs ~1 us, a server's rows all come from one allocator)
    if (n > 0 && is_device_ptr(rows[0])) return fail(c, LASR_EINVAL, "lasr_push_submit_rows takes host memory (rows[0] is a device pointer)");
    return push_submit_impl(c, slots, n, n > 0 ? rows[0] : nullptr, 0, ticket, rows);
}
static int push_submit_impl(lasr_ctx* c, const int* slots, int n, const float* pcm, int flags, long long* ticket, const float* const* rows) {
    RoctxRange roctx_range_("lasr_push_submit");
    if (ticket) *ticket = -1;
    RC(check_slots(c, slots, n, true));
    if (n == 0) return LASR_OK;
    if (!pcm) return fail(c, LASR_EINVAL, "pcm is null");
    // every check without side effects comes BEFORE the push: LASR_ESTATE / LASR_EINVAL from this call mean nothing was pushed
    // (what can still fail after the push is the HIP runtime: LASR_EHIP, with the chunk pushed)
    if ((int)c->pending.size() + 1 > lasr_max_inflight(c))
        return fail(c, LASR_ESTATE, "%d steps already in flight (limit %d): call lasr_step_wait (nothing was pushed)", (int)c->pending.size(), lasr_max_inflight(c));
    if (c->W > 1 && c->M > 512) return fail(c, LASR_ESTATE, "the pipelined protocol with beam > 1 takes up to 512 stream slots (nothing was pushed)");
    if (stream_window_fault(c))
        return fail(c, LASR_EINVAL, "chunk of %d samples is too short for the streaming window (nothing was pushed)", c->d.chunk);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->pending.empty()) RC(cont_pump(c, c->kick_n));
    PushSrc ps;
    RC(push_prepare(c, slots, n, pcm, flags, ps, rows));
    tr_mark(c, 1, c->stream);
    if (c->fe_fused) RC(materialize_pending(c, slots, n));
    const bool can_fuse = c->fe_fused;
    // a deferred chunk rides in this call's front-end launch only when it belongs to exactly these slots, in this order
    if (c->lazy.on && !(can_fuse && (int)c->lazy.slots.size() == n && std::equal(slots, slots + n, c->lazy.slots.begin()))) RC(flush_lazy(c));
    if (!can_fuse) RC(push_append_launch(c, slots, n, ps));
    for (int i = 0; i < n; ++i) c->n_chunks[slots[i]]++;
    bool fused_done = false;
    int rc = submit_impl(c, slots, n, can_fuse ? &ps : nullptr, &fused_done);
    if (rc) {       // (argument errors were caught above: what can fail here is the runtime)
        (void)flush_lazy(c);
        if (can_fuse && !fused_done) (void)push_append_launch(c, slots, n, ps);
        (void)push_finish(c, slots, n, ps, ticket, true);
        return rc;
    }
    if (can_fuse && !fused_done) {
        // no model step from this chunk.  Its append waits for the next call's front-end launch when the source stays readable
        // until then (the engine's own device staging entry of a host push; a device buffer the caller declared stable);
        // otherwise the plain append launch, now.
        RC(flush_lazy(c));                       // (an older deferred chunk goes first: ring order)
        const bool stable = c->lazy_on && (ps.dma || (!rows && (flags & LASR_PUSH_DEVICE_STABLE) && ps.ev_i < 0));
        if (stable) {
            c->lazy.on = true; c->lazy.src = ps.src; c->lazy.slots.assign(slots, slots + n); c->lazy.ev_i = ps.ev_i; c->lazy.dma = ps.dma;
            return push_finish(c, slots, n, ps, ticket, true, /*defer_event=*/true);
        }
        RC(push_append_launch(c, slots, n, ps));
    }
    return push_finish(c, slots, n, ps, ticket, true);
}

static int submit_impl(lasr_ctx* c, const int* slots, int n, const PushSrc* fused, bool* fused_done) {
    if (c->W > 1 && c->M > 512) return fail(c, LASR_ESTATE, "the pipelined protocol with beam > 1 takes up to 512 stream slots");
    {   // in-flight limit: the event / T_row rings (NFLY) and the per-row rings the decode loop runs through --
        // encoder frames not yet decoded (pe ring), tokens not yet collected (token ring), step boundary marks
        if ((int)c->pending.size() + 1 > lasr_max_inflight(c))
            return fail(c, LASR_ESTATE, "%d steps already in flight (limit %d for n_buffer %d, max_iters_stream %d): call lasr_step_wait",
                        (int)c->pending.size(), lasr_max_inflight(c), c->d.n_buffer, c->d.max_iters_stream);
    }
    HIPCHK(c, hipSetDevice(c->device));
    // keep the decode stream busy while the host enqueues (and the GPU runs) this chunk's encoder (a no-op with the pump thread)
    RC(cont_pump(c, c->kick_n));
    {   // the pump and every graph it can need BEFORE anything of this step is enqueued: a capture / instantiation failure then
        // leaves the host frame targets and the device frame counters in agreement
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->pump_on || c->cgraphs.empty()) RC(pump_start(c));
    }
    const int idx = (int)(c->model_steps % lasr_ctx::NFLY);
    std::vector<int> model_rows;
    int Tm = 0;
    const bool prof = c->profiling;
    c->profiling = false;
    int rc = enqueue_frontend_encoder(c, slots, n, model_rows, Tm, true, fused, fused_done);      // (the joint's encoder half goes into the ring)
    c->profiling = prof;
    if (rc) return rc;
    if (model_rows.empty()) {
        HIPCHK(c, hipGetLastError());
        return LASR_OK;
    }
    if (!c->fe_fused)       // (the fused front-end launch has already advanced the frame counters)
        hipLaunchKernelGGL(k_advance, dim3(grid1(c->M)), dim3(256), 0, c->stream, c->c_enc_frames, (const int*)c->T_row_dev, c->M);
    HIPCHK(c, hipEventRecord(c->ev_enc[idx], c->stream));
    tr_mark(c, 5, c->stream);
    lasr_ctx::PendingStep p;
    p.rows = model_rows; p.Tm = Tm; p.idx = idx; p.admitted = false;
    p.T_row_ptr = c->T_row_dev;             // lives in the command ring until long after this step is collected
    p.serial = c->model_steps;
    p.target.assign(c->M, 0);
    p.frame_off.assign(c->M, 0);
    for (int r : model_rows) {
        // alignment records: the continuous loop's frame cursor is global per row; what the slot has consumed since it was opened
        // is not (no step of the row is in flight while the difference changes: open and the synchronous steps need an idle slot)
        p.frame_off[r] = c->h_frames_sub[r] - c->slot_frames[r];
        c->slot_frames[r] += Tm;
        c->h_frames_sub[r] += Tm; p.target[r] = (int)c->h_frames_sub[r];
    }
    bool kicked = false;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (c->W > 1)       // beam_replay (pump thread, under c->mu) maps the records' global frames to the slot's count with it
            for (int r : p.rows) c->b_frame_off[r] = p.frame_off[r];
        c->pending.push_back(std::move(p));
        if (c->pump_on) { c->kick.fetch_add(1, std::memory_order_release); kicked = true; }     // (under c->mu: see pump_kick)
    }
    c->model_steps++;
    HIPCHK(c, hipGetLastError());
    if (kicked) { c->cv_pump.notify_one(); return LASR_OK; }
    // the enqueue above took tens of microseconds of host time: a group may have finished meanwhile.  If nothing is
    // left to decode the next group is queued behind this step's encoder event (stream-side wait)
    RC(cont_pump(c, c->kick_n));
    return LASR_OK;
}

// ---- the pinned marks and tokens of the continuous greedy loop (k_select stores them, see create_impl): host views
// token count of row r at the end of the model step of P it takes part in = end of that step's tokens in the row's ring
static long long step_end_mark(const lasr_ctx* c, const lasr_ctx::PendingStep& P, int r) {
    const int* h_end = c->cont_host + 16 + (size_t)lasr_ctx::NFLY * c->M;
    const int j = P.target[r] / P.Tm - 1;
    return h_end[(size_t)r * lasr_ctx::ENDSLOTS + (j % lasr_ctx::ENDSLOTS)];
}
// token q (counted since the row was opened) of row r
static int32_t ring_token(const lasr_ctx* c, int r, long long q) {
    const int* h_ring = c->cont_host + 16 + (size_t)(lasr_ctx::NFLY + lasr_ctx::ENDSLOTS) * c->M;
    return h_ring[(size_t)r * lasr_ctx::TOKRING + (q % lasr_ctx::TOKRING)];
}
// its alignment record (alignments on): the same ring position of the two record rings, the frame as the slot counts it
static BeamRec ring_record(const lasr_ctx* c, const lasr_ctx::PendingStep& P, int r, long long q) {
    const size_t at = (size_t)r * lasr_ctx::TOKRING + (q % lasr_ctx::TOKRING);
    const float* h_logp = (const float*)(c->align_host + (size_t)c->M * lasr_ctx::TOKRING);
    return {(int32_t)(c->align_host[at] - P.frame_off[r]), h_logp[at]};
}

// The submitted, uncollected steps of one slot, oldest first (c->mu held, cursors polled): *n_inflight counts them, *n_decoded the
// leading ones the decode loop has finished for the slot; those behind the `skip` oldest hand counts[k] tokens each to `tokens`.
// `who` names the caller in the LASR_EFULL text.
static int peek_walk(lasr_ctx* c, const char* who, int slot, int skip, int32_t* tokens, int cap, int32_t* counts, int cap_steps,
                     int* n_decoded, int* n_inflight) {
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    long long from = c->h_fetched[slot];
    int used = 0, kept = 0;
    bool open_run = true;
    for (const auto& P : c->pending) {
        if (P.target[slot] == 0) continue;                       // the slot is not part of this step
        const int k = (*n_inflight)++;
        if (!open_run || c->h_cur_seen[slot] < P.target[slot]) { open_run = false; continue; }
        const long long end = step_end_mark(c, P, slot);
        if (k >= skip) {
            const int cnt = (int)(end - from);
            if (kept >= cap_steps || used + cnt > cap) return fail(c, LASR_EFULL, "%s: buffers too small", who);
            if (counts) counts[kept] = cnt;
            if (tokens)
                for (long long q = from; q < end; ++q) tokens[used++] = ring_token(c, slot, q);
            kept++;
        }
        from = end;
        (*n_decoded)++;
    }
    return LASR_OK;
}

// Non-consuming look at the submitted, uncollected model steps of one slot (greedy decode): how many there are, how many of
// them (oldest first) the decode loop has finished for this slot, and the tokens of those -- counts[k] tokens for step k,
// concatenated in `tokens`.  lasr_step_wait / lasr_fetch hand the same tokens out later, in step order, as if nobody had looked.
// What it is for: a scheduler that must judge a stream's step before it may submit the stream's next one (the servicer's
// reset rule, api-server.py:131-134) learns the verdict when the row is decoded, not `steps in flight` collections later.
int lasr_peek_slot(lasr_ctx* c, int slot, int32_t* tokens, int cap, int32_t* counts, int cap_steps, int* n_decoded, int* n_inflight) {
    if (!c || !n_decoded || !n_inflight) return LASR_EINVAL;
    *n_decoded = 0; *n_inflight = 0;
    if (slot < 0 || slot >= c->d.max_streams || !c->open_[slot]) return fail(c, LASR_ESTATE, "slot %d is not open", slot);
    if (c->W > 1) return fail(c, LASR_ESTATE, "lasr_peek_slot serves greedy decode (beam = 1)");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->pump_on) cont_poll(c);
    return peek_walk(c, "lasr_peek_slot", slot, 0, tokens, cap, counts, cap_steps, n_decoded, n_inflight);
}

// lasr_peek_slot for n slots in one call: skip[i] oldest steps of slots[i] are of no interest (the caller has seen them);
// row i of tokens [n][cap] / counts [n][cap_steps] holds the decoded steps behind them; n_decoded[i] counts ALL decoded steps
// of the slot (the skipped ones included), n_inflight[i] its submitted steps.
int lasr_peek_many(lasr_ctx* c, const int* slots, int n, const int* skip, int32_t* tokens, int cap, int32_t* counts, int cap_steps,
                   int* n_decoded, int* n_inflight) {
    if (!c || !slots || !n_decoded || !n_inflight || n < 0) return LASR_EINVAL;
    if (c->W > 1) return fail(c, LASR_ESTATE, "lasr_peek_many serves greedy decode (beam = 1)");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->pump_on) cont_poll(c);
    for (int i = 0; i < n; ++i) {
        const int slot = slots[i];
        n_decoded[i] = 0; n_inflight[i] = 0;
        if (slot < 0 || slot >= c->d.max_streams || !c->open_[slot]) return fail(c, LASR_ESTATE, "slot %d is not open", slot);
        RC(peek_walk(c, "lasr_peek_many", slot, skip ? skip[i] : 0, tokens ? tokens + (size_t)i * cap : nullptr, cap,
                     counts ? counts + (size_t)i * cap_steps : nullptr, cap_steps, &n_decoded[i], &n_inflight[i]));
    }
    return LASR_OK;
}

int lasr_step_pending(lasr_ctx* c) { return c ? (int)c->pending.size() : 0; }     // (only the API thread changes the size)

int lasr_max_inflight(const lasr_ctx* c) {
    if (!c) return 0;
    const int Tm = c->d.n_buffer;
    int n = std::min(lasr_ctx::NFLY - 1, lasr_ctx::ENDSLOTS);
    n = std::min(n, lasr_ctx::RING / Tm);
    n = std::min(n, lasr_ctx::TOKRING / (Tm * c->d.max_iters_stream));
    return std::max(n, 0);
}

// ---- the decode loop of the pipelined protocol: groups of G iterations on stream_dec --------------------------------
// Decode-side state (c->pending, h_avail, h_cur_seen, work_left, group_inflight, cont_iters, the predictor / LM parities, the
// beam's host trees) is guarded by c->mu.  Groups are launched by the NATIVE PUMP THREAD (pump_main) while steps are in flight:
// it spins on the pinned flag word and replays the next group's hipGraph the moment the previous one has published its cursors,
// whatever the API thread is doing (its push_submit spends ~60 us per chunk enqueueing the front-end and the encoder cells on
// the main stream; round 3 launched groups only from inside API calls, so a finished group waited for the host: 5 % of the
// decode stream).  The pump never captures and never enqueues an iteration kernel by kernel: its path is event waits, one
// admission kernel with explicit arguments and a graph replay.  The launch helpers would let it (everything they need comes in a
// DecView, nothing from members another thread changes); it stays out because a capture takes milliseconds and may fail, and
// both belong to the API call that can report it: the API thread captures every graph the pump can need (ensure_group_graphs)
// before it hands the first step over.
// Without graphs (LASR_NO_GRAPH, LASR_DBG_TIMING), with more than 512 slots, or with LASR_PUMP=0 there is no pump thread and
// the API calls launch the groups themselves, as in round 3.

// decode-side kernel state of the continuous loop (v: its view)
static void cont_states(lasr_ctx* c, const DecView& v, DecState& s, BeamState& bs) {
    const int M = c->M;
    s = c->ds;
    static_cast<ContRound&>(s) = cont_round_state(c);
    s.t_idx = c->c_cur; s.iters = c->c_iters; s.step_ntok = c->c_ntotal; s.step_tok = c->c_tok_ring; s.tok_cap = lasr_ctx::TOKRING;
    s.step_frame = c->align_on ? c->c_frame_ring : nullptr; s.step_logp = c->align_on ? c->c_logp_ring : nullptr;
    s.host_ntot = c->tr_on ? c->c_hcur_dev + M : nullptr;
    s.ntok_end = c->c_ntok_end; s.step_T = c->d.n_buffer; s.end_slots = lasr_ctx::ENDSLOTS;
    s.dbg = c->dbg ? c->dbg + ((size_t)4 * 4096 + 4095) * 16 : nullptr;
    bs = c->W > 1 ? beam_state(c, v, true, c->d.max_iters_stream) : BeamState{};
}

// the G iterations of a group on v (API thread only, c->mu held): launch-invariant (the flag-ring slot comes from a device
// counter, the last selection kernel publishes the cursors and the "rows with frames left" word), so a group is one hipGraph
// per (G, ping-pong parities).  v ends on the parities the group leaves.
static int cont_enqueue(lasr_ctx* c, DecView& v, int G) {
    const int M = c->M, V = c->d.vocab;
    DecState s; BeamState bs;
    cont_states(c, v, s, bs);
    LmSide side_state;
    LmSide* side = c->lm.on && c->stream_lm != nullptr ? &side_state : nullptr;
    // pair launches (LASR_LM_PAIR, greedy, fp32 / bf16 LM of >= 3 layers beside a 2 x NBRC predictor -- configs[1] with the
    // reference's LM; other shapes keep the LM step in line)
    static const int pair_env = getenv("LASR_LM_PAIR") ? atoi(getenv("LASR_LM_PAIR")) : 1;
    const bool pair = pair_env && !side && c->W == 1 && c->lm.on && !c->lm.q8 && c->d.pred_cell == 0 && c->d.pred_layers == 2 && c->lm.L >= 3;
    bool lm_tail = false;
    for (int q = 0; q < G; ++q) {
        (c->W > 1 ? bs.host_flag : s.host_flag) = (q == G - 1) ? c->c_flag_dev : nullptr;
        if (!pair) {
            decode_iteration(c, v, s, c->W > 1 ? &bs : nullptr, 0, c->d.max_iters_stream, side);
            continue;
        }
        // LM step and predictor / joint chain of an iteration as PAIR launches (k_gemm2): LM layer l beside stage l of the chain;
        // the step's last layers run beside the NEXT iteration's logits GEMM (or alone, at the end of the group)
        lasr_ctx::Captured A, B;
        auto rec = [&](lasr_ctx::Captured& k, auto&& fn) { v.cap = &k; fn(); v.cap = nullptr; };
        if (lm_tail) {
            rec(A, [&] { launch_logits(c, v, c->logits, v.la * M, true); });
            rec(B, [&] { launch_lm(c, v, false, 3, 4, false); });
            launch_pair(c, v.stream, 3, false, A, B);
            launch_lm(c, v, false, 4, -1);                       // deeper layers (if any), output layer, k_lm_post, parity
            lm_tail = false;
        } else {
            launch_logits(c, v, c->logits, v.la * M, true);
        }
        launch_select<false>(v.stream, M, c->logits, V, c->d.blank, c->d.max_iters_stream, v.T_row, s, 0, nullptr, nullptr, v.la, M, bias_on(c));
        rec(A, [&] { launch_predictor(c, v, false, 0, 1); });
        rec(B, [&] { launch_lm(c, v, false, 0, 1, false); });
        launch_pair(c, v.stream, 0, true, A, B);
        rec(A, [&] { launch_predictor(c, v, false, 1, 2); });
        rec(B, [&] { launch_lm(c, v, false, 1, 2, false); });
        launch_pair(c, v.stream, 1, false, A, B);
        rec(A, [&] { launch_ppj(c, v); });
        rec(B, [&] { launch_lm(c, v, false, 2, 3, false); });
        launch_pair(c, v.stream, 2, false, A, B);
        if (c->lm.L > 3) lm_tail = true;
        else launch_lm(c, v, false, 3, -1);                      // (3 layers: only the output layer is left)
        if (q == G - 1 && lm_tail) { launch_lm(c, v, false, 3, -1); lm_tail = false; }
    }
    if (side) side->join(c, v);
    return LASR_OK;
}

// the group graph for (G, current parities): captured on first use (API thread, c->mu held)
static int cont_group_graph(lasr_ctx* c, int G, int pred_par, int lm_par, hipGraphExec_t* out) {
    const auto key = std::make_tuple(G, pred_par, lm_par);
    auto it = c->cgraphs.find(key);
    if (it == c->cgraphs.end()) {
        DecView v = cont_view(c);                      // the capture only records: the context's parities advance at launch
        v.pred_par = pred_par; v.lm_par = lm_par;
        hipGraphExec_t ex = nullptr;
        RC(capture_graph(c, v.stream, [&] { return cont_enqueue(c, v, G); }, &ex));
        it = c->cgraphs.emplace(key, ex).first;
    }
    *out = it->second;
    return LASR_OK;
}
// every graph the pump thread can need (it never captures): G = pump_G at each parity the loop can be in
static int ensure_group_graphs(lasr_ctx* c) {
    hipGraphExec_t ex;
    for (int pp = 0; pp < 2; ++pp)
        for (int lp = 0; lp < (c->lm.on ? 2 : 1); ++lp)
            RC(cont_group_graph(c, c->pump_G, pp, c->lm.on ? lp : c->lm.par, &ex));
    return LASR_OK;
}

// One group of G iterations on stream_dec for whatever rows have frames to decode; its last selection kernel publishes the
// rows' frame cursors and the "rows with frames left" word to pinned memory.  Does not wait.  c->mu held.  from_pump: called
// by the pump thread -- explicit stream / buffers only, never a capture (rc 1 = the graph is missing, nothing was launched)
static int cont_launch_group(lasr_ctx* c, int G, bool from_pump = false) {
    const int M = c->M, J = c->d.joint;
    hipStream_t sd = c->stream_dec;
    float* pe = c->pe_ring;
    const int R = lasr_ctx::RING, la = c->W > 1 ? 1 : c->la_stream;
    int* flag = c->cont_host;
    hipGraphExec_t ex = nullptr;
    const bool graphs = c->use_graphs && !c->dbg;
    if (graphs) {
        if (from_pump) {
            auto it = c->cgraphs.find(std::make_tuple(G, c->pred_par, c->lm.par));
            if (it == c->cgraphs.end()) return 1;
            ex = it->second;
        } else {
            RC(cont_group_graph(c, G, c->pred_par, c->lm.par, &ex));
        }
    } else if (from_pump) {
        return 1;
    }
    // admit encoded steps in order.  While rows still have frames to decode only steps whose encoder has finished are
    // admitted (the loop must not stall behind an encoder); when nothing is left the first one is admitted unconditionally:
    // the decode stream then waits for that encoder on the GPU and resumes by itself
    bool admitted_any = false;
    tr_mark(c, 10, sd);
    const bool by_value = M <= 512;
    for (auto& q : c->pending) {
        if (q.admitted) continue;
        const bool must = c->work_left == 0 && !admitted_any;
        if (!must && hipEventQuery(c->ev_enc[q.idx]) != hipSuccess) { (void)hipGetLastError(); break; }
        HIPCHK(c, hipStreamWaitEvent(sd, c->ev_enc[q.idx], 0));
        if (by_value) { for (int r : q.rows) c->h_avail[r] = q.target[r]; }
        else hipLaunchKernelGGL(k_advance, dim3(grid1(M)), dim3(256), 0, sd, c->c_avail, q.T_row_ptr, M);
        q.admitted = true;
        admitted_any = true;
    }
    if (admitted_any && c->W > 1) {     // beam: every hypothesis slot of the streams that have a frame to decode
        AvailV av;
        for (int r = 0; r < 512; ++r) av.v[r] = r < M ? c->h_avail[r] : 0;
        hipLaunchKernelGGL(k_ja_admit_beam, dim3(grid1((size_t)c->Md * J)), dim3(256), 0, sd, (const float*)pe, (const float*)cur_pp(c),
                           (const int*)c->c_cur, av, c->c_avail, c->ja, J, c->Md, c->W, M, c->MTj, R, c->bf);
    } else
    if (admitted_any) {  // rows that were idle need their joint activation for the new frames
        if (by_value) {
            AvailV av;
            for (int r = 0; r < 512; ++r) av.v[r] = r < M ? c->h_avail[r] : 0;
            hipLaunchKernelGGL(k_ja_admit, dim3(grid1((size_t)M * J)), dim3(256), 0, sd, (const float*)pe, (const float*)c->pp[0],
                               (const int*)c->c_cur, av, c->c_avail, c->ja, J, M, c->MTj, R, c->bf, la);
        } else {
            hipLaunchKernelGGL(k_ja, dim3(grid1((size_t)M * J)), dim3(256), 0, sd, pe, c->pp[0], c->c_cur,
                               c->c_avail, c->ja, J, M, c->MTj, R, c->bf, 1, M, la);
        }
    }
    tr_mark(c, 11 + 100 * G + (admitted_any ? 1000 : 0), sd);
    __atomic_store_n(flag, -1, __ATOMIC_RELEASE);      // before the launch that will overwrite it
    if (graphs) {
        { RoctxRange roctx_range_("lasr decode group"); HIPCHK(c, hipGraphLaunch(ex, sd)); }
        if (G & 1) { c->pred_par ^= 1; if (c->lm.on) c->lm.par ^= 1; }
    } else {
        DecView v = cont_view(c);
        RC(cont_enqueue(c, v, G));
        c->pred_par = v.pred_par; c->lm.par = v.lm_par;
    }
    tr_mark(c, 12, sd);
    c->tr_last_G = G;
    c->cont_iters += G;
    c->group_inflight = true;
    c->dec_tail_open = true;
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

// continuous beam loop: replay the rounds of the groups that have completed into the streams' hypothesis trees; a stream that
// finished a model step in a round gets that step's result (best alive slot by the scores the kernel stored for the step)
static void beam_replay(lasr_ctx* c) {
    const int W = c->W, Md = c->Md, M = c->M, Tm = c->d.n_buffer;
    const bool recs = c->beam_rec_on;
    for (long long it = c->b_rounds_replayed; it < c->cont_iters; ++it) {
        const int slot = (int)(it % lasr_ctx::TRING);
        const int* tre = c->b_tre_host + (size_t)slot * Md;
        const BeamRec* rr = recs ? c->b_rec_ring_host + (size_t)slot * Md : nullptr;
        const int* fd = c->b_fdone_host + (size_t)slot * M;
        for (int q = 0; q < c->d.max_streams; ++q) {
            const int* e = tre + (size_t)q * W;
            if (e[0] == -1) continue;                          // stream idle in this round
            BeamSlot& B = c->beams[q];
            bh_apply(B.tree, e, W, rr ? rr + (size_t)q * W : nullptr, -c->b_frame_off[q]);   // (global frame cursor -> the slot's own count)
            if (!fd[q]) continue;
            const long long frames = ++c->b_frames_done[q];
            if (frames % Tm) continue;
            const int es = (int)((frames / Tm - 1) % lasr_ctx::ENDSLOTS);
            const double* sc = c->b_endsc_host + ((size_t)q * lasr_ctx::ENDSLOTS + es) * W;
            const int am = c->b_endal_host[(size_t)q * lasr_ctx::ENDSLOTS + es];
            B.steps.push_back(B.build(sc, (unsigned)am, recs));
        }
    }
    c->b_rounds_replayed = c->cont_iters;
}

// non-blocking: if the in-flight group has finished, consume its flag and snapshot the rows' frame cursors
// (nothing writes them again until the next group is launched).  c->mu held.
static void cont_poll(lasr_ctx* c) {
    if (!c->group_inflight) return;
    const int v = __atomic_load_n((volatile int*)c->cont_host, __ATOMIC_ACQUIRE);
    if (v == -1) return;
    c->group_inflight = false;
    c->work_left = v;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    memcpy(c->h_cur_seen.data(), c->cont_host + 16, sizeof(int) * c->M);
    if (c->W > 1) beam_replay(c);
    if (c->tr_on) {     // iterations this group needed = most decisions (frames + tokens) any row made in it; rows that moved
        const int* nt = c->cont_host + 16 + c->M;
        int need = 0, rows = 0;
        for (int r = 0; r < c->M; ++r) {
            const int dlt = (c->h_cur_seen[r] - c->tr_prev_cur[r]) + (nt[r] - c->tr_prev_ntot[r]);
            need = std::max(need, dlt);
            rows += dlt > 0;
            c->tr_prev_cur[r] = c->h_cur_seen[r]; c->tr_prev_ntot[r] = nt[r];
        }
        tr_note(c, 20, need * 1000.0 + c->tr_last_G * 100.0 + v + rows / 1000.0);
    }
    c->progress.fetch_add(1, std::memory_order_release);
    c->cv_prog.notify_all();           // (c->mu held: a lasr_step_wait that sleeps on the counter checks it under the same mutex)
}

// non-blocking: launch the next group of G iterations if none is in flight and frames are waiting (or the encoder
// of a submitted step is still to be admitted).  c->mu held.
static int cont_pump_locked(lasr_ctx* c, int G, bool from_pump = false) {
    cont_poll(c);
    if (c->group_inflight || c->pending.empty()) return LASR_OK;
    bool unadmitted = false;
    for (const auto& q : c->pending) unadmitted |= !q.admitted;
    if (c->work_left == 0 && !unadmitted) return LASR_OK;        // everything encoded so far is decoded
    return cont_launch_group(c, G, from_pump);
}
// API-thread form: a no-op while the pump thread owns the launches
static int cont_pump(lasr_ctx* c, int G) {
    if (c->pump_on) return LASR_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    return cont_pump_locked(c, G);
}

// ---- the pump thread
static void pump_main(lasr_ctx* c) {
    (void)hipSetDevice(c->device);
    tl_err_sink = &c->pump_err;             // fail() on this thread writes the pump's own buffer (under c->mu), never c->err
    long long seen_kick = -1;
    // LASR_PUMP_NAP_PCT > 0: the pump sleeps through that share of a group's expected duration (moving average of the last groups)
    // before it starts to spin on the group's flag -- a group of 2 iterations runs ~170 us, and polling it from the first
    // microsecond keeps one host core per context at 100 %.  The timer slack of this thread goes down to 1 us for that.
    double ema_us = 0.0;
    if (c->pump_nap_pct > 0) (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    for (;;) {
        bool inflight = false, idle = false;
        {
            std::unique_lock<std::mutex> lk(c->mu);
            if (c->pump_stop.load(std::memory_order_acquire)) return;
            if (c->pump_on && c->pump_rc == 0) {
                const int rc = cont_pump_locked(c, c->pump_G, true);
                if (rc < 0) { c->pump_rc = rc; c->progress.fetch_add(1, std::memory_order_release); c->cv_prog.notify_all(); }
                // (rc 1: the graph for this parity is missing -- the API thread captures it with its next call)
            }
            inflight = c->group_inflight;
            idle = !inflight;
        }
        if (inflight) {
            // the group's flag: a plain spin (the pump is the only thing this thread does); a submit in the meantime changes nothing
            // before the group has finished
            const auto t_launch = std::chrono::steady_clock::now();
            if (c->pump_nap_pct > 0 && ema_us > 20.0) {
                const long ns = (long)(ema_us * 10.0 * c->pump_nap_pct);        // us * 1000 * pct / 100
                struct timespec ts{0, std::min(ns, 2000000L)};
                (void)nanosleep(&ts, nullptr);
            }
            unsigned long long spins = 0;
            while (__atomic_load_n((volatile int*)c->cont_host, __ATOMIC_ACQUIRE) == -1 && !c->pump_stop.load(std::memory_order_relaxed)) {
                __builtin_ia32_pause();
                if (++spins > (1ull << 31)) break;
            }
            if (c->pump_nap_pct > 0) {
                // (a group found finished right after the nap may have overslept: its duration is an upper bound, and the
                //  average then shrinks the next nap only through the shorter groups -- so count such a group at 80 %)
                double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_launch).count();
                if (spins < 4) us *= 0.8;
                ema_us = ema_us == 0.0 ? us : 0.875 * ema_us + 0.125 * us;
            }
            continue;
        }
        if (idle) {
            // nothing to launch: wait for the next submitted step.  Spin briefly (steps come every ~200 us under load), then PARK on
            // the condition variable: the kick counter moves under c->mu, so a kick cannot fall between the check and the sleep, and
            // an idle engine costs no CPU (the 2 ms timed wait of round 4 re-ran the 1-2 ms spin phase after every
            // time-out -- 30-50 % of a core per idle context).  The 250 ms time-out is a backstop only (lasr_step_wait kicks too).
            bool parked = false;
            for (int spins = 0; c->kick.load(std::memory_order_acquire) == seen_kick && !c->pump_stop.load(std::memory_order_relaxed); ++spins) {
                if (!parked && spins < 40000) { __builtin_ia32_pause(); continue; }
                std::unique_lock<std::mutex> lk(c->mu);
                c->cv_pump.wait_for(lk, std::chrono::milliseconds(250), [&] { return c->kick.load() != seen_kick || c->pump_stop.load(); });
                parked = true;               // (a time-out goes straight back to sleep: no second spin phase)
            }
            seen_kick = c->kick.load(std::memory_order_acquire);
        }
    }
}
// called by the API thread (c->mu held) when the first step is handed to the decode loop
static int pump_start(lasr_ctx* c) {
    static const int pump_env = getenv("LASR_PUMP") ? atoi(getenv("LASR_PUMP")) : 1;
    const bool can = pump_env != 0 && c->use_graphs && !c->dbg && c->M <= 512;
    if (!can) { c->pump_on = false; return LASR_OK; }
    RC(ensure_group_graphs(c));
    if (!c->pump_started) {
        c->pump_started = true;
        c->pump_th = std::thread(pump_main, c);
    }
    c->pump_on = true;
    return LASR_OK;
}
// The counter moves UNDER c->mu: the sleeping pump checks it and blocks under the same mutex, so a kick cannot fall between its
// check and its sleep.  (Round 4 first bumped it without the mutex: a kick in that window was lost and the pump slept out its
// timeout -- 20 ms then -- while a step waited; seen once, as a 25 ms stall in an 81 ms timed region.  The timeout is 2 ms now.)
static void pump_kick(lasr_ctx* c) {
    { std::lock_guard<std::mutex> lk(c->mu); c->kick.fetch_add(1, std::memory_order_release); }
    c->cv_pump.notify_one();
}

static bool cont_step_done(const lasr_ctx* c, const lasr_ctx::PendingStep& P) {
    for (int r : P.rows)
        if (c->h_cur_seen[r] < P.target[r]) return false;
    return true;
}

int lasr_step_wait(lasr_ctx* c, int* n_ran) {
    if (!c) return LASR_EINVAL;
    RoctxRange roctx_range_("lasr_step_wait");
    if (n_ran) *n_ran = 0;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (c->pending.empty()) return LASR_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    int* flag = c->cont_host;
    if (c->pump_on) {
        // the pump thread launches the groups and consumes their flags: wait for its progress counter
        for (unsigned long long guard = 0;; ++guard) {
            const long long seen = c->progress.load(std::memory_order_acquire);
            {
                std::lock_guard<std::mutex> lk(c->mu);
                if (c->pump_rc) return fail(c, c->pump_rc, "decode pump: %s", c->pump_err.c_str());
                if (cont_step_done(c, c->pending.front())) break;
            }
            // a short spin (a group that is about to publish), then the thread sleeps until the pump has consumed the next group's
            // flag (cont_poll notifies): with 20 steps in flight a collect has slack, and a rank no longer burns a core waiting
            // (round 5: 2.65 -> see profiles/r05 host cores per rank).  The time-out kicks a sleeping pump (backstop).
            unsigned long long spins = 0;
            while (c->progress.load(std::memory_order_acquire) == seen) {
                __builtin_ia32_pause();
                if (++spins > 3000) {
                    std::unique_lock<std::mutex> lk(c->mu);
                    const bool moved = c->cv_prog.wait_for(lk, std::chrono::milliseconds(10), [&] { return c->progress.load(std::memory_order_acquire) != seen || c->pump_rc != 0; });
                    lk.unlock();
                    if (!moved) pump_kick(c);
                    break;
                }
            }
            if (guard > (1u << 16)) return fail(c, LASR_EHIP, "decode loop did not converge");
        }
    } else {
        for (int guard = 0;; ++guard) {
            {
                std::lock_guard<std::mutex> lk(c->mu);
                cont_poll(c);
                if (cont_step_done(c, c->pending.front())) break;
                if (!c->group_inflight) RC(cont_launch_group(c, c->wait_n));
            }
            RC(spin_flag(c, flag, c->stream_dec));
            if (guard > 4096) return fail(c, LASR_EHIP, "decode loop did not converge");
        }
    }
    // results of the oldest step: tokens between the previous and this step boundary of every row, already
    // in pinned memory (written by the kernels of the groups that completed before the cursors were published)
    std::lock_guard<std::mutex> lk(c->mu);
    lasr_ctx::PendingStep& P = c->pending.front();
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (c->W > 1) {      // beam: the whole best hypothesis as of this model step (lasr_fetch semantics of beam > 1)
        for (int r : P.rows) {
            BeamSlot& B = c->beams[r];
            if (B.steps.empty()) return fail(c, LASR_EHIP, "beam: no result for slot %d although its step is decoded", r);
            B.deliver(std::move(B.steps.front()), c->results[r]);
            B.steps.pop_front();
        }
    } else
    for (int r : P.rows) {
        const long long end = step_end_mark(c, P, r);
        SlotResult& out = c->results[r];
        if (!c->align_on) for (long long q = c->h_fetched[r]; q < end; ++q) out.append(ring_token(c, r, q));
        else for (long long q = c->h_fetched[r]; q < end; ++q) out.append(ring_token(c, r, q), ring_record(c, P, r, q));
        c->h_fetched[r] = end;
    }
    c->stats.frames = P.Tm;
    c->stats.decode_iters = (int)(c->cont_iters - c->iters_reported);
    c->iters_reported = c->cont_iters;
    if (n_ran) *n_ran = (int)P.rows.size();
    c->pending.erase(c->pending.begin());
    c->cmd_inflight = 0;
    if (!c->pump_on) RC(cont_pump_locked(c, c->wait_n));
    return LASR_OK;
}

// ---------------------------------------------------------------------------- offline
// The front half of every offline entry point (lasr_transcribe_*, lasr_align_*, lasr_score_*): frame counts from the lengths, then the
// audio of the listed rows through the front-end and the encoder, behind a reset of the call's rows.
struct OfflineDims {
    std::vector<int> Tp, Tm;           // per utterance: encoder-input frames, log-mel frames (pcm only)
    int T_max = 0, Tmel_max = 0;
    long long total = 0;               // samples / frames of the call
};
// host arithmetic only: nothing has changed when they fail
static int offline_dims_pcm(lasr_ctx* c, int n, const int64_t* n_samples, OfflineDims& D) {
    const lasr_model_desc& d = c->d;
    D.Tp.assign(n, 0); D.Tm.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        if (n_samples[i] <= d.n_fft / 2) return fail(c, LASR_EINVAL, "utterance %d too short (%lld samples)", i, (long long)n_samples[i]);
        D.Tm[i] = 1 + (int)(n_samples[i] / d.hop);
        if (D.Tm[i] < d.n_stack) return fail(c, LASR_EINVAL, "utterance %d yields no stacked frame", i);
        D.Tp[i] = (D.Tm[i] - d.n_stack) / d.stride + 1;
        D.T_max = std::max(D.T_max, D.Tp[i]); D.Tmel_max = std::max(D.Tmel_max, D.Tm[i]);
        D.total += n_samples[i];
    }
    return LASR_OK;
}
static int offline_dims_feats(lasr_ctx* c, int n, const int32_t* n_frames, OfflineDims& D) {
    D.Tp.assign(n_frames, n_frames + n);
    for (int i = 0; i < n; ++i) {
        if (n_frames[i] < 1) return fail(c, LASR_EINVAL, "utterance %d has no frames", i);
        D.T_max = std::max(D.T_max, (int)n_frames[i]); D.total += n_frames[i];
    }
    return LASR_OK;
}
// Which rows a call touches.  audio [n]: the row that carries utterance i (lasr_score_*: its first candidate's; the other rows keep
// T_row = 0).  reset [n_reset]: every row of the call, back to a fresh stream.  lattice: a lattice call marks its start for lat_times
// in front of the reset; a decode call clears its beam records and marks behind it.
struct OfflineRows { const int* audio; int n; const int* reset; int n_reset; bool lattice; };
// inside the command the builder opened: the rows' reset, the commit, the reset itself and the call's first marker
static int offline_reset(lasr_ctx* c, const OfflineRows& r) {
    for (int j = 0; j < r.n_reset; ++j) {
        const int s = r.reset[j];
        c->hc.what[s] = 7;
        c->results[s].clear(); c->results[s].neg_logp = 0.0;
        if (!r.lattice) beam_host_reset(c, s, true);
    }
    RC(cmd_commit(c));
    if (r.lattice) lat_mark(c, c->lat, 0);
    RC(apply_reset(c, sync_view(c, c->la_offline), true));
    if (!r.lattice) rec(c, 0);
    return LASR_OK;
}
// pcm [D.total] (host or device), the utterances concatenated: log-mel, stack + LayerNorm, encoder -> pe_sync
static int offline_front_pcm(lasr_ctx* c, const float* pcm, const int64_t* n_samples, const OfflineDims& D, const OfflineRows& r) {
    const lasr_model_desc& d = c->d;
    RC(ensure_T(c, D.T_max));
    const float* src = nullptr;
    RC(stage_to_device(c, pcm, (size_t)D.total, &c->stage_pcm, &c->stage_pcm_floats, &src));
    RC(ensure_buf(c, &c->lm_buf, &c->lm_floats, (size_t)c->M * D.Tmel_max * d.n_mels));
    RC(cmd_begin(c));
    long long off = 0;
    for (int i = 0; i < r.n; ++i) {
        const int s = r.audio[i];
        c->hc.T_row[s] = D.Tp[i]; c->hc.row_frames[s] = D.Tm[i];
        c->hc.row_N[s] = n_samples[i]; c->hc.row_src_off[s] = off;
        off += n_samples[i];
    }
    RC(offline_reset(c, r));
    launch_logmel_offline(c, src, 0, c->M, D.Tmel_max, c->lm_buf, c->dc.row_N, c->dc.row_src_off, c->dc.row_frames);
    stack_ln_logmel(c, c->lm_buf, D.Tmel_max, d.stride, c->dc.T_row, D.T_max);
    RC(commit_T_rows(c, D.T_max));
    encode_step(c, D.T_max);
    return LASR_OK;
}
// feats [D.total][feat] (host or device): stack + LayerNorm, encoder -> pe_sync
static int offline_front_feats(lasr_ctx* c, const float* feats, const OfflineDims& D, const OfflineRows& r) {
    RC(ensure_T(c, D.T_max));
    const float* src = nullptr;
    RC(stage_to_device(c, feats, (size_t)D.total * c->d.feat, &c->feat_stage, &c->feat_stage_floats, &src));
    RC(cmd_begin(c));
    long long off = 0;
    for (int i = 0; i < r.n; ++i) {
        c->hc.T_row[r.audio[i]] = D.Tp[i]; c->hc.row_feat_off[r.audio[i]] = off;
        off += D.Tp[i];
    }
    RC(offline_reset(c, r));
    stack_ln_feats(c, src, c->dc.row_feat_off, c->dc.T_row, D.T_max);
    RC(commit_T_rows(c, D.T_max));
    encode_step(c, D.T_max);
    return LASR_OK;
}

// either kind of audio of a call: pcm with n_samples or stacked features with n_frames (the other null), utterances concatenated
struct OfflineAudio {
    const float* data; const int64_t* n_samples; const int32_t* n_frames;
    bool given() const { return data && (n_samples || n_frames); }
};
static int offline_dims(lasr_ctx* c, int n, const OfflineAudio& au, OfflineDims& D) {
    return au.n_samples ? offline_dims_pcm(c, n, au.n_samples, D) : offline_dims_feats(c, n, au.n_frames, D);
}
static int offline_front(lasr_ctx* c, const OfflineAudio& au, const OfflineDims& D, const OfflineRows& r) {
    return au.n_samples ? offline_front_pcm(c, au.data, au.n_samples, D, r) : offline_front_feats(c, au.data, D, r);
}

static int transcribe_impl(lasr_ctx* c, const int* slots, int n, const OfflineAudio& au) {
    if (!c) return LASR_EINVAL;
    RC(flush_lazy(c));
    RC(require_idle(c));
    RC(check_slots(c, slots, n, true));
    if (n == 0) return LASR_OK;
    if (!au.given()) return fail(c, LASR_EINVAL, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    OfflineDims D;
    RC(offline_dims(c, n, au, D));
    RC(offline_front(c, au, D, OfflineRows{slots, n, slots, n, false}));
    return decode_and_collect(c, D.T_max, c->d.max_iters_offline, true, std::vector<int>(slots, slots + n));
}
int lasr_transcribe_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples) {
    RoctxRange roctx_range_("lasr_transcribe");
    return transcribe_impl(c, slots, n, OfflineAudio{pcm, n_samples, nullptr});
}
int lasr_transcribe_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames) {
    return transcribe_impl(c, slots, n, OfflineAudio{feats, nullptr, n_frames});
}

// ---------------------------------------------------------------------------- teacher-forced lattice
// The banded lattice is compiled at the END of this unit -- lasr_lattice_band.hip.h, lasr_lattice_band_post.hip.h
// and their entry points follow the last function below -- and align_impl reaches it through these declarations.
namespace lasr {
constexpr int LAT_BAND_WMAX = 1536;    // window width: four diagonals of doubles (48 KB) + 16 KB of back-pointers = 64 KB of LDS
constexpr int LAT_BAND_UMAX = 32767;   // labels per transcript of a banded call (the teacher-forced predictor keeps (U + 1) rows x J)
}
namespace {
struct LatBandIO;
int lat_band_plan(lasr_ctx* c, const int* T, const int32_t* U, int n, const LatBandIO& io, bool post);
int lat_finish_band(lasr_ctx* c, const int* slots, int n, const int32_t* tokens, const LatOut& o, const LatBandIO& io, const LatPostOut* post);
}
// a posterior call keeps alpha and beta of every cell: refused beyond LAT_POST_CELLS, before anything is read or changed
static int post_check_cells(lasr_ctx* c, const int* T, const int32_t* U, int n) {
    long long cells = 0;
    for (int i = 0; i < n; ++i) cells += (long long)T[i] * (U[i] + 1);
    if (cells > LAT_POST_CELLS) return fail(c, LASR_EINVAL, "posteriors of a lattice of %lld cells (at most %lld)", cells, LAT_POST_CELLS);
    return LASR_OK;
}
// lasr_align_*.  post: the posterior outputs of lasr_align_post_* / lasr_align_band_post_* (null: none); band: lasr_align_band_* (null:
// the full lattice).  The cell limit of a posterior call counts the cells it keeps: the full lattice's here, a band's in lat_band_plan.
// A greedy, idle context, open slots, a valid transcript per utterance, and the refusals that need the frame counts: nothing has
// changed when it fails before the front half
struct AlignCall { const int* slots; int n; const int32_t* tokens; const int32_t* n_tokens; LatOut o; const LatPostOut* post; const LatBandIO* band; };
static int align_impl(lasr_ctx* c, const AlignCall& a, const OfflineAudio& au) {
    if (!c) return LASR_EINVAL;
    if (c->W > 1) return fail(c, LASR_EINVAL, "lasr_align_*: greedy contexts only (beam = %d)", c->W);
    RC(flush_lazy(c));
    RC(require_idle(c));
    RC(check_slots(c, a.slots, a.n, true));
    if (a.n == 0) return LASR_OK;
    if (!au.given() || !a.o.loglik) return fail(c, LASR_EINVAL, "null argument");
    RC(lat_check_tokens(c, a.n, a.tokens, a.n_tokens, a.band ? LAT_BAND_UMAX : LAT_UMAX));
    HIPCHK(c, hipSetDevice(c->device));
    OfflineDims D;
    RC(offline_dims(c, a.n, au, D));
    if (a.post && !a.band) RC(post_check_cells(c, D.Tp.data(), a.n_tokens, a.n));
    if (a.band) RC(lat_band_plan(c, D.Tp.data(), a.n_tokens, a.n, *a.band, a.post != nullptr));
    RC(offline_front(c, au, D, OfflineRows{a.slots, a.n, a.slots, a.n, true}));
    if (a.band) return lat_finish_band(c, a.slots, a.n, a.tokens, a.o, *a.band, a.post);
    return lat_finish(c, a.slots, a.n, D.Tp.data(), a.tokens, a.n_tokens, a.o, a.post);
}
int lasr_align_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                   const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp, float* emit_lp) {
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, nullptr, nullptr};
    return align_impl(c, a, OfflineAudio{pcm, n_samples, nullptr});
}
int lasr_align_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                     const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp, float* emit_lp) {
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, nullptr, nullptr};
    return align_impl(c, a, OfflineAudio{feats, nullptr, n_frames});
}
// lasr_align_* with the lattice's edge posteriors; all six posterior outputs null: lasr_align_* itself
int lasr_align_post_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                        const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp, float* emit_lp,
                        float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var, int32_t* tok_peak_frame, double* tok_peak) {
    const LatPostOut p{nullptr, nullptr, occ_blank, occ_emit, tok_mean, tok_var, tok_peak_frame, tok_peak};
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, lat_post_any(p) ? &p : nullptr, nullptr};
    return align_impl(c, a, OfflineAudio{pcm, n_samples, nullptr});
}
int lasr_align_post_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                          const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp, float* emit_lp,
                          float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var, int32_t* tok_peak_frame, double* tok_peak) {
    const LatPostOut p{nullptr, nullptr, occ_blank, occ_emit, tok_mean, tok_var, tok_peak_frame, tok_peak};
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, lat_post_any(p) ? &p : nullptr, nullptr};
    return align_impl(c, a, OfflineAudio{feats, nullptr, n_frames});
}
// ---- the dynamic programmes alone, on the caller's lattices (host or device); sizes and results are host memory; blocking
// behind the call's tables: the two lattices to the device (a device pointer is used where it is), what `run` enqueues over them, and
// the stream drained
extern "C++" template <class Run>
static int lattice_hook(lasr_ctx* c, const float* blank_lp, const float* emit_lp, long long cells, Run run) {
    lasr_ctx::Lattice& w = c->lat;
    const float *b = nullptr, *e = nullptr;
    RC(stage_to_device(c, blank_lp, (size_t)cells, &w.b, &w.b_n, &b));
    RC(stage_to_device(c, emit_lp, (size_t)cells, &w.e, &w.e_n, &e));
    RC(run(b, e));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}
// head of lasr_lattice_dp / lasr_lattice_post: the arguments, and the call description with every utterance on row 0
static int lattice_call(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, int n, const double* loglik,
                        LatCall& k) {
    if (!blank_lp || !emit_lp || !T || !U || !loglik || n < 1) return fail(c, LASR_EINVAL, "bad argument");
    k.n = n;
    k.T.assign(T, T + n); k.U.assign(U, U + n); k.slot.assign(n, 0);
    for (int i = 0; i < n; ++i)
        if (T[i] < 1 || U[i] < 0 || U[i] > LAT_UMAX) return fail(c, LASR_EINVAL, "lattice %d: T = %d, U = %d (T >= 1, 0 <= U <= %d)", i, T[i], U[i], LAT_UMAX);
    return LASR_OK;
}
// layout and tables of a full-lattice hook's call -> device (no labels: the programmes read none)
static int lattice_tables(lasr_ctx* c, LatCall& k, TabImage& img) {
    HIPCHK(c, hipSetDevice(c->device));
    RC(lat_layout_checked(c, k));
    lat_pack(k, nullptr, img);
    return lat_upload(c, c->lat, img);
}
int lasr_lattice_dp(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, int n, double* loglik,
                    double* viterbi, int32_t* frames) {
    if (!c) return LASR_EINVAL;
    LatCall k;
    TabImage img;
    RC(lattice_call(c, blank_lp, emit_lp, T, U, n, loglik, k));
    RC(lattice_tables(c, k, img));
    RC(lattice_hook(c, blank_lp, emit_lp, k.cells, [&](const float* b, const float* e) {
        return lat_run_dp(c, c->lat, k, b, e, viterbi || frames, frames != nullptr, false);
    }));
    return lat_copy_out(c, c->lat, k, LatOut{loglik, viterbi, frames, nullptr, nullptr, nullptr});
}
// the forward-backward programme
int lasr_lattice_post(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, int n, double* loglik,
                      double* loglik_bwd, float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var, int32_t* tok_peak_frame,
                      double* tok_peak) {
    if (!c) return LASR_EINVAL;
    LatCall k;
    TabImage img;
    RC(lattice_call(c, blank_lp, emit_lp, T, U, n, loglik, k));
    RC(post_check_cells(c, T, U, n));
    RC(lattice_tables(c, k, img));
    const LatPostOut p{loglik, loglik_bwd, occ_blank, occ_emit, tok_mean, tok_var, tok_peak_frame, tok_peak};
    RC(lattice_hook(c, blank_lp, emit_lp, k.cells, [&](const float* b, const float* e) { return lat_post_launch(c, c->lat, k, b, e, p); }));
    return lat_post_copy(c, c->lat, k, p);
}
// ---------------------------------------------------------------------------- n-best rescoring over a prefix tree
int lasr_prefix_tree(const int32_t* tokens, const int32_t* n_tokens, int k, int cap, int32_t* parent, int32_t* label, int32_t* depth,
                     int32_t* term, int* n_nodes) {
    return lasr_pt::prefix_tree(tokens, n_tokens, k, cap, parent, label, depth, term, n_nodes);
}
// common head of lasr_score_*: a greedy, idle context, one open slot and a valid transcript per candidate, a tree per utterance that
// fits -- nothing has changed when it fails.  *K = candidates of the call
static int score_prologue(lasr_ctx* c, const int* slots, int n, const void* audio, const void* lens, const int32_t* n_cands,
                          const int32_t* tokens, const int32_t* n_tokens, const double* loglik, int* K, std::vector<lasr_pt::Tree>& trees) {
    *K = 0;
    if (c->W > 1) return fail(c, LASR_EINVAL, "lasr_score_*: greedy contexts only (beam = %d)", c->W);
    RC(flush_lazy(c));
    RC(require_idle(c));
    if (n < 0 || n > c->d.max_streams) return fail(c, LASR_EINVAL, "bad utterance count (n=%d)", n);
    if (n == 0) return LASR_OK;
    if (!n_cands) return fail(c, LASR_EINVAL, "null argument");
    int k = 0;
    for (int i = 0; i < n; ++i) {
        if (n_cands[i] < 1) return fail(c, LASR_EINVAL, "utterance %d has %d candidates (>= 1)", i, n_cands[i]);
        if (n_cands[i] > c->d.max_streams - k) return fail(c, LASR_EINVAL, "more candidates than max_streams (%d)", c->d.max_streams);
        k += n_cands[i];
    }
    RC(check_slots(c, slots, k, true));
    if (!audio || !lens || !loglik) return fail(c, LASR_EINVAL, "null argument");
    RC(lat_check_tokens(c, k, tokens, n_tokens));
    trees.resize(n);
    long long at = 0;
    for (int i = 0, j = 0; i < n; j += n_cands[i], ++i) {
        lasr_pt::build(tokens + at, n_tokens + j, n_cands[i], trees[i]);
        if ((int)trees[i].parent.size() > LAT_NMAX)
            return fail(c, LASR_EINVAL, "utterance %d: the candidates' prefix tree has %d nodes (<= %d)", i, (int)trees[i].parent.size(), LAT_NMAX);
        for (int q = 0; q < n_cands[i]; ++q) at += n_tokens[j + q];
    }
    *K = k;
    return LASR_OK;
}
static int score_impl(lasr_ctx* c, const int* slots, int n, const OfflineAudio& au, const int32_t* n_cands, const int32_t* tokens,
                      const int32_t* n_tokens, const TreeOut& o) {
    if (!c) return LASR_EINVAL;
    int K = 0;
    std::vector<lasr_pt::Tree> trees;
    RC(score_prologue(c, slots, n, au.data, au.n_samples ? (const void*)au.n_samples : au.n_frames, n_cands, tokens, n_tokens, o.loglik, &K, trees));
    if (n == 0) return LASR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    OfflineDims D;
    RC(offline_dims(c, n, au, D));
    std::vector<int> first(n);                        // the audio of an utterance lives on the row of its first candidate
    for (int i = 0, j = 0; i < n; j += n_cands[i], ++i) first[i] = slots[j];
    RC(offline_front(c, au, D, OfflineRows{first.data(), n, slots, K, true}));
    return tree_finish(c, slots, n, n_cands, D.Tp.data(), tokens, n_tokens, trees, o);
}
int lasr_score_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* n_cands,
                   const int32_t* tokens, const int32_t* n_tokens, double* loglik, double* viterbi, float* blank_lp, float* emit_lp) {
    return score_impl(c, slots, n, OfflineAudio{pcm, n_samples, nullptr}, n_cands, tokens, n_tokens, TreeOut{loglik, viterbi, blank_lp, emit_lp});
}
int lasr_score_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* n_cands,
                     const int32_t* tokens, const int32_t* n_tokens, double* loglik, double* viterbi, float* blank_lp, float* emit_lp) {
    return score_impl(c, slots, n, OfflineAudio{feats, nullptr, n_frames}, n_cands, tokens, n_tokens, TreeOut{loglik, viterbi, blank_lp, emit_lp});
}
// the tree dynamic programme alone, on the caller's lattices (host or device); T, n_nodes, parent and the results are host memory; blocking
// (contiguous children are NOT required here: only k_lat_dp_tree runs, which reads parent / depth / dstart; the child tables that
// tree_upload derives are valid for lasr_prefix_tree's order alone and are not to be used behind this entry point)
int lasr_lattice_tree_dp(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* n_nodes,
                         const int32_t* parent, int n, double* loglik, double* viterbi) {
    if (!c) return LASR_EINVAL;
    if (!blank_lp || !emit_lp || !T || !n_nodes || !parent || !loglik || n < 1) return fail(c, LASR_EINVAL, "bad argument");
    TreeCall k;
    k.n = n;
    k.T.assign(T, T + n); k.N.assign(n_nodes, n_nodes + n);
    long long no = 0;
    for (int i = 0; i < n; ++i) {
        if (T[i] < 1 || n_nodes[i] < 1 || n_nodes[i] > LAT_NMAX)
            return fail(c, LASR_EINVAL, "lattice %d: T = %d, N = %d (T >= 1, 1 <= N <= %d)", i, T[i], n_nodes[i], LAT_NMAX);
        const int32_t* p = parent + no;
        if (p[0] != -1) return fail(c, LASR_EINVAL, "lattice %d: node 0 is the root (parent -1)", i);
        k.parent.push_back(-1); k.depth.push_back(0);
        for (int v = 1; v < n_nodes[i]; ++v) {
            if (p[v] < 0 || p[v] >= v) return fail(c, LASR_EINVAL, "lattice %d: parent[%d] = %d (0 <= parent < node)", i, v, p[v]);
            const int dv = k.depth[(size_t)no + p[v]] + 1;
            if (dv < k.depth.back()) return fail(c, LASR_EINVAL, "lattice %d: node %d is shallower than node %d (depth must not decrease)", i, v, v - 1);
            k.parent.push_back(p[v]); k.depth.push_back(dv);
        }
        no += n_nodes[i];
    }
    HIPCHK(c, hipSetDevice(c->device));
    lasr_ctx::Lattice& w = c->lat;
    TabImage img;
    RC(tree_upload(c, w, k, img));
    RC(lattice_hook(c, blank_lp, emit_lp, k.cells, [&](const float* b, const float* e) { return tree_run_dp(c, w, k, b, e, viterbi != nullptr); }));
    HIPCHK(c, hipMemcpy(loglik, w.res, sizeof(double) * (size_t)k.nodes, hipMemcpyDeviceToHost));
    if (viterbi) HIPCHK(c, hipMemcpy(viterbi, w.res + k.nodes, sizeof(double) * (size_t)k.nodes, hipMemcpyDeviceToHost));
    return LASR_OK;
}

// ---------------------------------------------------------------------------- LM sequence scoring
// A greedy context, valid arguments (host checks only: nothing has changed when one fails), an attached LM, an idle engine; then
// lm_score_run (lasr_lm_score.hip.h)
int lasr_lm_score(lasr_ctx* c, const int* slots, int n, const int32_t* tokens, const int32_t* n_tokens, int start, double* total, float* logps) {
    if (!c) return LASR_EINVAL;
    if (c->W > 1) return fail(c, LASR_EINVAL, "lasr_lm_score: greedy contexts only (beam = %d)", c->W);
    if (n < 1 || n > c->d.max_streams) return fail(c, LASR_EINVAL, "bad candidate count (n=%d)", n);
    if (!slots || !n_tokens || !total) return fail(c, LASR_EINVAL, "null argument");
    if (start < -1 || start >= c->d.vocab) return fail(c, LASR_EINVAL, "start token %d (-1: none, or 0..%d)", start, c->d.vocab - 1);
    std::vector<char> seen(c->d.max_streams, 0);
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        if (s < 0 || s >= c->d.max_streams || !c->open_[s]) return fail(c, LASR_EINVAL, "slot %d is not open", s);
        if (seen[s]) return fail(c, LASR_EINVAL, "slot %d listed twice", s);
        seen[s] = 1;
    }
    RC(lat_check_tokens(c, n, tokens, n_tokens));
    if (!c->lm.on) return fail(c, LASR_ESTATE, "lasr_lm_score: no LM is attached");
    RC(flush_lazy(c));
    RC(require_idle(c));
    HIPCHK(c, hipSetDevice(c->device));
    return lm_score_run(c, slots, n, tokens, n_tokens, start, total, logps);
}

// Transducer.transcribe_stream on feature chunks (models.py:506-575): carried encoder / predictor
// state, max_iters_stream.  feats [n, T, feat] (host or device), the same T for every listed slot.
int lasr_step_feats(lasr_ctx* c, const int* slots, int n, const float* feats, int T) {
    if (!c) return LASR_EINVAL;
    RC(flush_lazy(c));
    RC(require_idle(c));
    RC(check_slots(c, slots, n, true));
    if (n == 0) return LASR_OK;
    if (!feats || T < 1) return fail(c, LASR_EINVAL, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    const lasr_model_desc& d = c->d;
    RC(ensure_T(c, T));
    const float* src = nullptr;
    RC(stage_to_device(c, feats, (size_t)n * T * d.feat, &c->feat_stage, &c->feat_stage_floats, &src));
    RC(cmd_begin(c));
    std::vector<int> rows(slots, slots + n);
    for (int i = 0; i < n; ++i) { c->hc.T_row[slots[i]] = T; c->hc.row_feat_off[slots[i]] = (long long)i * T; }
    RC(cmd_commit(c));
    RC(commit_T_rows(c, T));
    rec(c, 0);
    stack_ln_feats(c, src, c->dc.row_feat_off, c->T_row_dev, T);
    encode_step(c, T);
    return decode_and_collect(c, T, d.max_iters_stream, false, rows);
}

// The fetch entry points: each validates its own arguments, then hands the slot's result out through one of these two.
static int open_slot(lasr_ctx* c, int slot) {
    if (slot < 0 || slot >= c->d.max_streams || !c->open_[slot]) return fail(c, LASR_ESTATE, "slot %d is not open", slot);
    return LASR_OK;
}
// one slot; have_bufs: every array the caller must supply is there.  Too little room (or no array): the need is reported, nothing
// is consumed.  Null frames / logps: the records are dropped with the tokens (and so is the rest of a beam: lasr_fetch_nbest
// consumes the same result)
static int fetch_one(lasr_ctx* c, int slot, int32_t* tokens, int32_t* frames, float* logps, bool have_bufs, int cap, int* n_new,
                     double* neg_logp, double* align) {
    RC(open_slot(c, slot));
    SlotResult& r = c->results[slot];
    if (!r.take(have_bufs ? tokens : nullptr, frames, logps, cap, n_new)) return fail(c, LASR_EFULL, "token buffer too small: need %d", *n_new);
    if (neg_logp) *neg_logp = r.neg_logp;
    if (align) *align = r.align;
    return LASR_OK;
}
// n slots into [n][cap] arrays: all of them are checked before anything is consumed (an error leaves n_new alone)
static int fetch_many(lasr_ctx* c, const int* slots, int n, int32_t* tokens, int32_t* frames, float* logps, int cap, int* n_new) {
    for (int i = 0; i < n; ++i) {
        RC(open_slot(c, slots[i]));
        const int need = c->results[slots[i]].need();
        if (need > cap) return fail(c, LASR_EFULL, "token buffer too small: slot %d needs %d", slots[i], need);
    }
    for (int i = 0; i < n; ++i) {
        const size_t o = (size_t)i * cap;
        (void)c->results[slots[i]].take(tokens + o, frames ? frames + o : nullptr, logps ? logps + o : nullptr, cap, &n_new[i]);   // (fits: checked above)
    }
    return LASR_OK;
}

int lasr_fetch(lasr_ctx* c, int slot, int32_t* tokens, int cap, int* n_new, double* neg_logp, double* align) {
    if (!c || !n_new) return LASR_EINVAL;
    return fetch_one(c, slot, tokens, nullptr, nullptr, tokens != nullptr, cap, n_new, neg_logp, align);
}

int lasr_fetch_many(lasr_ctx* c, const int* slots, int n, int32_t* tokens, int cap, int* n_new) {
    if (!c || !n_new || (n > 0 && !slots)) return LASR_EINVAL;
    return fetch_many(c, slots, n, tokens, nullptr, nullptr, cap, n_new);
}

// What a host read of the resident state and every switch of the decode kernels start from: the deferred append flushed, no step in
// flight (idle = false: lasr_debug_read looks whatever is in flight), the main and the decode stream drained
static int drain(lasr_ctx* c, bool idle = true) {
    RC(flush_lazy(c));
    if (idle) RC(require_idle(c));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream_dec) HIPCHK(c, hipStreamSynchronize(c->stream_dec));
    return LASR_OK;
}

// What the record switches (lasr_set_alignments, lasr_set_beam_records) and bias_attach do first: the engine idle and drained, no
// slot with an unfetched result (`unfetched`: the refusal's text, with the slot and its token count as arguments), the cached decode
// groups dropped
static int toggle_prologue(lasr_ctx* c, const char* unfetched) {
    RC(drain(c));
    for (int s = 0; s < c->M; ++s)
        if (c->results[s].unfetched()) return fail(c, LASR_ESTATE, unfetched, s, c->results[s].need());
    std::lock_guard<std::mutex> lk(c->mu);        // (the pump thread looks graphs up under c->mu; nothing is in flight)
    drop_decode_graphs(c);
    return LASR_OK;
}

// ---------------------------------------------------------------------------- per-token alignment records
// Greedy decode: k_select stores, next to every token, the frame cursor and the joint's log p of that decision (DecState::
// step_frame / step_logp; null pointers = off, the default).  Toggling changes what the decode launches store and how the
// synchronous result block is laid out, so the engine must be idle, and every cached decode graph (DecState is captured by
// value) is dropped.
int lasr_set_alignments(lasr_ctx* c, int on) {
    if (!c) return LASR_EINVAL;
    if (c->W > 1) return fail(c, LASR_EINVAL, "alignment records serve greedy decode (beam = 1)");
    const bool want = on != 0;
    if (want == c->align_on) return LASR_OK;       // (nothing to switch: also fine while steps are in flight)
    // tokens decoded before the switch would have no record (on) or lose theirs (off): they are fetched first
    RC(toggle_prologue(c, "slot %d has %d unfetched token(s): fetch them before the switch"));
    if (want && !c->align_host) {
        const size_t n = (size_t)c->M * lasr_ctx::TOKRING;
        HIPCHK(c, hipHostMalloc((void**)&c->align_host, sizeof(int) * 2 * n));
        memset(c->align_host, 0, sizeof(int) * 2 * n);
        void* dp = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(&dp, c->align_host, 0));
        c->c_frame_ring = (int*)dp;
        c->c_logp_ring = (float*)((int*)dp + n);
    }
    c->align_on = want;
    RC(alloc_results(c));
    return LASR_OK;
}

int lasr_fetch_aligned(lasr_ctx* c, int slot, int32_t* tokens, int32_t* frames, float* logps, int cap, int* n_new, double* neg_logp,
                       double* align) {
    if (!c || !n_new) return LASR_EINVAL;
    if (!c->align_on) return fail(c, LASR_ESTATE, "alignment records are off: call lasr_set_alignments first");
    return fetch_one(c, slot, tokens, frames, logps, tokens && frames && logps, cap, n_new, neg_logp, align);
}

int lasr_fetch_many_aligned(lasr_ctx* c, const int* slots, int n, int32_t* tokens, int32_t* frames, float* logps, int cap, int* n_new) {
    if (!c || !n_new || (n > 0 && (!slots || !tokens || !frames || !logps))) return LASR_EINVAL;
    if (!c->align_on) return fail(c, LASR_ESTATE, "alignment records are off: call lasr_set_alignments first");
    return fetch_many(c, slots, n, tokens, frames, logps, cap, n_new);
}

// ---------------------------------------------------------------------------- contextual biasing, greedy and beam
int lasr_bias_compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                      int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_bonus, int32_t* depth,
                      int* n_nodes, int* n_edges) {
    return lasr_bias::compile(tokens, n_tokens, weights, k, vocab, blank, cap_nodes, cap_edges, edge_off, edge_tok, edge_next, edge_bonus,
                              depth, n_nodes, n_edges);
}
int lasr_beam_bias_compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                           int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_gain, float* node_back,
                           int32_t* depth, int* n_nodes, int* n_edges) {
    return lasr_bias::beam_compile(tokens, n_tokens, weights, k, vocab, blank, cap_nodes, cap_edges, edge_off, edge_tok, edge_next, edge_gain,
                                   node_back, depth, n_nodes, n_edges);
}
int lasr_bias_walk(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_gain,
                   const float* node_back, int blank, const int32_t* tokens, int n, int start, int* end_node, double* total, float* gains) {
    return lasr_bias::walk(n_nodes, edge_off, edge_tok, edge_next, edge_gain, node_back, blank, tokens, n, start, end_node, total, gains);
}
// Attaching, replacing or detaching (n_nodes = 0) a graph, behind the setter's width refusal.  beam: the beam form -- edge_val is
// the gain and node_back the fifth column; else the greedy form -- edge_val is the bonus, node_back is not looked at.  `fn`: the
// entry point's name in the texts.  With a graph attached the decode launches run k_select<.., BIAS = true> at one frame per
// iteration (greedy) or k_beam_select_rw<.., BIAS = true> (beam), and every row carries its automaton node beside its predictor
// state (greedy) or through the parent indirection (beam).  Like the record switches this changes which kernel the decode launches
// run, so the engine must be idle and the cached groups are dropped.  The graph is checked on the host before anything changes; a
// failure behind the upload frees the new block and leaves the context as it was.  A beam's scores stay what they are, at
// switch-on and at switch-off.
static int bias_attach(lasr_ctx* c, bool beam, const char* fn, int n_nodes, const int32_t* edge_off, const int32_t* edge_tok,
                       const int32_t* edge_next, const float* edge_val, const float* node_back) {
    if (n_nodes == 0 && !bias_on(c)) return LASR_OK;            // (off already: also fine while steps are in flight)
    if (n_nodes != 0) {
        if (c->lm.on)
            return fail(c, LASR_ESTATE, beam ? "lasr_set_beam_bias refuses an attached LM (the combination with LM fusion is not served)"
                                             : "lasr_set_bias refuses an attached LM (the fuser re-picks on standardised scores, in which a "
                                               "bonus in log-prob units has no defined place)");
        const char* bad = lasr_bias::validate_form(beam, n_nodes, edge_off, edge_tok, edge_next, edge_val, node_back, c->d.vocab, c->d.blank);
        if (bad) return fail(c, LASR_EINVAL, "%s: %s", fn, bad);
    }
    RC(toggle_prologue(c, beam ? "slot %d holds a result that was not fetched: fetch it before the switch"
                               : "slot %d has %d unfetched token(s): fetch them before the switch"));
    lasr_ctx::Bias nb;
    if (n_nodes) {
        const std::vector<int32_t> img = lasr_bias::pack_block(n_nodes, edge_off, edge_tok, edge_next, edge_val, beam ? node_back : nullptr);
        nb.n_nodes = n_nodes; nb.n_edges = (size_t)edge_off[n_nodes]; nb.has_back = beam;
        const size_t rows = beam ? (size_t)c->Md : (size_t)c->M;
        auto stage = [&]() -> int {
            RC(upload(c, &nb.block, (const int*)img.data(), img.size()));
            if (!c->bias.node) RC(dalloc(c, &c->bias.node, rows));
            HIPCHK(c, hipMemset(c->bias.node, 0, sizeof(int) * rows));      // every slot starts over at the root
            return LASR_OK;
        };
        const int rc = stage();
        if (rc) { dfree(c, nb.block); return rc; }
    }
    std::lock_guard<std::mutex> lk(c->mu);
    dfree(c, c->bias.block);
    nb.node = c->bias.node;
    c->bias = nb;
    if (!beam) {            // (a beam's view is beam_state()'s)
        c->ds.bias = BiasEdges{};
        if (n_nodes) { c->ds.bias.node = nb.node; (void)lasr_bias::view_block(nb.block, nb.n_nodes, nb.n_edges, false, c->ds.bias); }
    }
    return LASR_OK;
}

int lasr_set_bias(lasr_ctx* c, int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_bonus) {
    if (!c) return LASR_EINVAL;
    if (c->W > 1)
        return fail(c, LASR_EINVAL, "lasr_set_bias serves greedy decode (beam = 1); beam search has lasr_set_beam_bias, where the bonus is "
                                    "part of the ranking score");
    return bias_attach(c, false, "lasr_set_bias", n_nodes, edge_off, edge_tok, edge_next, edge_bonus, nullptr);
}
int lasr_set_beam_bias(lasr_ctx* c, int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                       const float* edge_gain, const float* node_back) {
    if (!c) return LASR_EINVAL;
    if (c->W <= 1) return fail(c, LASR_EINVAL, "lasr_set_beam_bias serves beam search (beam > 1); greedy decode has lasr_set_bias");
    return bias_attach(c, true, "lasr_set_beam_bias", n_nodes, edge_off, edge_tok, edge_next, edge_gain, node_back);
}

// n words of the node row from row `at`, on the host (the caller has drained the streams)
static int read_bias_nodes(lasr_ctx* c, size_t at, int* out, size_t n) {
    HIPCHK(c, hipMemcpy(out, c->bias.node + at, sizeof(int) * n, hipMemcpyDeviceToHost));
    return LASR_OK;
}
// the start nodes an op-level call was handed: inside the attached graph
static int check_bias_nodes(lasr_ctx* c, const int32_t* node, size_t n) {
    for (size_t r = 0; r < n; ++r)
        if (node[r] < 0 || node[r] >= c->bias.n_nodes) return fail(c, LASR_EINVAL, "row %zu: node %d outside [0, %d)", r, node[r], c->bias.n_nodes);
    return LASR_OK;
}

int lasr_bias_state(lasr_ctx* c, const int* slots, int n, int32_t* nodes) {
    if (!c) return LASR_EINVAL;
    if (c->W > 1 || !bias_on(c)) return fail(c, LASR_ESTATE, "biasing is off: call lasr_set_bias first");
    RC(drain(c));
    RC(check_slots(c, slots, n, true));
    if (n == 0) return LASR_OK;
    if (!nodes) return fail(c, LASR_EINVAL, "null argument");
    std::vector<int> all((size_t)c->M);
    RC(read_bias_nodes(c, 0, all.data(), all.size()));
    for (int i = 0; i < n; ++i) nodes[i] = all[slots[i]];
    return LASR_OK;
}

int lasr_beam_bias_state(lasr_ctx* c, int slot, int32_t* nodes) {
    if (!c) return LASR_EINVAL;
    if (c->W <= 1) return fail(c, LASR_EINVAL, "lasr_beam_bias_state serves beam search (beam > 1); greedy decode has lasr_bias_state");
    if (!bias_on(c)) return fail(c, LASR_ESTATE, "beam biasing is off: call lasr_set_beam_bias first");
    RC(drain(c));
    RC(open_slot(c, slot));
    if (!nodes) return fail(c, LASR_EINVAL, "null argument");
    std::vector<int> al((size_t)c->W);
    RC(read_bias_nodes(c, (size_t)slot * c->W, nodes, al.size()));
    HIPCHK(c, hipMemcpy(al.data(), c->b_alive + (size_t)slot * c->W, sizeof(int) * al.size(), hipMemcpyDeviceToHost));
    for (int j = 0; j < c->W; ++j) if (!al[j]) nodes[j] = -1;      // (a dead slot has no node)
    return LASR_OK;
}

// one biased selection round on the caller's logits and slot state with the attached graph: the decode loop's own
// k_beam_select_rw<WT, true, false, true> on a scratch BeamState (synchronous form, round slot 0) -- no slot's state is read or written
int lasr_beam_bias_round(lasr_ctx* c, const float* logits, int n, const double* score, const int32_t* alive, const int32_t* inB,
                         const int32_t* node, const int32_t* rounds, int max_iters, int32_t* parent, int32_t* token, int32_t* emit,
                         double* score_out, int32_t* alive_out, int32_t* inB_out, int32_t* node_out, float* term) {
    if (!c) return LASR_EINVAL;
    if (c->W <= 1) return fail(c, LASR_EINVAL, "lasr_beam_bias_round serves beam search (beam > 1); greedy decode has lasr_bias_pick");
    if (!logits || !score || !alive || !inB || !node || !rounds || !parent || !token || !emit || !score_out || !alive_out || !inB_out ||
        !node_out || !term || n < 1 || n > c->d.max_streams || max_iters < 1)
        return fail(c, LASR_EINVAL, "bad argument");
    if (!bias_on(c)) return fail(c, LASR_ESTATE, "beam biasing is off: call lasr_set_beam_bias first");
    const int W = c->W, M = c->M;
    const size_t Md = (size_t)c->Md, nW = (size_t)n * W;
    RC(check_bias_nodes(c, node, nW));
    for (int q = 0; q < n; ++q)
        if (rounds[q] < 0) return fail(c, LASR_EINVAL, "stream %d: %d rounds done", q, rounds[q]);
    RC(flush_lazy(c));
    RC(require_idle(c));
    HIPCHK(c, hipSetDevice(c->device));
    // scratch: [Md] doubles (score), then int rows: alive, inB, node, token, emit, parent, trellis [Md each], rec [2 Md],
    // iters, t_idx, T_row [M each], unfinished [1]
    const size_t n_int = 9 * Md + 3 * (size_t)M + 1;
    if (!c->bias_round_dev) RC(dalloc(c, &c->bias_round_dev, Md + (n_int + 1) / 2));
    static_assert(sizeof(BeamRec) == 2 * sizeof(int), "BeamRec is two words");
    double* d_sc = c->bias_round_dev;
    int* d_i = (int*)(d_sc + Md);
    std::vector<double> h_sc(Md, -INFINITY);
    std::vector<int> h_i(n_int, 0);
    std::copy(score, score + nW, h_sc.begin());
    for (size_t r = 0; r < nW; ++r) { h_i[r] = alive[r] ? 1 : 0; h_i[Md + r] = inB[r] ? 1 : 0; h_i[2 * Md + r] = node[r]; }
    for (int q = 0; q < n; ++q) { h_i[9 * Md + q] = rounds[q]; h_i[9 * Md + 2 * (size_t)M + q] = 1; }      // (t_idx 0, T_row 1: one frame to decode)
    HIPCHK(c, hipMemcpyAsync(d_sc, h_sc.data(), sizeof(double) * Md, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_i, h_i.data(), sizeof(int) * n_int, hipMemcpyHostToDevice, c->stream));
    DecView v = sync_view(c, c->la_sync);
    BeamState b = beam_state(c, v, false, max_iters);
    b.score = d_sc; b.alive = d_i; b.inB = d_i + Md; b.bias.node = d_i + 2 * Md; b.token = d_i + 3 * Md; b.emit = d_i + 4 * Md;
    b.parent = d_i + 5 * Md; b.trellis = d_i + 6 * Md; b.rec = (BeamRec*)(d_i + 7 * Md);
    b.iters = d_i + 9 * Md; b.t_idx = d_i + 9 * Md + M; b.T_row = d_i + 9 * Md + 2 * (size_t)M; b.unfinished = d_i + 9 * Md + 3 * (size_t)M;
    b.seq_hash = nullptr; b.seq_len = nullptr; b.dbg = nullptr;
    b.lm_on = 0; b.done2 = nullptr;
    with_const<2, 4, 8>(W, [&](auto wt) {
        constexpr int WT = decltype(wt)::value;
        hipLaunchKernelGGL((k_beam_select_rw<WT, true, false, true>), dim3(n), dim3(64 * WT), 0, c->stream, logits, b, 0);      // (n workgroups: the caller's logits end there)
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_sc.data(), d_sc, sizeof(double) * Md, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_i.data(), d_i, sizeof(int) * n_int, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t r = 0; r < nW; ++r) {
        score_out[r] = h_sc[r]; alive_out[r] = h_i[r]; inB_out[r] = h_i[Md + r]; node_out[r] = h_i[2 * Md + r];
        emit[r] = h_i[4 * Md + r]; parent[r] = h_i[5 * Md + r];
        token[r] = emit[r] ? h_i[3 * Md + r] : -1;
        float tm = 0.f;
        if (emit[r]) memcpy(&tm, &h_i[7 * Md + 2 * r + 1], sizeof(float));
        term[r] = tm;
    }
    return LASR_OK;
}

// ---------------------------------------------------------------------------- beam: per-token records and the whole beam
// k_beam_select_rw<WT, true> stores, beside the trellis word of every slot it extends by a non-blank token, the frame cursor and the
// f32 term it added to the parent's score (BeamState::rec; null = off, the default: the <WT, false> instantiation).  Toggling
// changes which kernel the decode launches run and what the host keeps per node, so the engine must be idle, and the cached groups
// of the pipelined protocol (BeamState is captured by value) are dropped.
int lasr_set_beam_records(lasr_ctx* c, int on) {
    if (!c) return LASR_EINVAL;
    if (c->W <= 1) return fail(c, LASR_EINVAL, "beam records serve beam search (beam > 1); greedy decode has lasr_set_alignments");
    const bool want = on != 0;
    if (want == c->beam_rec_on) return LASR_OK;       // (nothing to switch: also fine while steps are in flight)
    RC(toggle_prologue(c, "slot %d holds a result that was not fetched: fetch it before the switch"));
    if (want && !c->b_rec_ring_host) {
        const size_t n = (size_t)lasr_ctx::TRING * c->Md;
        HIPCHK(c, hipHostMalloc((void**)&c->b_rec_ring_host, sizeof(BeamRec) * n));
        memset(c->b_rec_ring_host, 0, sizeof(BeamRec) * n);
        void* dp = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(&dp, c->b_rec_ring_host, 0));
        c->b_rec_ring_dev = (BeamRec*)dp;
    }
    if (want) RC(alloc_beam_recs(c));                 // sized for the trellis as it is now (it may have grown while the switch was off)
    else free_beam_recs(c);
    std::lock_guard<std::mutex> lk(c->mu);
    c->beam_rec_on = want;
    for (auto& B : c->beams) B.set_records(want);
    return LASR_OK;
}

// ---------------------------------------------------------------------------- beam: merging of equal hypotheses
// k_beam_select_rw<WT, REC, true> keeps an identity per slot (BeamState::seq_hash / seq_len; null = off, the default: the
// <WT, REC, false> instantiation) and merges the survivors of a round that hold the same tokens.  Like the records
// switch this changes which kernel the decode launches run, so the engine must be idle and the cached groups are dropped.  At a
// switch-on in mid-stream the identities come from the host: the engine is idle, so every stream's tree holds every live slot's
// tokens since the frozen prefix (a dead slot, cur = -1, gets the empty identity like an empty list).  With an LM attached those
// are the re-picked tokens (k_beam_fuse patches the trellis), which is what LASR_BEAM_MERGE_LM chains its identities from.
int lasr_set_beam_merge(lasr_ctx* c, int on) {
    if (!c) return LASR_EINVAL;
    if (c->W <= 1) return fail(c, LASR_EINVAL, "beam merging serves beam search (beam > 1)");
    // three modes: 0 off, 1 on, LASR_BEAM_MERGE_LM on and also under LM fusion (k_beam_fuse_merge); any other value is 1
    const int want = on == 0 ? 0 : (on == LASR_BEAM_MERGE_LM ? LASR_BEAM_MERGE_LM : 1);
    if (want == c->beam_merge) return LASR_OK;        // (nothing to switch: also fine while steps are in flight)
    if (want == 1 && c->lm.on)
        return fail(c, LASR_ESTATE, "lasr_set_beam_merge(c, 1) refuses an attached LM (the identity of the selection round would be of the token "
                                    "k_beam_fuse re-picks afterwards): LASR_BEAM_MERGE_LM merges under LM fusion");
    RC(toggle_prologue(c, "slot %d holds a result that was not fetched: fetch it before the switch"));
    if (want && !c->beam_merge) {                     // (1 <-> LASR_BEAM_MERGE_LM: both modes keep the identities up to date)
        const size_t Md = (size_t)c->Md;
        if (!c->b_seq_hash) {
            RC(dalloc(c, &c->b_seq_hash, Md + (Md + 1) / 2));         // [Md] 64-bit hashes, then [Md] 32-bit lengths
            c->b_seq_len = (int*)(c->b_seq_hash + Md);
        }
        std::vector<unsigned long long> img(Md + (Md + 1) / 2, 0ull);
        int* len = (int*)(img.data() + Md);
        for (int r = 0; r < c->M; ++r) {
            const BeamHost& B = c->beams[r].tree;
            for (int j = 0; j < c->W; ++j) {
                std::vector<int32_t> toks;
                if (j < (int)B.cur.size()) bh_tokens(B, B.cur[j], toks);
                uint64_t h = BM_SEED;
                for (int32_t v : toks) h = bm_append(h, v);
                img[(size_t)r * c->W + j] = h; len[(size_t)r * c->W + j] = (int)toks.size();
            }
        }
        HIPCHK(c, hipMemcpy(c->b_seq_hash, img.data(), sizeof(unsigned long long) * img.size(), hipMemcpyHostToDevice));
    }
    std::lock_guard<std::mutex> lk(c->mu);
    c->beam_merge = want;                             // (off: the block stays; the scores stay what they are)
    return LASR_OK;
}

int lasr_fetch_nbest(lasr_ctx* c, int slot, int max_hyps, int32_t* tokens, int32_t* frames, float* logps, int cap, int* n_tokens,
                     double* scores, int* n_hyps) {
    if (!c || !n_hyps) return LASR_EINVAL;
    if (c->W <= 1) return fail(c, LASR_EINVAL, "lasr_fetch_nbest serves beam search (beam > 1)");
    if (!c->beam_rec_on) return fail(c, LASR_ESTATE, "beam records are off: call lasr_set_beam_records first");
    RC(open_slot(c, slot));
    if (max_hyps < 0 || cap < 0 || (max_hyps > 0 && (!tokens || !n_tokens || !scores))) return fail(c, LASR_EINVAL, "bad argument");
    const auto& nb = c->results[slot].nbest;
    const int take = std::min(max_hyps, (int)nb.size());
    bool full = false;
    for (int i = 0; i < take; ++i) full |= (int)nb[i].tokens.size() > cap;
    if (full) {
        int need = 0;
        for (int i = 0; i < take; ++i) { n_tokens[i] = (int)nb[i].tokens.size(); need = std::max(need, n_tokens[i]); }
        *n_hyps = (int)nb.size();
        return fail(c, LASR_EFULL, "token buffers too small: need %d per hypothesis", need);
    }
    for (int i = 0; i < take; ++i) {
        const size_t o = (size_t)i * cap;
        nb[i].copy_to(tokens + o, frames ? frames + o : nullptr, logps ? logps + o : nullptr);
        n_tokens[i] = (int)nb[i].tokens.size();
        scores[i] = nb[i].score;
    }
    *n_hyps = (int)nb.size();
    c->results[slot].clear();
    return LASR_OK;
}

// ---------------------------------------------------------------------------- op-level entry points
int lasr_logmel(lasr_ctx* c, const float* pcm, int B, int64_t N, float* logmel) {
    if (!c || !pcm || !logmel || B < 1 || B > c->M) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    if (N <= c->d.n_fft / 2) return fail(c, LASR_EINVAL, "signal shorter than the reflect padding");
    HIPCHK(c, hipSetDevice(c->device));
    const lasr_model_desc& d = c->d;
    const int T = 1 + (int)(N / d.hop);
    launch_logmel_offline(c, pcm, N, B, T, logmel);
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

int lasr_stack(lasr_ctx* c, const float* logmel, int B, int T, float* feats, int* Tp) {
    if (!c) return LASR_EINVAL;
    const lasr_model_desc& d = c->d;
    const int tp = T < d.n_stack ? 0 : (T - d.n_stack) / d.stride + 1;
    if (Tp) *Tp = tp;
    if (tp == 0) return LASR_OK;                       // fewer than n_stack frames: no stacked frame
    if (!logmel || !feats || B < 1) return fail(c, LASR_EINVAL, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_stack, dim3(tp, B), dim3(256), 0, c->stream, logmel, T, d.n_mels, d.n_stack, d.stride, feats, tp, d.feat);
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

int lasr_encoder(lasr_ctx* c, const float* feats, int B, int Tp, float* out, float* h_out, float* c_out) {
    if (!c || !feats || !out || B < 1 || B > c->d.max_streams || Tp < 1) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const lasr_model_desc& d = c->d;
    const int H = d.hidden;
    RC(ensure_T(c, Tp));
    RC(cmd_begin(c));
    for (int r = 0; r < B; ++r) { c->hc.T_row[r] = Tp; c->hc.what[r] = 1; c->hc.row_feat_off[r] = (long long)r * Tp; }
    RC(cmd_commit(c));
    RC(apply_reset(c, sync_view(c, c->la_sync), false));
    RC(commit_T_rows(c, Tp));
    stack_ln_feats(c, feats, c->dc.row_feat_off, c->T_row_dev, Tp);
    run_encoder(c, c->stream, c->pe_sync, false, Tp);
    hipLaunchKernelGGL(k_enc_out, dim3(grid1((size_t)B * Tp * H)), dim3(256), 0, c->stream,
                       (const void*)c->ybuf[(d.enc_layers - 1) & 1], c->Tcap * c->MT, c->M, out, B, Tp, H, c->bf);
    for (int l = 0; l < d.enc_layers; ++l) {
        if (h_out)
            hipLaunchKernelGGL(k_from_frag, dim3(grid1((size_t)B * H)), dim3(256), 0, c->stream,
                               (const void*)c->enc_h[c->enc_par][l], c->MT, 0, h_out + (size_t)l * B * H, H, B, H, c->bf);
        if (c_out)
            hipLaunchKernelGGL(k_c_to_rows, dim3(grid1((size_t)B * H)), dim3(256), 0, c->stream,
                               (const float*)c->enc_c[l], c->M, c_out + (size_t)l * B * H, B, H);
    }
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

int lasr_predictor(lasr_ctx* c, const int32_t* tok, int B, int U, float* out) {
    if (!c || !tok || !out || B < 1 || B > c->d.max_streams || U < 1) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const int H = c->d.hidden;
    for (int i = 0; i < B * U; ++i)
        if (tok[i] < 0 || tok[i] >= c->d.vocab) return fail(c, LASR_EINVAL, "token %d out of range", tok[i]);
    // learned initial state, no implicit BOS
    RC(cmd_begin(c));
    for (int r = 0; r < B; ++r) c->hc.what[r] = 2;
    RC(cmd_commit(c));
    DecView v = sync_view(c, c->la_sync);
    RC(apply_reset(c, v, false, 3, true));
    for (int u = 0; u < U; ++u) {
        RC(cmd_begin(c));
        for (int r = 0; r < B; ++r) { c->hc.token[r] = tok[(size_t)r * U + u]; c->hc.emit[r] = 1; }
        RC(cmd_commit(c));
        if (c->Md > c->M) HIPCHK(c, hipMemsetAsync(c->ds.emit, 0, sizeof(int) * c->Md, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ds.token, c->dc.token, sizeof(int) * c->M, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ds.emit, c->dc.emit, sizeof(int) * c->M, hipMemcpyDeviceToDevice, c->stream));
        launch_predictor(c, v);
    }
    c->pred_par = v.pred_par;
    hipLaunchKernelGGL(k_from_elem, dim3(grid1((size_t)B * H)), dim3(256), 0, c->stream, (const void*)c->pred_y[0][c->d.pred_layers - 1],
                       out, (size_t)B * H, c->bf);
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

int lasr_joint(lasr_ctx* c, const float* h_pred, const float* h_enc, int B, float* logits, float* logp_max, int32_t* argmax) {
    if (!c || !h_pred || !h_enc || !logits || B < 1 || B > c->d.max_streams) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const int H = c->d.hidden, J = c->d.joint, V = c->d.vocab;
    RC(ensure_T(c, 1));
    const DecView v = sync_view(c, c->la_sync);
    {   // pp = h_pred W1p^T + b1 ; pe[0] = h_enc W1e^T   (row-major A)
        const void* ap = h_pred; const void* ae = h_enc;
        if (c->bf) {   // bf16 operands: round the f32 inputs once
            hipLaunchKernelGGL(k_to_elem, dim3(grid1((size_t)B * H)), dim3(256), 0, c->stream, h_pred, c->cvt_a, (size_t)B * H, 1);
            hipLaunchKernelGGL(k_to_elem, dim3(grid1((size_t)B * H)), dim3(256), 0, c->stream, h_enc, c->cvt_b, (size_t)B * H, 1);
            ap = c->cvt_a; ae = c->cvt_b;
        }
        GemmArgs g{}; set_operand(g, 0, ap, H, 0, 0, c->W1p); g.a_rows = B;
        EpiLinear::Args ea{}; ea.bias = c->b1; ea.out = c->pp[0]; ea.ldo = J; ea.n_rows = B; ea.t_idx = nullptr; ea.T_row = nullptr; ea.M = c->M;
        launch_linear<true, 3>(c, v, J / 16, (B + 15) / 16, g, H, ea);
        g.A[0] = ae; g.W[0] = c->W1e; ea.bias = nullptr; ea.out = v.pe;
        launch_linear<true, 3>(c, v, J / 16, (B + 15) / 16, g, H, ea);
    }
    hipLaunchKernelGGL(k_ja, dim3(grid1((size_t)c->M * J)), dim3(256), 0, c->stream, (const float*)v.pe, (const float*)c->pp[0],
                       (const int*)nullptr, (const int*)nullptr, c->ja, J, c->M, c->MTj, 1 << 30, c->bf, 1, c->M, 1);
    launch_logits(c, v, logits, B, false);
    if (logp_max && argmax) {
        // the joint's own argmax, whatever graph is attached (lasr_bias_pick is the biased one)
        launch_select<true>(c->stream, B, logits, V, c->d.blank, 1, nullptr, c->ds, 0, logp_max, argmax, 1, c->M, false);
    }
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

// one biased decision per row on the caller's logits with the attached graph: k_select<PLAIN, 1, KEEP, BIAS> on a node row of
// its own -- no slot's state is read or written
int lasr_bias_pick(lasr_ctx* c, const float* logits, const int32_t* node, int B, int32_t* tok, int32_t* next, float* logp) {
    if (!c || !logits || !node || !tok || !next || !logp || B < 1 || B > c->d.max_streams) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    if (c->W > 1 || !bias_on(c)) return fail(c, LASR_ESTATE, "biasing is off: call lasr_set_bias first");
    RC(check_bias_nodes(c, node, (size_t)B));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t M = (size_t)c->M;
    if (!c->bias_pick_dev) RC(dalloc(c, &c->bias_pick_dev, 3 * M));      // [node -> next | tok | log p]
    int* nd = c->bias_pick_dev;
    HIPCHK(c, hipMemcpyAsync(nd, node, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, c->stream));
    DecState s = c->ds;
    s.bias.node = nd;
    launch_select<true>(c->stream, B, logits, c->d.vocab, c->d.blank, 1, nullptr, s, 0, (float*)(nd + 2 * M), nd + M, 1, c->M, true);
    HIPCHK(c, hipGetLastError());
    std::vector<int> out(3 * M);
    HIPCHK(c, hipMemcpyAsync(out.data(), nd, sizeof(int) * 3 * M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < B; ++r) { next[r] = out[r]; tok[r] = out[M + r]; memcpy(&logp[r], &out[2 * M + r], sizeof(float)); }
    return LASR_OK;
}

// ---------------------------------------------------------------------------- resampling
static long long resample_num_out(long long n_in, int sr_in, int sr_out) {     // kaldi GetNumOutputSamples(flush = true)
    long long a = sr_in, b = sr_out;
    while (b) { const long long t = a % b; a = b; b = t; }
    const long long tick = (long long)sr_in / a * sr_out;
    const long long ticks_in = tick / sr_in, ticks_out = tick / sr_out;
    const long long length = n_in * ticks_in;
    if (length <= 0) return 0;
    long long last = length / ticks_out;
    if (last * ticks_out == length) last -= 1;
    return last + 1;
}

// Generic client windows (any chunk length, any sample rate): what ASRServicer.TranscribeStream + x_tfm_stream do per call
// (api-server.py:83-115; transforms.py:141-144 Resample of the WHOLE window, :306-323 log-mel of the window with reflect
// padding, :335-342 frames T//3 + 1 .. + n_stack, :436-441 stack, :463-471 Buffer) for windows the caller has concatenated:
// pcm = [n][N] float32 (host or device) at `sr` Hz, one window per listed slot.  Synchronous protocol; the fast path
// (lasr_push_pcm + lasr_step_*) is the same computation specialised to 16 kHz / fixed chunks with the window kept on the GPU.
int lasr_step_window(lasr_ctx* c, const int* slots, int n, const float* pcm, int64_t N, int sr, int* n_ran) {
    if (!c) return LASR_EINVAL;
    if (n_ran) *n_ran = 0;
    RC(check_slots(c, slots, n, true));
    RC(flush_lazy(c));
    RC(require_idle(c));
    if (n == 0) return LASR_OK;
    if (!pcm || N < 1) return fail(c, LASR_EINVAL, "bad window");
    if (c->M > 512) return fail(c, LASR_EINVAL, "lasr_step_window supports up to 512 stream slots");
    HIPCHK(c, hipSetDevice(c->device));
    const lasr_model_desc& d = c->d;
    const float* src = nullptr;
    RC(stage_to_device(c, pcm, (size_t)n * N, &c->stage_pcm, &c->stage_pcm_floats, &src));
    long long Nw = N;
    if (sr != d.sample_rate) {                              // Resample.encodes on the whole window (transforms.py:141-144)
        int64_t No = 0;
        RC(lasr_resample(c, src, n, N, sr, nullptr, &No));
        RC(ensure_buf(c, &c->win_rs, &c->win_rs_floats, (size_t)n * No));
        RC(lasr_resample(c, src, n, N, sr, c->win_rs, &No));
        src = c->win_rs; Nw = No;
    }
    const int T = 1 + (int)(Nw / d.hop);
    const int a0 = T / 3 + 1;                               // StreamPostprocess (transforms.py:335-342)
    if (T - a0 < d.n_stack) return fail(c, LASR_EINVAL, "window of %lld samples at 16 kHz yields %d < n_stack frames after the cut", Nw, T - a0);
    if (Nw <= d.n_fft / 2) return fail(c, LASR_EINVAL, "window shorter than the reflect padding");
    for (int i = 0; i < n; ++i) {           // validate every slot BEFORE any state changes: an error leaves nothing half-done
        const int s = slots[i];
        for (int j = 0; j < c->n_pend[s]; ++j)
            if (c->fe_fused && !c->pend_mat[(size_t)s * d.n_buffer + j])
                return fail(c, LASR_ESTATE, "slot %d has frames pending from lasr_push_pcm steps: do not mix the two streaming forms", s);
    }
    RC(cmd_begin(c));
    std::vector<int> model_rows;
    MelArgs m{};
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        m.dst_row_v[i] = (short)s;
        m.sel_v[i] = (short)(c->n_pend[s] * d.n_stack);
        c->pend_mat[(size_t)s * d.n_buffer + c->n_pend[s]] = 1;
        c->pend_serial[(size_t)s * d.n_buffer + c->n_pend[s]] = c->n_chunks[s];
        frame_collected(c, s, model_rows);
    }
    RC(cmd_commit(c));
    rec(c, 0);
    launch_logmel_window(c, m, src, Nw, a0, n);
    if (model_rows.empty()) {
        HIPCHK(c, hipGetLastError());
        return LASR_OK;
    }
    const int Tm = d.n_buffer;
    RC(ensure_T(c, Tm));
    RC(commit_T_rows(c, Tm));
    stack_ln_logmel(c, c->pend, d.n_buffer * d.n_stack, d.n_stack, c->T_row_dev, Tm);
    encode_step(c, Tm);
    RC(decode_and_collect(c, Tm, d.max_iters_stream, false, model_rows));
    if (n_ran) *n_ran = (int)model_rows.size();
    return LASR_OK;
}

int lasr_resample(lasr_ctx* c, const float* pcm, int B, int64_t N_in, int sr_in, float* out, int64_t* N_out) {
    if (!c || !N_out) return LASR_EINVAL;
    const int sr_out = c->d.sample_rate;
    if (B < 1 || N_in < 1 || sr_in < 1000 || sr_in > 384000) return fail(c, LASR_EINVAL, "bad argument");
    *N_out = resample_num_out(N_in, sr_in, sr_out);
    if (!out) return LASR_OK;                          // size query
    if (!pcm) return fail(c, LASR_EINVAL, "pcm is null");
    HIPCHK(c, hipSetDevice(c->device));
    auto it = c->resamplers.find(sr_in);
    if (it == c->resamplers.end()) {
        // one windowed-sinc filter per output phase, float32 arithmetic like torchaudio 0.6.0's
        // compliance/kaldi.py::_get_LR_indices_and_weights (lowpass_filter_width = 6, cutoff = 0.99 * min(sr) / 2)
        long long a = sr_in, b = sr_out;
        while (b) { const long long t = a % b; a = b; b = t; }
        lasr_ctx::Resampler r;
        r.in_unit = (int)(sr_in / a); r.U = (int)(sr_out / a);
        const double cutoff = 0.99 * 0.5 * std::min(sr_in, sr_out);
        const float width = (float)(6.0 / (2.0 * cutoff));
        std::vector<float> lo(r.U), hi(r.U), ot(r.U);
        int taps = 0;
        for (int p = 0; p < r.U; ++p) {
            ot[p] = (float)p / (float)sr_out;
            lo[p] = std::ceil((ot[p] - width) * (float)sr_in);
            hi[p] = std::floor((ot[p] + width) * (float)sr_in);
            taps = std::max(taps, (int)(hi[p] - lo[p] + 1.f));
        }
        r.taps = taps;
        std::vector<int> first(r.U);
        std::vector<float> w((size_t)r.U * taps, 0.f);
        const float cw = (float)(2.0 * M_PI * cutoff / 6.0), cs = (float)(2.0 * M_PI * cutoff), pi = (float)M_PI;
        for (int p = 0; p < r.U; ++p) {
            first[p] = (int)lo[p];
            for (int j = 0; j < taps; ++j) {
                const float dt = (lo[p] + (float)j) / (float)sr_in - ot[p];
                float v = 0.f;
                if (std::fabs(dt) < width) v = 0.5f * (1.f + std::cos(cw * dt));
                if (dt != 0.f) v *= std::sin(cs * dt) / (pi * dt);
                else v *= (float)(2.0 * cutoff);
                w[(size_t)p * taps + j] = v / (float)sr_in;
            }
        }
        RC(upload(c, &r.first, first.data(), first.size()));
        RC(upload(c, &r.w, w.data(), w.size()));
        it = c->resamplers.emplace(sr_in, r).first;
    }
    const lasr_ctx::Resampler& r = it->second;
    hipLaunchKernelGGL(k_resample, dim3((unsigned)((*N_out + 255) / 256), B), dim3(256), 0, c->stream, pcm, (long long)N_in,
                       (const int*)r.first, (const float*)r.w, r.U, r.taps, r.in_unit, out, (long long)*N_out);
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

// ---------------------------------------------------------------------------- LM shallow fusion
size_t lasr_lm_weight_count(const lasr_lm_desc* d) {
    if (!d || d->vocab <= 0 || d->embed <= 0 || d->hidden <= 0 || d->layers < 1 || d->layers > 8) return 0;
    const size_t V = d->vocab, E = d->embed, H = d->hidden;
    size_t n = V * E;
    for (int l = 0; l < d->layers; ++l) n += 4 * H * (l == 0 ? E : H) + 4 * H * H + 8 * H;
    return n + V * H + V;
}

// The LM's own stream (see cont_enqueue), LASR_LM_SIDE=1 (default: the LM step in line on the decode stream): created when an
// LM is attached, on a hardware queue shared with neither the main nor the decode stream (probed like the decode stream at
// lasr_create; a stream that cannot be placed is given up).  Opt-in because what it buys depends on where the RUNTIME places the
// branches of the replayed group graph, which the probe does not control: the same build measured 32.7 against 30.7 k in line on
// one lease / process shape and 27.0 against 30.5 k on another (profiles/r04/r04_experiments.txt N).
static int lm_side_setup(lasr_ctx* c) {
    static const int on = getenv("LASR_LM_SIDE") ? atoi(getenv("LASR_LM_SIDE")) : 0;
    if (!on || !c->stream_dec || c->stream_lm) return LASR_OK;
    static const int pick = getenv("LASR_DEC_STREAM_PICK") ? atoi(getenv("LASR_DEC_STREAM_PICK")) : 1;
    std::vector<hipStream_t> rejected;
    bool ok = false;
    for (int attempt = 0; attempt < 8 && !ok; ++attempt) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream_lm, hipStreamNonBlocking));
        if (!pick) { ok = true; break; }
        double r0 = 0.0, r1 = 0.0;
        if (overlap_probe_impl(c, 300, &r0, c->stream, c->stream_lm) != LASR_OK ||
            overlap_probe_impl(c, 300, &r1, c->stream_dec, c->stream_lm) != LASR_OK) { (void)hipGetLastError(); break; }
        c->lm_stream_ratio[0] = r0; c->lm_stream_ratio[1] = r1;
        ok = r0 < 1.5 && r1 < 1.5;
        if (!ok) { rejected.push_back(c->stream_lm); c->stream_lm = nullptr; }
    }
    for (hipStream_t st : rejected) (void)hipStreamDestroy(st);
    if (!ok && c->stream_lm) { (void)hipStreamDestroy(c->stream_lm); c->stream_lm = nullptr; }
    if (c->stream_lm) {
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_lm_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_lm_join, hipEventDisableTiming));
    }
    if (getenv("LASR_VERBOSE"))
        fprintf(stderr, "[lasr] LM stream: %s, overlap probe %.2f (main) %.2f (decode)\n", c->stream_lm ? "own" : "in line",
                c->lm_stream_ratio[0], c->lm_stream_ratio[1]);
    return LASR_OK;
}

// What attaching an LM in either form starts with: the argument checks (q8: those of the int8-served form), an idle, synchronised
// context, and the fields of c->lm both forms share
static int lm_attach_begin(lasr_ctx* c, const lasr_lm_desc* d, const float* weights, size_t n_weights, bool q8) {
    if (!c) return LASR_EINVAL;
    if (c->lm.on) return fail(c, LASR_ESTATE, "an LM is already attached");
    if (bias_on(c))
        return fail(c, LASR_ESTATE, c->W > 1 ? "a beam bias graph is set (the combination with LM fusion is not served): lasr_set_beam_bias(c, 0, ...) first"
                                             : "a bias graph is set (the fuser re-picks on standardised scores, in which a bonus in log-prob units "
                                               "has no defined place): lasr_set_bias(c, 0, ...) first");
    if (c->beam_merge == 1) return fail(c, LASR_ESTATE, "beam merging is on in the mode that refuses an LM (lasr_set_beam_merge(c, 0) or (c, LASR_BEAM_MERGE_LM) first)");
    if (q8 && c->W > 1) return fail(c, LASR_ESTATE, "LM shallow fusion is implemented for greedy decoding (beam = 1)");
    if (!d || !weights || n_weights != lasr_lm_weight_count(d) || n_weights == 0)
        return fail(c, LASR_EINVAL, "LM weight blob has %zu floats, expected %zu", n_weights, d ? lasr_lm_weight_count(d) : (size_t)0);
    if (d->vocab != c->d.vocab) return fail(c, LASR_EINVAL, "LM vocabulary %d != model vocabulary %d", d->vocab, c->d.vocab);
    if (!q8) {
        if (d->vocab > 4096) return fail(c, LASR_EINVAL, "LM fusion keeps a row's log-probs in registers: vocab <= 4096");
        if (d->embed % 16 || d->hidden % (c->bf ? 32 : 16)) return fail(c, LASR_EINVAL, "LM dims must be multiples of 16 (hidden: 32 for bf16)");
    } else {
        if (d->vocab > 4096 || d->vocab % 16) return fail(c, LASR_EINVAL, "LM fusion keeps a row's log-probs in registers: vocab <= 4096, multiple of 16");
        if (d->hidden % 4 || d->hidden > 1024 || d->embed > 1024 || d->embed < 1 || d->layers < 1 || d->layers > 8)
            return fail(c, LASR_EINVAL, "int8 LM: hidden a multiple of 4, embed / hidden <= 1024 (exact integer accumulation), 1..8 layers");
    }
    RC(flush_lazy(c));
    RC(require_idle(c));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lasr_ctx::LM& m = c->lm;
    m.E = d->embed; m.H = d->hidden; m.L = d->layers; m.alpha = d->alpha; m.theta = d->theta; m.min_val = d->min_val;
    return LASR_OK;
}
// ... and ends with: the decode loop sees the LM
static int lm_attach_finish(lasr_ctx* c, bool q8) {
    lasr_ctx::LM& m = c->lm;
    drop_decode_graphs(c);                                              // decode groups change shape
    // (round 4: lookahead stays on with an LM -- blank frames change neither the predictor nor the LM state, k_select re-picks the
    //  token of the first non-blank frame of its window; LASR_LM_LOOKAHEAD=0 restores one frame per iteration)
    if (getenv("LASR_LM_LOOKAHEAD") && atoi(getenv("LASR_LM_LOOKAHEAD")) == 0) c->la_stream = c->la_offline = c->la_sync = 1;
    c->ds.lmz = m.lmz[0]; c->ds.lm_valid = m.valid[0]; c->ds.lm_alpha = m.alpha; c->ds.lm_theta = m.theta; c->ds.lm_min = m.min_val;
    m.q8 = q8;
    m.on = true;
    return lm_side_setup(c);
}

int lasr_attach_lm(lasr_ctx* c, const lasr_lm_desc* d, const float* weights, size_t n_weights) {
    RC(lm_attach_begin(c, d, weights, n_weights, false));
    lasr_ctx::LM& m = c->lm;
    const int V = d->vocab, E = d->embed, H = d->hidden, L = d->layers;
    const int M = c->Md;                               // LM rows: streams, or hypothesis slots with beam > 1 (Md = M x W)
    Reader rd{weights, n_weights};
    const float* embed = rd.take((size_t)V * E);
    m.cells.resize(L);
    std::vector<float> in0_w, in0_b;
    for (int l = 0; l < L; ++l) RC(load_lstm(c, rd, m.cells[l], l == 0 ? E : H, H, true, l == 0 ? &in0_w : nullptr, l == 0 ? &in0_b : nullptr));
    const float* wout = rd.take((size_t)V * H); const float* bout = rd.take(V);
    if (!bout || rd.left != 0) return fail(c, LASR_EINVAL, "LM weight blob layout mismatch");
    {
        Packed pk;
        pack_tiles(pk, c->bf, V / 16, H, [&](int t, int ui, int k) { return wout[(size_t)(16 * t + ui) * H + k]; });
        RC(upload_packed(c, &m.Wout, pk));
        RC(upload(c, &m.bout, bout, V));
        std::vector<float> one(H, 1.f), zero(H, 0.f);
        RC(upload(c, &m.ones, one.data(), H)); RC(upload(c, &m.zeros, zero.data(), H));
    }
    {   // layer-0 input table (exact f32, as for the predictor): tab[v] = embed[v] * W_ih0^T + (b_ih + b_hh)
        float* emb_dev = nullptr; void* wt = nullptr; float* bt = nullptr;
        RC(upload(c, &emb_dev, embed, (size_t)V * E));
        Packed pk;
        pack_tiles(pk, 0, 4 * H / 16, E, [&](int t, int ui, int k) { return in0_w[(size_t)(16 * t + ui) * E + k]; });
        RC(upload_packed(c, &wt, pk)); RC(upload(c, &bt, in0_b.data(), in0_b.size()));
        RC(dalloc(c, &m.cells[0].tab, (size_t)V * 4 * H));
        GemmArgs g{}; set_operand(g, 0, emb_dev, E, 0, E / 16, wt); g.a_rows = V;
        EpiLinear::Args ea{}; ea.bias = bt; ea.out = m.cells[0].tab; ea.ldo = 4 * H; ea.n_rows = V; ea.t_idx = nullptr; ea.T_row = nullptr; ea.M = M;
        launch_table_gemm_f32(c, sync_view(c, c->la_sync), 4 * H / 16, V / 16, g, ea);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        dfree(c, emb_dev); dfree(c, wt); dfree(c, bt);
        // the x-side weights of layer 0 are folded into the table; its packed copy is not needed
        dfree(c, m.cells[0].WxA); m.cells[0].WxA = nullptr;
    }
    for (int p = 0; p < 2; ++p) m.h[p].resize(L);
    for (int l = 0; l < L; ++l)
        for (int p = 0; p < 2; ++p) RC(dalloc0(c, (char**)&m.h[p][l], (size_t)M * H * c->esz));
    RC(dalloc(c, &m.raw, (size_t)M * V));
    for (int p = 0; p < (c->W > 1 ? 2 : 1); ++p) {     // beam: second parity of everything a re-parented slot inherits
        m.y[p].assign(L, nullptr); m.cst[p].assign(L, nullptr);
        for (int l = 0; l < L; ++l) {
            RC(dalloc0(c, (char**)&m.y[p][l], (size_t)M * H * c->esz));
            RC(dalloc0(c, &m.cst[p][l], (size_t)M * H));
        }
        RC(dalloc0(c, &m.lmz[p], (size_t)M * V)); RC(dalloc0(c, &m.valid[p], M));
    }
    return lm_attach_finish(c, false);
}

// The LM as the reference serves it: load_lm (lm.py:86-100) runs maybe_quantize (utils.py:197-210) =
// torch.quantization.quantize_dynamic({nn.LSTM, nn.Linear}, qint8) on it.  Same blob as lasr_attach_lm; the weights are
// quantised here (per tensor, symmetric: scale = max|w| / 127.5, q = clamp(rint(w * (1 / scale)), -128, 127)), activations per
// row and per matmul (at run time the quantised image of every h is made once, by the cell kernel that produces it: k_lm_cell_q).  Numerics of the installed torch's x86 / fbgemm engine (restated in
// oracle/rnnt_oracle.py:dq_linear and pinned to the reference's quantised LM there).
int lasr_attach_lm_int8(lasr_ctx* c, const lasr_lm_desc* d, const float* weights, size_t n_weights) {
    RC(lm_attach_begin(c, d, weights, n_weights, true));
    lasr_ctx::LM& m = c->lm;
    const int V = d->vocab, E = d->embed, H = d->hidden, L = d->layers, M = c->M;
    auto pad32 = [](int k) { return (k + 31) / 32 * 32; };
    m.Kp_h = pad32(H);
    Reader rd{weights, n_weights};
    const float* embed = rd.take((size_t)V * E);
    // one quantised matrix [N][K] -> integer-valued bf16 tiles (16 outputs x padded K), its scale
    auto quantise = [&](const float* w, int N, int K, void** dev, float* scale) -> int {
        float amax = 0.f;
        for (size_t i = 0; i < (size_t)N * K; ++i) amax = std::max(amax, std::fabs(w[i]));
        float sw = (float)((double)amax / 127.5);
        if (sw < 1.1920928955078125e-07f) sw = 1.1920928955078125e-07f;           // MinMaxObserver: scale >= eps
        const float inv = 1.0f / sw;
        const int Kp = pad32(K);
        Packed pk;
        pack_tiles(pk, 1, N / 16, Kp, [&](int t, int ui, int k) {
            if (k >= K) return 0.f;
            const float q = std::nearbyint(w[(size_t)(16 * t + ui) * K + k] * inv);
            return std::min(127.f, std::max(-128.f, q));
        });
        *scale = sw;
        return upload_packed(c, dev, pk);
    };
    m.cells.assign(L, Cell{});
    m.qWih.assign(L, nullptr); m.qWhh.assign(L, nullptr); m.s_ih.assign(L, 0.f); m.s_hh.assign(L, 0.f);
    m.b_ih.assign(L, nullptr); m.b_hh.assign(L, nullptr); m.Kp_ih.assign(L, 0);
    for (int l = 0; l < L; ++l) {
        const int I = l == 0 ? E : H;
        const float* wih = rd.take((size_t)4 * H * I); const float* whh = rd.take((size_t)4 * H * H);
        const float* bih = rd.take(4 * H); const float* bhh = rd.take(4 * H);
        if (!bhh) return fail(c, LASR_EINVAL, "LM weight blob too short");
        m.Kp_ih[l] = pad32(I);
        RC(quantise(wih, 4 * H, I, &m.qWih[l], &m.s_ih[l]));
        RC(quantise(whh, 4 * H, H, &m.qWhh[l], &m.s_hh[l]));
        RC(upload(c, &m.b_ih[l], bih, 4 * H)); RC(upload(c, &m.b_hh[l], bhh, 4 * H));
    }
    const float* wout = rd.take((size_t)V * H); const float* bout = rd.take(V);
    if (!bout || rd.left != 0) return fail(c, LASR_EINVAL, "LM weight blob layout mismatch");
    RC(quantise(wout, V, H, &m.qWout, &m.s_out));
    RC(upload(c, &m.bout, bout, V));
    const int Kmax = std::max(m.Kp_h, m.Kp_ih[0]);
    {   // layer-0 input table: tab[v] = linear_dynamic(embed[v]; W_ih0) + b_ih0 -- a pure function of the token, quantisation included
        float* emb_dev = nullptr; unsigned short* qa = nullptr; float* sx = nullptr;
        RC(upload(c, &emb_dev, embed, (size_t)V * E));
        RC(dalloc(c, &qa, (size_t)V * m.Kp_ih[0])); RC(dalloc(c, &sx, V));
        RC(dalloc(c, &m.cells[0].tab, (size_t)V * 4 * H));
        lm_q_gemv(c, sync_view(c, c->la_sync), emb_dev, E, E, m.Kp_ih[0], m.qWih[0], m.s_ih[0], m.b_ih[0], m.cells[0].tab, 4 * H, V, qa, sx);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        dfree(c, emb_dev); dfree(c, qa); dfree(c, sx);
    }
    for (int p = 0; p < 2; ++p) m.h[p].resize(L);
    m.y[0].assign(L, nullptr); m.cst[0].resize(L);
    for (int l = 0; l < L; ++l) {
        float* h = nullptr;
        RC(dalloc0(c, &h, (size_t)M * H));
        m.h[0][l] = m.h[1][l] = h;                              // row-local in-place update: no ping-pong
        RC(dalloc0(c, &m.cst[0][l], (size_t)M * H));
    }
    m.qh.assign(L, nullptr); m.sxh.assign(L, nullptr);
    {   // quantised image of h = 0: zeros with scale 0.1 (what ChooseQuantizationParams makes of an all-zero row)
        std::vector<float> tenth(M, 0.1f);
        for (int l = 0; l < L; ++l) {
            RC(dalloc0(c, &m.qh[l], (size_t)M * m.Kp_h));
            RC(upload(c, &m.sxh[l], tenth.data(), (size_t)M));
        }
    }
    RC(dalloc(c, &m.gx, (size_t)M * 4 * H)); RC(dalloc(c, &m.gh, (size_t)M * 4 * H));
    RC(dalloc(c, &m.qa, (size_t)M * Kmax)); RC(dalloc(c, &m.sx, M));
    RC(dalloc(c, &m.raw, (size_t)M * V)); RC(dalloc0(c, &m.lmz[0], (size_t)M * V)); RC(dalloc0(c, &m.valid[0], M));
    return lm_attach_finish(c, true);
}

// ---------------------------------------------------------------------------- stats / bench
int lasr_get_stats(lasr_ctx* c, lasr_step_stats* s) {
    if (!c || !s) return LASR_EINVAL;
    *s = c->stats;
    return LASR_OK;
}
int lasr_set_profiling(lasr_ctx* c, int on) {
    if (!c) return LASR_EINVAL;
    c->profiling = on != 0;
    return LASR_OK;
}
// debug: copy the phase timestamps of the last launch of each GEMM kind (cell, pred0, pred1, ppj, logits)
int lasr_debug_timing(lasr_ctx* c, unsigned long long* out /*[5*4096*8]*/) {
    if (!c || !out) return LASR_EINVAL;
    if (!c->dbg) return fail(c, LASR_ESTATE, "set LASR_DBG_TIMING=1 before lasr_create");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->dbg, sizeof(unsigned long long) * 5 * 4096 * 16, hipMemcpyDeviceToHost));
    return LASR_OK;
}

// debug (LASR_DBG_ENCLOG=N at create): the checksum log of the first N model steps since create or the last read; see lasr_debug.h
int lasr_debug_enclog(lasr_ctx* c, unsigned* out, size_t cap, int* steps) {
    if (!c || !steps) return LASR_EINVAL;
    if (!c->enclog) return fail(c, LASR_ESTATE, "set LASR_DBG_ENCLOG=<steps> before lasr_create");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)c->enclog_n * 32 * c->M;
    *steps = c->enclog_n;
    if (n > cap) return fail(c, LASR_EFULL, "checksum log needs %zu words", n);
    if (n && out) HIPCHK(c, hipMemcpy(out, c->enclog, sizeof(unsigned) * n, hipMemcpyDeviceToHost));
    c->enclog_n = 0;
    return LASR_OK;
}

// debug: see lasr_debug.h.  The streaming front-end's log-mel launch (k_fe_mel) back to back on the main stream over the resident PCM
// ring, each launch followed by per-row checksums of its output, while the decode stream runs `aggressor` in a loop.
int lasr_debug_fe_race(lasr_ctx* c, int iters, int aggressor, int per_iter, int lds_pad, int* bad_launches, int* bad_rows) {
    if (!c || !bad_launches || !bad_rows || iters < 1) return LASR_EINVAL;
    *bad_launches = *bad_rows = 0;
    if (lds_pad < 0) lds_pad = c->fe_lds_pad;
    if (lds_pad > 160 * 1024 - 48 * 1024) return fail(c, LASR_EINVAL, "lds_pad too large");
    RC(flush_lazy(c));
    RC(require_idle(c));
    if (!c->fe_fused || !c->stream_dec || c->M > 512) return fail(c, LASR_ESTATE, "the race probe needs the fused front-end and the decode stream");
    HIPCHK(c, hipSetDevice(c->device));
    const lasr_model_desc& d = c->d;
    // (outputs go to scratch buffers: the slots' pending frames and the step's frame counts stay as they are)
    const size_t n_pend = (size_t)c->M * d.n_buffer * d.n_stack * d.n_mels;
    float* pend_x = nullptr; int* trow_x = nullptr;
    RC(dalloc(c, &pend_x, n_pend));
    RC(dalloc(c, &trow_x, (size_t)c->M));
    FeMelArgs m{};
    fill_fe_mel_args(c, m, pend_x);
    m.trow_out = trow_x;
    for (int r = 0; r < c->M; ++r) {
        m.tp_pk[r] = (unsigned char)((c->h_ring_pos[r] << 4) | d.n_buffer);
        unsigned pk = 0;
        for (int j = 0; j < d.n_buffer; ++j) pk |= (unsigned)(d.n_buffer - 1 - j) << (4 * j);
        m.age_pk[r] = (unsigned short)pk;
    }
    unsigned* log = nullptr;
    RC(dalloc(c, &log, (size_t)(iters + 1) * c->M));
    RowSumArgs ra{};
    ra.s[0] = RowSumSrc{pend_x, 2, 0, 0, d.n_buffer * d.n_stack * d.n_mels};
    DecView av = sync_view(c, c->la_sync);          // the aggressor's view: thrown away, the context's parities stay where they were
    av.stream = c->stream_dec;
    auto aggress = [&]() {
        if (aggressor == 1) launch_logits(c, av, c->logits, c->Md, false);
        else if (aggressor == 2) launch_predictor(c, av, c->W > 1);
        else if (aggressor == 3) launch_ppj(c, av, c->W > 1);
    };
    for (int i = 0; i <= iters; ++i) {
        if (i > 0) for (int q = 0; q < per_iter; ++q) aggress();
        hipLaunchKernelGGL((k_fe_mel<10>), dim3(2 * d.n_buffer, c->M), dim3(320), lds_pad, c->stream, m);
        hipLaunchKernelGGL(k_dbg_rowsum, dim3(c->M, 1), dim3(256), 0, c->stream, ra, c->M, c->bf, log + (size_t)i * c->M);
        if (i == 0) HIPCHK(c, hipStreamSynchronize(c->stream));       // the reference launch runs alone
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream_dec));
    std::vector<unsigned> h((size_t)(iters + 1) * c->M);
    hipError_t e = hipMemcpy(h.data(), log, sizeof(unsigned) * h.size(), hipMemcpyDeviceToHost);
    dfree(c, log); dfree(c, pend_x); dfree(c, trow_x);
    if (e != hipSuccess) return fail(c, LASR_EHIP, "race probe copy failed: %s", hipGetErrorString(e));
    for (int i = 1; i <= iters; ++i) {
        int nb = 0;
        for (int r = 0; r < c->M; ++r) nb += h[(size_t)i * c->M + r] != h[r];
        *bad_rows += nb;
        *bad_launches += nb != 0;
    }
    return LASR_OK;
}

// In-job timing of the dominant kernel: while on, every model step's encoder-cell sequence (enc_layers x frames
// back-to-back launches of k_gemm<EpiLSTM>) is bracketed by a HIP-event pair on the ctx stream.  lasr_cell_prof_read
// drains the outstanding pairs and returns the accumulated microseconds / cell launches since the last on-switch.
int lasr_cell_prof(lasr_ctx* c, int on) {
    if (!c) return LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    // on = 1: HIP-event pairs + in-kernel clocks; on = 2: in-kernel clocks only (an event record between two kernels
    // costs the stream a bubble of several microseconds: twice per model step in mode 1)
    c->cell_prof_events = on == 1 || on == 3;
    if ((on == 1 || on == 3) && !c->cp_ok) {
        for (auto& p : c->cp_ev)
            for (auto& e : p) HIPCHK(c, hipEventCreate(&e));
        c->cp_ok = true;
    }
    if (on) { cell_prof_harvest(c, true); c->cp_us = 0.0; c->cp_launches = 0; }
    if (on == 3) { dfree(c, c->cp_slots); c->cp_slots = nullptr; c->cp_slot_next = 0; }      // events only: the cells stay graph-replayable
    if (on && on != 3) {
        const size_t half = (size_t)PROF_W * lasr_ctx::NCELLSLOT;
        if (!c->cp_slots) {
            RC(dalloc(c, &c->cp_slots, 2 * half));
            int khz = 0;
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0) c->cp_clock_mhz = khz / 1e3;
            else (void)hipGetLastError();
        }
        HIPCHK(c, hipMemset(c->cp_slots, 0xff, half * sizeof(unsigned long long)));            // entry clocks: ~0 = not written
        HIPCHK(c, hipMemset(c->cp_slots + half, 0, half * sizeof(unsigned long long)));         // exit clocks
        c->cp_slot_next = 0;
        c->cp_slot_cells.assign(lasr_ctx::NCELLSLOT, 0);
    }
    c->cell_prof = on != 0;
    return LASR_OK;
}
// the cell kernels' own durations since lasr_cell_prof(c, 1): per launch, max exit - min entry of the device's constant
// wall clock over the kernel's workgroups (comparable with a kernel trace's duration column)
int lasr_cell_prof_kernel(lasr_ctx* c, double* us_total, long long* launches, long long* cells) {
    if (!c || !us_total || !launches) return LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    *us_total = 0.0; *launches = 0;
    if (cells) *cells = 0;
    if (!c->cp_slots || c->cp_slot_next == 0) return LASR_OK;
    HIPCHK(c, hipDeviceSynchronize());
    const size_t half = (size_t)PROF_W * lasr_ctx::NCELLSLOT, used = (size_t)PROF_W * c->cp_slot_next;
    std::vector<unsigned long long> he(used), hx(used);
    HIPCHK(c, hipMemcpy(he.data(), c->cp_slots, used * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hx.data(), c->cp_slots + half, used * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (long long i = 0; i < c->cp_slot_next; ++i) {
        unsigned long long lo = ~0ull, hi = 0ull;
        for (int w = 0; w < PROF_W; ++w) {
            lo = std::min(lo, he[(size_t)i * PROF_W + w]);
            hi = std::max(hi, hx[(size_t)i * PROF_W + w]);
        }
        if (lo == ~0ull || hi < lo) continue;
        *us_total += (double)(hi - lo) / c->cp_clock_mhz;
        *launches += 1;
        if (cells) *cells += c->cp_slot_cells[i];
    }
    return LASR_OK;
}
int lasr_cell_prof_read(lasr_ctx* c, double* us_total, long long* launches) {
    if (!c || !us_total || !launches) return LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    cell_prof_harvest(c, true);
    *us_total = c->cp_us; *launches = c->cp_launches;
    return LASR_OK;
}

// Stream timeline of the pipelined protocol: while on, timestamped marks (HIP events) are recorded on the main stream
// (1 push, 3 first cell, 4 last cell done, 5 model step enqueued) and on the decode stream (10 group reached,
// 11 + 100 G [+ 1000 if steps were admitted] admission done, 12 group done).  lasr_trace_read synchronises and
// returns the marks in record order with their time in microseconds since lasr_trace(on).
int lasr_trace(lasr_ctx* c, int on) {
    if (!c) return LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (on && c->tr_ev.empty()) {
        c->tr_ev.resize(lasr_ctx::NTRACE); c->tr_tag.assign(lasr_ctx::NTRACE, 0); c->tr_val.assign(lasr_ctx::NTRACE, 0.0);
        for (auto& e : c->tr_ev) HIPCHK(c, hipEventCreate(&e));
        HIPCHK(c, hipEventCreate(&c->tr_base));
    }
    if (on) {
        c->tr_n = 0;
        HIPCHK(c, hipEventRecord(c->tr_base, c->stream));
        c->tr_prev_cur = c->h_cur_seen;
        c->tr_prev_ntot.assign(c->M, 0);        // the first group after the switch reports a bogus token delta
    }
    c->tr_on = on != 0;
    return LASR_OK;
}
int lasr_trace_read(lasr_ctx* c, double* us, int* tags, int cap, int* n) {
    if (!c || !us || !tags || !n) return LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    *n = 0;
    const int n_marks = std::min(c->tr_n.load(), (int)lasr_ctx::NTRACE);
    for (int i = 0; i < n_marks && i < cap; ++i) {
        float ms = 0.f;
        tags[i] = c->tr_tag[i];
        if (tags[i] == 20) { us[i] = c->tr_val[i]; *n = i + 1; continue; }      // value record
        if (hipEventElapsedTime(&ms, c->tr_base, c->tr_ev[i]) != hipSuccess) { (void)hipGetLastError(); ms = -1.f; }
        us[i] = 1e3 * (double)ms;
        *n = i + 1;
    }
    return LASR_OK;
}

// Debug / test read-out of the resident state (synchronises the ctx stream and the decode stream): [rows][K] row-major f32
// into `out` (host).  what: 0 x0 (LayerNorm'ed features) of frame `index`; 1 enc_h / 2 enc_c of layer `index` (current
// parity); 3 pe (joint encoder half, synchronous buffer) of frame `index`; 4 pp; 5 pred_h of layer `index` (current parity,
// decoder rows); 6 PCM ring [M][ring_chunks * chunk]; 7 pending log-mel frames [M][n_buffer * n_stack * n_mels];
// 8 last encoder layer's output of frame `index`; 9 integers as floats [8][M]: ring_pos, host ring mirror, n_chunks,
// n_pend, T_row_fix, t_idx, token, emit; 11..18 the attached LM's state (lasr_debug.h).  *rows / *cols (optional) describe the
// matrix; cap = floats `out` holds.
int lasr_debug_read(lasr_ctx* c, int what, int index, float* out, size_t cap, int* rows, int* cols) {
    if (!c || !out) return LASR_EINVAL;
    RC(drain(c, false));
    const lasr_model_desc& d = c->d;
    const int M = c->M, H = d.hidden, F = d.feat, J = d.joint;
    int R = M, K = 0;
    const int mt_total = c->Tcap * c->MT;
    enum { FRAG, ROWMAJ_ELEM, ROWMAJ_F32, UNITMAJ, INTS, INT_ROW, LM_SXH } kind = ROWMAJ_F32;
    const void* src = nullptr; int frag_mt_total = 0, frag_mt_off = 0;
    int elem_bf = c->bf, unit_ld = M;      // element type of a ROWMAJ_ELEM source; row count of a UNITMAJ source
    // the LM's rows (11..18): streams, or hypothesis slots with a beam, at the parity the context holds (see lasr_debug.h)
    const lasr_ctx::LM& lm = c->lm;
    const bool lm_beam = c->W > 1;
    if (what >= 11 && what <= 18) {
        if (!lm.on) return fail(c, LASR_ESTATE, "no LM attached");
        if ((what == 17 || what == 18) && !lm.q8) return fail(c, LASR_ESTATE, "the quantised image of h exists in the int8-served form only");
        if ((what == 11 || what == 12 || what == 17) && (index < 0 || index >= lm.L)) return fail(c, LASR_EINVAL, "layer out of range");
    }
    switch (what) {
        case 0: if (index < 0 || index >= c->Tcap) return fail(c, LASR_EINVAL, "frame out of range");
                kind = FRAG; src = c->x0; K = F; frag_mt_total = mt_total; frag_mt_off = index * c->MT; break;
        case 1: if (index < 0 || index >= d.enc_layers) return fail(c, LASR_EINVAL, "layer out of range");
                kind = FRAG; src = c->enc_h[c->enc_par][index]; K = H; frag_mt_total = c->MT; frag_mt_off = 0; break;
        case 2: if (index < 0 || index >= d.enc_layers) return fail(c, LASR_EINVAL, "layer out of range");
                kind = UNITMAJ; src = c->enc_c[index]; K = H; break;
        case 3: if (index < 0 || index >= c->Tcap) return fail(c, LASR_EINVAL, "frame out of range");
                kind = ROWMAJ_F32; src = c->pe_sync + (size_t)index * M * J; K = J; break;
        case 4: kind = ROWMAJ_F32; src = cur_pp(c); K = J; R = c->Md; break;
        case 5: if (index < 0 || index >= d.pred_layers) return fail(c, LASR_EINVAL, "layer out of range");
                kind = ROWMAJ_ELEM; src = c->pred_h[c->pred_par][index]; K = H; R = c->Md; break;
        case 6: kind = ROWMAJ_F32; src = c->win; K = c->ring_chunks * d.chunk; break;
        case 7: kind = ROWMAJ_F32; src = c->pend; K = d.n_buffer * d.n_stack * d.n_mels; break;
        case 8: if (index < 0 || index >= c->Tcap) return fail(c, LASR_EINVAL, "frame out of range");
                kind = FRAG; src = c->ybuf[(d.enc_layers - 1) & 1]; K = H; frag_mt_total = mt_total; frag_mt_off = index * c->MT; break;
        case 9: kind = INTS; R = 8; K = M; break;
        case 10: if (!c->pendlog || index < 0 || index >= c->enclog_cap) return fail(c, LASR_EINVAL, "no pending-frame log (LASR_DBG_ENCLOG + LASR_DBG_PENDLOG) or step out of range");
                kind = ROWMAJ_F32; K = d.n_buffer * d.n_stack * d.n_mels; src = c->pendlog + (size_t)index * M * K; break;
        case 11: R = c->Md; K = lm.H; src = lm.h[lm.q8 ? 0 : lm.par][index];
                 if (lm.q8) kind = ROWMAJ_F32; else kind = ROWMAJ_ELEM;
                 break;
        case 12: kind = UNITMAJ; R = c->Md; K = lm.H; unit_ld = R; src = lm.cst[par_rd(lm_beam, lm.par)][index]; break;
        case 13: kind = ROWMAJ_F32; R = c->Md; K = d.vocab; src = lm.raw; break;
        case 14: kind = ROWMAJ_F32; R = c->Md; K = d.vocab; src = lm.lmz[par_rd(lm_beam, lm.par)]; break;
        case 15: kind = INT_ROW; R = 1; K = c->Md; src = lm.valid[par_rd(lm_beam, lm.par)]; break;
        case 16: kind = ROWMAJ_F32; R = d.vocab; K = 4 * lm.H; src = lm.cells[0].tab; break;
        case 17: kind = ROWMAJ_ELEM; elem_bf = 1; K = lm.Kp_h; src = lm.qh[index]; break;
        case 18: kind = LM_SXH; R = lm.L; K = M; break;
        default: return fail(c, LASR_EINVAL, "unknown debug read %d", what);
    }
    if (rows) *rows = R;
    if (cols) *cols = K;
    if ((size_t)R * K > cap) return fail(c, LASR_EFULL, "debug read needs %zu floats", (size_t)R * K);
    if (kind == INTS) {
        std::vector<int> tmp(M);
        auto put = [&](int row, const int* v) { for (int r = 0; r < M; ++r) out[(size_t)row * M + r] = (float)v[r]; };
        HIPCHK(c, hipMemcpy(tmp.data(), c->ring_pos, sizeof(int) * M, hipMemcpyDeviceToHost)); put(0, tmp.data());
        put(1, c->h_ring_pos.data()); put(2, c->n_chunks.data()); put(3, c->n_pend.data());
        HIPCHK(c, hipMemcpy(tmp.data(), c->T_row_fix, sizeof(int) * M, hipMemcpyDeviceToHost)); put(4, tmp.data());
        HIPCHK(c, hipMemcpy(tmp.data(), c->ds.t_idx, sizeof(int) * M, hipMemcpyDeviceToHost)); put(5, tmp.data());
        HIPCHK(c, hipMemcpy(tmp.data(), c->ds.token, sizeof(int) * M, hipMemcpyDeviceToHost)); put(6, tmp.data());
        HIPCHK(c, hipMemcpy(tmp.data(), c->ds.emit, sizeof(int) * M, hipMemcpyDeviceToHost)); put(7, tmp.data());
        return LASR_OK;
    }
    if (kind == ROWMAJ_F32) {
        HIPCHK(c, hipMemcpy(out, src, sizeof(float) * (size_t)R * K, hipMemcpyDeviceToHost));
        return LASR_OK;
    }
    if (kind == INT_ROW) {
        std::vector<int> tmp(K);
        HIPCHK(c, hipMemcpy(tmp.data(), src, sizeof(int) * (size_t)K, hipMemcpyDeviceToHost));
        for (int r = 0; r < K; ++r) out[r] = (float)tmp[r];
        return LASR_OK;
    }
    if (kind == LM_SXH) {
        for (int l = 0; l < R; ++l) HIPCHK(c, hipMemcpy(out + (size_t)l * K, lm.sxh[l], sizeof(float) * (size_t)K, hipMemcpyDeviceToHost));
        return LASR_OK;
    }
    float* tmp = nullptr;
    RC(dalloc(c, &tmp, (size_t)R * K));
    if (kind == FRAG)
        hipLaunchKernelGGL(k_from_frag, dim3(grid1((size_t)R * K)), dim3(256), 0, c->stream, src, frag_mt_total, frag_mt_off, tmp, K, R, K, c->bf);
    else if (kind == ROWMAJ_ELEM)
        hipLaunchKernelGGL(k_from_elem, dim3(grid1((size_t)R * K)), dim3(256), 0, c->stream, src, tmp, (size_t)R * K, elem_bf);
    else
        hipLaunchKernelGGL(k_c_to_rows, dim3(grid1((size_t)R * K)), dim3(256), 0, c->stream, (const float*)src, unit_ld, tmp, R, K);
    hipError_t e = hipMemcpy(out, tmp, sizeof(float) * (size_t)R * K, hipMemcpyDeviceToHost);
    dfree(c, tmp);
    if (e != hipSuccess) return fail(c, LASR_EHIP, "debug read copy failed: %s", hipGetErrorString(e));
    return LASR_OK;
}

int lasr_sync(lasr_ctx* c) {
    if (!c) return LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    RC(flush_lazy(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cmd_inflight = 0;
    return LASR_OK;
}

// Do the two streams of the pipelined protocol (the ctx stream and the decode stream) run CONCURRENTLY on this process's
// hardware queues?  One wave per stream holds its stream for delay_us; *ratio = wall time / delay_us: ~1 when the streams
// overlap, ~2 when the runtime has mapped both onto one hardware queue (seen with an eagerly initialised RCCL communicator:
// the job then runs at 0.74 of its rate, profiles/r03/r03_experiments.txt M).  bench.py reports it per rank.
int lasr_overlap_probe(lasr_ctx* c, int delay_us, double* ratio) {
    if (!c || !ratio || delay_us < 1 || delay_us > 1000000) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    RC(flush_lazy(c));
    RC(require_idle(c));
    HIPCHK(c, hipSetDevice(c->device));
    return overlap_probe_impl(c, delay_us, ratio);
}
static int overlap_probe_impl(lasr_ctx* c, int delay_us, double* ratio, hipStream_t sa, hipStream_t sb) {
    if (!sb) { sa = c->stream; sb = c->stream_dec; }
    hipEvent_t e0, e1, e2;
    HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1)); HIPCHK(c, hipEventCreate(&e2));
    const unsigned long long ticks = (unsigned long long)delay_us * 100ull;      // 100 MHz wall clock
    for (int rep = 0; rep < 2; ++rep) {                                            // (first pass: code object load, queue creation)
        HIPCHK(c, hipEventRecord(e0, sa));
        HIPCHK(c, hipStreamWaitEvent(sb, e0, 0));
        hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, sa, rep ? ticks : 100ull);
        hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, sb, rep ? ticks : 100ull);
        HIPCHK(c, hipEventRecord(e2, sb));
        HIPCHK(c, hipStreamWaitEvent(sa, e2, 0));
        HIPCHK(c, hipEventRecord(e1, sa));
        HIPCHK(c, hipEventSynchronize(e1));
    }
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
    *ratio = 1e3 * (double)ms / (double)delay_us;
    return LASR_OK;
}

// Experiment: a synthetic neighbour beside the job (see k_nb_mfma / k_nb_load).  kind 1 = MFMA only, 2 = loads from HBM (non-temporal,
// 512 MB), 3 = loads that hit in L2 (96 KB per wave, again and again), 4 = loads from the Infinity Cache (128 MB): n_wg one-wave
// workgroups run for `ms` on a third stream whose hardware queue is shared with neither engine stream (probed; a long kernel on a
// shared queue would simply block the stream behind it) -- the call returns at once.  kind 0: wait for the neighbour and report what
// it got done in *rate (kind 1: TFLOP/s, kind 2: GB/s).  Which resource the two-stream job is short of shows in what a neighbour
// that takes ONLY that resource costs it (bench.py --neighbour).
int lasr_bench_neighbour(lasr_ctx* c, int kind, int n_wg, int ms, double* rate) {
    if (!c || kind < 0 || kind > 4) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (kind == 0) {
        if (rate) *rate = 0.0;
        if (!c->stream_nb || !c->nb_kind) return LASR_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream_nb));
        std::vector<unsigned long long> done(c->nb_wgs);
        HIPCHK(c, hipMemcpy(done.data(), c->nb_done, sizeof(unsigned long long) * c->nb_wgs, hipMemcpyDeviceToHost));
        double total = 0.0;
        for (auto v : done) total += (double)v;
        // k_nb_mfma: iterations are MFMAs of 2 * 16 * 16 * 4 flop; k_nb_load: 1 KB loads
        if (rate) *rate = c->nb_kind == 1 ? total * 2048.0 / (c->nb_ms * 1e-3) * 1e-12 : total * 1024.0 / (c->nb_ms * 1e-3) * 1e-9;
        c->nb_kind = 0;
        return LASR_OK;
    }
    if (n_wg < 1 || n_wg > 4096 || ms < 1 || ms > 5000) return fail(c, LASR_EINVAL, "neighbour: 1..4096 workgroups, 1..5000 ms");
    if (c->nb_kind) return fail(c, LASR_ESTATE, "a neighbour is already running: collect it with kind 0");
    if (!c->stream_nb) {
        std::vector<hipStream_t> rejected;
        for (int attempt = 0; attempt < 8 && !c->stream_nb; ++attempt) {
            hipStream_t st = nullptr;
            HIPCHK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            double r0 = 0.0, r1 = 0.0;
            if (overlap_probe_impl(c, 300, &r0, c->stream, st) != LASR_OK || overlap_probe_impl(c, 300, &r1, c->stream_dec, st) != LASR_OK) {
                (void)hipGetLastError(); rejected.push_back(st); break;
            }
            if (r0 < 1.5 && r1 < 1.5) c->stream_nb = st; else rejected.push_back(st);
        }
        for (hipStream_t st : rejected) (void)hipStreamDestroy(st);
        if (!c->stream_nb) return fail(c, LASR_EHIP, "no hardware queue left for the neighbour stream");
        RC(dalloc(c, &c->nb_done, 4096));
        c->nb_floats = (size_t)128 << 20;                 // 512 MB: twice the Infinity Cache
        RC(dalloc0(c, &c->nb_buf, c->nb_floats));
        HIPCHK(c, hipDeviceSynchronize());
    }
    HIPCHK(c, hipMemsetAsync(c->nb_done, 0, sizeof(unsigned long long) * 4096, c->stream_nb));
    const unsigned long long ticks = (unsigned long long)ms * 100000ull;
    if (kind == 1) hipLaunchKernelGGL(k_nb_mfma, dim3(n_wg), dim3(64), 0, c->stream_nb, ticks, c->nb_done, c->nb_buf);
    else if (kind == 2) hipLaunchKernelGGL(k_nb_load, dim3(n_wg), dim3(64), 0, c->stream_nb, ticks, (const f32x4*)c->nb_buf, c->nb_floats / 4, (size_t)0, 0, c->nb_done, c->nb_buf);
    else if (kind == 3) hipLaunchKernelGGL(k_nb_load, dim3(n_wg), dim3(64), 0, c->stream_nb, ticks, (const f32x4*)c->nb_buf, c->nb_floats / 4, (size_t)(96 << 10) / 16, 1, c->nb_done, c->nb_buf);
    else hipLaunchKernelGGL(k_nb_load, dim3(n_wg), dim3(64), 0, c->stream_nb, ticks, (const f32x4*)c->nb_buf, (size_t)(128 << 20) / 16, (size_t)0, 1, c->nb_done, c->nb_buf);
    HIPCHK(c, hipGetLastError());
    c->nb_kind = kind; c->nb_wgs = n_wg; c->nb_ms = (double)ms;
    return LASR_OK;
}

// engine configuration as resolved at lasr_create (include/lasr_debug.h)
int lasr_debug_config(lasr_ctx* c, const char* key, int* value) {
    if (!c || !key || !value) return LASR_EINVAL;
    const struct { const char* k; int v; } tab[] = {
        {"enc_wave", c->enc_wave}, {"enc_u12", (int)c->enc_u12}, {"main_graph", (int)c->main_graph},
        {"pump_G", c->pump_G}, {"la_stream", c->la_stream}, {"la_offline", c->la_offline},
        {"cell_nw", c->cell_nw ? c->cell_nw : (c->bf ? 8 : 4)}, {"use_graphs", (int)c->use_graphs}, {"M", c->M},
        {"push_lazy", (int)c->lazy_on}, {"pump_nap_pct", c->pump_nap_pct}, {"lazy_taken", c->lazy_taken}, {"lazy_flushed", c->lazy_flushed},
        {"fe_lds_pad", c->fe_lds_pad}, {"roctx", roctx_state().push != nullptr ? 1 : 0},
        {"lat_R", LAT_R}, {"lat_umax", LAT_UMAX},      // lattice (lasr_align_*): rows per block, labels per transcript; with profiling on,
        {"lat_enc_us", c->lat.us[0]}, {"lat_pred_us", c->lat.us[1]}, {"lat_blocks_us", c->lat.us[2]}, {"lat_dp_us", c->lat.us[3]},   // the last call's stages
        {"lat_band_wmax", LAT_BAND_WMAX}, {"lat_band_umax", LAT_BAND_UMAX}, {"lat_bp_words", LAT_BP_WORDS},   // banded lattice (lasr_align_band_*): widest window, labels per transcript; back-pointer words a workgroup keeps in LDS
        {"lat_post_us", c->lat.us[4]},                 // (alpha / beta and occupancies of the last lasr_align_* / lasr_align_post_* / lasr_align_band_post_* / lasr_score_* call: 0 unless it asked for posteriors; the lasr_lattice_* hooks record no stage times)
    };
    for (const auto& e : tab)
        if (!strcmp(e.k, key)) { *value = e.v; return LASR_OK; }
    return fail(c, LASR_EINVAL, "lasr_debug_config: unknown key '%s'", key);
}

int lasr_bench_cell(lasr_ctx* c, int layer, int iters, double* us) {
    if (!c || !us || layer < 0 || layer >= c->d.enc_layers || iters < 1) return c ? fail(c, LASR_EINVAL, "bad argument") : LASR_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const int Tn = 1;
    RC(ensure_T(c, Tn));
    const int H = c->d.hidden, I = c->enc[layer].I, M = c->M;
    // random (not zero) operands: zero-filled data inflates the clock (DVFS)
    hipLaunchKernelGGL(k_fill_rand, dim3(grid1((size_t)c->Tcap * M * I)), dim3(256), 0, c->stream, layer == 0 ? c->x0 : c->ybuf[(layer - 1) & 1],
                       (size_t)c->Tcap * M * I, 17u, c->bf);
    for (int p = 0; p < 2; ++p)
        hipLaunchKernelGGL(k_fill_rand, dim3(grid1((size_t)M * H)), dim3(256), 0, c->stream, c->enc_h[p][layer], (size_t)M * H, 23u + p, c->bf);
    RC(cmd_begin(c));
    for (int r = 0; r < c->d.max_streams; ++r) c->hc.T_row[r] = Tn;
    RC(cmd_commit(c));
    RC(commit_T_rows(c, Tn));
    const void* xsrc = layer == 0 ? c->x0 : c->ybuf[(layer - 1) & 1];
    const int mt_total = c->Tcap * c->MT;
    auto one = [&]() { launch_enc_cell(c, c->stream, layer, 0, xsrc, mt_total, c->ybuf[layer & 1], mt_total); c->enc_par ^= 1; };
    for (int i = 0; i < 3; ++i) one();
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipEventRecord(e0, c->stream));
    for (int i = 0; i < iters; ++i) one();
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *us = (double)ms * 1000.0 / ((double)iters * Tn);
    c->cmd_inflight = 0;
    HIPCHK(c, hipGetLastError());
    return LASR_OK;
}

}  // extern "C"

#include "lasr_front.hip.h"

// ---------------------------------------------------------------------------- banded lattice and its posteriors (5.7)
#include "lasr_band_windows.hip.h"
#include "lasr_lattice_band.hip.h"
#include "lasr_lattice_band_post.hip.h"
extern "C" {
// lasr_align_* over a band of `band` labels per frame
int lasr_band_windows(int T, int U, int band, const int32_t* frames, const int32_t* lo_cur, int32_t* lo_out, int* touch) {
    return lasr_bw::band_windows(T, U, band, frames, lo_cur, lo_out, touch);
}
int lasr_align_band_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                        const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                        int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes, int32_t* touch) {
    LatCall k;
    const LatBandIO io{band, max_passes, lo_in, lo_out, passes, touch, &k};
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, nullptr, &io};
    return align_impl(c, a, OfflineAudio{pcm, n_samples, nullptr});
}
int lasr_align_band_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                          const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                          int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes, int32_t* touch) {
    LatCall k;
    const LatBandIO io{band, max_passes, lo_in, lo_out, passes, touch, &k};
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, nullptr, &io};
    return align_impl(c, a, OfflineAudio{feats, nullptr, n_frames});
}
// lasr_align_band_* with the band's edge posteriors; all six posterior outputs null: lasr_align_band_* itself
int lasr_align_band_post_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                             const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                             int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes, int32_t* touch,
                             float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var, int32_t* tok_peak_frame, double* tok_peak) {
    LatCall k;
    const LatBandIO io{band, max_passes, lo_in, lo_out, passes, touch, &k};
    const LatPostOut p{nullptr, nullptr, occ_blank, occ_emit, tok_mean, tok_var, tok_peak_frame, tok_peak};
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, lat_post_any(p) ? &p : nullptr, &io};
    return align_impl(c, a, OfflineAudio{pcm, n_samples, nullptr});
}
int lasr_align_band_post_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                               const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                               int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes, int32_t* touch,
                               float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var, int32_t* tok_peak_frame, double* tok_peak) {
    LatCall k;
    const LatBandIO io{band, max_passes, lo_in, lo_out, passes, touch, &k};
    const LatPostOut p{nullptr, nullptr, occ_blank, occ_emit, tok_mean, tok_var, tok_peak_frame, tok_peak};
    const AlignCall a{slots, n, tokens, n_tokens, LatOut{loglik, viterbi, frames, logps, blank_lp, emit_lp}, lat_post_any(p) ? &p : nullptr, &io};
    return align_impl(c, a, OfflineAudio{feats, nullptr, n_frames});
}

// head of lasr_lattice_band_dp / lasr_lattice_band_post: the arguments, the call description with W and lo [sum T] beside T and U, and
// its tables on the device.  post: the cell limit of a posterior call, before the windows or a lattice are read
static int lattice_band_call(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, const int32_t* W,
                             const int32_t* lo, int n, const double* loglik, bool post, LatCall& k, TabImage& img) {
    if (!blank_lp || !emit_lp || !T || !U || !W || !lo || !loglik || n < 1) return fail(c, LASR_EINVAL, "bad argument");
    k.n = n;
    k.T.assign(T, T + n); k.U.assign(U, U + n); k.W.assign(W, W + n); k.slot.assign(n, 0);
    for (int i = 0; i < n; ++i)
        if (T[i] < 1 || U[i] < 0 || U[i] > LAT_BAND_UMAX || W[i] < 1 || W[i] > std::min(U[i] + 1, LAT_BAND_WMAX) || (T[i] == 1 && W[i] != U[i] + 1))
            return fail(c, LASR_EINVAL, "lattice %d: T = %d, U = %d, W = %d (T >= 1, 0 <= U <= %d, 1 <= W <= min(U + 1, %d), W = U + 1 where T = 1)",
                        i, T[i], U[i], W[i], LAT_BAND_UMAX, LAT_BAND_WMAX);
    RC(lat_layout_checked(c, k));
    if (post) RC(lat_band_post_cells(c, k));
    k.lo.assign(lo, lo + k.sumT);
    for (int i = 0; i < n; ++i)
        if (!lasr_bw::valid(T[i], U[i], W[i], lo + k.lo_off[i])) return fail(c, LASR_EINVAL, "lattice %d: lo is not a valid set of windows of width %d", i, W[i]);
    HIPCHK(c, hipSetDevice(c->device));
    lat_pack(k, nullptr, img);
    return lat_upload(c, c->lat, img);
}
// the banded programme
int lasr_lattice_band_dp(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, const int32_t* W,
                         const int32_t* lo, int n, double* loglik, double* viterbi, int32_t* frames) {
    if (!c) return LASR_EINVAL;
    LatCall k;
    TabImage img;
    RC(lattice_band_call(c, blank_lp, emit_lp, T, U, W, lo, n, loglik, false, k, img));
    RC(lattice_hook(c, blank_lp, emit_lp, k.cells, [&](const float* b, const float* e) {
        return lat_band_run_dp(c, c->lat, k, b, e, viterbi || frames, frames != nullptr, false);
    }));
    return lat_copy_out(c, c->lat, k, LatOut{loglik, viterbi, frames, nullptr, nullptr, nullptr});
}
// the banded forward-backward programme
int lasr_lattice_band_post(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, const int32_t* W,
                           const int32_t* lo, int n, double* loglik, double* loglik_bwd, float* occ_blank, float* occ_emit, double* tok_mean,
                           double* tok_var, int32_t* tok_peak_frame, double* tok_peak) {
    if (!c) return LASR_EINVAL;
    LatCall k;
    TabImage img;
    RC(lattice_band_call(c, blank_lp, emit_lp, T, U, W, lo, n, loglik, true, k, img));
    const LatPostOut p{loglik, loglik_bwd, occ_blank, occ_emit, tok_mean, tok_var, tok_peak_frame, tok_peak};
    RC(lattice_hook(c, blank_lp, emit_lp, k.cells, [&](const float* b, const float* e) { return lat_band_post_launch(c, c->lat, k, b, e, p); }));
    return lat_post_copy(c, c->lat, k, p);
}
}  // extern "C"
