/*
 * lasr.h -- C ABI of liblasr_hip.so: the MI355X (gfx950) streaming RNN-Transducer inference path.
 *
 * The reference (iceychris/LibreASR) has NO FFI / plugin / operator interface: its hot path is a
 * Python call surface over torch CPU ops.  This header is therefore the boundary a maintainer
 * binds with ctypes (INTEGRATION.md shows the stub); each entry point names the reference
 * interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - every function returns LASR_OK (0) or a negative LASR_E* code; nothing throws or aborts;
 *     lasr_last_error() gives a human-readable message for the last failure on that ctx.
 *   - the caller owns every buffer it passes; the ctx owns all device memory it allocates.
 *   - a ctx is single-caller (one scheduler thread per GPU); all work is enqueued on the
 *     hipStream_t given at creation (pass torch.cuda.current_stream().cuda_stream, or NULL).
 *   - "row" == stream slot: slot s occupies batch row s of every device buffer, so there is no
 *     state gather/scatter; rows that do not take part in a call are masked.
 *   - pointers documented "host or device" are classified with hipPointerGetAttributes.
 */
#ifndef LASR_H
#define LASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LASR_OK 0
#define LASR_EINVAL (-1)   /* bad argument / unsupported shape          */
#define LASR_ENOMEM (-2)   /* device or host allocation failed          */
#define LASR_EHIP (-3)     /* a HIP runtime call failed                 */
#define LASR_ESTATE (-4)   /* call not valid in the slot's/ctx's state  */
#define LASR_EFULL (-5)    /* no free stream slot / output buffer small */

typedef struct lasr_ctx lasr_ctx;

/* Model + front-end description.  Mirrors config/testing.yaml:202-229 (model) and :133-143,
 * :350-374 (front-end), and Transducer.__init__ (libreasr/lib/models.py:190-234). */
typedef struct {
    int32_t feat;        /* feature_sz = n_mels * n_stack (1280)                       */
    int32_t hidden;      /* hidden_sz == out_sz (encoder.linear / predictor.linear = id) */
    int32_t enc_layers;  /* encoder LSTM layers                                          */
    int32_t pred_layers; /* predictor layers                                             */
    int32_t pred_cell;   /* 0 = NBRC/GRU cell (haste/nbrc.py), 1 = LSTM                  */
    int32_t embed;       /* embed_sz; if embed != hidden a Linear(embed,hidden) follows  */
    int32_t joint;       /* joint_sz                                                     */
    int32_t vocab;       /* vocab_sz                                                     */
    int32_t blank;       /* 0   (models.py:203)                                          */
    int32_t bos;         /* 2   (models.py:227)                                          */
    int32_t n_fft;       /* 1024 */
    int32_t win;         /* 400  */
    int32_t hop;         /* 160  */
    int32_t n_mels;      /* 128  */
    int32_t n_stack;     /* 10   */
    int32_t stride;      /* 8  (StackDownsample.downsample)                              */
    int32_t n_buffer;    /* 2  (Buffer.n_buffer, transforms.py:455-471)                  */
    int32_t n_window;    /* 3  (BUFFER_N_FRAMES, api-server.py:26)                       */
    int32_t chunk;       /* client chunk length in samples (1280 = 80 ms)                */
    int32_t sample_rate; /* 16000 */
    int32_t dtype;       /* 0 = f32; 1 = bf16 MFMA operands (weights + GEMM-input        */
                         /* activations), f32 accumulate / cell state / logits; needs    */
                         /* feat, hidden, joint % 32 == 0                                */
    int32_t max_streams; /* number of stream slots (= batch rows)                        */
    int32_t max_iters_offline; /* 3  (decode_greedy default, models.py:369)             */
    int32_t max_iters_stream;  /* 10 (transcribe_stream default, models.py:458)         */
    int32_t beam;        /* 1 = greedy (the only decode the reference has); 2..8 = beam  */
                         /* search width W (spec: oracle _beam_frame):     */
                         /* W hypothesis slots per stream, streams x W <= 1024 rows,     */
                         /* vocab <= 2048 (a hypothesis row's logits live in one wave).  */
                         /* lasr_fetch then returns the WHOLE current best hypothesis    */
                         /* after every model step (it may change retroactively),        */
                         /* neg_logp = -its score, align = 0; lasr_set_beam_records +     */
                         /* lasr_fetch_nbest: the whole beam with per-token frame and     */
                         /* log p.  Both protocols (the                                   */
                         /* pipelined one: <= 512 stream slots); an attached LM is fused  */
                         /* inside the beam (see lasr_attach_lm).  lasr_set_beam_merge:  */
                         /* hypotheses that hold the same tokens are merged; a score is  */
                         /* then the log of the summed probability of the alignments     */
                         /* merged into the hypothesis, not of one alignment.            */
} lasr_model_desc;

/* Fills `d` with the reference defaults listed above (4x1024 encoder, 2xNBRC predictor). */
void lasr_default_desc(lasr_model_desc* d);

/* Number of float32 values lasr_create expects in `weights` for `d` (0 if d is invalid).
 * The blob is the reference state_dict flattened in this order, every tensor in its reference
 * layout:
 *   encoder.input_norm.{weight,bias}
 *   per encoder layer i: rnn_stack.hs.i [2,H] (h0,c0); bns.i.{weight,bias,running_mean,running_var};
 *                        rnns.i.{weight_ih_l0 [4H,I], weight_hh_l0 [4H,H], bias_ih_l0, bias_hh_l0}
 *   predictor.embed.weight [V,E]; if E != H: predictor.ffn.{weight [H,E], bias}
 *   per predictor layer i: hs.i [S,H] (S=1 NBRC, 2 LSTM); bns.i.* (as above);
 *        NBRC: rnns.i.{kernel [I,3H], recurrent_kernel [H,3H], bias [3H], recurrent_bias [3H]}
 *        LSTM: rnns.i.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}
 *   joint.joint.0.{weight [J,2H], bias}; joint.joint.2.{weight [V,J], bias}                  */
size_t lasr_weight_count(const lasr_model_desc* d);

/* Replaces: load_stuff / Transducer.from_config + load_asr_model (libreasr/lib/inference.py:18-51,
 * models.py:236-259, model_utils.py:61-95).  Packs the weights into MFMA-fragment order, folds
 * BatchNorm(eval) into scale/shift, builds the predictor input tables, uploads everything. */
int lasr_create(int device, const lasr_model_desc* d, const float* weights, size_t n_weights,
                void* hip_stream, lasr_ctx** out);
void lasr_destroy(lasr_ctx* c);
const char* lasr_last_error(const lasr_ctx* c);

/* ---- stream slots: per-stream state lives on the device (replaces the Python closure state of
 * Transducer.transcribe_stream, models.py:466-500, the Buffer transform's `saved` list,
 * transforms.py:461-471, and the servicer's 3-chunk `frames` list, api-server.py:85-102). */
int lasr_stream_open(lasr_ctx* c, int* slot);
/* what: 1 = encoder state, 2 = predictor (re-run on BOS), 4 = LM state (reset_lm, models.py:491-492; no-op without an attached LM), 8 = front-end
 * window + frame buffer; OR-able.  reset() of models.py:494-497 == 1|2|4. */
#define LASR_RESET_IF_DECODED 16   /* OR into `what` (with bits 1 | 2 | 4 only): accept a slot whose submitted steps are uncollected  */
                                   /* but already DECODED for this slot (see lasr_peek_slot); without it a slot with a submitted,    */
                                   /* uncollected step is always refused (LASR_ESTATE)                                                */
int lasr_stream_reset(lasr_ctx* c, int slot, int what);
/* lasr_stream_reset of n distinct slots with the same `what` in one call (one command block, one set of launches): every slot is
 * checked before anything changes -- an error leaves all of them as they were.  A scheduler's tick that applies the servicer's
 * reset rule (api-server.py:131-134) to several streams at once. */
int lasr_stream_reset_many(lasr_ctx* c, const int* slots, int n, int what);
int lasr_stream_close(lasr_ctx* c, int slot);

/* ---- streaming hot path, batched over n slots ------------------------------------------------
 * lasr_push_pcm: one client chunk of `chunk` float32 samples per listed slot (replaces
 * tensorize + the window cat of api-server.py:88-102).  pcm: [n, chunk] host or device.
 *   - HOST memory (pageable or pinned): copied into the engine's pinned staging ring BEFORE the call returns (helper
 *     threads: LASR_PUSH_THREADS, default 2); the caller's buffer is free on return.
 *   - DEVICE memory: read by a kernel in stream order on the ctx stream, like hipMemcpyAsync(D2D) would.
 *   - lasr_push_pcm_ex with LASR_PUSH_PINNED_NOCOPY (opt-in): pcm must be PINNED host memory (hipHostMalloc /
 *     hipHostRegister / a torch pin_memory() tensor); nothing is copied, a kernel reads the buffer over PCIe AFTER the call
 *     has returned -- also after lasr_step_submit / lasr_push_submit have returned.  *ticket identifies the push: the buffer
 *     must stay untouched until lasr_push_consumed(ctx, ticket) returns 1 (0 = not yet; an event query, no blocking).
 *     Every host push gets a ticket (ticket may be NULL); device pushes report -1.
 *   - lasr_push_submit with LASR_PUSH_DEVICE_STABLE (opt-in, DEVICE memory): the caller promises that the buffer stays
 *     unchanged until the model step this chunk belongs to has been collected (lasr_step_wait) or lasr_sync has returned.  The
 *     chunk of a call that completes no model step is then not appended to the PCM ring by a launch of its own: the next
 *     lasr_push_submit of the same slots appends both chunks in its front-end launch (one launch less per model step on the
 *     stream that binds the job).  Host pushes get this without a flag -- their source is the engine's own staging entry.
 *     Results are the same either way; any other call that touches the ring appends the waiting chunk first.
 * lasr_step_stream: for every listed slot whose window is full, computes the log-mel frames of
 * the window's middle (TransformTime + StreamPostprocess + StackDownsample, transforms.py:
 * 306-342,436-441), buffers them (Buffer), and for slots whose buffer reached n_buffer runs
 * encoder + greedy decode with carried state (models.py:506-575).  Blocks until the tokens of
 * this step are on the host.  n_ran (optional) = number of slots the model ran for. */
#define LASR_PUSH_PINNED_NOCOPY 1
#define LASR_PUSH_DEVICE_STABLE 2
int lasr_push_pcm_ex(lasr_ctx* c, const int* slots, int n, const float* pcm, int flags, long long* ticket);
int lasr_push_consumed(lasr_ctx* c, long long ticket);
int lasr_push_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm);
int lasr_step_stream(lasr_ctx* c, const int* slots, int n, int* n_ran);

/* Generic streaming clients (any chunk length, any sample rate; the browser client sends 44.1 / 48 kHz,
 * apps/web/src/App.js:68): one call per servicer iteration with the window the servicer has concatenated from the
 * last 3 client frames (api-server.py:83-115).  pcm = [n][N] float32, host or device, one window per listed slot, at
 * `sr` Hz.  Does what x_tfm_stream does per call: Resample of the whole window to 16 kHz (transforms.py:141-144;
 * skipped when sr is 16000), log-mel of the window (reflect padding at both ends), frames T//3 + 1 .. + n_stack
 * (transforms.py:335-342), stack, Buffer(n_buffer); when a slot's buffer is full the model runs (synchronous protocol,
 * like lasr_step_stream; n_ran = slots that ran it; tokens through lasr_fetch).  LASR_EINVAL if the window is too short
 * for n_stack frames after the cut.  A slot uses EITHER this form OR lasr_push_pcm + lasr_step_* (LASR_ESTATE when a slot
 * that still has frames pending from the other form is passed).  At most 512 stream slots. */
int lasr_step_window(lasr_ctx* c, const int* slots, int n, const float* pcm, int64_t N, int sr, int* n_ran);

/* Pipelined form (throughput mode): lasr_step_submit enqueues this chunk's front-end + encoder on the
 * ctx stream and returns; lasr_step_wait keeps ONE greedy decode loop running on a second HIP stream and
 * blocks until the tokens of the OLDEST submitted model step are on the host (n_ran = its slot count,
 * 0 if no model step was pending); rows that finish a step early continue with the frames of the later,
 * already encoded steps.  Issue submit(k+1) ... before wait(k): the encoders of the next chunks then
 * overlap the latency-bound decode loop.  Up to lasr_max_inflight() model steps may be submitted and not
 * yet collected: 25 with the reference front-end (n_buffer 2, max_iters_stream 10; 15 until round 5); fewer when n_buffer *
 * max_iters_stream is large (the limit keeps the per-row rings of encoder frames (64) and tokens (512) from
 * wrapping).  A deep pipeline is what absorbs bursty streams: a row that emits many tokens on a few frames falls
 * behind while the others run ahead on the frames of later steps.  At the limit lasr_step_submit returns LASR_ESTATE and changes nothing (the pushed chunk stays
 * pushed: call lasr_step_wait, then submit again).
 * Every other state-changing call returns LASR_ESTATE while a submitted step is uncollected.
 * Results are identical to lasr_step_stream (same kernels, same order per stream).  With beam > 1 the selection loop runs
 * across chunk boundaries too (every stream on its own frame cursor); lasr_fetch after lasr_step_wait hands out the best
 * hypothesis as of that model step. */
int lasr_step_submit(lasr_ctx* c, const int* slots, int n);
/* lasr_push_pcm_ex + lasr_step_submit for the same slot list in ONE call (same results): when the chunk completes a model
 * step the front-end launch takes the newest chunk from `pcm` and appends it to the PCM ring itself -- one launch less on
 * the critical stream per model step.  LASR_ESTATE (in-flight limit reached, unsupported shape for the pipelined protocol) and
 * LASR_EINVAL mean NOTHING was pushed: call lasr_step_wait and repeat the call.  LASR_EHIP (the runtime failed underneath) leaves
 * the chunk pushed. */
int lasr_push_submit(lasr_ctx* c, const int* slots, int n, const float* pcm, int flags, long long* ticket);
/* lasr_push_submit with the chunk of slots[i] at rows[i] (HOST memory, pageable or pinned, `chunk` floats each; free on return):
 * what a server holds when every connection's frame sits in its own receive buffer (api-server.py:88-91 tensorizes one message
 * per stream; a scheduler that batches them would otherwise gather the rows into one array first).  The gather is the copy into
 * the engine's staging ring that a host push makes anyway.  Same error contract as lasr_push_submit. */
int lasr_push_submit_rows(lasr_ctx* c, const int* slots, int n, const float* const* rows, long long* ticket);
int lasr_step_wait(lasr_ctx* c, int* n_ran);
/* Non-consuming look at ONE slot's submitted, uncollected model steps (greedy decode): *n_inflight of them, of which the
 * oldest *n_decoded are finished for this slot; counts[k] (k < *n_decoded, at most cap_steps) = tokens of step k, concatenated
 * in tokens[cap].  lasr_step_wait / lasr_fetch still hand the same tokens out later.  A slot whose submitted steps are all
 * decoded may be reset (lasr_stream_reset with bits 1 | 2 | 4 and LASR_RESET_IF_DECODED) before they are collected: this is how a scheduler applies the
 * servicer's reset rule (api-server.py:44-50, 131-134: judge the step, maybe reset, only then run the stream's next step)
 * without waiting for `steps in flight` collections.  LASR_EFULL: buffers too small; LASR_ESTATE with beam > 1. */
int lasr_peek_slot(lasr_ctx* c, int slot, int32_t* tokens, int cap, int32_t* counts, int cap_steps, int* n_decoded,
                   int* n_inflight);
/* The same for n slots in one call: the skip[i] oldest steps of slots[i] are left out of row i of tokens [n][cap] /
 * counts [n][cap_steps] (skip may be NULL); n_decoded[i] counts every decoded step of the slot, the skipped ones included. */
int lasr_peek_many(lasr_ctx* c, const int* slots, int n, const int* skip, int32_t* tokens, int cap, int32_t* counts,
                   int cap_steps, int* n_decoded, int* n_inflight);
int lasr_step_pending(lasr_ctx* c);   /* submitted model steps not yet collected (0..lasr_max_inflight()) */
int lasr_max_inflight(const lasr_ctx* c);

/* ---- offline path (Transcribe RPC, api-server.py:64-80 -> Transducer.transcribe,
 * models.py:365-455): whole utterances, fresh state, max_iters_offline.
 * pcm: concatenated samples of the n utterances (host or device), n_samples[i] each (>= 2400).
 * Results are fetched with lasr_fetch on the same slots. */
int lasr_transcribe_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm,
                        const int64_t* n_samples);
/* Same, starting from stacked features [sum(n_frames), feat] row-major (x_tfm output). */
int lasr_transcribe_feats(lasr_ctx* c, const int* slots, int n, const float* feats,
                          const int32_t* n_frames);

/* Streaming on feature chunks instead of PCM (the reference's own split: x_tfm_stream output ->
 * Transducer.transcribe_stream, models.py:506-575): feats [n, T, feat] host or device, carried
 * state, max_iters_stream.  Blocks until the tokens are on the host. */
int lasr_step_feats(lasr_ctx* c, const int* slots, int n, const float* feats, int T);

/* New tokens of `slot` since the last fetch (int32 ids incl. nothing for blanks); with beam > 1
 * the complete best hypothesis as of the last model step (empty if no step ran since the last fetch).
 * neg_logp / align (optional): offline metrics of the last lasr_transcribe_* call
 * (-sum log p of every decision, models.py:420-422,455; alignment_score, models.py:445-453).
 * beam > 1 with lasr_set_beam_merge on: neg_logp = -log of the SUMMED probability of the alignments merged into the hypothesis. */
int lasr_fetch(lasr_ctx* c, int slot, int32_t* tokens, int cap, int* n_new, double* neg_logp,
               double* align);

/* Batched form: tokens [n, cap] (row i = new tokens of slots[i]), n_new [n].  One call per step
 * instead of one per stream. */
int lasr_fetch_many(lasr_ctx* c, const int* slots, int n, int32_t* tokens, int cap, int* n_new);

/* ---- Per-token alignment records (greedy decode): when was a token emitted, and how sure was the joint.
 * While on, every token the decode loop emits carries
 *   frame (int32): index of the encoder frame on which it was emitted; one frame = stride * hop / sample_rate seconds (80 ms with
 *       the reference front-end).  Counted per slot from 0 at lasr_stream_open for the streaming protocols (no lasr_stream_reset
 *       restarts it: audio time keeps running) and from the start of the utterance for lasr_transcribe_*.  When the per-frame cap
 *       (max_iters) is hit, all max_iters tokens carry that frame.
 *   logp (float32): the joint's log-softmax at the joint's argmax of that decision -- the term summed into neg_logp (models.py:
 *       420-422).  With an LM attached the token may be the fuser's re-pick; logp stays the joint's.  exp(logp) = confidence.
 * Results, buffer sizes and launches of a context that never turns them on are untouched.
 * Greedy decode only (LASR_EINVAL with beam > 1).  Default off.  A call that changes nothing returns LASR_OK at once; a switch
 * needs an idle context: LASR_ESTATE while a submitted step is uncollected or a slot holds tokens that were not fetched yet. */
int lasr_set_alignments(lasr_ctx* c, int on);
/* lasr_fetch plus, per token, its emission frame and log p.  LASR_ESTATE if alignments are off.
 * LASR_EFULL: nothing consumed, *n_new = needed.  neg_logp / align as in lasr_fetch (optional).
 * lasr_fetch / lasr_fetch_many keep working on such a context: they drop the records of the tokens they hand out.
 * lasr_peek_slot / lasr_peek_many and the native front (lasr_front_*) stay tokens-only. */
int lasr_fetch_aligned(lasr_ctx* c, int slot, int32_t* tokens, int32_t* frames, float* logps, int cap, int* n_new,
                       double* neg_logp, double* align);
/* Batched form: tokens / frames / logps [n, cap], n_new [n]. */
int lasr_fetch_many_aligned(lasr_ctx* c, const int* slots, int n, int32_t* tokens, int32_t* frames, float* logps,
                            int cap, int* n_new);

/* ---- Beam search (beam > 1): the whole beam per model step, every token with its emission frame and log p.
 * While on, the result of every model step is every alive hypothesis, best first, and every token of every hypothesis carries
 *   frame (int32): as for lasr_set_alignments -- counted per slot from 0 at lasr_stream_open (no lasr_stream_reset restarts it), from
 *       the start of the utterance for lasr_transcribe_*; at most max_iters tokens of a hypothesis sit on one frame.
 *   logp (float32): the joint's log-softmax of that extension -- the f32 term the beam added to the hypothesis's score.  With an LM
 *       attached the token is the fuser's re-pick; logp stays the joint's for the best non-blank token.  exp(logp) = confidence.
 * After a predictor reset (lasr_stream_reset bit 2) the best hypothesis is frozen with its records; every hypothesis handed out
 * afterwards is that prefix followed by a hypothesis of the restarted beam.  Tokens decoded before a switch-on have frame -1, logp 0.
 * Allocations, kernels and results of a context that never turns them on are untouched.
 * beam > 1 only (LASR_EINVAL on a greedy context: that one has lasr_set_alignments).  Default off.  A call that changes nothing
 * returns LASR_OK at once; a switch needs an idle context (LASR_ESTATE while a submitted step is uncollected or a slot holds a
 * result that was not fetched), and drops the cached decode graphs. */
int lasr_set_beam_records(lasr_ctx* c, int on);
/* lasr_fetch for a beam context, whole beam: consumes what lasr_fetch would have consumed.  Up to max_hyps hypotheses, best first
 * (score descending, then slot ascending); no merging: two hypotheses may hold the same tokens on different frames (unless
 * lasr_set_beam_merge is on: then the hypotheses are pairwise distinct, and scores[i] is the log of the summed probability of the
 * alignments merged into hypothesis i, while its frames / logps are those of the best-ranked alignment among them).
 * tokens / frames / logps: [max_hyps][cap] (frames, logps optional); n_tokens [max_hyps]; scores [max_hyps] = sum of log p of every
 * decision incl. blanks (scores[0] == -neg_logp of lasr_fetch); *n_hyps = hypotheses alive (may exceed max_hyps: the rest is dropped).
 * Hypothesis 0 is exactly what lasr_fetch returns.  With max_hyps > 0, tokens, n_tokens and scores are required (LASR_EINVAL if null);
 * max_hyps == 0 drops the result and reports *n_hyps.  LASR_ESTATE if the switch is off; LASR_EFULL (a hypothesis is longer than cap):
 * nothing consumed, n_tokens[i] = needed for i < min(max_hyps, *n_hyps), *n_hyps set; call again with cap >= the largest of them.
 * lasr_fetch / lasr_fetch_many keep working on such a context: they drop the rest of the beam with the result they hand out. */
int lasr_fetch_nbest(lasr_ctx* c, int slot, int max_hyps, int32_t* tokens, int32_t* frames, float* logps, int cap,
                     int* n_tokens, double* scores, int* n_hyps);

/* ---- Beam search (beam > 1): merging of hypotheses that hold the same tokens.
 * Without it the beam keeps alignments: up to W - 1 of its W slots may hold a transcript the beam already holds.  While on, after the W
 * survivors of a selection round are known (same candidates, same order as without), the survivors that hold the same token list since
 * the stream's last predictor reset AND are in the same state on the current frame (still expanding it / done with it) are merged: the
 * best-ranked one stays -- with its predictor state, frames and log p -- and its score becomes log(sum of exp(score)) over the group;
 * the others become dead slots.  At the end of every frame, hence of every model step, the live hypotheses are pairwise distinct.
 * Equality is decided on (length, 64-bit hash) of the token list (splitmix64 chain over the tokens): a collision would merge two
 * different lists of the same length; none occurs on the test inputs (checked against the lists themselves on the CPU).
 * scores / neg_logp change their meaning as said at lasr_fetch and lasr_fetch_nbest; a score may exceed the score of the same tokens
 * without merging, never the lattice total lasr_align_* reports for them -- except for a hypothesis that put max_iters tokens on one
 * frame, as described at lasr_align_pcm.  Switch-off keeps the scores as they are; the beam may hold duplicates again from then on.
 * Allocations, kernels and results of a context that never turns it on are untouched.
 * beam > 1 only (LASR_EINVAL on a greedy context).  Default off; independent of lasr_set_beam_records.  A call that changes nothing
 * returns LASR_OK at once; a switch needs an idle context (LASR_ESTATE while a submitted step is uncollected or a slot holds a result
 * that was not fetched), drops the cached decode graphs, and may happen in mid-stream.
 * on = 1 is NOT for an LM: LASR_ESTATE (nothing changed) when switching to 1 with an LM attached, and from lasr_attach_lm /
 * lasr_attach_lm_int8 while the switch is 1 -- the fuser re-picks the token after the selection round, so the identity of the round
 * would be of the wrong token.  Merging under LM fusion is a mode of its own:
 *
 * on = LASR_BEAM_MERGE_LM.  Without an LM attached it is on = 1 exactly (same kernels, bit-equal results).  With an LM attached
 * (lasr_attach_lm is accepted while this mode is on; lasr_attach_lm_int8 stays refused on a beam context) the rule above holds with
 * one change: a slot's identity is chained from the token the slot actually CARRIES after the round -- for a slot extended by a
 * non-blank token the fuser's re-pick where the parent's LM has advanced since its last reset, the joint's token otherwise -- and the
 * merge step runs on the round's W survivors AFTER the re-pick.  Everything else is as above: groups by (length, hash, state on the
 * frame); the lowest slot stays with its parent, token, predictor state, LM state, LM output, frames and log p (the log p of a record
 * stays the joint's term); its score becomes the log-sum over the group in ascending slot order; the others become dead slots; slots
 * are not compacted.  Everything a fetch returns describes the state after the merge.
 * What a score means in this mode: the term the beam adds for an emitted token is the joint's log p of its best non-blank token, not
 * of the token the fuser emitted, so a merged score is the log of a sum of such products and NOT log P(tokens | audio): the bound by
 * the lattice total of lasr_align_* is not claimed in this mode.
 * The LM state of a merged hypothesis is the kept slot's.  The members of a group hold the same tokens since the last predictor reset
 * behind the same frozen prefix, so they have fed the LM the same tokens -- except after lasr_stream_reset with bit 4 and without
 * bit 2 (LM reset, predictor kept): two equal token lists may then have fed the LM different suffixes; the kept slot's LM state and
 * its "has advanced" flag win.
 * Switches 0 <-> LASR_BEAM_MERGE_LM and 1 <-> LASR_BEAM_MERGE_LM are switches like 0 <-> 1 (idle context, results fetched, graphs
 * dropped, possible in mid-stream); with an LM attached LASR_BEAM_MERGE_LM -> 1 is LASR_ESTATE and changes nothing.  Any other
 * nonzero value of `on` means 1. */
#define LASR_BEAM_MERGE_LM 2   /* lasr_set_beam_merge(c, LASR_BEAM_MERGE_LM) */
int lasr_set_beam_merge(lasr_ctx* c, int on);

/* ---- Forced alignment and transcript scoring: the teacher-forced RNN-T lattice.  Replaces Transducer.forward (models.py:308-359:
 * log_softmax(joint(pred[u], enc[t])) for every (t, u)) followed by the forward algorithm of the loss (loss.py:77-79), for inference:
 * only the two entries per cell that the recursion reads are produced, and no gradient.
 * One utterance has T encoder frames f_0..f_{T-1} and labels y_1..y_U (U >= 0, every id in [0, vocab) and not blank).  g_0 = the
 * predictor on BOS from the learned initial state, g_u = the predictor stepped on y_u: what the offline greedy path feeds the joint
 * after it has emitted y_1..y_u.  lp[t,u,:] = log_softmax(joint(g_u, f_t)); b[t,u] = lp[t,u,blank] (0 <= u <= U);
 * e[t,u] = lp[t,u,y_{u+1}] (0 <= u < U).
 *   alpha[0,0] = 0; alpha[t,u] = logaddexp(alpha[t-1,u] + b[t-1,u], alpha[t,u-1] + e[t,u-1]) (a missing predecessor counts -inf)
 *   loglik  = alpha[T-1,U] + b[T-1,U] = log P(y | x) summed over all alignments = -rnnt_loss of loss.py
 *   viterbi = the same recursion with max, final blank included; the emission predecessor (t, u-1) wins only if it is STRICTLY
 *             greater than the blank predecessor (t-1, u): a tie takes the blank
 *   frames[u-1] = the frame t_u on which the best path takes e[t_u, u-1] (non-decreasing); logps[u-1] = e[t_u, u-1]
 * The lattice is the standard unconstrained one: the greedy loop's per-frame cap (max_iters) is NOT applied.  A capped greedy run can
 * therefore report a -neg_logp ABOVE the best lattice path of its own tokens (numpy oracle, tiny_lstm, 3.0 s: -20.39 against -37.68):
 * at a capped frame the greedy loop moves on without paying a blank.  Operand type, rounding points and accumulation of the joint are
 * the context's (dtype); b and e are f32 -- the log-softmax in the decode path's own order of operations, so given the same logits a
 * term IS the log p that lasr_fetch_aligned reports for the same predictor state and frame (the logits GEMM may run on another tiling
 * than the decode loop's: last bits); alpha, loglik and viterbi are accumulated in double on the device.
 * An attached LM plays no part: the lattice is the joint's.
 * Audio arguments as for lasr_transcribe_pcm / lasr_transcribe_feats (host or device, the same length checks).  tokens: the n transcripts
 * concatenated, HOST memory, n_tokens[i] = U_i <= 1535.  All outputs are HOST memory, filled before the call returns: loglik [n] (required);
 * viterbi [n], frames [sum U_i], logps [sum U_i] (each optional; the Viterbi pass is skipped when all three are null); blank_lp / emit_lp
 * (optional): per utterance [T_i][U_i + 1] f32 each, concatenated; column U_i of emit_lp is 0.
 * Like lasr_transcribe_*, the call needs an idle context (LASR_ESTATE otherwise), starts every listed slot from fresh state, clears the
 * slot's uncollected results, and leaves the slots as lasr_stream_reset(.., 1 | 2 | 4) would: a lasr_transcribe_* or streaming run on the
 * same slot afterwards gives the result it gives without the call.  LASR_EINVAL, nothing changed: a token out of range or equal to blank,
 * n_tokens[i] < 0 or too large, n > max_streams, beam > 1 (a beam context lays its predictor rows out per hypothesis slot; left for a
 * follow-up).  Workspaces are allocated at the first call and grow on demand; everything runs on the ctx stream. */
int lasr_align_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                   const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp, float* emit_lp);
int lasr_align_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                     const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp, float* emit_lp);

/* ---- Lattice posteriors: lasr_align_* plus the backward half of the forward-backward algorithm.  With b, e, alpha and loglik as above:
 *   beta[T-1,U] = b[T-1,U]; beta[t,u] = logaddexp(beta[t+1,u] + b[t,u], beta[t,u+1] + e[t,u])  (a missing successor counts -inf)
 *   occ_blank[t,u] = exp(alpha[t,u] + b[t,u] + beta[t+1,u] - loglik) (t < T-1); occ_blank[T-1,U] = 1, occ_blank[T-1,u<U] = 0
 *   occ_emit[t,u]  = exp(alpha[t,u] + e[t,u] + beta[t,u+1] - loglik) (u < U);   occ_emit[t,U] = 0
 * = the probability, over all alignments of the transcript, that the path takes that blank / emits label u + 1 on frame t
 * (= d loglik / d b[t,u], d loglik / d e[t,u]); sum_t occ_emit[t,u] = 1 (u < U) and sum_u occ_blank[t,u] = 1.  Per label u = 1..U,
 * with p(t) = occ_emit[t,u-1]: tok_mean = sum_t t p(t); tok_var = sum_t (t - tok_mean)^2 p(t); tok_peak_frame = the first t of the
 * largest p; tok_peak = that p.  alpha, beta and the occupancies are computed in double on the device; occ_* are rounded once to f32.
 * loglik = -inf (an impossible transcript): every occupancy 0, tok_mean -1, tok_var 0, tok_peak_frame -1, tok_peak 0; never a NaN.
 * Arguments, preconditions, state rules and errors of lasr_align_pcm / lasr_align_feats, followed by six optional HOST outputs:
 * occ_blank / occ_emit per utterance [T_i][U_i + 1] f32, concatenated (the layout of blank_lp / emit_lp); tok_mean, tok_var,
 * tok_peak double [sum U_i]; tok_peak_frame int32 [sum U_i].  All six null: the call is lasr_align_*.  Otherwise alpha and beta
 * occupy 16 bytes per cell of workspace: more than 2^24 cells in the call is LASR_EINVAL, nothing changed. */
int lasr_align_post_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                        const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp,
                        float* emit_lp, float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var, int32_t* tok_peak_frame,
                        double* tok_peak);
int lasr_align_post_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                          const int32_t* n_tokens, double* loglik, double* viterbi, int32_t* frames, float* logps, float* blank_lp,
                          float* emit_lp, float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var, int32_t* tok_peak_frame,
                          double* tok_peak);

/* ---- Banded forced alignment: the lattice restricted to w labels per frame, so that joint, dynamic programme and workspace grow
 * with T w instead of T (U + 1) and the transcript may have up to 32767 labels.
 * Per utterance, with a requested width band >= 1: w = U + 1 where T == 1, else min(band, U + 1); w <= 1536.  Frame t owns the columns
 * [lo[t], lo[t] + w).  Windows are VALID when lo[0] == 0, lo[T-1] == U + 1 - w, lo is non-decreasing and 0 <= lo[t] <= U + 1 - w: every
 * window cell is a lattice cell, (0,0) and (T-1,U) are inside.  b and e are lasr_align_*'s terms at the window cells and count -inf
 * outside; alpha, loglik, viterbi (with its tie rule), frames and logps are lasr_align_*'s recursions on that lattice (a predecessor
 * outside its frame's window counts -inf; never a NaN).  loglik <= the full lattice's; with w == U + 1 everything is the full lattice's.
 * Windows that do not overlap leave no path: loglik = viterbi = -inf, frames all -1, logps 0, touch 0.
 * BAND LAYOUT of a lattice array: per utterance [T_i][w_i], cell = off_i + t w_i + k holds u = lo[t] + k; emit_lp at u == U is 0.
 *
 * lasr_band_windows (host only: no context, no GPU; integer arithmetic only).  frames == NULL: the LINEAR windows
 * lo_out[t] = floor(t (U + 1 - w) / (T - 1)) (T == 1: 0), *touch = 0, lo_cur is not read.  Otherwise frames [U] is a best path found
 * inside the valid windows lo_cur [T], and with c(t) = #{u : frames[u] < t} (c(T) = U; the path occupies columns c(t)..c(t+1) on
 * frame t) the RECENTRED windows are lo_out[t] = clamp(floor((c(t) + c(t+1)) / 2) - floor(w / 2), 0, U + 1 - w), then lo_out[0] = 0
 * and lo_out[T-1] = U + 1 - w (always valid; lo_out may be lo_cur), and *touch (optional) = 1 iff some frame has lo_cur[t] > 0 and
 * c(t) == lo_cur[t], or lo_cur[t] + w < U + 1 and c(t+1) == lo_cur[t] + w - 1: the path ran along a window edge that is not the
 * lattice's own.  touch == 0 is evidence that the band did not constrain the path, not a proof that it is the full lattice's best.
 * LASR_EINVAL: T < 1, U < 0, band < 1, lo_out null, frames given and lo_cur null or not valid, frames decreasing or outside [0, T). */
int lasr_band_windows(int T, int U, int band, const int32_t* frames, const int32_t* lo_cur, int32_t* lo_out, int* touch);

/* lasr_align_band_*: every argument, precondition, state rule and error of lasr_align_pcm / lasr_align_feats, except that
 * n_tokens[i] <= 32767, and in addition: band >= 1, max_passes >= 1, lo_in (HOST, [sum T_i], T_i = the encoder frames of utterance i;
 * NULL: linear windows) the windows of the first pass.  The front-end, the encoder and the teacher-forced predictor run once.  A pass
 * evaluates the band cells of all utterances under the current windows and runs the banded dynamic programme.  With max_passes == 1
 * the Viterbi half runs only when viterbi, frames, logps or touch is asked for.  With max_passes > 1 the best paths come to the host
 * after every pass, and windows and touch are recomputed by lasr_band_windows' routine (an utterance without a path keeps its
 * windows, touch 0); the loop ends when no utterance touches, when no window changed, or at max_passes.  Outputs are the last
 * pass's: blank_lp / emit_lp in band layout, and optionally (HOST) lo_out [sum T_i] the windows of that pass, passes [n] the passes
 * run (the same for the whole call), touch [n].  LASR_EINVAL, nothing changed: as lasr_align_*, band < 1, max_passes < 1, a w beyond
 * 1536 (a single-frame utterance needs U + 1), lo_in not valid, 2^31 band cells or more. */
int lasr_align_band_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                        const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                        int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes, int32_t* touch);
int lasr_align_band_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                          const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                          int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes, int32_t* touch);

/* ---- Banded lattice posteriors: lasr_align_band_* plus the backward half of the forward-backward algorithm over the band (DESIGN
 * 5.7).  With w, valid windows lo, b / e in band layout counting -inf outside the windows, alpha and loglik as lasr_align_band_* has them:
 *   beta[T-1,U] = b[T-1,U]; beta[t,u] = logaddexp(beta[t+1,u] + b[t,u], beta[t,u+1] + e[t,u]) on window cells; a successor outside ITS
 *                 frame's window counts -inf: (t+1,u) is inside iff t < T-1 and u >= lo[t+1], (t,u+1) iff u + 1 < lo[t] + w
 *   occ_blank[t,u] = exp(alpha[t,u] + b[t,u] + beta[t+1,u] - loglik) where (t+1,u) is inside, else 0; occ_blank[T-1,U] = 1
 *   occ_emit[t,u]  = exp(alpha[t,u] + e[t,u] + beta[t,u+1] - loglik) where (t,u+1) is inside, else 0 (so 0 at k = w-1 and at u = U)
 * = lasr_align_post_*'s definition on the full [T][U + 1] lattice that holds -inf outside the windows: the probability, over the
 * alignments that stay inside the windows, that the path takes that edge; sum_t occ_emit[t,u] = 1 (u < U), sum_u occ_blank[t,u] = 1.
 * Per label u = 1..U, p(t) = occ_emit[t,u-1] over the frames whose window holds column u-1 (0 elsewhere): tok_mean, tok_var,
 * tok_peak_frame, tok_peak as lasr_align_post_*.  alpha, beta and the occupancies are double on the device; occ_* are rounded once to
 * f32.  loglik = -inf (windows that leave no path, or an impossible transcript): every occupancy 0, tok_mean -1, tok_var 0,
 * tok_peak_frame -1, tok_peak 0; never a NaN.  With w == U + 1 every output has lasr_align_post_*'s bits.
 * Arguments, preconditions, state rules, limits and errors of lasr_align_band_pcm / lasr_align_band_feats, followed by six optional
 * HOST outputs: occ_blank / occ_emit per utterance [T_i][w_i] f32 in band layout, concatenated (the layout of blank_lp / emit_lp);
 * tok_mean, tok_var, tok_peak double [sum U_i]; tok_peak_frame int32 [sum U_i].  With max_passes > 1 the posteriors are those of the
 * last pass's windows (lo_out).  All six null: the call is lasr_align_band_*.  Otherwise alpha and beta occupy 16 bytes per band cell
 * of workspace: more than 2^24 band cells (sum T_i w_i) in the call is LASR_EINVAL, nothing changed. */
int lasr_align_band_post_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* tokens,
                             const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                             int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes,
                             int32_t* touch, float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var,
                             int32_t* tok_peak_frame, double* tok_peak);
int lasr_align_band_post_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* tokens,
                               const int32_t* n_tokens, int band, int max_passes, const int32_t* lo_in, double* loglik, double* viterbi,
                               int32_t* frames, float* logps, float* blank_lp, float* emit_lp, int32_t* lo_out, int32_t* passes,
                               int32_t* touch, float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var,
                               int32_t* tok_peak_frame, double* tok_peak);

/* ---- N-best rescoring: one encoder pass per utterance and the lattice over a prefix tree of its candidates.
 * lasr_prefix_tree (host only: no context, no GPU) merges k >= 1 candidates -- tokens: concatenated, n_tokens[j] labels each -- into
 * a tree.  Node 0 is the empty prefix (parent -1, label -1, depth 0); every distinct non-empty prefix is one node; label[v] is the
 * label that leads from parent[v] to v, depth[v] the length of the prefix.  Order: depth ascending; within a depth parent ascending;
 * within a parent by first appearance (lowest candidate index).  Hence parent[v] < v, depth is non-decreasing, the nodes of one depth
 * are contiguous and so are the children of a node.  term[j] (k entries) is the node of candidate j: duplicates share a node, an empty
 * candidate maps to node 0.  parent / label / depth hold cap entries.  *n_nodes is always set (0 on LASR_EINVAL).  LASR_EFULL: cap is
 * too small, nothing else is written; LASR_EINVAL: a null argument, a negative length, k < 1. */
int lasr_prefix_tree(const int32_t* tokens, const int32_t* n_tokens, int k, int cap, int32_t* parent, int32_t* label, int32_t* depth,
                     int32_t* term, int* n_nodes);

/* lasr_score_*: log P(candidate | audio) of every candidate of n utterances (terms, recursions and number formats as lasr_align_*).
 * Utterance i has n_cands[i] >= 1 candidates; slots, n_tokens, loglik and viterbi are [sum n_cands], grouped by utterance; tokens: all
 * candidates concatenated in that order (HOST).  Every candidate occupies one open, distinct slot -- its predictor row -- so
 * sum n_cands <= max_streams; the audio of utterance i (pcm / n_samples or feats / n_frames: n entries, as for lasr_align_*) is
 * encoded once, on the slot of its first candidate.  The candidates of an utterance are merged by lasr_prefix_tree (N_i nodes) and each
 * distinct (frame, prefix) goes through the joint once; one dynamic programme over the tree gives every node v
 *   alpha[0,0] = 0; alpha[t,v] = logaddexp(alpha[t-1,v] + b[t-1,v], alpha[t,parent v] + e[t,v]);  final[v] = alpha[T-1,v] + b[T-1,v]
 * = log P(prefix_v | x), with b[t,v] = lp[t,v,blank] and e[t,v] = lp[t,parent v,label v] -- the emission that ENTERS v, e[t,0] = 0 --
 * and viterbi the same with max (a tie takes the blank).  loglik[j] / viterbi[j] = final[term[j]]: duplicate candidates get equal
 * results.  For a single candidate the rows, blocks and operations are lasr_align_*'s: blank_lp is bit-equal, emit_lp's column u + 1
 * is align's column u, loglik and viterbi are equal.
 * Outputs, HOST memory, filled before the call returns: loglik (required); viterbi (optional: the Viterbi half is skipped when null);
 * blank_lp / emit_lp (optional): per utterance [T_i][N_i] f32, concatenated, N_i as lasr_prefix_tree reports it.  No frames and no
 * back-pointers: lasr_align_* aligns a chosen candidate.
 * Idle context (LASR_ESTATE otherwise); every listed slot starts from fresh state, loses its uncollected results and is left as
 * lasr_stream_reset(.., 1 | 2 | 4) would leave it, as with lasr_align_*.  LASR_EINVAL, nothing changed: a token out of range or equal
 * to blank, n_tokens[j] < 0 or > 1535, n_cands[i] < 1, a slot listed twice, sum n_cands > max_streams, N_i > 2048, beam > 1 (a beam
 * context's predictor rows are hypothesis slots with their own reset and parity rules; left for a follow-up). */
int lasr_score_pcm(lasr_ctx* c, const int* slots, int n, const float* pcm, const int64_t* n_samples, const int32_t* n_cands,
                   const int32_t* tokens, const int32_t* n_tokens, double* loglik, double* viterbi, float* blank_lp, float* emit_lp);
int lasr_score_feats(lasr_ctx* c, const int* slots, int n, const float* feats, const int32_t* n_frames, const int32_t* n_cands,
                     const int32_t* tokens, const int32_t* n_tokens, double* loglik, double* viterbi, float* blank_lp, float* emit_lp);

/* ---- LM sequence scoring: log P_LM of n candidate transcripts by the attached LM (the second term of the usual second-pass
 * combination log P_rnnt(y | x) + lambda log P_LM(y) + gamma |y|; lasr_score_* gives the first).
 * Replaces: LM.forward on a whole sequence (lm.py:31-40) followed by the gather of the target labels' entries.
 * Candidate i is y_1..y_U, U = n_tokens[i]; tokens: the candidates concatenated (HOST).
 *   start >= 0:  the LM reads x = (start, y_1, .., y_{U-1}) from zero state; lp[u-1] = log_softmax(LM(x_1..x_u))[y_u], u = 1..U.
 *   start == -1: the LM reads y_1..y_{U-1}; lp[0] = 0 (no term: the reference's fuser has no LM distribution before the first emitted
 *                token, lm.py:46,58); lp[u-1] = log_softmax(LM(y_1..y_{u-1}))[y_u], u = 2..U.
 * total[i] = the sum of the f32 terms lp[0..U) in label order, accumulated in double on the device; U = 0 gives 0.  A term is
 * (z[y] - m) - lse with the maximum and the exp-sum taken as for the lattice's terms (lasr_align_*).  Operand type, rounding points and
 * accumulation are the attached LM's: f32, the context's bf16 operands, or the int8-served form (lasr_attach_lm_int8).
 * Every candidate occupies one open, distinct slot -- its LM row -- so n <= max_streams.  Outputs, HOST memory, filled before the call
 * returns: total [n] (required), logps [sum U_i] (optional).
 * LASR_ESTATE: no LM attached; a submitted step is uncollected.  The listed slots' LM state is reset at the start and at the end: they
 * are left as lasr_stream_reset(slot, 4) leaves them.  Nothing else changes: their encoder, predictor, front-end and uncollected results
 * stay, and so does every other slot's state, its LM state included.
 * LASR_EINVAL, nothing changed: a label out of [0, vocab) or equal to blank; start < -1 or start >= vocab (start may be any id, blank
 * included); n_tokens[i] < 0 or > 1535; n < 1 or n > max_streams; a slot listed twice or not open; a null required argument; beam > 1
 * (the LM rows of a beam context are hypothesis slots behind a parent indirection; the same follow-up as the lattice calls'). */
int lasr_lm_score(lasr_ctx* c, const int* slots, int n, const int32_t* tokens, const int32_t* n_tokens, int start, double* total,
                  float* logps);

/* ---- Contextual biasing (hotwords): greedy decode prefers the phrases of a list, through a phrase automaton.
 * Phrases: k >= 1 token lists of length >= 1 (concatenated in `tokens`, n_tokens[j] ids each), every id in [0, vocab) and not blank,
 * each with a weight weights[j], finite and >= 0, in log-prob units.
 * Trie: lasr_prefix_tree's nodes and order (node 0 = the root).  w(v), v >= 1: the largest weights[j] over the phrases that have node
 * v's prefix as a prefix.  Automaton: the Aho-Corasick DFA of the trie -- delta(v, a) is the node of the LONGEST suffix of path(v) . a
 * that is a trie prefix, 0 if there is none.  The edge list of node v holds every token a with delta(v, a) != 0, ascending in a, as
 * (tok, next = delta(v, a), bonus = w(next)); a token that is not listed has bonus 0 and leads to the root; blank is never listed.
 * Storage is CSR: edge_off[n_nodes + 1], edge_tok / edge_next / edge_bonus [n_edges].
 * The biased decision of a row in node v on the f32 logits z[0..V) of one joint evaluation: s(j) = z[j] + bonus(v, j) (one f32
 * addition, rounded to nearest) for the tokens listed at v, s(j) = z[j] otherwise; the row takes the first maximum of s (NaN counts as
 * the maximum, the lowest id wins among equals).  Blank: the frame is done and the node stays.  Any other token is emitted and the row
 * moves to delta(v, token).  The term that goes into neg_logp and the alignment records is the joint's log-softmax AT THE CHOSEN token,
 * (z[chosen] - max z) - log sum exp(z - max z): the bonus steers the choice and is not part of any reported score.  Frame cursor,
 * per-frame symbol cap and alignment score are untouched.  A graph whose bonuses are all 0 decodes bit for bit as no graph does.
 * Non-finite logits: the token is in [0, vocab), the node in [0, n_nodes), other rows are untouched; nothing else is promised.
 * Not served here: beam contexts (refused: they have lasr_set_beam_bias, below, where the bonus is part of the ranking score and a
 * partial match that fails hands it back -- greedy decode keeps no score to cancel it from); the combination with an attached LM
 * (refused); per-slot phrase lists (the graph is context-wide); negative weights (refused).
 *
 * lasr_bias_compile: phrases -> graph.  No context, no GPU, integer arithmetic and max only.  *n_nodes / *n_edges are always set (0 on
 * LASR_EINVAL).  LASR_EFULL: cap_nodes / cap_edges too small -- nothing else is written, the counts say what is needed.  LASR_EINVAL: a
 * null argument (depth, the trie depth per node, is optional), k < 1, an empty phrase, an id out of range or equal to blank, a weight
 * that is negative or not finite, more than 65536 nodes or 2^22 edges. */
int lasr_bias_compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                      int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_bonus, int32_t* depth,
                      int* n_nodes, int* n_edges);
/* Attach a graph (HOST arrays; copied) to the context: every slot is biased by it and restarts at node 0.  n_nodes == 0 turns biasing
 * off and frees the tables.  The graph is checked before anything changes -- LASR_EINVAL, nothing changed: n_nodes outside [1, 65536];
 * edge_off[0] != 0 or decreasing offsets; a node's tokens not ascending, outside [0, vocab) or blank; next outside [1, n_nodes); a bonus
 * negative or not finite; beam > 1.  LASR_ESTATE, nothing changed: an LM is attached (lasr_attach_lm / lasr_attach_lm_int8 in turn return
 * LASR_ESTATE while a graph is set: the fuser re-picks on standardised scores, in which a bonus in log-prob units has no defined
 * place); a submitted step is uncollected or a slot holds an unfetched result (like the record switches the change needs an idle
 * context, and may happen in mid-stream).  With a graph attached decode evaluates one frame per iteration on every protocol.
 * A row's node is 0 at lasr_stream_open, after every predictor reset (lasr_stream_reset bit 2, lasr_stream_reset_many, the native
 * front's reset rule), at the start of every lasr_transcribe_* utterance, after the lattice, score and lm-score calls (which leave
 * slots as reset 1 | 2 | 4 does) and after lasr_set_bias; reset bits 1, 4 and 8 alone leave it; it is carried across model steps
 * in both streaming protocols like the predictor state. */
int lasr_set_bias(lasr_ctx* c, int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                  const float* edge_bonus);
/* The current node of n open slots into nodes (HOST); synchronises.  LASR_ESTATE: biasing is off; a submitted step is uncollected. */
int lasr_bias_state(lasr_ctx* c, const int* slots, int n, int32_t* nodes);

/* ---- Contextual biasing in beam search: the bonus is part of the ranking score and is revoked when a match fails.
 * The graph in beam form.  Phrases, weights (finite, >= 0), trie nodes and order, w(v) and delta(v, a) are lasr_bias_compile's.  Per
 * node also: term(v) -- some phrase ends exactly at v; cum(0) = 0, cum(v) = cum(parent v) + w(v); held(0) = 0, held(v) = 0 if term(v),
 * else held(parent v) + w(v): the part of the bonus collected so far that is still revocable.  For a node v, a non-blank token a and
 * n = delta(v, a): gain(v, a) = w(n) if n is v's trie child by a; otherwise (a failure transition, n = 0 included) gain(v, a) =
 * cum(n) - held(v).  Node v's edge list holds every a with delta(v, a) != 0, ascending, as (tok, next, gain); back[v] = -held(v) is the
 * gain of every non-blank token that is NOT listed (it leads to the root).  Blank has gain 0 and the node stays.  Sums are taken in
 * double in path order; every gain and back is rounded once to f32.  The summed gains of any token string from the root equal the
 * bonus of its completed matches plus held(current node).  Stated limits: a token shared by a completed phrase and an overlapping
 * next match is credited in both; a phrase that completes only as a proper suffix of a longer partial match that then fails is not
 * credited; at the end of audio an unfinished match keeps its held bonus (the caller reads it as -back[node]).
 * Storage: lasr_bias_compile's CSR arrays with edge_gain [n_edges] (either sign) and node_back [n_nodes] (<= 0, node_back[0] = 0).
 *
 * The biased round is the beam's selection round (one per decode iteration and stream: the slots that are done with the frame are
 * carried, every other live slot offers extensions, the W best candidates survive in the order score descending, source slot
 * ascending, carried first, token id ascending) with three changes.  (1) A slot at node v with the joint's log-probs lp[0..V) forms
 * s(j) = lp[j] + g(v, j) (one f32 addition, rounded to nearest), g = gain for listed tokens, back[v] for other non-blank tokens, 0
 * for blank, and offers its W best tokens by s, descending, the lower id first among equals.  (2) A candidate's score is
 * (score + (double)lp[j]) + (double)g(v, j), the additions in that order.  (3) A survivor extended by a non-blank token j takes node
 * delta(v, j), v its PARENT's node; a blank extension and a carried slot keep the parent's node; a dead slot's node is 0.
 * The per-token record (lasr_set_beam_records) stays the joint's lp[j] without the gain; scores[] of lasr_fetch_nbest and neg_logp
 * are the ranking scores, gains included (lasr_bias_walk gives the gains of a token list back).  A graph whose gains and backs are
 * all 0 decodes bit for bit as no graph does.  Non-finite logits: tokens stay in [0, V), nodes in [0, n_nodes), other streams are
 * untouched; nothing else is promised.
 * Merging (lasr_set_beam_merge 1, or LASR_BEAM_MERGE_LM without an LM) is allowed and the identity is unchanged: equal token lists
 * since the last predictor reset have equal nodes and equal summed gains -- unless lasr_set_beam_bias was called since that reset; the
 * kept (lowest) slot's node then wins, as the kept slot's LM state does under LASR_BEAM_MERGE_LM.
 * Not served: the combination with an attached LM (refused both ways); per-slot phrase lists; negative weights; finalising a held
 * bonus at the end of audio.
 *
 * lasr_beam_bias_compile: phrases -> graph in beam form; lasr_bias_compile's contract (host only; counts always set; LASR_EFULL /
 * LASR_EINVAL as there), and LASR_EINVAL also if any |gain| or |back| exceeds 1000 (the selection kernel's pruning relies on it). */
int lasr_beam_bias_compile(const int32_t* tokens, const int32_t* n_tokens, const float* weights, int k, int vocab, int blank, int cap_nodes,
                           int cap_edges, int32_t* edge_off, int32_t* edge_tok, int32_t* edge_next, float* edge_gain, float* node_back,
                           int32_t* depth, int* n_nodes, int* n_edges);
/* Attach a graph in beam form (HOST arrays; copied) to a beam context: every hypothesis slot is biased by it and restarts at node 0;
 * the slots' scores stay what they are, at switch-on and at switch-off.  n_nodes == 0 turns biasing off and frees the tables.  A
 * context that never calls this launches the kernels it always launched.  Checked before anything changes -- LASR_EINVAL, nothing
 * changed: a greedy context (it has lasr_set_bias); lasr_set_bias' graph checks, except that a gain may have either sign; a gain or
 * back that is not finite or beyond 1000 in magnitude; back > 0; node_back[0] != 0; a null array.  LASR_ESTATE, nothing changed: an
 * LM is attached (lasr_attach_lm in turn returns LASR_ESTATE while a beam graph is set); a submitted step is uncollected or a slot
 * holds an unfetched result (the switch needs an idle context, drops the cached decode graphs, and may happen in mid-stream).
 * A slot's node is 0 at lasr_stream_open, after every predictor reset (bit 2: all W slots of the stream), at the start of every
 * lasr_transcribe_* utterance and after lasr_set_beam_bias; reset bits 1, 4 and 8 alone leave it; it is carried across model steps on
 * both streaming protocols. */
int lasr_set_beam_bias(lasr_ctx* c, int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                       const float* edge_gain, const float* node_back);
/* The nodes of the W hypothesis slots of one open stream, in slot order (HOST, nodes[beam]); -1 for a dead slot; synchronises.
 * LASR_ESTATE: beam biasing is off; a submitted step is uncollected. */
int lasr_beam_bias_state(lasr_ctx* c, int slot, int32_t* nodes);
/* Tokens through a graph in beam form, host only: from node `start`, n tokens (blank: gain 0, the node stays; a token that is not
 * listed: back[node], to the root) -> *end_node, *total = the double sum of the f32 gains in order, gains[n] (optional; so are the
 * other two).  score - total is the acoustic score of a hypothesis whose tokens were decoded since a reset.  LASR_EINVAL: a null
 * table, start outside [0, n_nodes), n < 0, a negative token, an edge target outside [0, n_nodes). */
int lasr_bias_walk(int n_nodes, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const float* edge_gain,
                   const float* node_back, int blank, const int32_t* tokens, int n, int start, int* end_node, double* total, float* gains);

/* ---- op-level entry points (parity tests and roofline micro-benchmarks).  Device pointers
 * unless noted; all enqueue on the ctx stream and return without synchronising. -------------- */
/* log-mel of whole signals: pcm [B, N] -> logmel [B, T, n_mels], T = 1 + N / hop. */
int lasr_logmel(lasr_ctx* c, const float* pcm, int B, int64_t N, float* logmel);
/* stacked features [B, T', feat] from logmel [B, T, n_mels] (StackDownsample). */
int lasr_stack(lasr_ctx* c, const float* logmel, int B, int T, float* feats, int* Tp);
/* Encoder.forward with fresh (learned) initial state: feats [B, T', feat] -> out [B, T', hidden]
 * (B <= max_streams).  h_out/c_out optional [enc_layers, B, hidden]. */
int lasr_encoder(lasr_ctx* c, const float* feats, int B, int Tp, float* out, float* h_out,
                 float* c_out);
/* Predictor on a token sequence per row from the learned initial state: tok [B, U] (host int32)
 * -> out [B, hidden] after the last token. */
int lasr_predictor(lasr_ctx* c, const int32_t* tok, int B, int U, float* out);
/* Joint + log-softmax: h_pred, h_enc [B, hidden] -> logits [B, vocab] (pre-softmax),
 * logp_max [B], argmax [B] (device). */
int lasr_joint(lasr_ctx* c, const float* h_pred, const float* h_enc, int B, float* logits,
               float* logp_max, int32_t* argmax);
/* One biased decision per row (see lasr_set_bias) on caller-supplied logits [B, vocab] (device) with the attached graph, row r in
 * node[r] (HOST, in [0, n_nodes)): tok, next (the node after the decision; node[r] itself on blank) and logp (the term of the
 * decision), HOST memory, filled before the call returns.  B <= max_streams.  Touches no slot's state.  LASR_ESTATE: biasing is off. */
int lasr_bias_pick(lasr_ctx* c, const float* logits, const int32_t* node, int B, int32_t* tok, int32_t* next, float* logp);
/* One biased selection round (see lasr_set_beam_bias) of n streams on caller-supplied logits [n * beam, vocab] (device, row = stream *
 * beam + slot) with the attached graph -- the decode loop's own kernel on a scratch state; no slot's state is read or written.  HOST
 * inputs per row: score, alive, inB (1: the slot is done with the frame and is carried), node in [0, n_nodes); per stream: rounds, the
 * selection rounds already done on the frame (the round is at the per-frame cap when rounds + 1 >= max_iters).  HOST outputs per row,
 * filled before the call returns: parent (slot of the same stream), emit (1: extended by a non-blank token), token (the extension's
 * token, -1 unless emit), score, alive, inB (all 0 when the stream's frame is finished), node, term (the joint's log p of the
 * extension, 0 unless emit).  n <= max_streams; needs an idle context.  LASR_ESTATE: beam biasing is off.  LASR_EINVAL: a greedy
 * context, a null argument, a node out of range, rounds < 0, max_iters < 1. */
int lasr_beam_bias_round(lasr_ctx* c, const float* logits, int n, const double* score, const int32_t* alive, const int32_t* inB,
                         const int32_t* node, const int32_t* rounds, int max_iters, int32_t* parent, int32_t* token, int32_t* emit,
                         double* score_out, int32_t* alive_out, int32_t* inB_out, int32_t* node_out, float* term);

/* The lattice dynamic programme alone (see lasr_align_*), on n caller-supplied lattices: blank_lp / emit_lp host or device, per lattice
 * [T_i][U_i + 1] f32, concatenated (column U_i of emit_lp is not read); T, U: HOST int32 [n] (T >= 1, 0 <= U <= 1535).  Results in HOST
 * memory, filled before the call returns (this one synchronises): loglik [n] (required), viterbi [n], frames [sum U_i] (optional). */
int lasr_lattice_dp(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, int n,
                    double* loglik, double* viterbi, int32_t* frames);

/* The banded dynamic programme alone (see lasr_align_band_*), on n caller-supplied band lattices: blank_lp / emit_lp host or device,
 * per lattice [T_i][W_i] f32 in band layout, concatenated (emit_lp at u == U is not read); T, U, W: HOST int32 [n]; lo: HOST int32
 * [sum T_i], valid windows of width W_i.  W_i must be an effective width: 1 <= W <= min(U + 1, 1536), and W == U + 1 where T == 1;
 * T >= 1, 0 <= U <= 32767, fewer than 2^31 cells in the call; LASR_EINVAL otherwise.  Results in HOST memory, filled before the call
 * returns (this one synchronises): loglik [n] (required), viterbi [n], frames [sum U_i] (optional).  With W == U + 1 the results
 * are lasr_lattice_dp's bit for bit. */
int lasr_lattice_band_dp(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, const int32_t* W,
                         const int32_t* lo, int n, double* loglik, double* viterbi, int32_t* frames);

/* Forward-backward alone (see lasr_align_post_*), on n caller-supplied lattices: inputs and range checks as lasr_lattice_dp, and at
 * most 2^24 cells in the call (LASR_EINVAL before anything is read).  Results in HOST memory, filled before the call returns (this
 * one synchronises): loglik [n] (required; the forward sum, bit for bit lasr_lattice_dp's); optional: loglik_bwd [n] = beta[0,0]
 * (loglik up to rounding), occ_blank / occ_emit [cells] f32, tok_mean / tok_var / tok_peak double and tok_peak_frame int32 [sum U_i]. */
int lasr_lattice_post(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, int n,
                      double* loglik, double* loglik_bwd, float* occ_blank, float* occ_emit, double* tok_mean, double* tok_var,
                      int32_t* tok_peak_frame, double* tok_peak);

/* Banded forward-backward alone (see lasr_align_band_post_*), on n caller-supplied band lattices: inputs and range checks as
 * lasr_lattice_band_dp, and at most 2^24 band cells in the call (LASR_EINVAL before the windows or a lattice are read).  Results in
 * HOST memory, filled before the call returns (this one synchronises): loglik [n] (required; the forward sum, bit for bit
 * lasr_lattice_band_dp's); optional: loglik_bwd [n] = beta[0,0] (loglik up to rounding), occ_blank / occ_emit [cells] f32 in band
 * layout, tok_mean / tok_var / tok_peak double and tok_peak_frame int32 [sum U_i].  With W == U + 1 the results are
 * lasr_lattice_post's bit for bit. */
int lasr_lattice_band_post(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* U, const int32_t* W,
                           const int32_t* lo, int n, double* loglik, double* loglik_bwd, float* occ_blank, float* occ_emit,
                           double* tok_mean, double* tok_var, int32_t* tok_peak_frame, double* tok_peak);

/* The tree dynamic programme alone (see lasr_score_*), on n caller-supplied lattices: blank_lp / emit_lp host or device, per lattice
 * [T_i][N_i] f32, concatenated (emit_lp[t][0] is not read); T, n_nodes [n] and parent [sum N_i] (ids local to the lattice): HOST int32.
 * LASR_EINVAL unless T >= 1, 1 <= N <= 2048, parent[0] == -1, 0 <= parent[v] < v and the depth derived from parent is non-decreasing.
 * Results per NODE in HOST memory, [sum N_i], filled before the call returns (this one synchronises): loglik (required), viterbi
 * (optional). */
int lasr_lattice_tree_dp(lasr_ctx* c, const float* blank_lp, const float* emit_lp, const int32_t* T, const int32_t* n_nodes,
                         const int32_t* parent, int n, double* loglik, double* viterbi);

/* ---- timing / introspection ------------------------------------------------------------------ */
typedef struct {
    double frontend_ms, encoder_ms, decode_ms; /* HIP-event time of the last step's stages     */
    int32_t decode_iters;                      /* joint evaluations rounds in the last step    */
    int32_t frames;                            /* encoder frames (T) of the last step          */
    double cell_ms;                            /* sum over the LSTM-cell launches of last step */
    int32_t cell_launches;
} lasr_step_stats;
int lasr_get_stats(lasr_ctx* c, lasr_step_stats* s);
/* enable per-stage HIP-event timing (costs a few us per step) */
int lasr_set_profiling(lasr_ctx* c, int on);
/* hipStreamSynchronize on the ctx stream */
int lasr_sync(lasr_ctx* c);

/* ---- Resampling for non-16 kHz clients.  Replaces Resample.encodes, transforms.py:135-144
 * (torchaudio 0.6.0 transforms.Resample == compliance.kaldi.resample_waveform, lowpass_filter_width 6: a
 * dependency that is NOT in the reference tree -- restated from its published algorithm, parity unpinned).
 * pcm / out: device [B][N_in] / [B][*N_out] float32; out == NULL only returns *N_out.  The reference
 * resamples every transform call separately (the whole utterance, or each 3-chunk window), and so do the
 * mirrors in libreasr_amd/lib/transforms.py; the fused streaming entry points take 16 kHz PCM. */
int lasr_resample(lasr_ctx* c, const float* pcm, int B, int64_t N_in, int sr_in, float* out, int64_t* N_out);

/* ---- LM shallow fusion.  Replaces LMFuser / LM of lm.py:20-83 as wired into both greedy
 * loops (models.py:401,431,440 / :478,558,569; attached to the model at config.py:143-157): after a
 * non-blank decision the token is re-picked as argmax(alpha * standardize(LM log-probs) + theta *
 * standardize(joint log-softmax)) with entry 0 forced to min_val on both sides; the LM is stepped on every
 * emitted token.  The blank / non-blank decision and the accumulated log p are those of the joint alone.
 * fp32 (or the ctx's bf16 operand mode); the int8-served form of the reference (lm.py:97) is lasr_attach_lm_int8 (greedy only).
 * With beam > 1 (no reference: spec = oracle _beam_frame with an LM) every hypothesis slot carries its own LM state; a hypothesis
 * offers its blank extension and its BEST non-blank extension per round, and the token a selected non-blank extension emits is the
 * fuser's re-pick -- beam = 1 is then exactly the reference's greedy loop with fusion.  lasr_stream_reset bit 4 resets the LM state
 * (reset_lm, models.py:491-492); lasr_transcribe_* start every utterance with a fresh LM state.
 * Weight blob (float32): embed.weight [V,E]; per layer l: rnn.weight_ih_l{l} [4H,I], rnn.weight_hh_l{l}
 * [4H,H], rnn.bias_ih_l{l} [4H], rnn.bias_hh_l{l} [4H] (torch gate order i,f,g,o); linear.weight [V,H]
 * (equal to embed.weight when tied, lm.py:27-29); linear.bias [V]. */
typedef struct {
    int32_t vocab, embed, hidden, layers;
    float alpha, theta, min_val;      /* lm.py:13-15: 0.1, 1.0, -10.0 */
} lasr_lm_desc;
size_t lasr_lm_weight_count(const lasr_lm_desc* d);
int lasr_attach_lm(lasr_ctx* c, const lasr_lm_desc* d, const float* weights, size_t n_weights);
/* The same LM as the reference SERVES it: load_lm (lm.py:86-100) applies maybe_quantize (utils.py:197-210) =
 * torch.quantization.quantize_dynamic({nn.LSTM, nn.Linear}, qint8).  Same weight blob; the engine quantises the weights
 * (per tensor, symmetric int8) and, per row and per matmul at run time, the activations (7 bits), accumulates in exact
 * integer arithmetic and dequantises -- the numerics of the installed torch's x86 / fbgemm engine (un-vendored upstream;
 * restated in oracle/rnnt_oracle.py and pinned there to the reference's own quantised LM).  embed, hidden <= 1024. */
int lasr_attach_lm_int8(lasr_ctx* c, const lasr_lm_desc* d, const float* weights, size_t n_weights);

/* ---- Native serving front.  Replaces the per-RPC worker threads of the reference servicer
 * (api-server.py:82-115: the per-stream frame list and window; :139: ThreadPoolExecutor(max_workers=4), one batch-1 model call per
 * stream and chunk) and the Python tick loop of libreasr_amd.server.Scheduler for the per-stream-producer form: every stream owns
 * a single-producer ring of client chunks in host memory; ONE native thread owns the engine, batches one chunk of every stream
 * that has one waiting into lasr_push_submit_rows (ring addresses, no gather), keeps up to `depth` model steps in flight
 * (<= lasr_max_inflight) and delivers every collected step's tokens to the streams' result queues.  reset_steps > 0 applies the
 * servicer's reset rule (api-server.py:44-50,131-134: after reset_steps model steps since the last reset -- 25 = 4000 ms / 160 ms
 * for the reference geometry -- the first step whose text is empty resets encoder, predictor and LM) between two model steps of
 * the stream, as the reference does; 0 = no rule.  "Text is empty" = the step emitted no token, or only tokens named by
 * lasr_front_set_empty_tokens (pieces the servicer's tokenizer decodes to "": the reference tests `y_one != ""`, :124).  Greedy decode, 16 kHz chunks of lasr_model_desc.chunk samples (the fused
 * streaming path); other client rates / frame lengths keep going through lasr_step_window.  While a front exists it is the only
 * caller of the engine's streaming entry points; lasr_front_pause hands the engine to the caller (unary Transcribe).
 * Thread-safety: one producer (push / eof) and one consumer (next) per stream, any number of streams, any threads. */
typedef struct lasr_front lasr_front;
int lasr_front_create(lasr_ctx* c, int depth, int reset_steps, lasr_front** out);
/* Shutdown in two steps.  lasr_front_stop: the front thread stops submitting; every producer blocked on a full ring and every
 * consumer blocked in lasr_front_next returns LASR_ESTATE (results already queued are still handed out); the handle stays valid,
 * so the application can join those threads.  lasr_front_destroy: collects what is in flight, closes the front's streams, joins
 * its threads, frees the handle -- no other thread may be inside a lasr_front_* call any more; the front must go before
 * lasr_destroy of its context.  (destroy without stop is fine when nothing can be blocked.) */
int lasr_front_stop(lasr_front* f);
void lasr_front_destroy(lasr_front* f);
/* Stream id = engine slot | generation << 16: an id that outlives its stream (a reader thread still holding it after close, while
 * the slot already serves the next client) names nothing -- push / eof / next / close on it return LASR_ESTATE and touch no state.
 * LASR_EFULL when no slot is free. */
int lasr_front_open(lasr_front* f, int* stream);
/* n_chunks client chunks ([n_chunks][chunk] float32, host memory) appended to the stream; copied before the call returns; blocks
 * while the stream's ring (64 chunks) is full -- until there is room, or the stream is closed / the front stopped (LASR_ESTATE). */
int lasr_front_push(lasr_front* f, int stream, const float* pcm, int n_chunks);
int lasr_front_eof(lasr_front* f, int stream);          /* no more chunks: an end-of-stream result follows the last step's */
/* Next result of the stream, in model-step order.  *flags: 1 = a model step (n_tokens new ids, possibly none), 2 = the reset rule
 * fired after this step, 4 = end of stream.  Blocks up to timeout_ms (< 0: until there is one); returns 1 on time-out,
 * LASR_EFULL if cap is too small (nothing consumed). */
int lasr_front_next(lasr_front* f, int stream, int32_t* tokens, int cap, int* n_tokens, int* flags, int timeout_ms);
/* Takes no more input (a producer blocked in lasr_front_push returns LASR_ESTATE, and close waits until it has), waits for the
 * stream's steps in flight, then frees the slot; a consumer blocked in lasr_front_next returns LASR_ESTATE. */
int lasr_front_close(lasr_front* f, int stream);
/* The reset rule's emptiness test on TEXT: ids[0..n) decode to the empty string in the servicer's tokenizer (a lone word-boundary
 * piece); a step whose tokens are all among them counts as empty, like a step without tokens.  Default (never called / n = 0):
 * only "no token".  Call before streams are opened. */
int lasr_front_set_empty_tokens(lasr_front* f, const int32_t* ids, int n);
/* Collect every step in flight and keep the front thread out of the engine until lasr_front_resume (same thread; does not nest). */
int lasr_front_pause(lasr_front* f);
int lasr_front_resume(lasr_front* f);
/* Counters since create: lasr_push_submit_rows calls, model steps submitted, rows of those steps, resets by the rule. */
int lasr_front_stats(lasr_front* f, long long* ticks, long long* steps, long long* rows, long long* resets);
const char* lasr_front_error(const lasr_front* f);      /* text of the engine error that stopped the front, if any */

/* Bench / debug / trace entry points (lasr_bench_*, lasr_debug_*, lasr_trace*, lasr_cell_prof*, lasr_overlap_probe) are not part
 * of the drop-in surface: they are declared in include/lasr_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* LASR_H */
