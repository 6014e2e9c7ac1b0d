"""
Engine: thin Python owner of one lasr_ctx (one per process and GPU).

Everything numeric happens in liblasr_hip.so (hand-written gfx950 kernels); this class only
marshals arguments.  PyTorch is used for device memory and the HIP stream.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .weights import flatten_lm_state_dict, flatten_state_dict, infer_cfg

FRONTEND_DEFAULTS = dict(n_fft=1024, win=400, hop=160, n_mels=128, n_stack=10, stride=8, n_buffer=2,
                         n_window=3, chunk=1280, sample_rate=16000)


def _ptr(x):
    """void* of a torch tensor / numpy array / None."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return C.c_void_p(x.data_ptr())
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    raise TypeError(type(x))


def _ragged(lists, dtype=np.int32, pad=0):
    """lists of numbers (token lists, candidates, windows, parents) -> (their concatenation with room for `pad` more, int32 counts)"""
    parts = [np.asarray(x, dtype=dtype).reshape(-1) for x in lists]
    return np.ascontiguousarray(np.concatenate(parts + [np.zeros(pad, dtype)])), np.array([x.size for x in parts], dtype=np.int32)


def _rows(x, oc, t, w):
    """a copy of t rows of w cells from cell oc of a flat lattice output"""
    return x[oc:oc + t * w].reshape(t, w).copy()


class BiasGraph:
    """The phrase automaton of contextual biasing as CSR edge lists (int32 / float32 host arrays).  Greedy form (lasr_set_bias'
    layout): edge_val is the bonus per edge, finite and >= 0, and node_back is None.  Beam form (lasr_set_beam_bias' layout):
    edge_val is a signed gain per edge, and node_back holds, per node, the gain of every non-blank token that is not listed
    (<= 0).  edge_bonus and edge_gain both name the one float column.  depth: the trie depth per node."""

    def __init__(self, edge_off, edge_tok, edge_next, edge_val, depth=None, node_back=None):
        self.edge_off = np.ascontiguousarray(edge_off, dtype=np.int32)
        self.edge_tok = np.ascontiguousarray(edge_tok, dtype=np.int32)
        self.edge_next = np.ascontiguousarray(edge_next, dtype=np.int32)
        self.edge_val = np.ascontiguousarray(edge_val, dtype=np.float32)
        self.node_back = None if node_back is None else np.ascontiguousarray(node_back, dtype=np.float32)
        self.depth = None if depth is None else np.ascontiguousarray(depth, dtype=np.int32)
        self.n_nodes = int(self.edge_off.size) - 1
        self.n_edges = int(self.edge_tok.size)

    edge_bonus = edge_gain = property(lambda self: self.edge_val)


class BeamBiasGraph(BiasGraph):
    """BiasGraph in beam form, with the columns in lasr_set_beam_bias' order"""

    def __init__(self, edge_off, edge_tok, edge_next, edge_gain, node_back, depth=None):
        super().__init__(edge_off, edge_tok, edge_next, edge_gain, depth, node_back)


def _bias_compile(lib, beam, phrases, weights, vocab, blank):
    """lasr_bias_compile / lasr_beam_bias_compile (beam; no context, no GPU): sized by a first call with no room, filled by the
    second"""
    name = "beam_bias_compile" if beam else "bias_compile"
    fn = getattr(lib, "lasr_" + name)
    tok, nt = _ragged(phrases, pad=1)
    k = int(nt.size)
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
    if k < 1 or w.size != k:
        raise ValueError(name + ": at least one phrase and one weight per phrase")
    nn, ne = C.c_int(0), C.c_int(0)

    def call(cap_nodes, cap_edges, n, e, with_depth):      # room for n nodes and e edges (the back column in beam form only)
        off, etok, enxt, val = np.zeros(n + 1, np.int32), np.zeros(e, np.int32), np.zeros(e, np.int32), np.zeros(e, np.float32)
        back, dep = np.zeros(max(n, 1), np.float32), np.zeros(n, np.int32) if with_depth else None
        cols = [off, etok, enxt, val] + ([back] if beam else []) + [dep]
        rc = fn(_ptr(tok), _ptr(nt), _ptr(w), k, int(vocab), int(blank), cap_nodes, cap_edges, *[_ptr(x) for x in cols], C.byref(nn),
                C.byref(ne))
        return rc, off, etok, enxt, val, back, dep

    rc = call(0, 0, 0, 1, False)[0]
    if rc != N.LASR_EFULL:
        raise N.LasrError(rc, "lasr_" + name + ": phrases of >= 1 ids in [0, vocab) other than blank, weights finite and >= 0"
                              + (", no gain beyond 1000" if beam else ""))
    n, e = nn.value, ne.value
    rc, off, etok, enxt, val, back, dep = call(n, e, n, max(e, 1), True)
    if rc != 0:
        raise N.LasrError(rc, "lasr_" + name)
    return BeamBiasGraph(off, etok[:e], enxt[:e], val[:e], back, dep) if beam else BiasGraph(off, etok[:e], enxt[:e], val[:e], dep)


def bias_compile(lib, phrases, weights, vocab, blank):
    return _bias_compile(lib, False, phrases, weights, vocab, blank)


def beam_bias_compile(lib, phrases, weights, vocab, blank):
    return _bias_compile(lib, True, phrases, weights, vocab, blank)


def bias_walk(lib, graph, tokens, blank, start=0):
    """lasr_bias_walk (no context, no GPU): tokens through a BeamBiasGraph from node `start` -> (end node, the double sum of the
    f32 gains in order, the gains float32 [n])"""
    tok = np.ascontiguousarray(np.asarray(tokens, dtype=np.int32).reshape(-1))
    gains = np.zeros(max(tok.size, 1), np.float32)
    end, total = C.c_int(0), C.c_double(0.0)
    rc = lib.lasr_bias_walk(int(graph.n_nodes), _ptr(graph.edge_off), _ptr(graph.edge_tok), _ptr(graph.edge_next), _ptr(graph.edge_gain),
                            _ptr(graph.node_back), int(blank), _ptr(tok), int(tok.size), int(start), C.byref(end), C.byref(total),
                            _ptr(gains))
    if rc != 0:
        raise N.LasrError(rc, "lasr_bias_walk: start in [0, n_nodes), tokens >= 0")
    return end.value, total.value, gains[:tok.size]


class Engine:
    def __init__(self, state_dict, cfg=None, max_streams=64, device=0, max_iters_offline=3,
                 max_iters_stream=10, blank=0, bos=2, dtype="f32", beam=1, **frontend):
        self.lib = N.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("libreasr_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                               "and there is no CPU fallback")
        cfg = dict(cfg) if cfg is not None else infer_cfg(state_dict)
        self.cfg = cfg
        fe = dict(FRONTEND_DEFAULTS)
        fe.update(frontend)
        d = N.ModelDesc()
        self.lib.lasr_default_desc(C.byref(d))
        d.feat, d.hidden, d.embed, d.joint, d.vocab = cfg["feat"], cfg["hidden"], cfg["embed"], cfg["joint"], cfg["vocab"]
        d.enc_layers, d.pred_layers = cfg["enc_layers"], cfg["pred_layers"]
        d.pred_cell = 1 if cfg["pred_cell"] == "LSTM" else 0
        d.blank, d.bos = blank, bos
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        d.dtype = 1 if dtype == "bf16" else 0      # bf16: weights + GEMM-input activations, f32 accumulate
        self.dtype = dtype
        d.beam = int(beam)                         # 1 = greedy; 2..8 = beam search (both protocols)
        self.beam = int(beam)
        self.beam_bias = None                      # the BeamBiasGraph attached by set_beam_bias
        for k, v in fe.items():
            setattr(d, k, int(v))
        d.max_streams = int(max_streams)
        d.max_iters_offline, d.max_iters_stream = int(max_iters_offline), int(max_iters_stream)
        self.desc = d
        self.device = torch.device("cuda", device)
        blob = flatten_state_dict(state_dict, cfg)
        want = self.lib.lasr_weight_count(C.byref(d))
        if want == 0:
            raise ValueError("model description rejected by liblasr_hip (dims must be multiples of 16; 32 for bf16)")
        if blob.size != want:
            raise ValueError(f"weight blob has {blob.size} floats, liblasr_hip expects {want}")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
        ctx = C.c_void_p()
        rc = self.lib.lasr_create(device, C.byref(d), blob.ctypes.data_as(C.c_void_p), blob.size,
                                  C.c_void_p(stream), C.byref(ctx))
        self.ctx = ctx
        if rc != 0:
            msg = self.lib.lasr_last_error(ctx).decode() if ctx else "no ctx"
            if ctx:
                self.lib.lasr_destroy(ctx)
            self.ctx = None
            raise N.LasrError(rc, msg)
        self.max_streams = int(max_streams)

    lm_cfg = None          # set by attach_lm

    def attach_lm(self, lm_state_dict, alpha=0.1, theta=1.0, min_val=-10.0, int8=False):
        """LM shallow fusion (lm.py LM / LMFuser; constants lm.py:13-15).  int8=False: fp32 / bf16 operands like the
        model; int8=True: the LM as the reference serves it (load_lm -> quantize_dynamic qint8, lm.py:97)."""
        cfg, blob = flatten_lm_state_dict(lm_state_dict)
        d = N.LmDesc(cfg["vocab"], cfg["embed"], cfg["hidden"], cfg["layers"], alpha, theta, min_val)
        fn = self.lib.lasr_attach_lm_int8 if int8 else self.lib.lasr_attach_lm
        self._chk(fn(self.ctx, C.byref(d), blob.ctypes.data_as(C.c_void_p), blob.size))
        self.lm_cfg = cfg

    # ------------------------------------------------------------------ plumbing
    def _chk(self, rc):
        if rc != 0:
            raise N.LasrError(rc, self.lib.lasr_last_error(self.ctx).decode())

    def close(self):
        if getattr(self, "ctx", None):
            for fr in list(getattr(self, "_fronts", ())):      # a native front's threads use the context: they go first
                fr.destroy()
            self.lib.lasr_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _slots(slots):
        a = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
        return a, a.ctypes.data_as(C.c_void_p), int(a.size)

    # ------------------------------------------------------------------ slots
    def open(self):
        s = C.c_int(-1)
        self._chk(self.lib.lasr_stream_open(self.ctx, C.byref(s)))
        return s.value

    def reset(self, slot, what=7, if_decoded=False):
        """what: 1 encoder | 2 predictor | 4 LM | 8 front-end.  if_decoded: accept a slot whose submitted steps are uncollected but
        already decoded for it (peek says so); otherwise a slot with a step in flight is refused."""
        self._chk(self.lib.lasr_stream_reset(self.ctx, int(slot), int(what) | (N.LASR_RESET_IF_DECODED if if_decoded else 0)))

    def reset_many(self, slots, what=7, if_decoded=False):
        """reset(slot, what, if_decoded) for several distinct slots in ONE call (lasr_stream_reset_many): all or nothing."""
        a, p, n = self._slots(slots)
        if n:
            self._chk(self.lib.lasr_stream_reset_many(self.ctx, p, n, int(what) | (N.LASR_RESET_IF_DECODED if if_decoded else 0)))

    def close_slot(self, slot):
        self._chk(self.lib.lasr_stream_close(self.ctx, int(slot)))

    # ------------------------------------------------------------------ streaming
    def _pcm(self, pcm, n):
        if isinstance(pcm, torch.Tensor):
            pcm = pcm.contiguous()
            assert pcm.dtype == torch.float32 and pcm.numel() == n * self.desc.chunk
        else:
            pcm = np.ascontiguousarray(pcm, dtype=np.float32)
            assert pcm.size == n * self.desc.chunk
        return pcm

    def push(self, slots, pcm, pinned_nocopy=False):
        """pcm: [n, chunk] float32 torch (cuda or cpu) tensor or numpy array.  Host memory (pageable or pinned) is copied before
        the call returns; device memory is read in stream order.  pinned_nocopy=True (the tensor must be pinned host memory):
        nothing is copied, the GPU reads the buffer later -- keep it untouched until push_consumed(ticket) is True.
        Returns the push ticket (-1 for device memory)."""
        a, p, n = self._slots(slots)
        pcm = self._pcm(pcm, n)
        t = C.c_longlong(-1)
        self._chk(self.lib.lasr_push_pcm_ex(self.ctx, p, n, _ptr(pcm), N.LASR_PUSH_PINNED_NOCOPY if pinned_nocopy else 0, C.byref(t)))
        return t.value

    def push_submit(self, slots, pcm, pinned_nocopy=False, device_stable=False):
        """push(slots, pcm) + submit(slots) in one call (lasr_push_submit): the front-end launch of a model step takes the newest
        chunk from `pcm` itself.  Same memory rules and results as push + submit.  device_stable=True (a cuda tensor): the caller
        keeps the tensor unchanged until the model step the chunk belongs to is collected (LASR_PUSH_DEVICE_STABLE: a chunk that
        completes no model step is appended by the next call's launch).  Returns the push ticket."""
        a, p, n = self._slots(slots)
        pcm = self._pcm(pcm, n)
        t = C.c_longlong(-1)
        flags = (N.LASR_PUSH_PINNED_NOCOPY if pinned_nocopy else 0) | (N.LASR_PUSH_DEVICE_STABLE if device_stable else 0)
        self._chk(self.lib.lasr_push_submit(self.ctx, p, n, _ptr(pcm), flags, C.byref(t)))
        return t.value

    def push_submit_rows(self, slots, addrs):
        """push_submit with the chunk of slots[i] at host address addrs[i] (uint64 array; `chunk` float32 each, e.g.
        arr.ctypes.data + row * arr.strides[0]): lasr_push_submit_rows -- no gather into one array on this side.  The memory must
        stay alive until the call returns (it is copied before that)."""
        a, p, n = self._slots(slots)
        addrs = np.ascontiguousarray(addrs, dtype=np.uint64)
        assert addrs.size == n
        t = C.c_longlong(-1)
        self._chk(self.lib.lasr_push_submit_rows(self.ctx, p, n, addrs.ctypes.data_as(C.c_void_p), C.byref(t)))
        return t.value

    def push_consumed(self, ticket):
        """True once the source buffer of the push that returned `ticket` has been read by the GPU."""
        rc = self.lib.lasr_push_consumed(self.ctx, int(ticket))
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def max_inflight(self):
        return int(self.lib.lasr_max_inflight(self.ctx))

    def step(self, slots):
        a, p, n = self._slots(slots)
        ran = C.c_int(0)
        self._chk(self.lib.lasr_step_stream(self.ctx, p, n, C.byref(ran)))
        return ran.value

    def step_window(self, slots, windows, sr=16000):
        """Generic clients (any chunk length / sample rate): windows = [n, N] float32 (the last 3 client frames of every
        listed slot, concatenated as the servicer does); returns the number of slots whose model ran (lasr_step_window)."""
        a, p, n = self._slots(slots)
        if isinstance(windows, torch.Tensor):
            windows = windows.contiguous()
            assert windows.dtype == torch.float32 and windows.shape[0] == n
        else:
            windows = np.ascontiguousarray(windows, dtype=np.float32)
            assert windows.shape[0] == n
        ran = C.c_int(0)
        self._chk(self.lib.lasr_step_window(self.ctx, p, n, _ptr(windows), int(windows.shape[1]), int(sr), C.byref(ran)))
        return ran.value

    def submit(self, slots):
        """Pipelined step: enqueue front-end + encoder of the chunk just pushed; returns immediately."""
        a, p, n = self._slots(slots)
        self._chk(self.lib.lasr_step_submit(self.ctx, p, n))

    def pending(self):
        return int(self.lib.lasr_step_pending(self.ctx))

    def wait(self):
        """Decode the oldest submitted model step; returns the number of slots it ran for (0 = none pending)."""
        ran = C.c_int(0)
        self._chk(self.lib.lasr_step_wait(self.ctx, C.byref(ran)))
        return ran.value

    def peek(self, slot, cap=1024, cap_steps=32):
        """-> (token lists of the slot's submitted model steps that are already decoded, oldest first; steps in flight).  Non-consuming
        (lasr_peek_slot): wait() / fetch hand the same tokens out later.  A slot whose steps in flight are all decoded may be reset."""
        buf = np.empty(cap, dtype=np.int32)
        cnt = np.zeros(cap_steps, dtype=np.int32)
        nd, nf = C.c_int(0), C.c_int(0)
        self._chk(self.lib.lasr_peek_slot(self.ctx, int(slot), buf.ctypes.data_as(C.c_void_p), cap, cnt.ctypes.data_as(C.c_void_p), cap_steps,
                                          C.byref(nd), C.byref(nf)))
        out, o = [], 0
        for k in range(nd.value):
            out.append(buf[o:o + cnt[k]].tolist())
            o += int(cnt[k])
        return out, nf.value

    _peek_bufs = None

    def peek_many(self, slots, skip, cap=256, cap_steps=16):
        """lasr_peek_many: for every listed slot the token lists of its decoded, uncollected model steps behind the first skip[i]
        ones, and its steps in flight -> (list of lists of token lists, n_decoded array, n_inflight array)."""
        a, p, n = self._slots(slots)
        sk = np.ascontiguousarray(np.asarray(skip, dtype=np.int32))
        b = self._peek_bufs
        if b is None or b[0].shape[0] < n or b[0].shape[1] != cap or b[1].shape[1] != cap_steps:
            b = self._peek_bufs = (np.empty((max(n, 64), cap), np.int32), np.zeros((max(n, 64), cap_steps), np.int32),
                                   np.zeros(max(n, 64), np.int32), np.zeros(max(n, 64), np.int32))
        tok, cnt, nd, nf = b
        self._chk(self.lib.lasr_peek_many(self.ctx, p, n, sk.ctypes.data_as(C.c_void_p), tok.ctypes.data_as(C.c_void_p), cap,
                                          cnt.ctypes.data_as(C.c_void_p), cap_steps, nd.ctypes.data_as(C.c_void_p), nf.ctypes.data_as(C.c_void_p)))
        out = []
        for i in range(n):
            k_new = int(nd[i]) - int(sk[i])
            if k_new <= 0:
                out.append([])
                continue
            o, steps = 0, []
            for k in range(k_new):
                steps.append(tok[i, o:o + cnt[i, k]].tolist())
                o += int(cnt[i, k])
            out.append(steps)
        return out, nd[:n].copy(), nf[:n].copy()

    def step_feats(self, slots, feats):
        """feats [n, T, feat] (torch cuda/cpu or numpy): one streaming model call with carried state."""
        a, p, n = self._slots(slots)
        if isinstance(feats, torch.Tensor):
            feats = feats.contiguous().float()
            T = feats.shape[1]
        else:
            feats = np.ascontiguousarray(feats, dtype=np.float32)
            T = feats.shape[1]
        assert feats.shape[0] == n and feats.shape[2] == self.desc.feat
        self._chk(self.lib.lasr_step_feats(self.ctx, p, n, _ptr(feats), int(T)))

    def fetch(self, slot, cap=65536):
        buf = np.empty(cap, dtype=np.int32)
        n = C.c_int(0)
        nl, al = C.c_double(0.0), C.c_double(0.0)
        self._chk(self.lib.lasr_fetch(self.ctx, int(slot), buf.ctypes.data_as(C.c_void_p), cap, C.byref(n),
                                      C.byref(nl), C.byref(al)))
        return [int(v) for v in buf[:n.value]], nl.value, al.value

    def fetch_many(self, slots, cap=256):
        """New tokens of every listed slot in one call -> list of lists."""
        a, p, n = self._slots(slots)
        buf = np.empty((n, cap), dtype=np.int32)
        cnt = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.lasr_fetch_many(self.ctx, p, n, buf.ctypes.data_as(C.c_void_p), cap,
                                           cnt.ctypes.data_as(C.c_void_p)))
        cl = cnt.tolist()
        mx = max(cl) if n else 0
        if mx == 0:
            return [[] for _ in range(n)]
        rows = buf[:, :mx].tolist()          # (one conversion of the occupied columns instead of a slice + tolist per slot)
        return [r[:c] for r, c in zip(rows, cl)]

    # ------------------------------------------------------------------ per-token alignment records
    def set_alignments(self, on=True):
        """Per-token emission frame and log p from greedy decode (lasr_set_alignments): off by default; to switch, the engine
        must be idle (no submitted step uncollected, no token unfetched).  beam > 1: LasrError (LASR_EINVAL)."""
        self._chk(self.lib.lasr_set_alignments(self.ctx, 1 if on else 0))

    def fetch_aligned(self, slot, cap=65536):
        """fetch(slot) plus the records -> (tokens, frames, logps, neg_logp, align): frames[i] = encoder frame (since open / start
        of the utterance) on which tokens[i] was emitted, logps[i] = the joint's log p of that decision (float32 arrays)."""
        tok = np.empty(cap, dtype=np.int32)
        fr = np.empty(cap, dtype=np.int32)
        lp = np.empty(cap, dtype=np.float32)
        n = C.c_int(0)
        nl, al = C.c_double(0.0), C.c_double(0.0)
        self._chk(self.lib.lasr_fetch_aligned(self.ctx, int(slot), tok.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p),
                                              lp.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(nl), C.byref(al)))
        k = n.value
        return [int(v) for v in tok[:k]], fr[:k].copy(), lp[:k].copy(), nl.value, al.value

    def fetch_many_aligned(self, slots, cap=256):
        """fetch_many plus the records -> list of (tokens, frames, logps) per listed slot."""
        a, p, n = self._slots(slots)
        tok = np.empty((n, cap), dtype=np.int32)
        fr = np.empty((n, cap), dtype=np.int32)
        lp = np.empty((n, cap), dtype=np.float32)
        cnt = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.lasr_fetch_many_aligned(self.ctx, p, n, tok.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p),
                                                   lp.ctypes.data_as(C.c_void_p), cap, cnt.ctypes.data_as(C.c_void_p)))
        return [(tok[i, :k].tolist(), fr[i, :k].copy(), lp[i, :k].copy()) for i, k in enumerate(cnt.tolist())]

    # ------------------------------------------------------------------ beam: per-token records and the whole beam
    def set_beam_records(self, on=True):
        """Whole-beam results with per-token emission frame and log p from beam decode (lasr_set_beam_records): off by default; to
        switch, the engine must be idle (no submitted step uncollected, no result unfetched).  beam = 1: LasrError (LASR_EINVAL)."""
        self._chk(self.lib.lasr_set_beam_records(self.ctx, 1 if on else 0))

    def set_beam_merge(self, on=True, lm=False):
        """Merging of beam hypotheses that hold the same tokens (lasr_set_beam_merge): off by default.  While on, the live hypotheses
        are pairwise distinct after every frame and a score is the log of the summed probability of the alignments merged into the
        hypothesis.  To switch, the engine must be idle; not with an LM attached (LasrError, LASR_ESTATE) unless lm=True.  beam = 1:
        LasrError (LASR_EINVAL).
        lm=True (with on): LASR_BEAM_MERGE_LM, the mode that also merges under LM shallow fusion -- identities follow the fuser's
        re-picked tokens, attach_lm is accepted while it is on, and without an LM it is exactly on=True.  A merged score is then a
        log-sum of products of the JOINT's terms, not log P(tokens | audio): see include/lasr.h."""
        self._chk(self.lib.lasr_set_beam_merge(self.ctx, (N.LASR_BEAM_MERGE_LM if lm else 1) if on else 0))

    def fetch_nbest(self, slot, max_hyps=None, cap=65536):
        """fetch(slot) for the whole beam -> [(tokens, frames, logps, score)], best first (score descending, then hypothesis slot
        ascending; no merging): up to max_hyps (default: the beam width) of the hypotheses alive after the last model step.
        frames / logps as in fetch_aligned; score = sum of log p of every decision; entry 0 is what fetch would have returned."""
        k = self.beam if max_hyps is None else int(max_hyps)
        tok = np.empty((max(k, 1), cap), dtype=np.int32)
        fr = np.empty((max(k, 1), cap), dtype=np.int32)
        lp = np.empty((max(k, 1), cap), dtype=np.float32)
        cnt = np.zeros(max(k, 1), dtype=np.int32)
        sc = np.zeros(max(k, 1), dtype=np.float64)
        nh = C.c_int(0)
        self._chk(self.lib.lasr_fetch_nbest(self.ctx, int(slot), k, tok.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p),
                                            lp.ctypes.data_as(C.c_void_p), cap, cnt.ctypes.data_as(C.c_void_p),
                                            sc.ctypes.data_as(C.c_void_p), C.byref(nh)))
        return [(tok[i, :cnt[i]].tolist(), fr[i, :cnt[i]].copy(), lp[i, :cnt[i]].copy(), float(sc[i]))
                for i in range(min(k, nh.value))]

    # ------------------------------------------------------------------ offline
    def _cat_pcm(self, pcm_list):
        """-> (all utterances concatenated: one device tensor if every one is, else one host array; int64 sample counts)"""
        if all(isinstance(x, torch.Tensor) and x.is_cuda for x in pcm_list):
            cat = torch.cat([x.reshape(-1).float() for x in pcm_list]).contiguous()
        else:   # mixed / host inputs: gather on the host, one H2D copy inside the library
            cat = np.ascontiguousarray(np.concatenate([
                np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32).reshape(-1)
                for x in pcm_list]))
        return cat, np.array([int(np.prod(x.shape)) for x in pcm_list], dtype=np.int64)

    def _cat_feats(self, feats_list):
        """-> (all [T', feat] blocks concatenated, device or host as _cat_pcm; int32 frame counts)"""
        F = self.desc.feat
        if all(isinstance(x, torch.Tensor) and x.is_cuda for x in feats_list):
            arrs = [x.reshape(-1, F).float() for x in feats_list]
            cat = torch.cat(arrs).contiguous()
        else:
            arrs = [np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32).reshape(-1, F) for x in feats_list]
            cat = np.ascontiguousarray(np.concatenate(arrs))
        return cat, np.array([x.shape[0] for x in arrs], dtype=np.int32)

    def _cat(self, pcm, slots, audio):
        """the audio of an offline call, one utterance per listed slot -> (slot pointer, n, _cat_pcm's or _cat_feats' pair)"""
        a, p, n = self._slots(slots)
        assert len(audio) == n
        return p, n, (self._cat_pcm(audio) if pcm else self._cat_feats(audio))

    def transcribe_pcm(self, slots, pcm_list):
        """pcm_list: list of 1-D float32 arrays/tensors (one utterance per slot)."""
        p, n, (cat, ns) = self._cat(True, slots, pcm_list)
        self._chk(self.lib.lasr_transcribe_pcm(self.ctx, p, n, _ptr(cat), _ptr(ns)))

    def transcribe_feats(self, slots, feats_list):
        """feats_list: list of [T', feat] float32 arrays/tensors."""
        p, n, (cat, nf) = self._cat(False, slots, feats_list)
        self._chk(self.lib.lasr_transcribe_feats(self.ctx, p, n, _ptr(cat), _ptr(nf)))

    # ------------------------------------------------------------------ the optional outputs of the lattice calls, and utterance i of them
    @staticmethod
    def _vit_buffers(n, n_tok, viterbi, logps=True):
        """host outputs of the alignment pass, in the order of the C arguments: viterbi [n], frames and (logps=True) logps [n_tok];
        None each without the pass"""
        k = max(n_tok, 1)
        return (np.zeros(n, dtype=np.float64) if viterbi else None, np.zeros(k, dtype=np.int32) if viterbi else None,
                np.zeros(k, dtype=np.float32) if viterbi and logps else None)

    @staticmethod
    def _vit_slice(vit, i, u, o):
        """one utterance of the alignment pass' outputs: entry i, u labels from o"""
        v, fr, lp = vit
        if v is None:
            return {}
        r = dict(viterbi=float(v[i]), frames=fr[o:o + u].copy())
        return r if lp is None else dict(r, logps=lp[o:o + u].copy())

    @staticmethod
    def _post_buffers(cells, n_tok):
        """host outputs of a posterior call, in the order of the C arguments: occ_blank, occ_emit, tok_mean, tok_var, tok_peak_frame, tok_peak"""
        k = max(n_tok, 1)
        return (np.zeros(cells, dtype=np.float32), np.zeros(cells, dtype=np.float32), np.zeros(k, dtype=np.float64),
                np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.float64))

    @staticmethod
    def _post_slice(post, t, w, u, oc, o):
        """one utterance of the posterior outputs: t rows of w cells from oc, u labels from o"""
        ob, oe, mean, var, pf, peak = post
        return dict(occ_blank=_rows(ob, oc, t, w), occ_emit=_rows(oe, oc, t, w),
                    tok_mean=mean[o:o + u].copy(), tok_var=var[o:o + u].copy(), tok_peak_frame=pf[o:o + u].copy(), tok_peak=peak[o:o + u].copy())

    @staticmethod
    def _walk(U, T=None, W=None):
        """per utterance (i, u labels, t frames, w cells per row -- None: the full lattice's u + 1 --, and where its labels, cells and
        frames start in the concatenated outputs: o, oc, ot)"""
        o = oc = ot = 0
        for i, u in enumerate(U):
            u, t = int(u), 0 if T is None else int(T[i])
            w = u + 1 if W is None else int(W[i])
            yield i, u, t, w, o, oc, ot
            o, oc, ot = o + u, oc + t * w, ot + t

    def _align_frames(self, lens, pcm):
        d = self.desc
        if not pcm:
            return [int(v) for v in lens]
        return [((1 + int(v) // d.hop) - d.n_stack) // d.stride + 1 for v in lens]

    # ------------------------------------------------------------------ forced alignment / transcript scoring
    def _align(self, pcm, slots, audio, token_lists, lattice, viterbi, posteriors=False, band=None, max_passes=1, windows=None):
        """lasr_align_[band_][post_]{pcm,feats}, by name from (band, posteriors, pcm).  A row of utterance i has U_i + 1 cells, with a
        band w_i (band layout); the band adds "lo", "width", "passes", "touch", posteriors add lattice_post's six fields."""
        p, n, (cat, lens) = self._cat(pcm, slots, audio)
        assert len(token_lists) == n
        tok, U = _ragged(token_lists)
        Ts = self._align_frames(lens, pcm)      # what the library derives from the audio: the encoder frames of the utterance
        W = [int(u) + 1 if band is None or t == 1 else min(int(band), int(u) + 1) for t, u in zip(Ts, U)]
        cells, n_tok = max(sum(t * w for t, w in zip(Ts, W)), 1), int(tok.size)
        loglik = np.zeros(n, dtype=np.float64)
        vit = self._vit_buffers(n, n_tok, viterbi)
        b, e = (np.zeros(cells, dtype=np.float32), np.zeros(cells, dtype=np.float32)) if lattice else (None, None)
        args, outs = [self.ctx, p, n, _ptr(cat), _ptr(lens), _ptr(tok), _ptr(U)], [loglik, *vit, b, e]
        if band is not None:
            lo_in = None
            if windows is not None:
                assert len(windows) == n
                lo_in = _ragged(windows)[0]
                if lo_in.size != sum(Ts):
                    raise N.LasrError(N.LASR_EINVAL, "windows: one start per encoder frame of every utterance")
            lo, passes, touch = np.zeros(max(sum(Ts), 1), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            args += [int(band), int(max_passes), _ptr(lo_in)]
            outs += [lo, passes, touch]
        post = self._post_buffers(cells, n_tok) if posteriors else ()
        fn = getattr(self.lib, "lasr_align_" + ("band_" if band is not None else "") + ("post_" if posteriors else "") + ("pcm" if pcm else "feats"))
        self._chk(fn(*args, *[_ptr(x) for x in (*outs, *post)]))
        out = []
        for i, u, t, w, o, oc, ot in self._walk(U, Ts, W):
            r = {"loglik": float(loglik[i]), **self._vit_slice(vit, i, u, o)}
            if lattice:
                r.update(blank_lp=_rows(b, oc, t, w), emit_lp=_rows(e, oc, t, w))
            if band is not None:
                r.update(lo=lo[ot:ot + t].copy(), width=w, passes=int(passes[i]), touch=int(touch[i]))
            if posteriors:
                r.update(self._post_slice(post, t, w, u, oc, o))
            out.append(r)
        return out

    @staticmethod
    def band_windows(T, U, band, frames=None, lo=None):
        """The window arithmetic of the banded lattice (lasr_band_windows; host only, no context: callable on the class).  frames=None: the linear windows of T frames,
        U labels and the requested width band; otherwise the windows recentred on the best path `frames` [U] that was found inside
        the windows `lo` [T].  -> (lo int32 [T], touch: 1 iff that path ran along an edge of `lo` that is not the lattice's own)."""
        out = np.zeros(max(int(T), 1), dtype=np.int32)
        touch = C.c_int(0)
        fr = cur = None
        if frames is not None:
            fr = np.ascontiguousarray(np.asarray(frames, dtype=np.int32).reshape(-1))
            if fr.size != int(U) or lo is None:
                raise N.LasrError(N.LASR_EINVAL, "lasr_band_windows: frames needs U entries and the windows it was found in")
            fr = np.concatenate([fr, np.zeros(1, np.int32)])          # (never null, so U = 0 still means "recentre")
            cur = np.ascontiguousarray(np.asarray(lo, dtype=np.int32).reshape(-1))
            if cur.size != int(T):
                raise N.LasrError(N.LASR_EINVAL, "lasr_band_windows: lo needs T entries")
        rc = N.lib().lasr_band_windows(int(T), int(U), int(band), _ptr(fr), _ptr(cur), _ptr(out), C.byref(touch))
        if rc != 0:
            raise N.LasrError(rc, "lasr_band_windows: bad argument")
        return out[:int(T)].copy(), int(touch.value)

    def lattice_band_dp(self, blank, emit, lo, U, viterbi=True):
        """The banded dynamic programme alone (lasr_lattice_band_dp) on caller-supplied band lattices: blank / emit = lists of
        [T_i, w_i] float32 arrays in band layout (row t holds the columns lo_i[t] .. lo_i[t] + w_i - 1), lo = their window starts,
        U = their label counts.  -> per lattice {"loglik", "viterbi", "frames"}."""
        return self._lattice_dp(self.lib.lasr_lattice_band_dp, self._band_lattices(blank, emit, lo, U), viterbi)

    @staticmethod
    def _lattices(blank, emit):
        """caller-supplied lattices concatenated -> (n, b, e, T, their second dimension)"""
        n = len(blank)
        assert n == len(emit) and n >= 1
        bs, es = ([np.asarray(x, dtype=np.float32) for x in xs] for xs in (blank, emit))
        assert all(x.ndim == 2 and x.shape == y.shape for x, y in zip(bs, es))
        b, e = (np.ascontiguousarray(np.concatenate([x.reshape(-1) for x in xs])) for xs in (bs, es))
        return n, b, e, np.array([x.shape[0] for x in bs], dtype=np.int32), np.array([x.shape[1] for x in bs], dtype=np.int32)

    def _band_lattices(self, blank, emit, lo, U):
        """the inputs of lattice_band_dp / lattice_band_post in the order of the C arguments: (b, e, T, U, W, lo)"""
        n, b, e, T, W = self._lattices(blank, emit)
        assert n == len(lo) == len(U)
        los = _ragged(lo)[0]
        assert los.size == int(T.sum())
        return b, e, T, np.array([int(u) for u in U], dtype=np.int32), W, los

    def _lattice_dp(self, fn, ins, viterbi):
        """lasr_lattice_dp / lasr_lattice_band_dp on ins = (b, e, T, U, ..), the C inputs in order"""
        U = ins[3]
        n = int(U.size)
        loglik, vit = np.zeros(n, dtype=np.float64), self._vit_buffers(n, int(U.sum()), viterbi, logps=False)
        self._chk(fn(self.ctx, *[_ptr(x) for x in ins], n, _ptr(loglik), _ptr(vit[0]), _ptr(vit[1])))
        return [{"loglik": float(loglik[i]), **self._vit_slice(vit, i, u, o)} for i, u, _, _, o, _, _ in self._walk(U)]

    def _lattice_post(self, fn, ins, W):
        """lasr_lattice_post / lasr_lattice_band_post on ins = (b, e, T, U, ..), the C inputs in order; W: the cells per row"""
        b, _, T, U = ins[:4]
        n = int(U.size)
        loglik, bwd, post = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64), self._post_buffers(int(b.size), int(U.sum()))
        self._chk(fn(self.ctx, *[_ptr(x) for x in ins], n, _ptr(loglik), _ptr(bwd), *[_ptr(x) for x in post]))
        return [{"loglik": float(loglik[i]), "loglik_bwd": float(bwd[i]), **self._post_slice(post, t, w, u, oc, o)}
                for i, u, t, w, o, oc, _ in self._walk(U, T, W)]

    def lattice_band_post(self, blank, emit, lo, U):
        """Banded forward-backward alone (lasr_lattice_band_post) on caller-supplied band lattices, the arguments of lattice_band_dp.
        -> per lattice lattice_post's dict, "occ_blank" / "occ_emit" [T, w] float32 in band layout."""
        ins = self._band_lattices(blank, emit, lo, U)
        return self._lattice_post(self.lib.lasr_lattice_band_post, ins, ins[4])

    def align_pcm(self, slots, pcm_list, token_lists, lattice=False, viterbi=True, posteriors=False, band=None, max_passes=1, windows=None):
        """Teacher-forced RNN-T lattice of every (utterance, transcript) pair (lasr_align_pcm): pcm_list as for transcribe_pcm,
        token_lists[i] = non-blank ids.  -> per utterance {"loglik": log P(y | x) over all alignments, "viterbi": best path's score,
        "frames" / "logps": per label the encoder frame it falls on and the joint's log p there}; lattice=True adds "blank_lp" /
        "emit_lp" [T, U + 1] float32; viterbi=False skips the alignment pass (scoring only).  posteriors=True (lasr_align_post_pcm)
        adds the lattice's edge posteriors over all alignments: "occ_blank" / "occ_emit" [T, U + 1] float32 (occ_emit[t, u] = the
        probability that label u + 1 is emitted on frame t) and per label "tok_mean" / "tok_var" (mean and variance of its emission
        frame), "tok_peak_frame" / "tok_peak" (its most probable frame and the probability there).  The slots are left freshly reset.
        band=W (lasr_align_band_pcm): the lattice restricted to W labels per frame -- w = min(W, U + 1) (U + 1 on a single frame) --
        starting from `windows` (per utterance the T window starts; None: linear) and recentred on the best path for up to max_passes
        passes; transcripts of up to 32767 labels.  The dict then also has "lo" int32 [T] (the last pass's windows), "width",
        "passes" and "touch", and the lattice arrays are [T, w] in band layout (row t holds the columns lo[t] .. lo[t] + w - 1).
        band with posteriors=True raises ValueError: the band's posteriors are align_band_post_pcm's."""
        return self._align_public(True, slots, pcm_list, token_lists, lattice, viterbi, posteriors, band, max_passes, windows)

    def _align_public(self, pcm, slots, audio, token_lists, lattice, viterbi, posteriors, band, max_passes, windows):
        """align_pcm / align_feats: _align, minus the combination that has methods of its own"""
        if band is not None and posteriors:
            raise ValueError("posteriors with a band: use align_band_post_pcm / align_band_post_feats")
        return self._align(pcm, slots, audio, token_lists, lattice, viterbi, posteriors, band, max_passes, windows)

    def align_feats(self, slots, feats_list, token_lists, lattice=False, viterbi=True, posteriors=False, band=None, max_passes=1, windows=None):
        """align_pcm from stacked features (lasr_align_feats; with a band lasr_align_band_feats): feats_list as for transcribe_feats."""
        return self._align_public(False, slots, feats_list, token_lists, lattice, viterbi, posteriors, band, max_passes, windows)

    def align_band_post_pcm(self, slots, pcm_list, token_lists, band, max_passes=1, windows=None, lattice=False, viterbi=True):
        """align_pcm(band=...) with the BAND's edge posteriors (lasr_align_band_post_pcm): the dicts of the banded call -- "lo", "width",
        "passes", "touch", lattice arrays [T, w] in band layout -- plus "occ_blank" / "occ_emit" [T, w] float32 in band layout
        (occ_emit[t, k] = the probability, over the alignments inside the windows, that label lo[t] + k + 1 is emitted on frame t) and
        per label "tok_mean", "tok_var", "tok_peak_frame", "tok_peak" as align_pcm(posteriors=True).  With max_passes > 1 they are
        those of the last pass's windows ("lo").  No path through the windows (loglik -inf): occupancies 0, tok_mean -1, tok_var 0,
        tok_peak_frame -1, tok_peak 0.  At most 2^24 band cells in the call."""
        return self._align(True, slots, pcm_list, token_lists, lattice, viterbi, True, int(band), max_passes, windows)

    def align_band_post_feats(self, slots, feats_list, token_lists, band, max_passes=1, windows=None, lattice=False, viterbi=True):
        """align_band_post_pcm from stacked features (lasr_align_band_post_feats): feats_list as for transcribe_feats."""
        return self._align(False, slots, feats_list, token_lists, lattice, viterbi, True, int(band), max_passes, windows)

    def lattice_dp(self, blank, emit, viterbi=True):
        """The lattice dynamic programme alone (lasr_lattice_dp) on caller-supplied lattices: blank / emit = lists of [T_i, U_i + 1]
        float32 arrays (column U_i of emit is not read).  -> per lattice {"loglik", "viterbi", "frames"}."""
        _, b, e, T, W = self._lattices(blank, emit)
        return self._lattice_dp(self.lib.lasr_lattice_dp, (b, e, T, W - 1), viterbi)

    def lattice_post(self, blank, emit):
        """Forward-backward alone (lasr_lattice_post) on caller-supplied lattices, blank / emit as for lattice_dp.  -> per lattice
        {"loglik", "loglik_bwd", "occ_blank", "occ_emit" [T, U + 1] float32, "tok_mean", "tok_var", "tok_peak_frame", "tok_peak" [U]}."""
        _, b, e, T, W = self._lattices(blank, emit)
        return self._lattice_post(self.lib.lasr_lattice_post, (b, e, T, W - 1), W)

    # ------------------------------------------------------------------ n-best rescoring over a prefix tree
    def prefix_tree(self, token_lists):
        """The candidates merged into a prefix tree (lasr_prefix_tree; host only).  -> {"parent", "label", "depth": int32 [N],
        "term": int32 [k], the node of every candidate}: node 0 is the empty prefix, parent[v] < v, depth non-decreasing, the
        children of a node contiguous."""
        tok, nt = _ragged(token_lists)
        k, cap = int(nt.size), int(nt.sum()) + 1
        par, lab, dep = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        term = np.zeros(max(k, 1), dtype=np.int32)
        n = C.c_int(0)
        rc = self.lib.lasr_prefix_tree(_ptr(tok), _ptr(nt), k, cap, _ptr(par), _ptr(lab), _ptr(dep), _ptr(term), C.byref(n))
        if rc != 0:
            raise N.LasrError(rc, "lasr_prefix_tree: bad candidate list")
        return {"parent": par[:n.value].copy(), "label": lab[:n.value].copy(), "depth": dep[:n.value].copy(), "term": term[:k].copy()}

    # ------------------------------------------------------------------ contextual biasing (hotwords)
    def bias_compile(self, phrases, weights):
        """Phrases (token-id lists) and one weight each (log-prob units, finite, >= 0) -> BiasGraph, the phrase automaton of
        lasr_bias_compile (host only; include/lasr.h has the definition)."""
        return bias_compile(self.lib, phrases, weights, self.desc.vocab, self.desc.blank)

    def set_bias(self, graph):
        """Attach a BiasGraph to the context (every slot is biased and restarts at the root); None turns biasing off.  Needs
        an idle context and greedy decode without an LM (lasr_set_bias)."""
        if graph is None:
            self._chk(self.lib.lasr_set_bias(self.ctx, 0, None, None, None, None))
            return
        if graph.node_back is not None:
            raise ValueError("set_bias: a graph in beam form (it carries node_back); bias_compile gives the greedy form")
        self._chk(self.lib.lasr_set_bias(self.ctx, int(graph.n_nodes), _ptr(graph.edge_off), _ptr(graph.edge_tok),
                                         _ptr(graph.edge_next), _ptr(graph.edge_bonus)))

    def bias_state(self, slots):
        """-> int32 [n]: the automaton node of every listed slot (synchronises)"""
        a, p, n = self._slots(slots)
        out = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self.lib.lasr_bias_state(self.ctx, p, n, _ptr(out)))
        return out[:n]

    def bias_pick(self, logits, nodes):
        """One biased decision per row: logits [B, vocab] (device f32), nodes [B] -> (tok int32 [B], next int32 [B], logp
        float32 [B]) on the host (lasr_bias_pick; no slot's state is touched)."""
        logits = logits.contiguous()
        B = int(logits.shape[0])
        nd = np.ascontiguousarray(np.asarray(nodes, dtype=np.int32).reshape(-1))
        if nd.size != B or logits.shape[1] != self.desc.vocab or logits.dtype != torch.float32:
            raise ValueError("bias_pick: logits [B, vocab] float32 and one node per row")
        tok, nxt, lp = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
        self._chk(self.lib.lasr_bias_pick(self.ctx, _ptr(logits), _ptr(nd), B, _ptr(tok), _ptr(nxt), _ptr(lp)))
        return tok, nxt, lp

    # ------------------------------------------------------------------ contextual biasing in the beam
    def beam_bias_compile(self, phrases, weights):
        """Phrases (token-id lists) and one weight each (log-prob units, finite, >= 0) -> BeamBiasGraph, the phrase automaton in
        beam form (lasr_beam_bias_compile, host only; include/lasr.h has the definition)."""
        return beam_bias_compile(self.lib, phrases, weights, self.desc.vocab, self.desc.blank)

    def set_beam_bias(self, graph):
        """Attach a BeamBiasGraph to a beam context (every hypothesis slot is biased and restarts at the root; the scores stay);
        None turns biasing off.  Needs an idle context and no LM (lasr_set_beam_bias).  The attached graph is kept as
        self.beam_bias for bias_walk."""
        if graph is None:
            self._chk(self.lib.lasr_set_beam_bias(self.ctx, 0, None, None, None, None, None))
            self.beam_bias = None
            return
        if graph.node_back is None:
            raise ValueError("set_beam_bias: a graph in greedy form (no node_back); beam_bias_compile gives the beam form")
        self._chk(self.lib.lasr_set_beam_bias(self.ctx, int(graph.n_nodes), _ptr(graph.edge_off), _ptr(graph.edge_tok),
                                              _ptr(graph.edge_next), _ptr(graph.edge_gain), _ptr(graph.node_back)))
        self.beam_bias = graph

    def beam_bias_state(self, slot):
        """-> int32 [beam]: the automaton nodes of the stream's hypothesis slots in slot order, -1 for a dead slot (synchronises)"""
        out = np.zeros(self.beam, dtype=np.int32)
        self._chk(self.lib.lasr_beam_bias_state(self.ctx, int(slot), _ptr(out)))
        return out

    def bias_walk(self, tokens, start=0, graph=None):
        """Tokens through `graph` (default: the attached one) from node `start` -> (end node, summed gain, gains float32 [n]);
        host only (lasr_bias_walk).  score - summed gain is a hypothesis' acoustic score."""
        graph = self.beam_bias if graph is None else graph
        if graph is None:
            raise ValueError("bias_walk: no graph attached and none given")
        return bias_walk(self.lib, graph, tokens, self.desc.blank, start)

    def beam_bias_round(self, logits, score, alive, inB, node, rounds, max_iters):
        """One biased selection round of n streams: logits [n * beam, vocab] (device f32), per-row score / alive / inB / node and
        per-stream rounds done -> dict of host arrays parent, token, emit, score, alive, inB, node, term (lasr_beam_bias_round;
        no slot's state is touched)."""
        logits = logits.contiguous()
        R = int(logits.shape[0])
        sc = np.ascontiguousarray(np.asarray(score, dtype=np.float64).reshape(-1))
        al, ib, nd = (np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(-1)) for x in (alive, inB, node))
        rd = np.ascontiguousarray(np.asarray(rounds, dtype=np.int32).reshape(-1))
        n = rd.size
        if R != n * self.beam or any(x.size != R for x in (sc, al, ib, nd)) or logits.shape[1] != self.desc.vocab or logits.dtype != torch.float32:
            raise ValueError("beam_bias_round: logits [n * beam, vocab] float32, one score / alive / inB / node per row, rounds [n]")
        torch.cuda.synchronize(self.device)
        o = {k: np.zeros(R, np.int32) for k in ("parent", "token", "emit", "alive", "inB", "node")}
        o["score"], o["term"] = np.zeros(R, np.float64), np.zeros(R, np.float32)
        self._chk(self.lib.lasr_beam_bias_round(self.ctx, _ptr(logits), n, _ptr(sc), _ptr(al), _ptr(ib), _ptr(nd), _ptr(rd), int(max_iters),
                                                _ptr(o["parent"]), _ptr(o["token"]), _ptr(o["emit"]), _ptr(o["score"]), _ptr(o["alive"]),
                                                _ptr(o["inB"]), _ptr(o["node"]), _ptr(o["term"])))
        return o

    def _score(self, pcm, slots_per_utt, audio, cand_lists, viterbi, lattice):
        n = len(slots_per_utt)
        assert len(audio) == n
        cat, lens = self._cat_pcm(audio) if pcm else self._cat_feats(audio)
        assert len(cand_lists) == n and all(len(s) == len(c) for s, c in zip(slots_per_utt, cand_lists))
        a, p, K = self._slots([s for grp in slots_per_utt for s in grp])
        nc = np.array([len(c) for c in cand_lists], dtype=np.int32)
        tok, nt = _ragged([t for c in cand_lists for t in c])
        loglik = np.zeros(max(K, 1), dtype=np.float64)
        vit = np.zeros(max(K, 1), dtype=np.float64) if viterbi else None
        trees = Ts = Nn = b = e = None
        if lattice:      # the tree is what the library builds from the same candidates; T_i what it derives from the audio
            trees = [self.prefix_tree(c) for c in cand_lists]
            Ts, Nn = self._align_frames(lens, pcm), [int(tr["parent"].size) for tr in trees]
            cells = max(sum(t * nn for t, nn in zip(Ts, Nn)), 1)
            b, e = np.zeros(cells, dtype=np.float32), np.zeros(cells, dtype=np.float32)
        fn = self.lib.lasr_score_pcm if pcm else self.lib.lasr_score_feats
        self._chk(fn(self.ctx, p, n, _ptr(cat), _ptr(lens), _ptr(nc), _ptr(tok), _ptr(nt), _ptr(loglik), _ptr(vit), _ptr(b), _ptr(e)))
        out = []
        for i, k, t, nn, o, oc, _ in self._walk(nc, Ts, Nn):
            r = {"loglik": loglik[o:o + k].copy()}
            if viterbi:
                r["viterbi"] = vit[o:o + k].copy()
            if lattice:
                r.update(tree=trees[i], blank_lp=_rows(b, oc, t, nn), emit_lp=_rows(e, oc, t, nn))
            out.append(r)
        return out

    def score_pcm(self, slots_per_utt, pcm_list, cand_lists, viterbi=False, lattice=False):
        """log P(candidate | audio) of every candidate of every utterance (lasr_score_pcm): each utterance is encoded once, its
        candidates share every joint row they have a prefix in common for.  slots_per_utt[i]: one open slot per candidate of
        utterance i (all distinct); cand_lists[i]: its candidates (non-blank ids).  -> per utterance {"loglik": float64 [k]};
        viterbi=True adds "viterbi" [k]; lattice=True adds "tree" (prefix_tree of the candidates) and "blank_lp" / "emit_lp"
        [T, N] float32 (emit_lp[t, v] = the emission that enters node v).  The slots are left freshly reset."""
        return self._score(True, slots_per_utt, pcm_list, cand_lists, viterbi, lattice)

    def score_feats(self, slots_per_utt, feats_list, cand_lists, viterbi=False, lattice=False):
        """score_pcm from stacked features (lasr_score_feats): feats_list as for transcribe_feats."""
        return self._score(False, slots_per_utt, feats_list, cand_lists, viterbi, lattice)

    def lm_score(self, slots, token_lists, start=None):
        """log P_LM of every candidate by the attached LM (lasr_lm_score): slots[i] = one open slot per candidate (all distinct, its LM
        row), token_lists[i] = its non-blank ids.  start=None: the LM reads y_1..y_{U-1} and the first label has no term (0); start=id:
        the LM reads (start, y_1, .., y_{U-1}) and every label has one.  -> per candidate {"total": float, "logps": float32 [U]}.
        The slots' LM state is left reset (reset(slot, 4)); nothing else changes."""
        a, p, n = self._slots(slots)
        assert len(token_lists) == n
        tok, nt = _ragged(token_lists)
        total = np.zeros(max(n, 1), dtype=np.float64)
        lp = np.zeros(max(int(tok.size), 1), dtype=np.float32)
        self._chk(self.lib.lasr_lm_score(self.ctx, p, n, _ptr(tok), _ptr(nt), -1 if start is None else int(start), _ptr(total), _ptr(lp)))
        return [{"total": float(total[i]), "logps": lp[o:o + u].copy()} for i, u, _, _, o, _, _ in self._walk(nt)]

    def lattice_tree_dp(self, blank, emit, parent, viterbi=True):
        """The tree dynamic programme alone (lasr_lattice_tree_dp) on caller-supplied lattices: blank / emit = lists of [T_i, N_i]
        float32 arrays (emit[:, 0] is not read), parent = lists of N_i node ids (-1 at node 0, parent[v] < v, depth
        non-decreasing).  -> per lattice {"loglik": float64 [N_i], "viterbi": float64 [N_i]}: log P(prefix_v | x) per node."""
        n, b, e, T, Nn = self._lattices(blank, emit)
        assert n == len(parent)
        par, sizes = _ragged(parent)
        assert np.array_equal(sizes, Nn)
        loglik = np.zeros(int(Nn.sum()), dtype=np.float64)
        vit = np.zeros(int(Nn.sum()), dtype=np.float64) if viterbi else None
        self._chk(self.lib.lasr_lattice_tree_dp(self.ctx, _ptr(b), _ptr(e), _ptr(T), _ptr(Nn), _ptr(par), n, _ptr(loglik), _ptr(vit)))
        return [{"loglik": loglik[o:o + k].copy(), **({"viterbi": vit[o:o + k].copy()} if viterbi else {})}
                for _, k, _, _, o, _, _ in self._walk(Nn)]

    # ------------------------------------------------------------------ op-level (tests, microbench)
    def logmel(self, pcm):
        """pcm [B, N] cuda float32 -> [B, T, n_mels]"""
        assert pcm.is_cuda and pcm.dtype == torch.float32 and pcm.dim() == 2
        pcm = pcm.contiguous()
        B, Ns = pcm.shape
        T = 1 + Ns // self.desc.hop
        out = torch.empty(B, T, self.desc.n_mels, device=pcm.device, dtype=torch.float32)
        self._chk(self.lib.lasr_logmel(self.ctx, _ptr(pcm), B, Ns, _ptr(out)))
        return out

    def resample(self, pcm, sr_in):
        """pcm [B, N] float32 cuda at `sr_in` Hz -> [B, N'] at the model's rate (Resample, transforms.py:135-144)."""
        assert pcm.is_cuda and pcm.dtype == torch.float32 and pcm.dim() == 2
        pcm = pcm.contiguous()
        B, N = pcm.shape
        n_out = C.c_int64(0)
        self._chk(self.lib.lasr_resample(self.ctx, None, B, N, int(sr_in), None, C.byref(n_out)))
        out = torch.empty(B, n_out.value, device=pcm.device, dtype=torch.float32)
        self._chk(self.lib.lasr_resample(self.ctx, _ptr(pcm), B, N, int(sr_in), _ptr(out), C.byref(n_out)))
        return out

    def stack(self, logmel):
        logmel = logmel.contiguous()
        B, T, _ = logmel.shape
        d = self.desc
        Tp = 0 if T < d.n_stack else (T - d.n_stack) // d.stride + 1
        out = torch.empty(B, Tp, d.feat, device=logmel.device, dtype=torch.float32)
        tp = C.c_int(0)
        self._chk(self.lib.lasr_stack(self.ctx, _ptr(logmel), B, T, _ptr(out), C.byref(tp)))
        assert tp.value == Tp
        return out

    def encoder(self, feats, return_state=False):
        """feats [B, T', feat] cuda -> [B, T', hidden] (fresh learned initial state; clobbers rows 0..B-1)."""
        feats = feats.contiguous()
        B, Tp, _ = feats.shape
        H, L = self.desc.hidden, self.desc.enc_layers
        out = torch.empty(B, Tp, H, device=feats.device, dtype=torch.float32)
        h = torch.empty(L, B, H, device=feats.device, dtype=torch.float32) if return_state else None
        c = torch.empty(L, B, H, device=feats.device, dtype=torch.float32) if return_state else None
        self._chk(self.lib.lasr_encoder(self.ctx, _ptr(feats), B, Tp, _ptr(out), _ptr(h), _ptr(c)))
        return (out, h, c) if return_state else out

    def predictor(self, tokens):
        """tokens [B, U] int (host) -> h_pred [B, hidden] after the last token, from the learned initial state."""
        tok = np.ascontiguousarray(np.asarray(tokens, dtype=np.int32))
        B, U = tok.shape
        out = torch.empty(B, self.desc.hidden, device=self.device, dtype=torch.float32)
        self._chk(self.lib.lasr_predictor(self.ctx, tok.ctypes.data_as(C.c_void_p), B, U, _ptr(out)))
        return out

    def joint(self, h_pred, h_enc):
        h_pred, h_enc = h_pred.contiguous(), h_enc.contiguous()
        B = h_pred.shape[0]
        logits = torch.empty(B, self.desc.vocab, device=h_pred.device, dtype=torch.float32)
        lp = torch.empty(B, device=h_pred.device, dtype=torch.float32)
        am = torch.empty(B, device=h_pred.device, dtype=torch.int32)
        self._chk(self.lib.lasr_joint(self.ctx, _ptr(h_pred), _ptr(h_enc), B, _ptr(logits), _ptr(lp), _ptr(am)))
        return logits, lp, am

    # ------------------------------------------------------------------ stats
    def set_profiling(self, on=True):
        self._chk(self.lib.lasr_set_profiling(self.ctx, 1 if on else 0))

    def stats(self):
        s = N.StepStats()
        self._chk(self.lib.lasr_get_stats(self.ctx, C.byref(s)))
        return {k: getattr(s, k) for k, _ in N.StepStats._fields_}

    def sync(self):
        self._chk(self.lib.lasr_sync(self.ctx))

    DEBUG_READS = dict(x0=0, enc_h=1, enc_c=2, pe=3, pp=4, pred_h=5, ring=6, pend=7, enc_out=8, ints=9, pendlog=10,
                       lm_h=11, lm_c=12, lm_raw=13, lmz=14, lm_valid=15, lm_tab=16, lm_qh=17, lm_sxh=18)

    def debug_read(self, what, index=0):
        """Resident state as a [rows, cols] float32 array (lasr_debug_read; tests and the soak tool)."""
        w = self.DEBUG_READS[what] if isinstance(what, str) else int(what)
        r, k = C.c_int(0), C.c_int(0)
        probe = np.empty(1, dtype=np.float32)
        rc = self.lib.lasr_debug_read(self.ctx, w, int(index), probe.ctypes.data_as(C.c_void_p), 0, C.byref(r), C.byref(k))
        if rc != N.LASR_EFULL:
            self._chk(rc)
        out = np.empty((r.value, k.value), dtype=np.float32)
        self._chk(self.lib.lasr_debug_read(self.ctx, w, int(index), out.ctypes.data_as(C.c_void_p), out.size, C.byref(r), C.byref(k)))
        return out

    def debug_enclog(self):
        """lasr_debug_enclog (LASR_DBG_ENCLOG=N): [steps, 32, M] uint32 checksums of the encoder's inputs and state behind each step."""
        n = C.c_int(0)
        rc = self.lib.lasr_debug_enclog(self.ctx, None, 0, C.byref(n))
        if rc != N.LASR_EFULL:
            self._chk(rc)
            return np.zeros((0, 32, self.config("M")), dtype=np.uint32)
        M = self.config("M")
        out = np.empty((n.value, 32, M), dtype=np.uint32)
        self._chk(self.lib.lasr_debug_enclog(self.ctx, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out

    def debug_fe_race(self, iters, aggressor, per_iter=4, lds_pad=-1):
        """lasr_debug_fe_race: (launches, (launch, row) pairs) of the log-mel kernel whose output changed beside the aggressor."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.lib.lasr_debug_fe_race(self.ctx, int(iters), int(aggressor), int(per_iter), int(lds_pad), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def config(self, key):
        """lasr_debug_config: the engine's resolved configuration (defaults + LASR_* switches), e.g. "enc_wave", "pump_G", "la_stream"."""
        v = C.c_int(0)
        self._chk(self.lib.lasr_debug_config(self.ctx, key.encode(), C.byref(v)))
        return int(v.value)

    def cell_prof(self, on=True):
        """In-job HIP-event timing of the encoder-cell launches (see lasr_cell_prof)."""
        self._chk(self.lib.lasr_cell_prof(self.ctx, int(on)))      # True / 1: events + in-kernel clocks; 2: clocks only

    def cell_prof_kernel(self):
        """-> (microseconds, launches, cells): the cell kernels' own durations since cell_prof(True) (in-kernel wall clock)
        and the LSTM cells they computed (a layer-wavefront launch holds several independent cells)."""
        us, n, k = C.c_double(0.0), C.c_longlong(0), C.c_longlong(0)
        self._chk(self.lib.lasr_cell_prof_kernel(self.ctx, C.byref(us), C.byref(n), C.byref(k)))
        return float(us.value), int(n.value), int(k.value)

    def trace(self, on=True):
        """Timestamped marks on the main / decode streams of the pipelined protocol (see lasr_trace)."""
        self._chk(self.lib.lasr_trace(self.ctx, 1 if on else 0))

    def trace_read(self, cap=8192):
        """-> [(tag, microseconds since trace(True)), ...] in record order."""
        us = (C.c_double * cap)()
        tags = (C.c_int * cap)()
        n = C.c_int(0)
        self._chk(self.lib.lasr_trace_read(self.ctx, us, tags, cap, C.byref(n)))
        return [(int(tags[i]), float(us[i])) for i in range(n.value)]

    def cell_prof_read(self):
        """-> (microseconds, cell launches) accumulated since cell_prof(True)."""
        us, n = C.c_double(0.0), C.c_longlong(0)
        self._chk(self.lib.lasr_cell_prof_read(self.ctx, C.byref(us), C.byref(n)))
        return us.value, n.value

    def bench_neighbour(self, kind, n_wg=0, ms=0):
        """Experiment: kind 1 (MFMA only) / 2 (HBM loads) / 3 (L2 hits) / 4 (Infinity Cache loads) starts a synthetic neighbour of n_wg one-wave workgroups for `ms` ms on a
        stream of its own and returns at once; kind 0 waits for it and returns what it achieved (TFLOP/s / GB/s)."""
        r = C.c_double(0.0)
        self._chk(self.lib.lasr_bench_neighbour(self.ctx, int(kind), int(n_wg), int(ms), C.byref(r)))
        return r.value

    def overlap_probe(self, delay_us=10000):
        """wall time / delay of two delay kernels, one per engine stream: ~1 = the streams overlap, ~2 = one hardware queue."""
        r = C.c_double(0.0)
        self._chk(self.lib.lasr_overlap_probe(self.ctx, int(delay_us), C.byref(r)))
        return r.value

    def bench_cell(self, layer=1, iters=200):
        us = C.c_double(0.0)
        self._chk(self.lib.lasr_bench_cell(self.ctx, int(layer), int(iters), C.byref(us)))
        return us.value
