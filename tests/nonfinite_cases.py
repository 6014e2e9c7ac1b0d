"""Non-finite audio: the inputs and the oracle's answers shared by test_nonfinite_cpu.py and the test_gpu_nonfinite_*.py files
(no GPU here).  One sample of an utterance is replaced by NaN, +Inf, -Inf or a huge finite value; everything the numpy oracle
makes of that is computed once per process and never modified.

What the oracle defines (asserted in test_nonfinite_cpu.py):
  log-mel    the frame is multiplied by the Hann window zero-padded to n_fft, so a NaN or Inf sample poisons every frame whose
             1024-sample span holds it (0 * NaN = NaN); a huge finite sample only the frames that weigh it with a non-zero
             window weight (its square overflows the power spectrum -> log(inf), then inf - inf in the LayerNorm).
  encoder    one non-finite feature makes the LSTM state NaN; in streaming the state is carried, so every later frame is NaN.
  decisions  np.argmax of an all-NaN row is 0: with blank 0 the stream goes quiet; with a nonzero blank token 0 is emitted up
             to the symbol cap on every frame.  No exception anywhere."""
import numpy as np

from libreasr_amd import synth
from oracle import rnnt_oracle as O

F32 = np.float32
HUGE = 1e30                # squared it overflows float32 even under the smallest non-zero Hann weight (about 6e-5)
BAD = {"nan": np.nan, "inf": np.inf, "ninf": -np.inf, "huge": HUGE}
N_SAMPLES, POS = 32000, 16000          # 2 s at 16 kHz, the bad sample in the middle of a chunk
CHUNK, LEAD, TAIL = 1280, 1, 4
N_FFT, WIN, HOP = 1024, 400, 160
ROW = 3                    # the utterance that is poisoned: it still emits behind the bad sample, and the huge value (3 frames
                           # touched) and NaN (7 frames) cut its transcript at different tokens
NZ_MODEL = ("tiny", 2064, 2063)        # the nonzero-blank model (tests/decision_edges.py)

_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def clean_pcm():
    """[4, N_SAMPLES] float32 (read-only)"""
    def make():
        p = synth.synth_pcm(4, N_SAMPLES, seed=1234)
        p.setflags(write=False)
        return p
    return _once("pcm", make)


def poisoned(kind, row=ROW, pos=POS):
    """utterance `row` with sample `pos` replaced (a copy)"""
    p = clean_pcm()[row].copy()
    p[pos] = F32(BAD[kind])
    return p


def touched_frames(kind, pos, n_samples):
    """the log-mel frames of an n_samples signal (offline: centred, reflect-padded) that sample `pos` reaches, away from the
    reflected borders: NaN / Inf through any position of the n_fft span, the huge value through a non-zero window weight"""
    assert N_FFT // 2 < pos < n_samples - N_FFT // 2
    w = O.hann_periodic(WIN)
    out = []
    for t in range(1 + n_samples // HOP):
        if kind == "huge":
            k = pos - (t * HOP - WIN // 2)
            if 0 <= k < WIN and w[k] != 0:
                out.append(t)
        elif t * HOP - N_FFT // 2 <= pos < t * HOP + N_FFT // 2:
            out.append(t)
    return out


def tiny():
    """(state dict, cfg, oracle) of `tiny`, blank 0"""
    def make():
        cfg = synth.model_cfg("tiny")
        sd = synth.synth_state_dict(cfg, seed=0)
        return sd, cfg, O.OracleTransducer(sd, cfg)
    return _once("tiny", make)


def nonzero_blank():
    """the decision-edge model with blank = V - 1 (tests/decision_edges.py): .sd, .cfg, .blank, .bos, .m"""
    import decision_edges as D
    return D.model(*NZ_MODEL)


def chunks(pcm_row):
    return synth.stream_chunks(pcm_row, CHUNK, lead=LEAD, tail=TAIL)


def stream_feats(pcm_row):
    """the oracle's streaming front-end: [features of every model step]"""
    fe, out = O.StreamFrontend(), []
    for ch in chunks(pcm_row):
        o = fe.push(ch)
        if o is not None:
            out.append(o)
    return out


class StreamRef:
    """one stream through the oracle: steps = tokens per model step, tokens = all of them, T = frames per step"""

    def __init__(self, m, pcm_row, cap, operand=None):
        with np.errstate(all="ignore"):
            dec, self.steps, self.T = m.stream_decoder(max_iters=cap), [], []
            for o in stream_feats(pcm_row):
                self.steps.append([int(v) for v in dec.step(o)])
                self.T.append(o.shape[0])
        self.tokens = [v for s in self.steps for v in s]


def stream_ref(model, kind, cap=10, row=ROW):
    """model: "tiny", "tiny_bf16" or "nz"; kind: a key of BAD or None (clean).  Computed once."""
    def make():
        if model == "nz":
            m = nonzero_blank().m
        elif model == "tiny_bf16":
            sd, cfg, _ = tiny()
            m = O.OracleTransducer(sd, cfg, operand="bf16")
        else:
            m = tiny()[2]
        return StreamRef(m, clean_pcm()[row] if kind is None else poisoned(kind, row), cap)
    return _once(("stream", model, kind, cap, row), make)


def onset_step(kind, row=ROW):
    """index of the first model step whose features are not finite"""
    def make():
        with np.errstate(all="ignore"):
            bad = [not np.isfinite(o).all() for o in stream_feats(poisoned(kind, row))]
        return bad.index(True)
    return _once(("onset", kind, row), make)


def offline_ref(model, kind, cap=3, row=ROW):
    """-> tokens of decode_greedy over the whole utterance"""
    def make():
        m = nonzero_blank().m if model == "nz" else tiny()[2]
        with np.errstate(all="ignore"):
            return [int(v) for v in m.decode_greedy(O.features_offline(clean_pcm()[row] if kind is None else poisoned(kind, row)), max_iters=cap)[0]]
    return _once(("offline", model, kind, cap, row), make)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.int32)


def same_bits_or_nan(a, b):
    """NaN where the other is NaN, the same bit pattern everywhere else"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(bits(a)[~na], bits(b)[~nb]))
