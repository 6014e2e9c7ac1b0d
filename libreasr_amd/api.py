"""`LibreASR` facade named by the north star: load / transcribe / stream on top of the fused
device path (PCM in, token ids / text out; features never leave the GPU).

    asr = LibreASR.load("en", synthetic="cfg2")
    text = asr.transcribe(pcm)                       # 1-D float32 16 kHz, or path to a .flac / .wav (any rate: resampled on the GPU)
    for text_so_far in asr.stream(chunks): ...       # 80 ms float32 chunks (bytes / arrays / tensors)
"""
import contextlib

import numpy as np
import torch

from .lib.inference import load_stuff
from .lib.utils import tensorize


class LibreASR:
    def __init__(self, conf, lang, model, x_tfm, x_tfm_stream):
        self.conf, self.lang, self.model = conf, lang, model
        self.x_tfm, self.x_tfm_stream = x_tfm, x_tfm_stream
        self.engine = model.engine

    @classmethod
    def load(cls, lang="en", **kw):
        return cls(*load_stuff(lang, **kw))

    @staticmethod
    def _pcm(x):
        if isinstance(x, (bytes, bytearray)):
            return tensorize(bytes(x))[0].numpy()
        if isinstance(x, str):
            from . import flac
            pcm, sr, _ = flac.decode(x)
            if sr != 16000:
                raise NotImplementedError("only 16 kHz input is in scope")
            return pcm
        if isinstance(x, torch.Tensor):
            return x.reshape(-1)
        return np.asarray(x, dtype=np.float32).reshape(-1)

    def _utterance(self, x):
        """One utterance at the model rate.  Files (.flac, .wav; first channel, as ChannelCut transforms.py:128-132) at another rate
        go through the engine's resampler, the call the servicer makes for a unary request (Resample.encodes, transforms.py:135-144)."""
        if not isinstance(x, str):
            return self._pcm(x)
        if x.lower().endswith((".wav", ".wave")):
            from . import wav
            pcm, sr, _ = wav.decode(x)
        else:
            from . import flac
            pcm, sr, _ = flac.decode(x)
        if sr != self.engine.desc.sample_rate:
            pcm = self.engine.resample(torch.as_tensor(np.ascontiguousarray(pcm)[None]).to(self.engine.device), sr)[0]
        return pcm

    @contextlib.contextmanager
    def _open(self, n):
        """n open slots for the body of the `with`; every slot that was opened is closed on any exit, a failed open() included"""
        slots = []
        try:
            for _ in range(n):
                slots.append(self.engine.open())
            yield slots
        finally:
            for s in slots:
                self.engine.close_slot(s)

    def _groups(self, ys, call):
        """the candidates in groups of up to max_streams, each with one open slot per candidate: yields call(slots, group), the
        group's slots closed again"""
        g = self.engine.max_streams
        for i in range(0, len(ys), g):
            with self._open(len(ys[i:i + g])) as slots:
                res = call(slots, ys[i:i + g])
            yield res

    def _want_alignment(self):
        """Turns the engine's per-token records on (greedy decode only; a no-op when they are on already)."""
        if self.engine.beam > 1:
            raise NotImplementedError("return_alignment needs greedy decode; a beam engine returns its hypotheses with per-token "
                                      "times and confidences through nbest=k")
        self.engine.set_alignments(True)

    def _aligned(self, tokens, frames, logps):
        """-> [(token_id, time_s, confidence)]: time_s = frame * stride * hop / sample_rate, confidence = exp(log p)."""
        d = self.engine.desc
        dt = d.stride * d.hop / d.sample_rate
        return [(int(t), float(f) * dt, float(np.exp(np.float64(lp)))) for t, f, lp in zip(tokens, frames, logps)]

    def _want_nbest(self, nbest):
        """Turns the engine's whole-beam results on (beam search only; a no-op when they are on already)."""
        if self.engine.beam <= 1:
            raise ValueError("nbest= needs a beam engine (beam > 1); greedy decode has return_alignment=True")
        if int(nbest) < 1:
            raise ValueError("nbest must be >= 1")
        self.engine.set_beam_records(True)

    def _want_merge(self, merge):
        """merge=None leaves the engine's switch alone, True / False set it (lasr_set_beam_merge; beam search only); "lm" selects
        LASR_BEAM_MERGE_LM, the mode that also merges with an LM attached (synthetic_lm= / conf["lm"])."""
        if merge is None:
            return
        if self.engine.beam <= 1:
            raise ValueError("merge= needs a beam engine (beam > 1)")
        if isinstance(merge, str):
            if merge != "lm":
                raise ValueError('merge= takes None, True, False or "lm"')
            self.engine.set_beam_merge(True, lm=True)
        else:
            self.engine.set_beam_merge(bool(merge))

    def _nbest(self, slot, k, bonus=False):
        """-> up to k hypotheses, best first: {"score": sum of log p of every decision, "tokens": [(token_id, time_s, confidence)]}.
        With merging on (merge=True, Engine.set_beam_merge) the hypotheses are pairwise distinct and "score" is the log of the SUMMED
        probability of the alignments that were merged into the hypothesis; its times and confidences are those of the best-ranked
        alignment among them.
        bonus=True (offline results with beam hotwords set): "score" is the ranking score, hotword gains included, and "bonus" the
        summed gain of the hypothesis' tokens from the root (Engine.bias_walk): score - bonus is the acoustic score."""
        out = [{"score": sc, "tokens": self._aligned(t, f, lp)} for t, f, lp, sc in self.engine.fetch_nbest(slot, int(k))]
        if bonus:
            for h in out:
                h["bonus"] = float(self.engine.bias_walk([t[0] for t in h["tokens"]])[1])
        return out

    def transcribe(self, audio, return_ids=False, return_alignment=False, nbest=None, merge=None):
        """Whole utterance(s): fresh state, greedy, max_iters_offline (Transcribe RPC, api-server.py:64-80).
        return_alignment=True: per utterance a list of (token_id, time_s, confidence) instead of text -- time_s is the start of the
        80 ms encoder frame on which the token was emitted, confidence the joint's probability of that decision.  Greedy decode;
        a beam engine raises NotImplementedError: use nbest=.
        nbest=k (beam engines; ValueError on a greedy one): per utterance up to k hypotheses of the final beam, best first, each
        {"score": float, "tokens": [(token_id, time_s, confidence)]} with time_s / confidence as above; no merging, no length norm.
        With set_beam_hotwords in force "score" includes the hotword gains and each hypothesis also carries "bonus", their sum.
        merge=True / False (beam engines; ValueError on a greedy one) turns the merging of hypotheses that hold the same tokens on /
        off and the engine keeps the setting; None leaves it as it is.  See _nbest for what "score" means then.  merge=True raises
        on an engine with an LM attached; merge="lm" merges there too (identities follow the LM fuser's re-picked tokens; a score is
        then a log-sum of products of the joint's terms, not log P(tokens | audio)) and is merge=True on an engine without an LM."""
        batch = audio if isinstance(audio, (list, tuple)) else [audio]
        self._want_merge(merge)
        if return_alignment:
            self._want_alignment()
        if nbest is not None:
            self._want_nbest(nbest)
        with self._open(len(batch)) as slots:
            self.engine.transcribe_pcm(slots, [self._utterance(a) for a in batch])
            if nbest is not None:
                out = [self._nbest(s, nbest, bonus=getattr(self.engine, "beam_bias", None) is not None) for s in slots]
            elif return_alignment:
                out = [self._aligned(*self.engine.fetch_aligned(s)[:3]) for s in slots]
            else:
                ids = [self.engine.fetch(s)[0] for s in slots]
        if not return_alignment and nbest is None:
            out = ids if return_ids else [self.lang.denumericalize(i) for i in ids]
        return out if isinstance(audio, (list, tuple)) else out[0]

    def _ids(self, transcript):
        """A transcript as token ids: a sequence of ids, or text when the language object can numericalize."""
        if isinstance(transcript, str):
            if not hasattr(self.lang, "numericalize"):
                raise TypeError("this language object cannot numericalize text: pass token ids")
            transcript = self.lang.numericalize(transcript)
        return [int(t) for t in transcript]

    def _hotwords(self, who, phrases, boost):
        """the phrases as token-id lists and one boost each, for set_hotwords / set_beam_hotwords (`who`: the name in the text)"""
        ids = [self._ids(p) for p in phrases]
        w = [float(boost)] * len(ids) if np.ndim(boost) == 0 else [float(b) for b in boost]
        if len(w) != len(ids):
            raise ValueError("boost: one float, or one per phrase")
        if any(len(p) == 0 for p in ids) or not all(np.isfinite(b) and b >= 0 for b in w):
            raise ValueError(who + ": phrases of at least one token, boosts finite and >= 0")
        return ids, w

    def set_hotwords(self, phrases, boost=2.0):
        """Contextual biasing: greedy decode (transcribe and stream alike) prefers the listed phrases from now on.  phrases: lists
        of non-blank token ids, or text when the language object can numericalize (the rule `align` uses); boost: one float, or
        one per phrase -- finite, >= 0, in log-prob units, added to the joint's logit of a token that continues a phrase (the
        largest boost among the phrases that share the matched prefix).  None or [] clears.  The default 2.0 is a PLACEHOLDER for a
        knob nobody has tuned on real data: choose a value on held-out audio.  The bonus steers the choice only; reported
        confidences and scores stay the joint's.  Raises ValueError on a beam engine (it has set_beam_hotwords, where the bonus
        is part of the ranking score and a partial match that fails hands it back) and with an LM attached (the fuser re-picks
        on standardised scores, in which a bonus in log-prob units has no defined place)."""
        if phrases is None or len(phrases) == 0:
            self.engine.set_bias(None)
            return
        if self.engine.beam > 1:
            raise ValueError("set_hotwords needs greedy decode (beam = 1); a beam engine has set_beam_hotwords")
        if self.engine.lm_cfg is not None:
            raise ValueError("set_hotwords refuses an attached LM: the fuser re-picks on standardised scores, in which a bonus in "
                             "log-prob units has no defined place")
        self.engine.set_bias(self.engine.bias_compile(*self._hotwords("set_hotwords", phrases, boost)))

    def set_beam_hotwords(self, phrases, boost=1.0):
        """Contextual biasing of beam search (transcribe and stream alike): a hypothesis that matches a listed phrase token by token
        gains the phrase's boost in its RANKING score, spread over the tokens, and a partial match that fails hands back what it
        had gained -- so the bonus demotes as well as promotes, which greedy decode (set_hotwords) cannot do.  phrases and boost
        follow set_hotwords' rules: lists of non-blank token ids or text, one float or one per phrase, finite and >= 0, in
        log-prob units per matched token.  None or [] clears.  The default 1.0 is a PLACEHOLDER for a knob nobody has tuned on
        real data: choose a value on held-out audio.  With hotwords set, offline transcribe(nbest=...) results carry "bonus" (the
        summed gain of the hypothesis); "score" stays the ranking score.  Streams do not report the bonus: a frozen prefix hides
        where resets fell.  Raises ValueError on a greedy engine (it has set_hotwords) and with an LM attached (the combination
        is not served)."""
        if self.engine.beam <= 1:
            raise ValueError("set_beam_hotwords needs a beam engine (beam > 1); greedy decode has set_hotwords")
        if phrases is None or len(phrases) == 0:
            self.engine.set_beam_bias(None)
            return
        if self.engine.lm_cfg is not None:
            raise ValueError("set_beam_hotwords refuses an attached LM: the combination with LM fusion is not served")
        self.engine.set_beam_bias(self.engine.beam_bias_compile(*self._hotwords("set_beam_hotwords", phrases, boost)))

    def _posteriors(self, r):
        """per token of an align_pcm(posteriors=True) or align_band_post_pcm result: the lattice's view of where the token is, over all
        alignments (of a band: over those inside its windows; occ_emit is then in band layout, column u - lo[frame]).  Both
        probabilities are float32 values ("peak" is tok_peak rounded as occ_emit was), so posterior <= peak <= 1 holds exactly.  A
        token without a best-path frame (-1: no path through the windows) has posterior 0, no times and peak 0."""
        d = self.engine.desc
        dt = d.stride * d.hop / d.sample_rate
        lo = r.get("lo")
        out = []
        for k in range(len(r["frames"])):
            f = int(r["frames"][k])
            if f < 0:
                out.append({"posterior": 0.0, "time_mean_s": None, "time_std_s": None, "peak_time_s": None, "peak": 0.0})
                continue
            out.append({"posterior": float(r["occ_emit"][f, k if lo is None else k - int(lo[f])]),
                        "time_mean_s": float(r["tok_mean"][k]) * dt, "time_std_s": float(np.sqrt(r["tok_var"][k])) * dt,
                        "peak_time_s": float(r["tok_peak_frame"][k]) * dt, "peak": float(np.float32(r["tok_peak"][k]))})
        return out

    def _align_run(self, audio, transcript, call, posteriors, band):
        """the body of align / align_band: `call(slots, utterances, transcripts)` is the engine call"""
        many = isinstance(audio, (list, tuple))
        batch = list(audio) if many else [audio]
        ys = [self._ids(t) for t in (transcript if many else [transcript])]
        if len(ys) != len(batch):
            raise ValueError("one transcript per utterance")
        with self._open(len(batch)) as slots:
            res = call(slots, [self._utterance(a) for a in batch], ys)
        out = [{"score": r["loglik"], "viterbi": r["viterbi"], "tokens": self._aligned(y, r["frames"], r["logps"])} for r, y in zip(res, ys)]
        if posteriors:
            for o, r in zip(out, res):
                o["posteriors"] = self._posteriors(r)
        if band:
            for o, r in zip(out, res):
                o["band"] = {"width": int(r["width"]), "passes": int(r["passes"]), "touch": bool(r["touch"])}
        return out if many else out[0]

    def align(self, audio, transcript, posteriors=False, band=None, max_passes=4):
        """Forced alignment of a transcript the caller already has (the teacher-forced RNN-T lattice; greedy engines).  transcript: a
        list of non-blank token ids, or text when the language object can numericalize; lists of utterances / transcripts are batched.
        -> {"score": log P(transcript | audio) summed over all alignments, "viterbi": the best alignment's log-probability,
        "tokens": [(token_id, time_s, confidence)]} with time_s the start of the 80 ms encoder frame the token falls on in the best
        alignment and confidence the joint's probability of the token there.  posteriors=True adds "posteriors": per token
        {"posterior": the probability, over ALL alignments, that the token is emitted on that frame, "time_mean_s" / "time_std_s":
        mean and standard deviation of its emission time, "peak_time_s" / "peak": its most probable frame and the probability there}.
        band=W restricts the lattice to W labels per frame (lasr_align_band_pcm: cost linear in the audio's length, transcripts of
        up to 32767 labels), the windows recentred on the best path for up to max_passes passes; score and viterbi are then those of
        the band (score <= the full lattice's), and "band": {"width": the effective width, "passes": passes run, "touch": whether the
        last pass's path still ran along a window edge -- False is evidence, not proof, that the band did not constrain it} is added.
        band with posteriors=True raises ValueError: the band's posteriors are align_band's."""
        if band is not None and posteriors:
            raise ValueError("align: posteriors=True with a band is align_band(..., posteriors=True)")
        if band is None:
            call = lambda slots, pcm, ys: self.engine.align_pcm(slots, pcm, ys, posteriors=bool(posteriors))
        else:
            call = lambda slots, pcm, ys: self.engine.align_pcm(slots, pcm, ys, band=int(band), max_passes=int(max_passes))
        return self._align_run(audio, transcript, call, posteriors, band is not None)

    def align_band(self, audio, transcript, band=64, max_passes=4, posteriors=True):
        """align(band=...) for long recordings, with the band's own posteriors: align's dict with "band", and with posteriors=True
        (lasr_align_band_post_pcm) also "posteriors" as align(posteriors=True) gives them, over the alignments that stay inside the
        last pass's windows -- where "touch" cannot tell whether the band constrained the path, a token's posterior, time spread and
        peak are what shows how far its time can be trusted.  A token without a best-path frame (no path through the windows) gets
        {"posterior": 0.0, "time_mean_s": None, "time_std_s": None, "peak_time_s": None, "peak": 0.0}.  At most 2^24 band cells
        (frames x width, summed over the call) with posteriors."""
        if posteriors:
            call = lambda slots, pcm, ys: self.engine.align_band_post_pcm(slots, pcm, ys, int(band), max_passes=int(max_passes))
        else:
            call = lambda slots, pcm, ys: self.engine.align_pcm(slots, pcm, ys, band=int(band), max_passes=int(max_passes))
        return self._align_run(audio, transcript, call, posteriors, True)

    def score(self, audio, candidates):
        """log P(candidate | audio), summed over all alignments, of every candidate transcript of ONE utterance (rescoring an n-best
        list): one engine call per group of up to max_streams candidates.  The audio is encoded again for every candidate:
        `rescore` encodes it once per group and shares the candidates' common prefixes."""
        ys = [self._ids(t) for t in candidates]
        pcm = self._utterance(audio)
        call = lambda slots, part: self.engine.align_pcm(slots, [pcm] * len(part), part, viterbi=False)
        return [r["loglik"] for res in self._groups(ys, call) for r in res]

    def rescore(self, audio, candidates, viterbi=False):
        """log P(candidate | audio), summed over all alignments, of every candidate transcript of ONE utterance, in the candidates'
        order (text or ids, as in `score`), over a prefix tree of the candidates: per group of up to max_streams candidates one
        engine call that encodes the audio once and sends every distinct (frame, prefix) through the joint once (greedy engines).
        viterbi=True: -> (scores, best-alignment log-probabilities)."""
        ys = [self._ids(t) for t in candidates]
        pcm = self._utterance(audio)
        out, vit = [], []
        for r in self._groups(ys, lambda slots, part: self.engine.score_pcm([slots], [pcm], [part], viterbi=viterbi)[0]):
            out += [float(v) for v in r["loglik"]]
            if viterbi:
                vit += [float(v) for v in r["viterbi"]]
        return (out, vit) if viterbi else out

    def lm_score(self, candidates, start=None):
        """log P_LM(candidate) by the attached LM, of every candidate transcript (text or ids, as in `score`), in the candidates'
        order: one engine call per group of up to max_streams candidates.  start=None: the LM reads the labels themselves and the
        first one has no term; start=id: the LM reads that token first and every label has a term."""
        ys = [self._ids(t) for t in candidates]
        call = lambda slots, part: self.engine.lm_score(slots, part, start=start)
        return [float(r["total"]) for res in self._groups(ys, call) for r in res]

    def rescore_lm(self, audio, candidates, lm_weight, length_bonus=0.0, start=None):
        """Second-pass combination of ONE utterance's candidates: score = log P(candidate | audio) + lm_weight * log P_LM(candidate)
        + length_bonus * |candidate|, in float64.  Per group of up to max_streams candidates the slots are opened once and serve
        `rescore`'s engine call and `lm_score`'s.  -> {"am": rescore's scores, "lm": lm_score's totals, "score": the combination,
        "best": index of the largest score (a tie takes the lowest index), "order": indices by score descending, ties by index}."""
        ys = [self._ids(t) for t in candidates]
        pcm = self._utterance(audio)
        am, lm = [], []
        call = lambda slots, part: (self.engine.score_pcm([slots], [pcm], [part])[0]["loglik"], self.engine.lm_score(slots, part, start=start))
        for a, l in self._groups(ys, call):
            am += [float(v) for v in a]
            lm += [float(r["total"]) for r in l]
        score = [float(np.float64(a) + np.float64(lm_weight) * np.float64(l) + np.float64(length_bonus) * np.float64(len(y)))
                 for a, l, y in zip(am, lm, ys)]
        order = sorted(range(len(score)), key=lambda j: (-score[j], j))
        return {"am": am, "lm": lm, "score": score, "best": order[0] if order else None, "order": order}

    def stream(self, chunks, return_ids=False, return_alignment=False, nbest=None, merge=None):
        """One stream of client chunks (TranscribeStream RPC, api-server.py:82-134): yields the
        hypothesis so far after every model call.
        return_alignment=True: yields the list of (token_id, time_s, confidence) of the hypothesis so far.  time_s is NOMINAL for a
        stream: the streaming front-end takes each frame from the middle chunk of its 3-chunk window, so frame k * 80 ms is where
        the frame sits in the stream of model frames, not an exact position in the client's audio.
        nbest=k (beam engines): yields up to k hypotheses of the beam after that model call, as transcribe(nbest=k) returns them.
        merge=: as for transcribe."""
        eng = self.engine
        self._want_merge(merge)
        if return_alignment:
            self._want_alignment()
        if nbest is not None:
            self._want_nbest(nbest)
        slot = eng.open()
        y = []
        try:
            for ch in chunks:
                pcm = self._pcm(ch)
                pcm = pcm if isinstance(pcm, torch.Tensor) else np.asarray(pcm, np.float32)
                n = eng.desc.chunk
                if pcm.shape[0] < n:              # api-client.py:40-41 pads the last slice with zeros
                    pad = np.zeros(n, np.float32)
                    pad[: pcm.shape[0]] = np.asarray(pcm)
                    pcm = pad
                eng.push([slot], pcm[None] if not isinstance(pcm, torch.Tensor) else pcm[None])
                if eng.step([slot]):
                    if nbest is not None:
                        yield self._nbest(slot, nbest)
                        continue
                    if return_alignment:
                        y = y + self._aligned(*eng.fetch_aligned(slot)[:3])
                        yield list(y)
                        continue
                    got = eng.fetch(slot)[0]
                    y = got if eng.beam > 1 else y + got      # beam: the whole best hypothesis
                    yield list(y) if return_ids else self.lang.denumericalize(y)
        finally:
            eng.close_slot(slot)
