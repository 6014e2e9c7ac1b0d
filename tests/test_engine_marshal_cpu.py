"""The marshalling of Engine's offline methods without a GPU: a real Engine object over a fake library of plain Python functions.
Every fake entry point reads the count arrays through the pointers it is given, records the call (scalars, which pointers are null,
copies of the inputs), writes `BASE[name] + flat index` into every non-null output and returns 0.  The tests then know every element
of every returned array: a wrong offset, row width, dtype, argument order or null pointer shows as a wrong number."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from libreasr_amd import _native as N
from libreasr_amd.engine import Engine

FEAT = 16
I32, I64, F32, F64 = np.int32, np.int64, np.float32, np.float64
POST = ("occ_blank", "occ_emit", "tok_mean", "tok_var", "tok_peak_frame", "tok_peak")
OUTS = ("loglik", "vit", "fr", "lp", "b", "e", "lo", "passes", "touch", "bwd") + POST + ("par", "lab", "dep", "term", "total")
BASE = {k: 1000 * (i + 1) for i, k in enumerate(OUTS)}


def _null(p):
    return p is None or (isinstance(p, C.c_void_p) and p.value is None)


def _view(p, dtype, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(max(int(n), 1),))[:int(n)]


def _post(cells, su):
    return [("occ_blank", F32, cells), ("occ_emit", F32, cells), ("tok_mean", F64, su), ("tok_var", F64, su),
            ("tok_peak_frame", I32, su), ("tok_peak", F64, su)]


class FakeLib:
    """lasr_* entry points as Python functions.  calls: one dict per call -- "fn", "scalars", "nonnull" (the names of the pointer
    arguments that were not null) and "in" (copies of the input arrays)."""

    def __init__(self, desc):
        self.desc, self.calls = desc, []
        for k in dir(type(self)):      # one function object per entry point for the life of the library, as a CDLL's attributes are
            if k.startswith("lasr_"):
                setattr(self, k, getattr(self, k))

    def frames(self, lens, pcm):
        d = self.desc
        return np.array([((1 + int(v) // d.hop) - d.n_stack) // d.stride + 1 for v in lens] if pcm else lens, dtype=np.int64)

    def _run(self, fn, scalars, ins, outs):
        """ins / outs: (name, pointer, dtype, count).  An input that is null is recorded as absent."""
        rec = {"fn": fn, "scalars": scalars, "in": {}, "nonnull": {k for k, p, _, _ in ins + outs if not _null(p)}}
        for k, p, dt, n in ins:
            if not _null(p):
                rec["in"][k] = _view(p, dt, n).copy()
        for k, p, dt, n in outs:
            if not _null(p):
                _view(p, dt, n)[:] = BASE[k] + np.arange(int(n))
        self.calls.append(rec)
        return 0

    # ---- transcribe
    def _transcribe(self, pcm, ctx, slots, n, cat, lens):
        assert ctx is None
        ln = _view(lens, I64 if pcm else I32, n).copy()
        return self._run("transcribe_" + ("pcm" if pcm else "feats"), {"n": n},
                         [("slots", slots, I32, n), ("cat", cat, F32, ln.sum() * (1 if pcm else FEAT)), ("lens", lens, ln.dtype, n)], [])

    def lasr_transcribe_pcm(self, *a):
        return self._transcribe(True, *a)

    def lasr_transcribe_feats(self, *a):
        return self._transcribe(False, *a)

    # ---- the eight alignment entry points
    def _align(self, name, pcm, band, post, ctx, slots, n, cat, lens, tok, U, *rest):
        assert ctx is None
        rest = list(rest)
        ln, u = _view(lens, I64 if pcm else I32, n).copy(), _view(U, I32, n).copy().astype(np.int64)
        T = self.frames(ln, pcm)
        scalars, ins = {"n": n}, [("slots", slots, I32, n), ("cat", cat, F32, ln.sum() * (1 if pcm else FEAT)), ("lens", lens, ln.dtype, n),
                                  ("tok", tok, I32, u.sum()), ("U", U, I32, n)]
        if band:
            scalars.update(band=rest.pop(0), max_passes=rest.pop(0))
            ins.append(("lo_in", rest.pop(0), I32, T.sum()))
            W = np.array([x + 1 if t == 1 else min(scalars["band"], x + 1) for t, x in zip(T, u)], dtype=np.int64)
        else:
            W = u + 1
        cells, su = int((T * W).sum()), int(u.sum())
        spec = [("loglik", F64, n), ("vit", F64, n), ("fr", I32, su), ("lp", F32, su), ("b", F32, cells), ("e", F32, cells)]
        if band:
            spec += [("lo", I32, T.sum()), ("passes", I32, n), ("touch", I32, n)]
        if post:
            spec += _post(cells, su)
        assert len(rest) == len(spec), name
        return self._run(name, scalars, ins, [(k, p, dt, m) for (k, dt, m), p in zip(spec, rest)])

    # ---- caller-supplied lattices
    def _lattice(self, name, band, post, ctx, b, e, T, U, *rest):
        assert ctx is None
        rest = list(rest)
        W = lo = None
        if band:
            W, lo = rest.pop(0), rest.pop(0)
        n = rest.pop(0)
        t, u = _view(T, I32, n).copy().astype(np.int64), _view(U, I32, n).copy().astype(np.int64)
        w = _view(W, I32, n).copy().astype(np.int64) if band else u + 1
        cells, su = int((t * w).sum()), int(u.sum())
        ins = [("b", b, F32, cells), ("e", e, F32, cells), ("T", T, I32, n), ("U", U, I32, n)]
        if band:
            ins += [("W", W, I32, n), ("lo_in", lo, I32, t.sum())]
        spec = [("loglik", F64, n)] + ([("bwd", F64, n)] + _post(cells, su) if post else [("vit", F64, n), ("fr", I32, su)])
        assert len(rest) == len(spec), name
        return self._run(name, {"n": n}, ins, [(k, p, dt, m) for (k, dt, m), p in zip(spec, rest)])

    def lasr_lattice_tree_dp(self, ctx, b, e, T, Nn, par, n, loglik, vit):
        assert ctx is None
        t, nn = _view(T, I32, n).copy().astype(np.int64), _view(Nn, I32, n).copy().astype(np.int64)
        cells = int((t * nn).sum())
        return self._run("lattice_tree_dp", {"n": n}, [("b", b, F32, cells), ("e", e, F32, cells), ("T", T, I32, n), ("N", Nn, I32, n),
                                                       ("parent", par, I32, nn.sum())],
                         [("loglik", loglik, F64, nn.sum()), ("vit", vit, F64, nn.sum())])

    # ---- prefix tree: a chain of sum(n_tokens) + 1 nodes (the engine uses the node count only)
    def lasr_prefix_tree(self, tok, nt, k, cap, par, lab, dep, term, n_out):
        m = _view(nt, I32, k).copy()
        nodes = int(m.sum()) + 1
        assert cap >= nodes
        n_out._obj.value = nodes
        return self._run("prefix_tree", {"k": k, "cap": cap}, [("tok", tok, I32, m.sum()), ("nt", nt, I32, k)],
                         [("par", par, I32, nodes), ("lab", lab, I32, nodes), ("dep", dep, I32, nodes), ("term", term, I32, k)])

    # ---- scoring
    def _score(self, pcm, ctx, slots, n, cat, lens, nc, tok, nt, loglik, vit, b, e):
        assert ctx is None
        ln, c = _view(lens, I64 if pcm else I32, n).copy(), _view(nc, I32, n).copy()
        K = int(c.sum())
        m = _view(nt, I32, K).copy()
        nodes = [int(m[o:o + k].sum()) + 1 for o, k in zip(np.cumsum(c) - c, c)]
        cells = int(sum(int(t) * v for t, v in zip(self.frames(ln, pcm), nodes)))
        return self._run("score_" + ("pcm" if pcm else "feats"), {"n": n},
                         [("slots", slots, I32, K), ("cat", cat, F32, ln.sum() * (1 if pcm else FEAT)), ("lens", lens, ln.dtype, n),
                          ("nc", nc, I32, n), ("tok", tok, I32, m.sum()), ("nt", nt, I32, K)],
                         [("loglik", loglik, F64, K), ("vit", vit, F64, K), ("b", b, F32, cells), ("e", e, F32, cells)])

    def lasr_score_pcm(self, *a):
        return self._score(True, *a)

    def lasr_score_feats(self, *a):
        return self._score(False, *a)

    def lasr_lm_score(self, ctx, slots, n, tok, nt, start, total, lp):
        assert ctx is None
        m = _view(nt, I32, n).copy()
        return self._run("lm_score", {"n": n, "start": start}, [("slots", slots, I32, n), ("tok", tok, I32, m.sum()), ("nt", nt, I32, n)],
                         [("total", total, F64, n), ("lp", lp, F32, m.sum())])

    def lasr_last_error(self, ctx):
        return b"fake"


for _pcm, _band, _post_ in itertools.product((True, False), (False, True), (False, True)):
    _name = "lasr_align_" + ("band_" if _band else "") + ("post_" if _post_ else "") + ("pcm" if _pcm else "feats")
    setattr(FakeLib, _name, (lambda nm, p, bd, po: lambda self, *a: self._align(nm[5:], p, bd, po, *a))(_name, _pcm, _band, _post_))
for _band, _post_ in itertools.product((False, True), (False, True)):
    _name = "lasr_lattice_" + ("band_" if _band else "") + ("post" if _post_ else "dp")
    setattr(FakeLib, _name, (lambda nm, bd, po: lambda self, *a: self._lattice(nm[5:], bd, po, *a))(_name, _band, _post_))


def make_engine():
    d = N.ModelDesc()
    d.hop, d.n_stack, d.stride, d.feat = 160, 10, 8, FEAT
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.desc, eng.beam = FakeLib(d), None, d, 1
    return eng


# ----------------------------------------------------------------------------------------------------------------- shapes and inputs
BATCHES = {"three": dict(U=[3, 0, 1], T=[4, 1, 2], ns=[5280, 1600, 2720], band=2, W=[2, 1, 2]),
           "single": dict(U=[3], T=[1], ns=[1600], band=2, W=[4])}          # one frame: w = U + 1 whatever the band
KINDS = ("numpy", "torch", "mixed")


def audio(batch, pcm, kind):
    """-> (the list handed to the engine, the concatenation the library must see)"""
    rng = np.random.default_rng(3)
    arrs = [rng.standard_normal(n if pcm else (t, FEAT)).astype(F32) for n, t in zip(batch["ns"], batch["T"])]
    as_torch = {"numpy": lambda i: False, "torch": lambda i: True, "mixed": lambda i: i % 2 == 0}[kind]
    return [torch.from_numpy(a.copy()) if as_torch(i) else a for i, a in enumerate(arrs)], np.concatenate([a.reshape(-1) for a in arrs])


def tokens(batch):
    return [list(range(10 * i + 1, 10 * i + 1 + u)) for i, u in enumerate(batch["U"])]


def check(arr, name, start, shape, dtype):
    """arr is an owned array of that dtype and shape holding BASE[name] + start, + start + 1, ..."""
    assert isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.shape == tuple(shape), (name, arr.dtype, arr.shape)
    assert arr.base is None and arr.flags.owndata, name
    want = (BASE[name] + start + np.arange(int(np.prod(shape)))).reshape(shape).astype(dtype)
    assert np.array_equal(arr, want), (name, arr, want)


def check_inputs(rec, slots, cat, lens, lens_dtype, toks=None):
    assert np.array_equal(rec["in"]["slots"], np.asarray(slots, I32))
    assert rec["in"]["cat"].dtype == F32 and np.array_equal(rec["in"]["cat"], cat)
    assert rec["in"]["lens"].dtype == lens_dtype and rec["in"]["lens"].tolist() == list(lens)
    if toks is not None:
        assert rec["in"]["tok"].tolist() == [t for y in toks for t in y]
        assert rec["in"]["U"].tolist() == [len(y) for y in toks]


def check_post(r, t, u, w, oc, o):
    check(r["occ_blank"], "occ_blank", oc, (t, w), F32)
    check(r["occ_emit"], "occ_emit", oc, (t, w), F32)
    check(r["tok_mean"], "tok_mean", o, (u,), F64)
    check(r["tok_var"], "tok_var", o, (u,), F64)
    check(r["tok_peak_frame"], "tok_peak_frame", o, (u,), I32)
    check(r["tok_peak"], "tok_peak", o, (u,), F64)


def check_align(out, batch, W, viterbi, lattice, posteriors, band):
    """the dicts of an align call: every field from its offset; W = the row width per utterance"""
    assert len(out) == len(batch["U"])
    o = oc = ot = 0
    for i, (r, u, t, w) in enumerate(zip(out, batch["U"], batch["T"], W)):
        keys = {"loglik"} | ({"viterbi", "frames", "logps"} if viterbi else set()) | ({"blank_lp", "emit_lp"} if lattice else set())
        keys |= (set(POST) if posteriors else set()) | ({"lo", "width", "passes", "touch"} if band else set())
        assert set(r) == keys
        assert type(r["loglik"]) is float and r["loglik"] == BASE["loglik"] + i
        if viterbi:
            assert type(r["viterbi"]) is float and r["viterbi"] == BASE["vit"] + i
            check(r["frames"], "fr", o, (u,), I32)
            check(r["logps"], "lp", o, (u,), F32)
        if lattice:
            check(r["blank_lp"], "b", oc, (t, w), F32)
            check(r["emit_lp"], "e", oc, (t, w), F32)
        if band:
            check(r["lo"], "lo", ot, (t,), I32)
            assert (r["width"], r["passes"], r["touch"]) == (w, BASE["passes"] + i, BASE["touch"] + i)
            assert all(type(r[k]) is int for k in ("width", "passes", "touch"))
        if posteriors:
            check_post(r, t, u, w, oc, o)
        o, oc, ot = o + u, oc + t * w, ot + t


ALIGN_IN = {"slots", "cat", "lens", "tok", "U"}


def align_nonnull(viterbi, lattice, posteriors, band=False, windows=False):
    return (ALIGN_IN | {"loglik"} | ({"vit", "fr", "lp"} if viterbi else set()) | ({"b", "e"} if lattice else set())
            | (set(POST) if posteriors else set()) | ({"lo", "passes", "touch"} if band else set()) | ({"lo_in"} if windows else set()))


# ----------------------------------------------------------------------------------------------------------------- transcribe
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pcm", [True, False])
def test_transcribe(pcm, kind):
    eng, batch = make_engine(), BATCHES["three"]
    xs, cat = audio(batch, pcm, kind)
    assert (eng.transcribe_pcm if pcm else eng.transcribe_feats)([4, 2, 7], xs) is None
    (rec,) = eng.lib.calls
    assert rec["fn"] == "transcribe_" + ("pcm" if pcm else "feats") and rec["scalars"] == {"n": 3}
    assert rec["nonnull"] == {"slots", "cat", "lens"}
    check_inputs(rec, [4, 2, 7], cat, batch["ns"] if pcm else batch["T"], I64 if pcm else I32)


def test_pcm_is_flattened_and_converted():
    """pcm of any shape and float type: flattened, float32, the sample count its number of elements"""
    eng = make_engine()
    x = [np.arange(12, dtype=np.float64).reshape(3, 4), torch.arange(5, dtype=torch.float64).requires_grad_(True)]
    eng.transcribe_pcm([0, 1], x)
    rec = eng.lib.calls[0]
    check_inputs(rec, [0, 1], np.concatenate([np.arange(12), np.arange(5)]).astype(F32), [12, 5], I64)


def test_feats_requires_grad_is_accepted():
    """A host feature tensor that requires grad is accepted, as a pcm one is.  (The one test of this file that fails before the
    packers were folded: the feats copies called x.cpu() without detach(), and np.asarray of such a tensor raises.)"""
    eng, batch = make_engine(), BATCHES["three"]
    xs, cat = audio(batch, False, "torch")
    xs = [x.requires_grad_(True) for x in xs]
    eng.transcribe_feats([0, 1, 2], xs)
    eng.align_feats([0, 1, 2], xs, tokens(batch))
    eng.score_feats([[0], [1], [2]], xs, [[y] for y in tokens(batch)])
    assert all(np.array_equal(rec["in"]["cat"], cat) for rec in eng.lib.calls)


# ----------------------------------------------------------------------------------------------------------------- full lattice
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("viterbi,lattice,posteriors", list(itertools.product([True, False], repeat=3)))
@pytest.mark.parametrize("pcm", [True, False])
def test_align_full(pcm, viterbi, lattice, posteriors, kind):
    eng, batch = make_engine(), BATCHES["three"]
    xs, cat = audio(batch, pcm, kind)
    ys = tokens(batch)
    out = (eng.align_pcm if pcm else eng.align_feats)([5, 0, 3], xs, ys, lattice=lattice, viterbi=viterbi, posteriors=posteriors)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "align_" + ("post_" if posteriors else "") + ("pcm" if pcm else "feats") and rec["scalars"] == {"n": 3}
    assert rec["nonnull"] == align_nonnull(viterbi, lattice, posteriors)
    check_inputs(rec, [5, 0, 3], cat, batch["ns"] if pcm else batch["T"], I64 if pcm else I32, ys)
    check_align(out, batch, [u + 1 for u in batch["U"]], viterbi, lattice, posteriors, False)


# ----------------------------------------------------------------------------------------------------------------- band
def windows_of(batch):
    return [list(range(7 * i, 7 * i + t)) for i, t in enumerate(batch["T"])]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("windows", [False, True])
@pytest.mark.parametrize("viterbi,lattice,posteriors", list(itertools.product([True, False], repeat=3)))
@pytest.mark.parametrize("pcm", [True, False])
@pytest.mark.parametrize("which", ["three", "single"])
def test_align_band(which, pcm, viterbi, lattice, posteriors, windows, kind):
    eng, batch = make_engine(), BATCHES[which]
    xs, cat = audio(batch, pcm, kind)
    ys, slots = tokens(batch), list(range(len(batch["U"])))[::-1]
    win = windows_of(batch) if windows else None
    if posteriors:      # banded calls with posteriors go through align_band_post_*
        out = (eng.align_band_post_pcm if pcm else eng.align_band_post_feats)(slots, xs, ys, batch["band"], max_passes=3, windows=win,
                                                                                lattice=lattice, viterbi=viterbi)
    else:
        out = (eng.align_pcm if pcm else eng.align_feats)(slots, xs, ys, lattice=lattice, viterbi=viterbi, band=batch["band"], max_passes=3,
                                                          windows=win)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "align_band_" + ("post_" if posteriors else "") + ("pcm" if pcm else "feats")
    assert rec["scalars"] == {"n": len(slots), "band": batch["band"], "max_passes": 3}
    assert all(type(v) is int for v in rec["scalars"].values())
    assert rec["nonnull"] == align_nonnull(viterbi, lattice, posteriors, True, windows)
    check_inputs(rec, slots, cat, batch["ns"] if pcm else batch["T"], I64 if pcm else I32, ys)
    if windows:
        assert rec["in"]["lo_in"].tolist() == [v for w in win for v in w]
    check_align(out, batch, batch["W"], viterbi, lattice, posteriors, True)


def test_band_defaults():
    """max_passes defaults to 1 on both routes into the band, and align_band_post_* default to viterbi without the lattice"""
    eng, batch = make_engine(), BATCHES["three"]
    xs, _ = audio(batch, True, "numpy")
    eng.align_pcm([0, 1, 2], xs, tokens(batch), band=2)
    out = eng.align_band_post_pcm([0, 1, 2], xs, tokens(batch), 2)
    assert [rec["scalars"]["max_passes"] for rec in eng.lib.calls] == [1, 1]
    assert eng.lib.calls[1]["nonnull"] == align_nonnull(True, False, True, True)
    check_align(out, batch, batch["W"], True, False, True, True)


@pytest.mark.parametrize("pcm", [True, False])
@pytest.mark.parametrize("post", [False, True])
def test_windows_of_the_wrong_length(pcm, post):
    eng, batch = make_engine(), BATCHES["three"]
    xs, _ = audio(batch, pcm, "numpy")
    win = windows_of(batch)
    win[2] = win[2] + [0]
    with pytest.raises(N.LasrError) as ei:
        if post:
            (eng.align_band_post_pcm if pcm else eng.align_band_post_feats)([0, 1, 2], xs, tokens(batch), 2, windows=win)
        else:
            (eng.align_pcm if pcm else eng.align_feats)([0, 1, 2], xs, tokens(batch), band=2, windows=win)
    assert ei.value.code == N.LASR_EINVAL and "windows: one start per encoder frame of every utterance" in str(ei.value)
    assert eng.lib.calls == []


@pytest.mark.parametrize("pcm", [True, False])
def test_band_with_posteriors_is_refused(pcm):
    eng, batch = make_engine(), BATCHES["three"]
    xs, _ = audio(batch, pcm, "numpy")
    with pytest.raises(ValueError, match="posteriors with a band: use align_band_post_pcm / align_band_post_feats"):
        (eng.align_pcm if pcm else eng.align_feats)([0, 1, 2], xs, tokens(batch), posteriors=True, band=2)
    assert eng.lib.calls == []


def test_mismatched_lengths_assert():
    eng, batch = make_engine(), BATCHES["three"]
    xs, _ = audio(batch, True, "numpy")
    with pytest.raises(AssertionError):
        eng.align_pcm([0, 1], xs, tokens(batch))
    with pytest.raises(AssertionError):
        eng.align_pcm([0, 1, 2], xs, tokens(batch)[:2])
    with pytest.raises(AssertionError):
        eng.align_pcm([0, 1, 2], xs, tokens(batch), band=2, windows=windows_of(batch)[:2])
    with pytest.raises(AssertionError):
        eng.transcribe_pcm([0, 1], xs)
    with pytest.raises(AssertionError):
        eng.score_pcm([[0], [1]], xs, [[[1]], [[2]]])


# ----------------------------------------------------------------------------------------------------------------- caller-supplied lattices
def lattices(T, W):
    rng = np.random.default_rng(11)
    bs = [rng.standard_normal((t, w)).astype(F32) for t, w in zip(T, W)]
    es = [rng.standard_normal((t, w)) for t, w in zip(T, W)]           # float64 on purpose: converted on the way in
    return bs, es, np.concatenate([x.reshape(-1) for x in bs]), np.concatenate([x.reshape(-1) for x in es]).astype(F32)


@pytest.mark.parametrize("viterbi", [True, False])
def test_lattice_dp(viterbi):
    eng, batch = make_engine(), BATCHES["three"]
    bs, es, b, e = lattices(batch["T"], [u + 1 for u in batch["U"]])
    out = eng.lattice_dp(bs, es, viterbi=viterbi)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "lattice_dp" and rec["scalars"] == {"n": 3}
    assert rec["nonnull"] == {"b", "e", "T", "U", "loglik"} | ({"vit", "fr"} if viterbi else set())
    assert np.array_equal(rec["in"]["b"], b) and np.array_equal(rec["in"]["e"], e)
    assert rec["in"]["T"].tolist() == batch["T"] and rec["in"]["U"].tolist() == batch["U"]
    o = 0
    for i, (r, u) in enumerate(zip(out, batch["U"])):
        assert set(r) == ({"loglik", "viterbi", "frames"} if viterbi else {"loglik"}) and r["loglik"] == BASE["loglik"] + i
        if viterbi:
            assert r["viterbi"] == BASE["vit"] + i
            check(r["frames"], "fr", o, (u,), I32)
        o += u


def test_lattice_post():
    eng, batch = make_engine(), BATCHES["three"]
    bs, es, b, e = lattices(batch["T"], [u + 1 for u in batch["U"]])
    out = eng.lattice_post(bs, es)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "lattice_post" and rec["scalars"] == {"n": 3}
    assert rec["nonnull"] == {"b", "e", "T", "U", "loglik", "bwd"} | set(POST)
    assert np.array_equal(rec["in"]["b"], b) and np.array_equal(rec["in"]["e"], e)
    assert rec["in"]["T"].tolist() == batch["T"] and rec["in"]["U"].tolist() == batch["U"]
    o = oc = 0
    for i, (r, u, t) in enumerate(zip(out, batch["U"], batch["T"])):
        assert set(r) == {"loglik", "loglik_bwd"} | set(POST)
        assert (r["loglik"], r["loglik_bwd"]) == (BASE["loglik"] + i, BASE["bwd"] + i)
        check_post(r, t, u, u + 1, oc, o)
        o, oc = o + u, oc + t * (u + 1)


@pytest.mark.parametrize("which", ["three", "single"])
@pytest.mark.parametrize("viterbi", [True, False])
def test_lattice_band_dp(which, viterbi):
    eng, batch = make_engine(), BATCHES[which]
    bs, es, b, e = lattices(batch["T"], batch["W"])
    lo = windows_of(batch)
    out = eng.lattice_band_dp(bs, es, lo, batch["U"], viterbi=viterbi)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "lattice_band_dp" and rec["scalars"] == {"n": len(bs)}
    assert rec["nonnull"] == {"b", "e", "T", "U", "W", "lo_in", "loglik"} | ({"vit", "fr"} if viterbi else set())
    assert np.array_equal(rec["in"]["b"], b) and np.array_equal(rec["in"]["e"], e)
    assert [rec["in"][k].tolist() for k in ("T", "U", "W")] == [batch["T"], batch["U"], batch["W"]]
    assert rec["in"]["lo_in"].tolist() == [v for w in lo for v in w]
    o = 0
    for i, (r, u) in enumerate(zip(out, batch["U"])):
        assert set(r) == ({"loglik", "viterbi", "frames"} if viterbi else {"loglik"}) and r["loglik"] == BASE["loglik"] + i
        if viterbi:
            assert r["viterbi"] == BASE["vit"] + i
            check(r["frames"], "fr", o, (u,), I32)
        o += u


@pytest.mark.parametrize("which", ["three", "single"])
def test_lattice_band_post(which):
    eng, batch = make_engine(), BATCHES[which]
    bs, es, b, e = lattices(batch["T"], batch["W"])
    lo = windows_of(batch)
    out = eng.lattice_band_post(bs, es, lo, batch["U"])
    (rec,) = eng.lib.calls
    assert rec["fn"] == "lattice_band_post" and rec["scalars"] == {"n": len(bs)}
    assert rec["nonnull"] == {"b", "e", "T", "U", "W", "lo_in", "loglik", "bwd"} | set(POST)
    assert np.array_equal(rec["in"]["b"], b) and np.array_equal(rec["in"]["e"], e)
    assert [rec["in"][k].tolist() for k in ("T", "U", "W")] == [batch["T"], batch["U"], batch["W"]]
    assert rec["in"]["lo_in"].tolist() == [v for w in lo for v in w]
    o = oc = 0
    for i, (r, u, t, w) in enumerate(zip(out, batch["U"], batch["T"], batch["W"])):
        assert set(r) == {"loglik", "loglik_bwd"} | set(POST)
        assert (r["loglik"], r["loglik_bwd"]) == (BASE["loglik"] + i, BASE["bwd"] + i)
        check_post(r, t, u, w, oc, o)
        o, oc = o + u, oc + t * w


@pytest.mark.parametrize("viterbi", [True, False])
def test_lattice_tree_dp(viterbi):
    eng, T, Nn = make_engine(), [4, 1, 2], [4, 1, 2]
    bs, es, b, e = lattices(T, Nn)
    parent = [[-1, 0, 1, 1], [-1], [-1, 0]]
    out = eng.lattice_tree_dp(bs, es, parent, viterbi=viterbi)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "lattice_tree_dp" and rec["scalars"] == {"n": 3}
    assert rec["nonnull"] == {"b", "e", "T", "N", "parent", "loglik"} | ({"vit"} if viterbi else set())
    assert np.array_equal(rec["in"]["b"], b) and np.array_equal(rec["in"]["e"], e)
    assert rec["in"]["T"].tolist() == T and rec["in"]["N"].tolist() == Nn
    assert rec["in"]["parent"].tolist() == [v for q in parent for v in q]
    o = 0
    for r, nn in zip(out, Nn):
        assert set(r) == ({"loglik", "viterbi"} if viterbi else {"loglik"})
        check(r["loglik"], "loglik", o, (nn,), F64)
        if viterbi:
            check(r["viterbi"], "vit", o, (nn,), F64)
        o += nn


def test_lattice_shape_asserts():
    eng = make_engine()
    z = np.zeros((2, 3), F32)
    for call in (lambda: eng.lattice_dp([z], [z, z]), lambda: eng.lattice_dp([], []), lambda: eng.lattice_dp([z], [z[:, :2]]),
                 lambda: eng.lattice_post([z.reshape(-1)], [z.reshape(-1)]), lambda: eng.lattice_band_dp([z], [z], [[0]], [2]),
                 lambda: eng.lattice_band_post([z], [z], [[0, 0]], [2, 2]), lambda: eng.lattice_tree_dp([z], [z], [[-1, 0]])):
        with pytest.raises(AssertionError):
            call()
    assert eng.lib.calls == []


# ----------------------------------------------------------------------------------------------------------------- prefix tree, scoring
def test_prefix_tree():
    eng = make_engine()
    cands = [[5, 6, 7], [], np.array([5], np.int64)]
    tr = eng.prefix_tree(cands)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "prefix_tree" and rec["scalars"] == {"k": 3, "cap": 5}
    assert rec["nonnull"] == {"tok", "nt", "par", "lab", "dep", "term"}
    assert rec["in"]["tok"].tolist() == [5, 6, 7, 5] and rec["in"]["nt"].tolist() == [3, 0, 1]
    assert set(tr) == {"parent", "label", "depth", "term"}
    check(tr["parent"], "par", 0, (5,), I32)
    check(tr["label"], "lab", 0, (5,), I32)
    check(tr["depth"], "dep", 0, (5,), I32)
    check(tr["term"], "term", 0, (3,), I32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("viterbi,lattice", list(itertools.product([True, False], repeat=2)))
@pytest.mark.parametrize("pcm", [True, False])
def test_score(pcm, viterbi, lattice, kind):
    """two utterances with 2 and 1 candidates, one of them empty"""
    eng, batch = make_engine(), dict(T=[4, 2], ns=[5280, 2720])
    xs, cat = audio(batch, pcm, kind)
    cands, slots = [[[5, 6, 7], []], [[9]]], [[6, 1], [3]]
    out = (eng.score_pcm if pcm else eng.score_feats)(slots, xs, cands, viterbi=viterbi, lattice=lattice)
    rec = eng.lib.calls[-1]
    assert [c["fn"] for c in eng.lib.calls[:-1]] == (["prefix_tree"] * 2 if lattice else [])
    assert rec["fn"] == "score_" + ("pcm" if pcm else "feats") and rec["scalars"] == {"n": 2}
    assert rec["nonnull"] == ({"slots", "cat", "lens", "nc", "tok", "nt", "loglik"} | ({"vit"} if viterbi else set())
                              | ({"b", "e"} if lattice else set()))
    check_inputs(rec, [6, 1, 3], cat, batch["ns"] if pcm else batch["T"], I64 if pcm else I32)
    assert [rec["in"][k].tolist() for k in ("nc", "tok", "nt")] == [[2, 1], [5, 6, 7, 9], [3, 0, 1]]
    o = oc = 0
    for r, k, t, nodes in zip(out, [2, 1], batch["T"], [4, 2]):
        assert set(r) == {"loglik"} | ({"viterbi"} if viterbi else set()) | ({"tree", "blank_lp", "emit_lp"} if lattice else set())
        check(r["loglik"], "loglik", o, (k,), F64)
        if viterbi:
            check(r["viterbi"], "vit", o, (k,), F64)
        if lattice:
            check(r["blank_lp"], "b", oc, (t, nodes), F32)
            check(r["emit_lp"], "e", oc, (t, nodes), F32)
            check(r["tree"]["parent"], "par", 0, (nodes,), I32)
            check(r["tree"]["term"], "term", 0, (k,), I32)
        o, oc = o + k, oc + t * nodes


@pytest.mark.parametrize("start,want", [(None, -1), (2, 2)])
def test_lm_score(start, want):
    eng = make_engine()
    ys = [[5, 6, 7], [], (9,)]
    out = eng.lm_score([2, 0, 1], ys, start=start)
    (rec,) = eng.lib.calls
    assert rec["fn"] == "lm_score" and rec["scalars"] == {"n": 3, "start": want} and type(rec["scalars"]["start"]) is int
    assert rec["nonnull"] == {"slots", "tok", "nt", "total", "lp"}
    assert [rec["in"][k].tolist() for k in ("slots", "tok", "nt")] == [[2, 0, 1], [5, 6, 7, 9], [3, 0, 1]]
    o = 0
    for i, (r, y) in enumerate(zip(out, ys)):
        assert set(r) == {"total", "logps"} and type(r["total"]) is float and r["total"] == BASE["total"] + i
        check(r["logps"], "lp", o, (len(y),), F32)
        o += len(y)
