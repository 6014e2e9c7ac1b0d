"""tests/frontend_ref.py is right, and it bites (no GPU).

* The float64 reference agrees, within its own bound, with the numpy oracle (O.logmel, O.stack_downsample, O.StreamFrontend) and
  with what the reference project itself produced (tests/golden/frontend.npz), in every geometry the GPU file uses.
* The bound is not too tight: an independent float32 pipeline (torch.stft, a float32 filterbank product, torch's float32
  LayerNorm) stays at or below HALF the bound on every element, for every signal and geometry of tests/test_gpu_frontend.py.
* The bound is not too loose: every planted defect (frontend_ref.DEFECTS) moves the float64 result past the bound."""
import os

import numpy as np
import pytest
import torch

import frontend_ref as R
from libreasr_amd import synth
from oracle import rnnt_oracle as O

F32 = np.float32


def mel_kw(g):
    return dict(win=g["win"], hop=g["hop"], n_mels=g["n_mels"])


# ------------------------------------------------------------------------------------------------ the float32 pipeline
def logmel_f32(pcm, g, first=0, count=None):
    """torch.stft in float32 (window: the periodic Hann evaluated in double and rounded, as the engine's table is -- torch.hann_window
    evaluates 0.5 - 0.5 cos in float32, which loses the window's first and last samples to cancellation: 1e-3 relative at n = 1,
    visible on the "edges" signal and on nothing else), float32 power, float32 filterbank product, float32 log"""
    w = torch.from_numpy(R.hann(g["win"]).astype(F32))
    S = torch.stft(torch.from_numpy(np.ascontiguousarray(pcm, dtype=F32)), R.N_FFT, hop_length=g["hop"], win_length=g["win"], window=w,
                   center=True, pad_mode="reflect", return_complex=True)
    P = S.real ** 2 + S.imag ** 2
    fb = torch.from_numpy(R.htk_filterbank(g["n_mels"]).astype(F32))
    out = torch.log(P.T @ fb + 1e-6).numpy()
    return out[first:] if count is None else out[first:first + count]


def window_f32(win_pcm, g):
    T = 1 + len(win_pcm) // g["hop"]
    return logmel_f32(win_pcm, g, T // 3 + 1, g["n_stack"])


def ln_f32(x, w, b):
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
    return torch.nn.functional.layer_norm(x, x.shape[-1:], torch.from_numpy(w), torch.from_numpy(b), 1e-5).numpy()


def ln_params(g):
    _, sd = R.tiny_model(g)
    return np.asarray(sd["encoder.input_norm.weight"], F32), np.asarray(sd["encoder.input_norm.bias"], F32)


# ------------------------------------------------------------------------------------------------ agreement
def fb_built_in_float32(n_mels=128, sr=16000):
    """The filterbank TABLE of the reference project: torchaudio 0.6.0's create_fb_matrix evaluates the mel points, the band edges
    and the slopes in float32 tensors (the engine and the oracle evaluate them in double and round once).  Its weights differ from
    the exact ones by up to 1.3e-5 absolute, which moves a log-mel value by up to 9e-5 -- 18 times the rounding bound of the
    pipeline's arithmetic.  That is a difference between two tables, not rounding of the pipeline: the golden vectors are compared
    with the float64 pipeline run on THEIR table, within the unchanged bound."""
    import math
    top = 2595.0 * math.log10(1.0 + (sr / 2.0) / 700.0)
    freqs = torch.linspace(0, sr // 2, R.N_FFT // 2 + 1)
    f_pts = 700.0 * (10 ** (torch.linspace(0.0, top, n_mels + 2) / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - freqs.unsqueeze(1)
    fb = torch.max(torch.zeros(1), torch.min(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))
    return fb.numpy().astype(np.float64)


def test_reference_agrees_with_the_oracle_and_the_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "frontend.npz"))
    pcm = synth.synth_pcm(2, 16000 + 937, seed=7)
    fb32 = fb_built_in_float32()
    assert 1e-6 < np.abs(fb32 - R.htk_filterbank(128)).max() < 1e-4
    for s in range(2):
        v, b = R.logmel64(pcm[s])
        gv, gb = R.logmel64(pcm[s], fb=fb32)
        assert v.shape == g[f"logmel_{s}"].shape
        r_exact, r_own = R.ratio(g[f"logmel_{s}"], v, b), R.ratio(g[f"logmel_{s}"], gv, gb)
        print(f"\nreference golden logmel_{s}: error / bound {r_own:.3f} on its own float32-built table, {r_exact:.1f} on the exact table")
        assert r_own <= 1.0
        assert R.ratio(O.logmel(pcm[s]), v, b) <= 1.0
        assert R.ratio(g[f"feats_{s}"], R.stack(gv, 10, 8), R.stack(gb, 10, 8)) <= 1.0
        assert R.ratio(O.features_offline(pcm[s]), R.stack(v, 10, 8), R.stack(b, 10, 8)) <= 1.0
        m32 = O.logmel(pcm[s])
        assert np.array_equal(R.stack(m32, 10, 8), O.stack_downsample(m32))            # the stacking itself: exact
    v, b = R.logmel64(np.zeros(3840, F32), fb=fb32)
    assert R.ratio(g["logmel_zero"], v, b) <= 1.0
    # the servicer's stream: which calls hand out features, and the features
    chunks = synth.stream_chunks(pcm[0], 1280, lead=1, tail=2)
    ref, gref, fe = R.StreamRef(R.DEFAULT), R.StreamRef(R.DEFAULT, fb=fb32), O.StreamFrontend()
    pattern, k = [], 0
    for ch in chunks:
        ref.push(ch)
        gref.push(ch)
        out, gout, o = ref.collect(), gref.collect(), fe.push(ch)
        pattern.append(int(out is not None))
        assert (out is None) == (o is None) == (gout is None)
        if out is not None:
            assert R.stack(out[0], 10, 10).shape == (2, 1280)
            assert R.ratio(g["stream_feats"][k], R.stack(gout[0], 10, 10), R.stack(gout[1], 10, 10)) <= 1.0
            assert R.ratio(o, R.stack(out[0], 10, 10), R.stack(out[1], 10, 10)) <= 1.0
            k += 1
    # (the golden's pattern has one entry per call of the transform pipeline: the calls before the window is full are not in it)
    assert pattern[:2] == [0, 0] and pattern[2:] == list(g["stream_pattern"]) and k == len(g["stream_feats"])


@pytest.mark.parametrize("name", sorted(R.OFFLINE_GEOMETRIES))
def test_reference_agrees_with_the_oracle_offline(name):
    g = R.OFFLINE_GEOMETRIES[name]
    for sig in R.SIGNALS:
        for n in (513, 801, 2077):
            x = R.signal(sig, 1, n)[0]
            v, b = R.logmel64(x, **g)
            got = O.logmel(x, **mel_kw(g))
            assert got.shape == v.shape == (1 + n // g["hop"], g["n_mels"])
            assert R.ratio(got, v, b) <= 1.0, (name, sig, n)
            assert np.array_equal(R.stack(got, g["n_stack"], g["stride"]), O.stack_downsample(got, g["n_stack"], g["stride"]))


@pytest.mark.parametrize("name", sorted(R.STREAM_GEOMETRIES))
def test_reference_agrees_with_the_oracle_streaming(name):
    g = R.STREAM_GEOMETRIES[name]
    n = R.stream_len(g)
    pcm = R.stream_pcm(g, 2, n)
    for r in range(2):
        ref = R.StreamRef(g)
        fe = O.StreamFrontend(n_stack=g["n_stack"], downsample=g["stride"], n_buffer=g["n_buffer"], n_window=g["n_window"], **mel_kw(g))
        steps = 0
        for k in range(n):
            ref.push(pcm[r, k])
            out, o = ref.collect(), fe.push(pcm[r, k])
            assert (out is None) == (o is None)
            if out is not None:
                ns = g["n_stack"]
                assert R.ratio(o, R.stack(out[0], ns, ns), R.stack(out[1], ns, ns)) <= 1.0, (name, r, k)
                steps += 1
        assert steps >= 2


# ------------------------------------------------------------------------------------------------ not too tight
def _half(got, v, b, what):
    r = R.ratio(got, v, b)
    assert r <= 0.5, (what, r)
    return r


@pytest.mark.parametrize("name", sorted(R.OFFLINE_GEOMETRIES))
def test_float32_pipeline_stays_under_half_the_bound_offline(name):
    g = R.OFFLINE_GEOMETRIES[name]
    w, b = ln_params(g)
    worst = {}
    for sig in R.SIGNALS:
        rl = rn = 0.0
        for n in R.OFFLINE_LENGTHS:
            x = R.signal(sig, 3, n)
            for r in range(3):
                v, bd = R.logmel64(x[r], **g)
                got = logmel_f32(x[r], g)
                rl = max(rl, _half(got, v, bd, (name, sig, n, r)))
                st = R.stack(got, g["n_stack"], g["stride"])
                if len(st):
                    y, yb = R.layer_norm64(st, w, b)
                    rn = max(rn, _half(ln_f32(st, w, b), y, yb, (name, sig, n, r, "LayerNorm")))
        worst[sig] = (round(rl, 3), round(rn, 3))
    print(f"\noffline {name}: worst error / bound of the float32 pipeline (log-mel, LayerNorm) {worst}")


@pytest.mark.parametrize("name", sorted(R.STREAM_GEOMETRIES))
def test_float32_pipeline_stays_under_half_the_bound_streaming(name):
    g = R.STREAM_GEOMETRIES[name]
    w, b = ln_params(g)
    n, ns = R.stream_len(g), g["n_stack"]
    pcm = R.stream_pcm(g, 4, n)
    worst = {}
    for r in range(4):
        rl = rn = 0.0
        for k in range(g["n_window"], n + 1):
            win = pcm[r, k - g["n_window"]:k].reshape(-1)
            v, bd = R.window_logmel64(win, g)
            got = window_f32(win, g)
            rl = max(rl, _half(got, v, bd, (name, r, k)))
            y, yb = R.stream_x0_64(got, g, w, b)
            rn = max(rn, _half(ln_f32(R.stack(got, ns, ns), w, b), y, yb, (name, r, k, "LayerNorm")))
        worst[R.STREAM_SIGNALS[r]] = (round(rl, 3), round(rn, 3))
    print(f"\nstreaming {name}: worst error / bound of the float32 pipeline (log-mel, LayerNorm) {worst}")


def test_float32_pipeline_stays_under_half_the_bound_on_whole_windows():
    g = R.DEFAULT
    for N in R.WINDOW_LENGTHS:
        wins = R.step_windows(N, 2, 6)
        for r in range(2):
            for i in range(6):
                v, bd = R.window_logmel64(wins[r, i], g)
                _half(window_f32(wins[r, i], g), v, bd, (N, r, i))


# ------------------------------------------------------------------------------------------------ not too loose
# defect -> the signal that is asserted to show it (every log-mel defect shows on all five; the test prints the full table)
CAUGHT_ON = dict(tap_low="noise", tap_mid="synth", tap_high="synth", shift="edges", hann_symmetric="edges", pad_zero="edges",
                 pad_edge="tone", pad_symmetric="edges", win_off="chirp", stack_transposed="chirp", var_unbiased="synth")


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_exceeds_the_bound(defect):
    g = R.DEFAULT
    w, b = ln_params(g)
    seen = {}
    for sig in R.SIGNALS:
        x = R.signal(sig, 1, 2077)[0]
        v, bd = R.logmel64(x, **g)
        if defect in ("stack_transposed", "var_unbiased"):
            mel = v[:10].astype(F32)                                   # a given log-mel array; the defect sits behind it
            y, yb = R.stream_x0_64(mel, g, w, b)
            seen[sig] = R.ratio(R.stream_x0_64(mel, g, w, b, defect=defect)[0], y, yb)
        else:
            seen[sig] = R.ratio(R.logmel64(x, defect=defect, **g)[0], v, bd)
    print(f"\n{defect}: largest change / bound per signal {({k: round(r, 1) for k, r in seen.items()})}")
    assert seen[CAUGHT_ON[defect]] > 1.0, (defect, seen)


def test_the_top_filters_last_tap_carries_weight():
    """bin 512 closes the top filter with weight 0: the tap dropped by `tap_high` is the one before it"""
    for n_mels in (40, 64, 128):
        fb = R.htk_filterbank(n_mels)
        k = R.last_tap(fb, n_mels - 1)
        assert k == 511 and fb[k, n_mels - 1] > 1e-3 and fb[512, n_mels - 1] < 1e-9


def test_geometries_of_the_gpu_file():
    """what tests/test_gpu_frontend.py relies on: which geometries take the fused kernels, and how many ring slots they have"""
    G = R.STREAM_GEOMETRIES
    assert [n for n in sorted(G) if R.fused(G[n])] == ["chunk1282", "default", "nbuf1", "nbuf4"]
    assert R.ring_chunks(G["default"]) == 4 and R.ring_chunks(G["default"], legacy=True) == 3
    assert R.ring_chunks(G["nbuf4"]) == 6 and R.ring_chunks(G["ring17"]) == 16       # 17 slots would not fit the packed ring position
    assert {n: R.stream_len(G[n]) for n in ("default", "ring17")} == {"default": 11, "ring17": 50}
    assert all(1 + n // 160 - (1 + n // 160) // 3 - 1 >= 10 for n in R.WINDOW_LENGTHS) and 1 + 2399 // 160 == 15
