"""Non-finite numbers at the op-level entry points (needs an MI355X): log-mel, the joint with its argmax, and the four lattice
dynamic programmes.  These entry points hand the argmax out and never index with it, so every test here is safe on any build.

Expected values: numpy's argmax (NaN is the maximum, the first one wins, a row of -inf gives 0), the oracle's log-mel, and the
float64 references tests/lattice_ref.py, lattice_post_ref.py, lattice_tree_ref.py, lattice_band_ref.py.  Every comparison is exact:
NaN masks first, then bit patterns of the rest.  Cases: tests/nonfinite_cases.py (pinned on the CPU by test_nonfinite_cpu.py)."""
import numpy as np
import pytest
import torch

import lattice_band_ref as B
import lattice_post_ref as P
import lattice_ref as R
import lattice_tree_ref as TR
import nonfinite_cases as NC
from libreasr_amd import synth
from oracle import rnnt_oracle as O

pytestmark = pytest.mark.gpu

_ENGINES = {}


def make(sd, cfg, **kw):
    import __graft_entry__ as graft
    from libreasr_amd.engine import Engine
    graft.build()
    return Engine(sd, cfg, max_streams=16, **kw)


def tiny_engine(dtype="f32"):
    if dtype not in _ENGINES:
        sd, cfg, _ = NC.tiny()
        _ENGINES[dtype] = make(sd, cfg, dtype=dtype)
    return _ENGINES[dtype]


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------- log-mel
LM_N, LM_POS = 3840, 1900


@pytest.mark.parametrize("kind", list(NC.BAD))
def test_logmel(kind):
    """one bad sample at a known index of a 3840-sample row: the frames it reaches are non-finite in every bin, every other frame
    and the second row of the call are bit-identical to the clean call.  "Reaches" is the oracle's: NaN and Inf through any of
    the 1024 positions of the frame (the zero padding of the window included), the huge value through a non-zero weight"""
    eng = tiny_engine()
    pcm = NC.clean_pcm()[:2, :LM_N].copy()
    want = eng.logmel(dev(pcm)).cpu().numpy()
    assert np.isfinite(want).all()
    bad = pcm.copy()
    bad[0, LM_POS] = np.float32(NC.BAD[kind])
    got = eng.logmel(dev(bad)).cpu().numpy()
    touched = NC.touched_frames(kind, LM_POS, LM_N)
    assert len(touched) == (3 if kind == "huge" else 7)
    with np.errstate(all="ignore"):
        ref_mask = ~np.isfinite(O.logmel(bad[0]))
    mask = np.zeros(got.shape[1:], bool)
    mask[touched] = True
    assert np.array_equal(ref_mask, mask)                            # (the oracle agrees on which frames those are)
    assert np.array_equal(~np.isfinite(got[0]), mask), np.flatnonzero((~np.isfinite(got[0])).any(1))
    assert np.array_equal(NC.bits(got[0][~mask]), NC.bits(want[0][~mask]))
    assert np.array_equal(NC.bits(got[1]), NC.bits(want[1]))


# ------------------------------------------------------------------------------- the joint and its argmax
def joint_rows(eng, H, seed=5):
    rng = np.random.default_rng(seed)
    hp = rng.standard_normal((5, H)).astype(np.float32) * 0.5
    he = rng.standard_normal((5, H)).astype(np.float32) * 0.5
    return hp, he


def check_joint_nan_row(eng, V, H):
    hp, he = joint_rows(eng, H)
    z0, lp0, am0 = (x.cpu().numpy() for x in eng.joint(dev(hp), dev(he)))
    assert np.isfinite(z0).all() and np.isfinite(lp0).all()
    assert [int(a) for a in am0] == [int(a) for a in z0.argmax(-1)]
    he_bad = he.copy()
    he_bad[2] = np.nan
    z, lp, am = (x.cpu().numpy() for x in eng.joint(dev(hp), dev(he_bad)))
    assert z.shape == (5, V)
    assert np.isnan(z[2]).all()
    assert np.isnan(lp[2])
    assert 0 <= int(am[2]) < V, int(am[2])
    assert int(am[2]) == 0 == int(np.argmax(z[2]))
    keep = [0, 1, 3, 4]
    assert np.array_equal(NC.bits(z[keep]), NC.bits(z0[keep]))
    assert np.array_equal(NC.bits(lp[keep]), NC.bits(lp0[keep]))
    assert np.array_equal(am[keep], am0[keep])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_joint_nan_row_tiny(dtype):
    """V = 64: every thread of k_select holds at most one logit"""
    check_joint_nan_row(tiny_engine(dtype), 64, 64)


def test_joint_nan_row_cfg2():
    """V = 2048: all 8 register slots of every thread (KEEP = 8)"""
    cfg = synth.model_cfg("cfg2")
    eng = make(synth.synth_state_dict(cfg, seed=0), cfg)
    try:
        check_joint_nan_row(eng, 2048, 1024)
    finally:
        eng.close()


def test_joint_nan_row_big_vocabulary():
    """V = 4112 (tests/decision_edges.py): KEEP = 16 and the tail of the row that is read again from memory; blank 300"""
    import decision_edges as D
    mod = D.model("tiny", 4112, 300)
    eng = make(mod.sd, mod.cfg, blank=mod.blank, bos=mod.bos)
    try:
        check_joint_nan_row(eng, 4112, 64)
    finally:
        eng.close()


@pytest.mark.parametrize("j", [37, 63])
def test_joint_partially_nan_row(j):
    """joint.joint.2.bias[j] = NaN: logit j of every row is NaN and nothing else is; the argmax is j, as np.argmax of the oracle's
    logits gives (NaN is the maximum)"""
    sd, cfg, _ = NC.tiny()
    sd = dict(sd)
    b = sd["joint.joint.2.bias"].copy()
    b[j] = np.nan
    sd["joint.joint.2.bias"] = b
    eng = make(sd, cfg)
    try:
        hp, he = joint_rows(eng, 64)
        z, lp, am = (x.cpu().numpy() for x in eng.joint(dev(hp), dev(he)))
        with np.errstate(all="ignore"):
            ref_z = O.OracleTransducer(sd, cfg).joint_logp(hp, he)[1]
        assert [int(a) for a in ref_z.argmax(-1)] == [j] * 5
        only_j = np.zeros(64, bool)
        only_j[j] = True
        assert all(np.array_equal(np.isnan(z[r]), only_j) for r in range(5))
        assert [int(a) for a in am] == [j] * 5
        assert np.isnan(lp).all()
    finally:
        eng.close()


def test_joint_row_of_minus_inf():
    """every bias -inf: all logits are -inf; the argmax is 0 (np.argmax), log p is NaN (inf - inf), as the oracle's"""
    sd, cfg, _ = NC.tiny()
    sd = dict(sd)
    sd["joint.joint.2.bias"] = np.full(64, -np.inf, np.float32)
    eng = make(sd, cfg)
    try:
        hp, he = joint_rows(eng, 64)
        z, lp, am = (x.cpu().numpy() for x in eng.joint(dev(hp), dev(he)))
        assert np.isneginf(z).all()
        with np.errstate(all="ignore"):
            ref_lp, ref_z = O.OracleTransducer(sd, cfg).joint_logp(hp, he)
        assert np.isneginf(ref_z).all() and [int(a) for a in ref_z.argmax(-1)] == [0] * 5 and np.isnan(ref_lp).all()
        assert [int(a) for a in am] == [0] * 5
        assert np.isnan(lp).all()
    finally:
        eng.close()


# ------------------------------------------------------------------------------- the lattice dynamic programmes
T, U = 6, 3


def lattices():
    """(b, e) of the poisoned lattice [T, U + 1] -- NaN in blank[2, 0] (a cell of column 0: one predecessor) and in emit[3, 1] --,
    of the same lattice with a NaN only in the column of `emit` that is never read, and of a finite lattice [5, 3]"""
    rng = np.random.default_rng(11)
    def rand(t, u):
        return (-rng.integers(1, 256, (t, u + 1)) / 64.0).astype(np.float32), (-rng.integers(1, 256, (t, u + 1)) / 64.0).astype(np.float32)
    b, e = rand(T, U)
    e[:, U] = 0
    bn, en = b.copy(), e.copy()
    bn[2, 0] = np.nan
    en[3, 1] = np.nan
    eu = e.copy()
    eu[4, U] = np.nan
    b2, e2 = rand(5, 2)
    e2[:, 2] = 0
    return (bn, en), (b, eu), (b, e), (b2, e2)


def same_result(a, b):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            assert np.array_equal(np.isnan(x), np.isnan(y)), k
            assert np.array_equal(x[~np.isnan(x)].view(np.int64 if x.dtype == np.float64 else np.int32),
                                  y[~np.isnan(y)].view(np.int64 if y.dtype == np.float64 else np.int32)), k
        else:
            assert np.array_equal(x, y), k


def test_lattice_dp():
    eng = tiny_engine()
    (bn, en), (bu, eu), (b, e), (b2, e2) = lattices()
    with np.errstate(all="ignore"):
        ref = R.forward(bn, en, U)
    assert np.isnan(ref)
    solo = eng.lattice_dp([b2], [e2])[0]
    clean = eng.lattice_dp([b], [e])[0]
    assert np.isfinite(solo["loglik"]) and np.isfinite(clean["loglik"])
    got = eng.lattice_dp([bn, b2, bu, bn], [en, e2, eu, e])
    assert np.isnan(got[0]["loglik"]) == np.isnan(ref)
    # the NaN of column 0 alone: cell (3, 0) has the blank predecessor only, and the NaN must survive the missing one
    with np.errstate(all="ignore"):
        assert np.isnan(R.forward(bn, e, U))
    assert np.isnan(got[3]["loglik"])
    assert all(-1 <= int(f) < T for f in got[0]["frames"]) and len(got[0]["frames"]) == U
    same_result(got[1], solo)                                       # the finite lattice beside it: its solo result, bit for bit
    same_result(got[2], clean)                                      # column U of emit is not read: a NaN there changes nothing
    assert np.isfinite(R.forward(bu, eu, U))


def test_lattice_post():
    eng = tiny_engine()
    (bn, en), (bu, eu), (b, e), (b2, e2) = lattices()
    with np.errstate(all="ignore"):
        _, _, ref, ref_bwd = P.alpha_beta(bn, en, U)
    assert np.isnan(ref) and np.isnan(ref_bwd)
    solo = eng.lattice_post([b2], [e2])[0]
    clean = eng.lattice_post([b], [e])[0]
    got = eng.lattice_post([bn, b2, bu, bn], [en, e2, eu, e])
    assert np.isnan(got[0]["loglik"]) == np.isnan(ref) and np.isnan(got[0]["loglik_bwd"]) == np.isnan(ref_bwd)
    with np.errstate(all="ignore"):
        _, _, ref0, ref0_bwd = P.alpha_beta(bn, e, U)                # the NaN of column 0 alone (one predecessor)
    assert np.isnan(ref0) and np.isnan(ref0_bwd)
    assert np.isnan(got[3]["loglik"]) and np.isnan(got[3]["loglik_bwd"])
    assert all(-1 <= int(f) < T for f in got[0]["tok_peak_frame"])
    same_result(got[1], solo)
    same_result(got[2], clean)


def test_lattice_tree_dp():
    """a tree of 4 nodes with two branches below the root: the NaN enters node 1, so nodes 1 and 3 (its child) are NaN and nodes
    0 and 2 keep finite values -- NaN exactly where the float64 reference has it"""
    eng = tiny_engine()
    (bn, en), _, (b, e), (b2, e2) = lattices()
    parent = [-1, 0, 0, 1]
    bt, et = b.copy(), e.copy()
    et[3, 1] = np.nan                                               # e[t, v]: the emission that enters node v
    bt[2, 3] = np.nan                                               # (a blank of node 3, below node 1)
    with np.errstate(all="ignore"):
        ref = TR.tree_dp(bt, et, parent)
    assert [bool(v) for v in np.isnan(ref)] == [False, True, False, True]
    p2 = [-1, 0, 1]
    solo = eng.lattice_tree_dp([b2], [e2], [p2])[0]
    got = eng.lattice_tree_dp([bt, b2], [et, e2], [parent, p2])
    assert np.array_equal(np.isnan(got[0]["loglik"]), np.isnan(ref))
    fin = ~np.isnan(ref)
    assert np.abs(got[0]["loglik"][fin] - ref[fin]).max() <= 1e-8    # (float64 on both sides: the bound of test_gpu_lattice_tree.py on caller-supplied lattices)
    same_result(got[1], solo)


def test_lattice_band_dp():
    """width 3 of 4 columns, the windows advancing at frame 2; the NaNs sit behind that frame: blank[3, 1] on the lower edge of its
    window (a cell with the blank predecessor alone) and emit[4, 2].  (A NaN that reaches a cell whose blank predecessor lies
    outside the windows is not asked for here: lattice_band_ref.forward decides "impossible" there by Python's max(), which
    returns its first argument against a NaN, while np.logaddexp -- lattice_ref.py, and the kernel -- keeps the NaN.)"""
    eng = tiny_engine()
    _, _, (b, e), (b2, e2) = lattices()
    band = 3
    w = B.width(T, U, band)
    lo = [0, 0, 1, 1, 1, 1]
    assert w == 3 and B.valid(T, U, w, lo)
    bn, en = b.copy(), e.copy()
    bn[3, 1] = np.nan
    en[4, 2] = np.nan
    bb, eb = B.cut(bn, lo, w), B.cut(en, lo, w)
    assert np.isnan(bb).sum() == 1 and np.isnan(eb).sum() == 1       # both NaN cells lie inside their windows
    with np.errstate(all="ignore"):
        ref = B.forward(bb, eb, lo, U)
    assert np.isnan(ref)
    w2, lo2 = B.width(5, 2, band), B.linear(5, 2, band)
    solo = eng.lattice_band_dp([B.cut(b2, lo2, w2)], [B.cut(e2, lo2, w2)], [lo2], [2])[0]
    assert np.isfinite(solo["loglik"])
    got = eng.lattice_band_dp([bb, B.cut(b2, lo2, w2)], [eb, B.cut(e2, lo2, w2)], [lo, lo2], [U, 2])
    assert np.isnan(got[0]["loglik"]) == np.isnan(ref)
    assert all(-1 <= int(f) < T for f in got[0]["frames"]) and len(got[0]["frames"]) == U
    same_result(got[1], solo)
