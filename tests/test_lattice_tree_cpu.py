"""N-best rescoring over a prefix tree, without a GPU: lasr_prefix_tree through the library against the Python trie of
tests/lattice_tree_ref.py and the order contract of lasr_prefix_tree.hip.h; the same header stand-alone under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/c/trie_check.cpp); and the float64 tree recursions that the GPU tests take their expected values
from, per candidate against tests/lattice_ref.py on the gathered chain."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lattice_ref as R
import lattice_tree_ref as TR
from libreasr_amd import _native as N


def _lib():
    import __graft_entry__ as graft
    graft.build()
    return N.lib()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def native_trie(cands, cap=None):
    """-> (rc, n_nodes, parent, label, depth, term); the arrays hold cap entries and keep their fill of -7 where nothing is written"""
    lib = _lib()
    k = len(cands)
    nt = np.array([len(c) for c in cands], np.int32)
    tok = np.array([t for c in cands for t in c], np.int32)
    cap = int(nt.sum()) + 1 if cap is None else cap
    par, lab, dep = (np.full(max(cap, 1), -7, np.int32) for _ in range(3))
    term = np.full(max(k, 1), -7, np.int32)
    n = C.c_int(-1)
    rc = lib.lasr_prefix_tree(_p(tok), _p(nt), k, cap, _p(par), _p(lab), _p(dep), _p(term), C.byref(n))
    return rc, n.value, par, lab, dep, term


def check_contract(cands):
    rc, n, par, lab, dep, term = native_trie(cands)
    assert rc == N.LASR_OK
    rp, rl, rd, rt = TR.trie(cands)
    assert n == len(rp)
    assert par[:n].tolist() == rp and lab[:n].tolist() == rl and dep[:n].tolist() == rd and term[:len(cands)].tolist() == rt
    assert np.all(par[n:] == -7) and np.all(lab[n:] == -7) and np.all(dep[n:] == -7)
    # the order's consequences, on the library's own output
    assert (par[0], lab[0], dep[0]) == (-1, -1, 0)
    assert len({tuple(TR.path(rp, v)) for v in range(n)}) == n
    prefixes = {tuple(c[:u]) for c in cands for u in range(len(c) + 1)}
    assert n == len(prefixes)                                           # every distinct prefix is exactly one node
    for v in range(1, n):
        assert 0 <= par[v] < v and dep[v] == dep[par[v]] + 1
        assert dep[v] >= dep[v - 1]                                     # depth non-decreasing: the nodes of one depth are contiguous
        assert dep[v] > dep[v - 1] or par[v] >= par[v - 1]              # parents ascending within a depth: children contiguous
    for j, c in enumerate(cands):
        assert [int(lab[v]) for v in TR.path(rp, int(term[j]))[1:]] == [int(t) for t in c]
    for a in range(len(cands)):
        for b in range(len(cands)):
            assert (term[a] == term[b]) == (list(cands[a]) == list(cands[b]))
    return n


def test_symbols_and_python_surface():
    names = {n for n, _, _ in N.SYMBOLS}
    assert {"lasr_prefix_tree", "lasr_score_pcm", "lasr_score_feats", "lasr_lattice_tree_dp"} <= names
    from libreasr_amd.api import LibreASR
    from libreasr_amd.engine import Engine
    for meth in ("prefix_tree", "score_pcm", "score_feats", "lattice_tree_dp"):
        assert callable(getattr(Engine, meth, None)), meth
    assert callable(getattr(LibreASR, "rescore", None))
    lib = _lib()
    assert lib.lasr_lattice_tree_dp(None, None, None, None, None, None, 1, None, None) == N.LASR_EINVAL      # no context: an error code
    assert lib.lasr_score_feats(None, None, 0, None, None, None, None, None, None, None, None, None) == N.LASR_EINVAL


def test_trie_named_cases():
    assert check_contract([[5, 6, 7]]) == 4                                         # k = 1
    assert check_contract([[]]) == 1
    assert check_contract([[5, 6], [5, 6], [5, 6]]) == 3                            # duplicates share a node
    assert check_contract([[5, 6], [], [5]]) == 3                                   # an empty candidate; one a prefix of another
    assert check_contract([[5, 6], [7, 6], [9], [8, 6, 6]]) == 9                    # branching at the root
    assert check_contract([[5, 6, 7], [5, 6, 8], [5, 6, 9]]) == 6                   # branching at the last label
    # first appearance, not label order: 9 before 3 under the root; the children of node 2 (label 3) follow those of node 1
    rc, n, par, lab, dep, term = native_trie([[9, 1], [3, 2], [9, 0], [3, 1]])
    assert rc == 0 and lab[:n].tolist() == [-1, 9, 3, 1, 0, 2, 1] and par[:n].tolist() == [-1, 0, 0, 1, 1, 2, 2]
    assert term[:4].tolist() == [3, 5, 4, 6]


def test_trie_random_lists():
    rng = np.random.default_rng(4)
    for _ in range(200):
        k = int(rng.integers(1, 10))
        check_contract([[int(t) for t in rng.integers(1, 5, int(rng.integers(0, 7)))] for _ in range(k)])


def test_trie_capacity_and_arguments():
    cands = [[5, 6, 7], [5, 6, 8], [4]]
    rc, n, par, lab, dep, term = native_trie(cands, cap=6)              # exactly enough
    assert rc == N.LASR_OK and n == 6
    rc, n, par, lab, dep, term = native_trie(cands, cap=5)
    assert rc == N.LASR_EFULL and n == 6                                # the need is reported, nothing else is written
    assert np.all(par == -7) and np.all(lab == -7) and np.all(dep == -7) and np.all(term == -7)
    lib = _lib()
    nt, tok, out, n = np.array([2], np.int32), np.array([1, 2], np.int32), np.zeros(4, np.int32), C.c_int(-1)
    args = lambda **kw: [kw.get("tok", _p(tok)), kw.get("nt", _p(nt)), kw.get("k", 1), 4, _p(out), _p(out), _p(out), kw.get("term", _p(out)), C.byref(n)]
    assert lib.lasr_prefix_tree(*args(k=0)) == N.LASR_EINVAL and n.value == 0
    assert lib.lasr_prefix_tree(*args(nt=_p(np.array([-1], np.int32)))) == N.LASR_EINVAL
    assert lib.lasr_prefix_tree(*args(tok=None)) == N.LASR_EINVAL
    assert lib.lasr_prefix_tree(*args(term=None)) == N.LASR_EINVAL
    assert lib.lasr_prefix_tree(_p(tok), _p(nt), 1, 4, _p(out), _p(out), _p(out), _p(out), None) == N.LASR_EINVAL


def test_trie_under_asan_ubsan(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ is part of the image"
    exe = str(tmp_path / "trie_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(root, "tests", "c", "trie_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "trie_check: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


# ------------------------------------------------------------------------------- the reference tree DP
def chain_of(b, e, parent, v):
    """the lattice_ref arrays of the candidate that ends in node v: (b[:, path], e[:, path[1:]] + the unused last column), U"""
    p = TR.path(parent, v)
    U = len(p) - 1
    ec = np.zeros((b.shape[0], U + 1), b.dtype)
    ec[:, :U] = e[:, p[1:]]
    return b[:, p], ec, U


def check_tree_dp(b, e, parent):
    ll, vit = TR.tree_dp(b, e, parent), TR.tree_dp(b, e, parent, best=True)
    for v in range(len(parent)):
        bc, ec, U = chain_of(b, e, parent, v)
        assert abs(ll[v] - R.forward(bc, ec, U)) <= 1e-12, v
        assert abs(vit[v] - R.viterbi(bc, ec, U)[0]) <= 1e-12, v
        assert vit[v] <= ll[v] + 1e-12


def test_tree_dp_against_the_chain_reference_random():
    rng = np.random.default_rng(11)
    for _ in range(12):
        k = int(rng.integers(1, 7))
        parent = TR.trie([[int(t) for t in rng.integers(1, 4, int(rng.integers(0, 9)))] for _ in range(k)])[0]
        T, Nn = int(rng.integers(1, 12)), len(parent)
        check_tree_dp(-rng.random((T, Nn)).astype(np.float32) * 8, -rng.random((T, Nn)).astype(np.float32) * 8, parent)


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_tree_dp_brute_force_sizes(T):
    """every tree over two labels down to depth 3 (U <= 3): each node's chain is one of the sizes test_lattice_cpu.py checks against
    the enumeration of every path"""
    rng = np.random.default_rng(T)
    cands = [[a, b, c][:u] for a in (1, 2) for b in (1, 2) for c in (1, 2) for u in range(4)]
    parent = TR.trie(cands)[0]
    assert len(parent) == 15
    b = -rng.random((T, 15)).astype(np.float32) * 8
    e = -rng.random((T, 15)).astype(np.float32) * 8
    check_tree_dp(b, e, parent)
    ll = TR.tree_dp(b, e, parent)
    for v in range(15):
        bc, ec, U = chain_of(b, e, parent, v)
        scores = [R.path_score(bc, ec, list(fr)) for fr in R.all_paths(T, U)]
        assert abs(ll[v] - float(np.logaddexp.reduce(scores))) <= 1e-12
