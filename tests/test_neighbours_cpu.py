"""The nearest-image search without a GPU: its header (include/subgc_neighbours_hip.h, a row of `_lib.HEADERS`; what holds for every
row, the invokers' refusals included, is in test_headers_cpu.py), the exported symbols, every host-side refusal through ctypes, and the
contract in numpy (`neighbours.find_nn_restatement`) against the fixture the reference's own `find_NNimg` wrote (tests/golden/make_golden_neighbours.py).

The tie rule (tests/neighbours_golden.py: compare_lists): outside groups of exactly equal distances every list position holds the
reference's index; a group wholly inside the list holds the reference's set of indices; inside a group the order is ascending index.
How much of a case may be left out as ties is a condition of its own, derived from how the case is built, not from what comes out."""
import os

import numpy as np
import pytest

import neighbours_golden as G
from subgc import _lib, neighbours as NB
from subgc._lib import SubgcError

NAMES = {"subgc_nn_dist_f64", "subgc_nn_select_f64"}
META, ARR = G.load()
CASES = sorted(META["cases"])


def test_the_header_declares_exactly_the_two_entry_points():
    assert os.path.basename(_lib.NEIGHBOURS_HEADER) == "subgc_neighbours_hip.h" and os.path.isfile(_lib.NEIGHBOURS_HEADER)
    protos = _lib.parse_header(_lib.NEIGHBOURS_HEADER)
    assert set(protos) == NAMES
    L = _lib.lib()
    assert _lib.PROTOS["neighbours"] == protos and all(hasattr(L, n) for n in NAMES)
    every = [set(_lib.parse_header(os.path.join(os.path.dirname(_lib.HEADER), h))) for k, h in _lib.HEADERS.items() if k != "neighbours"]
    assert len(every) == len(_lib.HEADERS) - 1 >= 12
    assert not NAMES & set().union(*every)                                  # no name is declared in two headers
    assert sum(len(e) for e in every) == len(set().union(*every))
    assert L.subgc_version() == 1


def test_host_side_refusals_need_no_gpu():
    L = _lib.lib()
    err = lambda: L.subgc_last_error().decode()
    dist = lambda *a: L.subgc_nn_dist_f64(*a)
    # q, ldq, Q, x, ldx, N, D, dist, ldd, stream
    assert dist(None, 8, 2, 16, 8, 3, 8, 16, 3, None) == -1 and "null pointer" in err()
    assert dist(16, 8, 2, None, 8, 3, 8, 16, 3, None) == -1 and "null pointer" in err()
    assert dist(16, 8, 2, 16, 8, 3, 8, None, 3, None) == -1 and "null pointer" in err()
    assert dist(16, 8, 0, 16, 8, 3, 8, 16, 3, None) == -1 and "Q = 0, N = 3, D = 8" in err()
    assert dist(16, 8, 2, 16, 8, 0, 8, 16, 3, None) == -1 and "Q = 2, N = 0, D = 8" in err()
    assert dist(16, 8, 2, 16, 8, 3, 0, 16, 3, None) == -1 and "Q = 2, N = 3, D = 0" in err()
    assert dist(16, 7, 2, 16, 8, 3, 8, 16, 3, None) == -1 and "ldq = 7, ldx = 8" in err() and "D = 8" in err()
    assert dist(16, 8, 2, 16, 5, 3, 8, 16, 3, None) == -1 and "ldq = 8, ldx = 5" in err()
    assert dist(16, 8, 2, 16, 8, 3, 8, 16, 2, None) == -1 and "ldd = 2" in err() and "N = 3" in err()
    assert dist(16, 8, 2, 16, 8, 1 << 31, 8, 16, 1 << 31, None) == -1 and "N = 2147483648" in err() and "2^31" in err()
    sel = lambda *a: L.subgc_nn_select_f64(*a)
    # dist, ldd, Q, N, k, idx, val, stream
    assert sel(None, 5, 2, 5, 3, 16, None, None) == -1 and "null pointer" in err()
    assert sel(16, 5, 2, 5, 3, None, 16, None) == -1 and "null pointer" in err()
    assert sel(16, 5, 0, 5, 3, 16, None, None) == -1 and "Q = 0, N = 5" in err()
    assert sel(16, 5, 2, 0, 3, 16, None, None) == -1 and "Q = 2, N = 0" in err()
    assert sel(16, 4, 2, 5, 3, 16, None, None) == -1 and "ldd = 4" in err() and "N = 5" in err()
    assert sel(16, 1 << 31, 2, 1 << 31, 3, 16, None, None) == -1 and "N = 2147483648" in err()
    assert sel(16, 5, 2, 5, 0, 16, None, None) == -1 and "k = 0" in err() and "min(N, 1024) = 5" in err()
    assert sel(16, 5, 2, 5, 6, 16, None, None) == -1 and "k = 6" in err() and "min(N, 1024) = 5" in err()
    assert sel(16, 5000, 2, 5000, 1025, 16, None, None) == -1 and "k = 1025" in err() and "min(N, 1024) = 1024" in err()


def test_the_host_module_refuses_what_it_cannot_serve():
    with pytest.raises(SubgcError, match="distance_metric = 'cosine'; only 'euclidean'"):
        NB.ImageIndex(np.zeros((3, 2)), device=None, distance_metric="cosine")
    f = np.ones((5, 3), np.float32)
    f[3, 1] = np.inf
    with pytest.raises(SubgcError, match="training feature row 3 holds a non-finite value"):
        NB.ImageIndex(f, device=None)
    with pytest.raises(SubgcError, match="real numbers are needed"):
        NB.ImageIndex(np.zeros((3, 2), np.complex128), device=None)
    with pytest.raises(SubgcError, match=r"an \[N, D\] matrix"):
        NB.ImageIndex(np.zeros(4), device=None)
    ix = NB.ImageIndex(np.arange(12, dtype=np.int16).reshape(4, 3), device=None)
    assert ix.features.dtype == np.float64 and ix.n == 4 and ix.dim == 3
    with pytest.raises(SubgcError, match=r"k = 5; 1 <= k <= min\(N = 4, 1024\)"):
        ix.check_k(5)
    with pytest.raises(SubgcError, match="not on a device"):
        ix.search(np.zeros((1, 3)), k=2)
    with pytest.raises(SubgcError, match="image id 'b' .annotation 1. has no feature vector"):
        NB.ImageIndex.from_annotations({"a": [1.0, 2.0]}, [{"id": "a"}, {"id": "b"}], device=None)
    # the arrangement of consensus_reranking.py:85-87: rows in list order, whatever the dictionary's order
    ix = NB.ImageIndex.from_annotations({"a": np.float32([1, 2]), "b": [3, 4], "c": [5, 6]}, [{"id": "c"}, {"id": "a"}], device=None)
    assert ix.features.tolist() == [[5.0, 6.0], [1.0, 2.0]]


def test_the_fixture_is_the_references_own_run():
    assert META["written_by"] == "the reference's Consensus_Reranking.find_NNimg"
    shapes = {tuple(c["shape"]): c["ks"] for c in META["cases"].values()}
    assert shapes[(5, 97, 7)] == [1, 10, 97] and shapes[(65, 600, 300)] == [100] and shapes[(3, 1001, 2048)] == [1000] and shapes[(1, 4099, 64)] == [1024]
    for name, c in META["cases"].items():
        assert c["branches_agree"] and c["branch_distances_bit_equal"] and c["restatement_distances_bit_equal_scipy"], name
        te, tr = G.features(META, ARR, name)
        assert [len(te), len(tr), te.shape[1]] == c["shape"] and ARR[name + "_cdist"].shape == (len(te), len(tr))


def tie_cap(name, c):
    """How many list positions of a case may lie inside exact-tie groups, from how the case is built."""
    Q, N, _ = c["shape"]
    if c["all_duplicates"]:
        return c["list_positions"], c["list_positions"]                      # every distance of a row is equal: all of them, exactly
    if c["nonfinite"]:
        # the all-1e200 train row and the train row with an inf are both at +inf from each of the Q - 1 finite queries (2 positions each);
        # the query with an inf is at +inf from N - 1 train rows and at NaN from one
        n = 2 * (Q - 1) + (N - 1)
        return n, n
    if c["duplicates"]:
        return 1, c["list_positions"] // 4                                   # some, at most 25 %
    return 0, 0


@pytest.mark.parametrize("name", CASES)
def test_the_references_lists_stay_within_the_tie_caps(name):
    c = META["cases"][name]
    lo, hi = tie_cap(name, c)
    assert lo <= c["tie_positions"] <= hi
    d, k = ARR[name + "_cdist"], c["num_NNimg"]
    assert sum(int(G.tie_positions(d[i], k).sum()) for i in range(len(d))) == c["tie_positions"]      # the meta counts what the matrix shows
    if not c["tie_positions"]:
        assert c["positions_differing_from_stable_order"] == 0


_RESTATED = {}


def restated(name):
    if name not in _RESTATED:
        te, tr = G.features(META, ARR, name)
        _RESTATED[name] = NB.find_nn_restatement(te, tr, META["cases"][name]["num_NNimg"])
    return _RESTATED[name]


@pytest.mark.parametrize("name", CASES)
def test_restated_distances_are_scipys_bits(name):
    _, dist = restated(name)
    ref = ARR[name + "_cdist"]
    nan = np.isnan(ref)
    assert (np.isnan(dist) == nan).all()
    assert (dist.view(np.uint64)[~nan] == ref.view(np.uint64)[~nan]).all()
    if META["cases"][name]["nonfinite"]:
        assert nan.sum() == 1 and np.isinf(ref).sum() == 2 * 3 + 69


@pytest.mark.parametrize("name", CASES)
def test_restated_lists_are_the_references_under_the_tie_rule(name):
    c = META["cases"][name]
    lists, _ = restated(name)
    ref, d = ARR[name + "_lists"], ARR[name + "_cdist"]
    lo, hi = tie_cap(name, c)
    for k in c["ks"]:
        left_out = G.compare_lists(lists, ref, d, k)
        if k == c["num_NNimg"]:
            assert lo <= left_out <= hi and left_out == c["tie_positions"]
        if not hi:
            assert left_out == 0 and (lists[:, :k] == ref[:, :k]).all()
        if c["all_duplicates"]:
            assert (lists[:, :k] == np.arange(k)).all()                      # all equal: the index order
    if c["nonfinite"]:
        nan_at = np.argwhere(np.isnan(d))
        assert len(nan_at) == 1 and lists[nan_at[0][0], -1] == nan_at[0][1] == ref[nan_at[0][0], -1]      # NaN is last, here and there


def test_the_duplicate_case_has_ties_inside_the_lists_and_across_the_cut():
    d, k = ARR["dup_cdist"], 100
    s = np.sort(G.keys(d), axis=1)
    assert (s[:, k - 1] == s[:, k]).any()                                    # a group across the k-th cut
    assert ((s[:, 1:k - 1] == s[:, :k - 2]).sum(1) > 0).sum() >= 10          # groups inside many lists
    assert (s[:, 0] == 0).sum() == 9                                         # the queries that are train rows: distance 0


def test_the_long_case_has_a_zero_distance():
    assert (ARR["long_cdist"] == 0).sum() == 1 and ARR["long_lists"][0, 0] == 4097
