"""Attention of the beams without a GPU: the ancestry bookkeeping of the host `beam.search` (the restatement `subgc_beam_step_anc` is
tested against) over a stand-in decoder whose attention rows are a closed-form code of the tokens a row was fed (beam_att_fake), the
tenth header and its binding, and the refusals that happen on the host."""
import ctypes

import numpy as np
import pytest

import beam_att_fake as FK
from subgc import _lib, beam
from subgc._lib import SubgcError

NAMES = {
    "subgc_beam_step_anc": ["tv", "ti", "seq", "lps", "sums", "done_cnt", "done_seq", "done_lps", "done_p", "done_len", "anc", "done_anc", "tok", "src",
                            "n", "t", "T", "G", "bd", "kk", "unk", "constraint", "lam", "cap", "stream"],
    "subgc_beam_att_gather": ["al_step", "ld_step", "steps", "rows", "N", "done_anc", "done_len", "pick", "n", "G", "bd", "cap", "T", "out", "ld_t",
                              "ld_row", "stream"],
}
N_SUB, T, N, LENS = 3, 6, 5, (5, 2, 4)
CONFIGS = [(1, 1), (3, 1), (2, 2), (4, 2)]                                       # (beam, groups)


def run(beam_size, G, constraint, salt):
    eng = FK.HostEngine(N_SUB, beam_size, LENS, N, salt)
    opt = dict(beam_size=beam_size, group_size=G, diversity_lambda=0.5, decoding_constraint=constraint)
    return beam.search(eng, T, opt, return_att=True), beam.search(FK.HostEngine(N_SUB, beam_size, LENS, N, salt), T, opt)


@pytest.mark.parametrize("constraint", [0, 1])
@pytest.mark.parametrize("beam_size,G", CONFIGS)
def test_backtracked_attention_is_the_code_of_the_beams_own_token_chain(beam_size, G, constraint):
    ends_at_0 = ends_last = ends_mid = 0
    for salt in range(6):
        (seq, seqlp, done, att), plain = run(beam_size, G, constraint, salt)
        assert seq.equal(plain[0]) and seqlp.equal(plain[1])                     # the search itself does not change
        assert att["AL"].shape == (T + 1, N_SUB, N) and att["len"].shape == (N_SUB,)
        for s in range(N_SUB):
            assert len(done[s]) == beam_size
            for b, pb in zip(done[s], plain[2][s]):                              # EVERY kept beam, not only the winner
                assert b["seq"].equal(pb["seq"]) and b["logps"].equal(pb["logps"]) and b["p"] == pb["p"] and b["unaug_p"] == pb["unaug_p"]
                L = b["len"]
                words = b["seq"].tolist()
                assert L == (words.index(0) + 1 if 0 in words else T)
                FK.check_beam(words, b["att"], L, s, salt, LENS[s], N)
                ends_at_0 += L == 1
                ends_last += 0 not in words
                ends_mid += 1 < L < T
            w = done[s][0]
            assert att["len"][s] == w["len"]
            np.testing.assert_array_equal(att["AL"][:w["len"], s], w["att"])
            assert not att["AL"][w["len"]:, s].any()                             # zero from the length on; no T + 1-th entry under beam search
    assert ends_mid > 0 and ends_last > 0                                        # beams that end early and beams that end only at the last step
    if beam_size > 1:
        assert ends_at_0 > 0                                                     # ... and a beam whose first word is the end token


def test_tenth_header_parses_and_the_other_nine_keep_their_counts():
    protos = _lib.parse_header(_lib.BEAM_ATT_HEADER)
    assert sorted(protos) == sorted(NAMES)
    for name, want in NAMES.items():
        ret, args = protos[name]
        assert ret is ctypes.c_int and [a for _, a in args] == want, name
        t = dict((a, ty) for ty, a in args)
        assert t["stream"] is ctypes.c_void_p and t["done_anc"] is ctypes.c_void_p and all(t[a] is ctypes.c_int for a in ("n", "T", "G", "bd", "cap"))
    t = dict((a, ty) for ty, a in protos["subgc_beam_att_gather"][1])
    assert t["ld_step"] is ctypes.c_int64 and t["ld_t"] is ctypes.c_int64 and t["ld_row"] is ctypes.c_int64
    assert dict((a, ty) for ty, a in protos["subgc_beam_step_anc"][1])["lam"] is ctypes.c_float
    src = open(_lib.BEAM_ATT_HEADER).read()
    for cite in ("misc/eval_utils.py:45", "AttModel.py:179-234", "AttModel.py:328-340", "CaptionModel.py:170-171", "tenth public header", "4096"):
        assert cite in src, cite
    for name in NAMES:                                                           # every prototype's own comment cites the reference lines
        head = src[:src.index("int " + name + "(")]
        own = head[head.rindex("/*"):]
        assert "CaptionModel.py:" in own and "<=" in own, name
    # subgc_beam_step keeps its signature
    core = _lib.parse_header()["subgc_beam_step"][1]
    assert [a for _, a in core] == [a for a in NAMES["subgc_beam_step_anc"] if a not in ("anc", "done_anc")]


def test_limits_are_refused_on_the_host_with_the_number_in_the_text():
    L = _lib.lib()
    err = lambda: L.subgc_last_error().decode()
    step = lambda T_, bd, kk: L.subgc_beam_step_anc(None, None, None, None, None, None, None, None, None, None, None, None, None, None, 2, 0, T_, 1, bd,
                                                    kk, 11, 0, 0.5, bd * T_, None)
    assert step(65, 2, 4) == -1 and "T <= 64" in err()
    assert step(6, 17, 4) == -1 and "<= 16" in err()
    assert step(6, 2, 19) == -1 and "kk <= 18" in err()
    assert step(6, 2, 4) == -1 and "null pointer" in err()                       # in range: only then are the pointers looked at
    gather = lambda N_, steps=6, T_=6, rows=4: L.subgc_beam_att_gather(None, rows * N_, steps, rows, N_, None, None, None, 2, 1, 2, 12, T_, None,
                                                                       2 * N_, N_, None)
    assert gather(4097) == -1 and "4096" in err()
    assert gather(0) == -1 and "4096" in err()
    assert gather(5, T_=65, steps=65) == -1 and "T <= 64" in err()
    assert gather(5, steps=5) == -1 and "T + G - 1" in err()                     # a step buffer that cannot hold the search
    assert gather(5, rows=6) == -1 and "n * G * bd" in err()
    assert gather(5) == -1 and "null pointer" in err()
    with pytest.raises(SubgcError, match="4097 attention columns; the limit is 4096"):
        beam.check_att_limits(6, 2, 4, 4097)
    with pytest.raises(SubgcError, match="T <= 64"):
        beam.check_att_limits(65, 2, 4, 5)
    beam.check_att_limits(64, 16, 18, 4096)


def test_out_of_range_picks_are_refused_before_the_gather():
    cnt = np.array([[2, 3], [4, 2]])
    assert beam.check_picks([[0, 1], [1, 1]], cnt).dtype == np.int32
    with pytest.raises(SubgcError, match="sub-graph 1 picks group 2; the search has 2"):
        beam.check_picks([[0, 0], [2, 0]], cnt)
    with pytest.raises(SubgcError, match="sub-graph 0 picks group -1"):
        beam.check_picks([[-1, 0], [0, 0]], cnt)
    with pytest.raises(SubgcError, match="sub-graph 0 picks finished beam 2 of group 0, which finished 2"):
        beam.check_picks([[0, 2], [0, 0]], cnt)
    with pytest.raises(SubgcError, match="finished beam -1"):
        beam.check_picks([[0, 0], [1, -1]], cnt)
    with pytest.raises(SubgcError, match=r"picks \[n, 2\]"):
        beam.check_picks([[0, 0, 0]], cnt)


def test_an_engine_without_attention_says_so():
    class NoAtt(FK.HostEngine):
        def attention(self):
            raise ValueError("this engine was built without attention output (return_att)")
    with pytest.raises(ValueError, match="without attention output"):
        beam.search(NoAtt(N_SUB, 2, LENS, N, 0), T, dict(beam_size=2), return_att=True)
