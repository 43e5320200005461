"""The caption rule of csrc/caption.h (load_row) as three kernel families expose it: the same hand-written token rows through
subgc_consensus_cook in row mode (blen = max(L - 1, 0)), subgc_accuracy_rows (SUBGC_ACC_TESTLEN = L) and subgc_diversity_best
(SUBGC_DIV_WORDS of a one-row selection = max(L, 1)), each against tests/diversity_golden.py's rows_to_ids on the host.  Grounding and
controllability show the length only through outputs their own suites pin with remove_bad_endings on and off."""
import numpy as np
import pytest
import torch

import diversity_golden as G
from subgc import ops
from subgc._lib import call_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAD_N = 8                     # the bad-endings table covers ids 0 .. 7 ...
BAD = {3, 4}                  # ... of which 3 and 4 are bad endings; an id >= BAD_N is never one
TESTLEN, ROW_INT, ROW_F64 = 0, 10, 6          # SUBGC_ACC_TESTLEN, SUBGC_ACC_ROW_INT, SUBGC_ACC_ROW_F64
DIV_WORDS, WANT_WORDS = 3, 2                  # SUBGC_DIV_WORDS, SUBGC_DIV_WANT_WORDS


def rows_for(T):
    """The rows of the rule's edges at width T: an id list is cut to T and padded with zeros."""
    good = [(1, 2)[i % 2] for i in range(T)]
    bad = [(3, 4)[i % 2] for i in range(T)]
    lists = [
        [0] * T,                                     # all zeros
        good,                                        # no terminator at all: L = T (T = 64: every lane)
        good[:T // 2] + [-7] + good[T // 2 + 1:],    # a negative id in the middle ends the caption
        [1, 0, 2, 3],                                # ids behind the first zero do not count
        bad,                                         # every word a bad ending, no terminator: stays whole
        [3, 4, 3],                                   # ... and a short one
        good[:max(T - 2, 0)] + [3, 4],               # two trailing bad endings in the last lanes: trimmed
        [1, 2, 3, 4],                                # ... and in front of a terminator
        [1, 3, 2],                                   # a bad ending followed by a good word: kept
        [1, 2, 3, 1, 4, 4, 4],                       # only the trailing run goes
        [1, 2, 9],                                   # an id >= bad_n at the end: never bad
        [2, 70000],                                  # ... and one beyond 16 bits
        [4, BAD_N],                                  # the first id the table does not cover
    ]
    out = np.zeros((len(lists), T), np.int64)
    for r, ids in enumerate(lists):
        ids = ids[:T]
        out[r, :len(ids)] = ids
    return out


def device_lengths(tok, bad):
    """-> (blen of the cook launch, TESTLEN of accuracy_rows, WORDS of diversity_best) per row, as host lists"""
    rows, T = tok.shape
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    none_k, none_w = torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.float64, device=DEV)
    # consensus: a corpus of zero keys
    ck, cw, cc, cl, cn = ops.consensus_cook(tok, none_k, none_w, 0.0, bad=bad)
    # accuracy: one image holding every row, one reference image with one one-word caption, no BLEU table, a flat length factor
    rwoff, rtok = i32([0, 1]), i32([1])
    rk, rw, rc, rl, rn = ops.consensus_cook(rtok, none_k, none_w, 0.0, woff=rwoff, max_words=1)
    seg, zero, cap_off, boff = i32([0, rows]), i32([0]), i32([0, 1]), i32([0, 0])
    gauss = torch.ones(1, dtype=torch.float64, device=DEV)
    row_i = torch.full((rows, ROW_INT), -1, dtype=torch.int32, device=DEV)
    row_d = torch.zeros(rows, ROW_F64, dtype=torch.float64, device=DEV)
    P, s = ops._ptr, ops._stream()
    call_metrics("subgc_accuracy_rows", P(tok), int(tok.dtype == torch.int64), T, P(bad), 0 if bad is None else bad.numel(), rows, P(seg), 1,
                 P(zero), 1, P(ck), P(cw), P(cc), P(cl), P(cn), P(cap_off), 1, P(rwoff), P(rtok), 1, P(rk), P(rw), P(rc), P(rl), P(rn),
                 P(boff), None, None, 0, P(gauss), 1, 1.2 ** 2, P(row_i), ROW_INT, P(row_d), ROW_F64, s)
    # diversity: set r draws row r alone, so its selection is that row
    n_best = 2
    out_i = torch.full((rows, ops.DIV_COLS + n_best), -1, dtype=torch.int32, device=DEV)
    out_d = torch.zeros(rows, n_best + 1, dtype=torch.float64, device=DEV)
    set_img, set_off, draw = i32([0] * rows), i32(list(range(rows + 1))), i32(list(range(rows)))
    flags = i32([WANT_WORDS] * rows)
    ops.diversity_select(torch.zeros(rows, device=DEV), seg, 1, rows, set_img, set_off, draw, rows, rows, 1, n_best, out_i)
    ops.diversity_best(tok, bad, seg, 1, set_img, flags, rows, n_best, None, None, 0, out_i, out_d)
    torch.cuda.synchronize()
    return cl[:rows].tolist(), row_i[:, TESTLEN].tolist(), out_i[:, DIV_WORDS].tolist()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("T", [1, 5, 64])
def test_three_families_read_a_row_alike(T, dtype):
    rows = rows_for(T)
    tok = torch.from_numpy(rows).to(DEV).to(dtype)
    table = torch.zeros(BAD_N, dtype=torch.uint8, device=DEV)
    table[sorted(BAD)] = 1
    for name, bad_dev, bad_host in (("bad endings", table, BAD), ("no table", None, None)):
        want = [len(ids) for ids in G.rows_to_ids(rows, bad_host)]
        blen, testlen, words = device_lengths(tok, bad_dev)
        for r, L in enumerate(want):                                         # every row, every output: nothing is skipped
            got = (blen[r], testlen[r], words[r])
            assert got == (max(L - 1, 0), L, max(L, 1)), (name, T, r, rows[r].tolist(), L, got)
    if T >= 5:                                                               # the cases are what their comments say at these widths
        L_bad, L_none = ([len(x) for x in G.rows_to_ids(rows, b)] for b in (BAD, None))
        assert L_bad[4] == T and L_bad[6] == T - 2 and L_none[6] == T and L_bad[7:13] == [2, 3, 4, 3, 2, 2] and L_none[2] == T // 2
