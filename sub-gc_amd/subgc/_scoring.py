"""What the evaluation scorers (consensus, diversity, accuracy, grounding, grounding_gt, controllability) share on the host: the same
sentence with another prefix lives here once; a check whose wording differs stays in its module."""
from __future__ import annotations

import numpy as np

from ._lib import SubgcError

MAX_IDS = 65535          # word ids 1 .. 65535 (16-bit lanes of the n-gram key; 0 = no word)


def bad_table(ix_to_word):
    """uint8 [largest id + 1]: 1 where the word is one of `eval_glue.BAD_ENDINGS`."""
    from .eval_glue import BAD_ENDINGS
    bad = np.zeros(max((int(k) for k in ix_to_word), default=0) + 1, np.uint8)
    for k, w in ix_to_word.items():
        bad[int(k)] = w in BAD_ENDINGS
    return bad


def resolve_device(device):
    """`device="auto"`: the current GPU; None stays None (host tables only); anything else -> torch.device."""
    import torch
    if device == "auto":
        return torch.device("cuda", torch.cuda.current_device())
    return None if device is None else torch.device(device)


def check_index(who, image_index, n_img):
    """The reference image of every batch image as python ints; one outside the references is refused."""
    idx = [int(x) for x in image_index]
    for i, j in enumerate(idx):
        if not 0 <= j < n_img:
            raise SubgcError(f"{who}: batch image {i} names reference image {j}; the references hold {n_img} images")
    return idx


def csr(counts):
    """Counts -> int64 offsets [n + 1]."""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def token_rows(who, tok, limit=None):
    """Device token rows must be contiguous int32 / int64 [rows, T] with T <= limit -> (is-int64 flag, T)."""
    import torch
    if tok.dtype not in (torch.int32, torch.int64) or not tok.is_contiguous() or tok.dim() != 2:
        raise SubgcError(f"{who}: contiguous int32 / int64 token rows [rows, T], got {tok.dtype} {tuple(tok.shape)}")
    if limit is not None and tok.size(1) > limit:
        raise SubgcError(f"{who}: token rows of {tok.size(1)} words; the limit is {limit}")
    return int(tok.dtype == torch.int64), tok.size(1)


def id_rows(who, rows, limit):
    """Id lists -> zero-padded int64 [rows, T], T = the longest (at least 1); more than `limit` words are refused."""
    T = max([len(r) for r in rows] + [1])
    if T > limit:
        raise SubgcError(f"{who}: a caption of {T} words; the limit is {limit}")
    seq = np.zeros((len(rows), T), np.int64)
    for r, ids in enumerate(rows):
        seq[r, :len(ids)] = ids
    return seq


def dtypes(arena):
    """numpy or torch: the namespace whose float32 / float64 / uint8 / int8 re-view an int32 arena of that kind."""
    return np if isinstance(arena, np.ndarray) else __import__("torch")
