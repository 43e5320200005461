"""The nearest-image search of consensus re-ranking on the device (`find_NNimg`,
misc/consensus_reranking/concensus_reranking_utils/consensus_reranking.py:59-119): for every test image the `num_NNimg` training images
whose features lie nearest -- a float64 `scipy.spatial.distance.cdist(..., 'euclidean')` over 2048-dimensional ResNet features and
`np.argsort(...)[:, :num_NNimg]` (conf_cr.py:14,42,51).

The lists are the REFERENCE'S lists, not lists close to them.  scipy's euclidean cdist is, bit for bit, the sequential sum
`s = 0; for d ascending: t = a[d] - b[d]; s = s + t * t; sqrt(s)` with every operation rounded on its own and a correctly rounded
square root; `subgc_nn_dist_f64` (include/subgc_neighbours_hip.h) follows that loop on the fp64 vector ALU, so its distances are scipy's
bits, and `subgc_nn_select_f64` orders them by (distance, index) with integer work only.

Tie rule: `np.argsort` (quicksort) leaves the order inside a group of exactly equal distances unspecified, and duplicated training images
make such groups real.  Here the lower index comes first; outside such groups the order is the reference's.  NaN (inf - inf) sorts last,
as np.argsort puts it.

`ImageIndex` is the one-time setup (numpy allowed): the training features in float64 on the device -- 29 000 x 2048 x 8 B = 475 MB for
Flickr30k's train + val images, 113 000 x 2048 x 8 B = 1.85 GB for COCO's.
`search` is the per-batch path and only enqueues C-ABI launches; `find_nn` is the drop-in for `self.NNimg_list`;
`find_nn_restatement` states the contract in numpy.  Only `distance_metric = 'euclidean'` (conf_cr.py:42) is supported.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import SubgcError
from ._scoring import resolve_device

NUM_NNIMG = 1000                     # conf_cr.py:51
MAX_K = ops.NN_MAX_K                 # entries of one list (subgc_nn_select_f64)
WORKSPACE_BYTES = 256 << 20          # default limit of the distance workspace of one `search` chunk


def _check_metric(distance_metric):
    if distance_metric != "euclidean":
        raise SubgcError(f"neighbours: distance_metric = {distance_metric!r}; only 'euclidean' (conf_cr.py:42) is supported")


def _as_f64(who, a):
    """What `feat_arr[ind, :] = dct_feat[...]` into an np.float64 array leaves (consensus_reranking.py:85-90): the values converted to
    float64, exactly for every float32 / float16 / integer input."""
    a = np.asarray(a)
    if a.dtype.kind not in "fiub":
        raise SubgcError(f"neighbours: {who} are {a.dtype}; real numbers are needed")
    return np.ascontiguousarray(a, dtype=np.float64)


def find_nn_restatement(te, tr, k):
    """The contract in numpy -> (lists int64 [Q, k], distances fp64 [Q, N]).  Distances: the sequential sum over ascending d, one IEEE
    rounding per operation (numpy's element-wise operations do not fuse), np.sqrt (correctly rounded).  Lists: the stable ascending
    order of the keys (the bit pattern with the sign bit cleared), so equal distances come in ascending index and NaN comes last."""
    te, tr = _as_f64("the query features", te), _as_f64("the training features", tr)
    if te.ndim != 2 or tr.ndim != 2 or te.shape[1] != tr.shape[1]:
        raise SubgcError(f"neighbours: features {te.shape} and {tr.shape} do not share a width")
    if not 1 <= k <= tr.shape[0]:
        raise SubgcError(f"neighbours: k = {k}; 1 <= k <= N = {tr.shape[0]}")
    s = np.zeros((te.shape[0], tr.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(te.shape[1]):
            t = te[:, d, None] - tr[None, :, d]
            s = s + t * t
        dist = np.sqrt(s)
    keys = dist.view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)
    return np.argsort(keys, axis=1, kind="stable")[:, :k].astype(np.int64), dist


class ImageIndex:
    """The training images' features, arranged once: `features` [N, D] of any real dtype, row i = training image i in the order of the
    consensus corpus (`anno_list_ref`).  device="auto": the current GPU; None: host only (`.to(device)` uploads later).  The float64
    matrix is uploaded once and stays: N x D x 8 bytes (475 MB for Flickr30k's 29 000 x 2048, 1.85 GB for COCO's 113 000)."""

    def __init__(self, features, device="auto", distance_metric="euclidean"):
        _check_metric(distance_metric)
        f = _as_f64("the training features", features)
        if f.ndim != 2 or f.shape[0] < 1 or f.shape[1] < 1:
            raise SubgcError(f"neighbours: training features of shape {f.shape}; an [N, D] matrix with N, D >= 1 is needed")
        if f.shape[0] >= 1 << 31:
            raise SubgcError(f"neighbours: {f.shape[0]} training images; the lists hold 32-bit indices")
        bad = np.flatnonzero(~np.isfinite(f).all(1))
        if len(bad):
            raise SubgcError(f"neighbours: training feature row {int(bad[0])} holds a non-finite value ({len(bad)} such rows)")
        self.features, self.n, self.dim = f, f.shape[0], f.shape[1]
        self.device, self.d_features, self._ws = None, None, None
        if device is not None:
            self.to(resolve_device(device))

    @classmethod
    def from_annotations(cls, dct_feat, anno_list, device="auto", distance_metric="euclidean"):
        """Row i = dct_feat[anno_list[i]['id']]: the arrangement of consensus_reranking.py:85-87."""
        if len(anno_list) < 1:
            raise SubgcError("neighbours: an empty annotation list")
        rows = []
        for ind, anno in enumerate(anno_list):
            if anno["id"] not in dct_feat:
                raise SubgcError(f"neighbours: image id {anno['id']!r} (annotation {ind}) has no feature vector")
            rows.append(np.asarray(dct_feat[anno["id"]]).reshape(-1))
        return cls(np.stack(rows), device=device, distance_metric=distance_metric)

    def to(self, device):
        self.device = torch.device(device)
        self.d_features = torch.from_numpy(self.features).to(self.device)
        self._ws = None
        return self

    def queries(self, queries):
        """-> a device fp64 [Q, D] tensor with unit inner stride: a device tensor as it is, a host array converted like the training
        features and uploaded once."""
        if self.device is None:
            raise SubgcError("neighbours: the index is not on a device (ImageIndex(..., device=...) or .to(device))")
        if torch.is_tensor(queries) and queries.is_cuda:
            q = queries
            if q.dtype != torch.float64:
                raise SubgcError(f"neighbours: device queries are {q.dtype}; float64 is needed (the reference's feat_arr_te)")
        else:
            q = torch.from_numpy(_as_f64("the query features", queries.numpy() if torch.is_tensor(queries) else queries)).to(self.device)
        if q.dim() != 2 or q.size(1) != self.dim or q.size(0) < 1:
            raise SubgcError(f"neighbours: queries of shape {tuple(q.shape)}; a [Q, {self.dim}] matrix with Q >= 1 is needed")
        return q if q.stride(1) == 1 or q.size(1) == 1 else q.contiguous()

    def check_k(self, k):
        k = int(k)
        if not 1 <= k <= min(self.n, MAX_K):
            raise SubgcError(f"neighbours: k = {k}; 1 <= k <= min(N = {self.n}, {MAX_K})")
        return k

    def search(self, queries, k=NUM_NNIMG, workspace_bytes=WORKSPACE_BYTES, idx=None, dist=None, want_dist=True):
        """-> (idx int32 [Q, k], dist fp64 [Q, k]) on the device: per query the k nearest training rows in ascending (distance, index)
        order and their distances.  Enqueued on the current stream only: no host copy, no synchronisation.  The [rows, N] distance
        matrix is a workspace: the queries are walked in chunks of workspace_bytes // (8 N) rows (default limit 256 MiB: 1156 rows at
        N = 29 000), and the chunking does not change a bit -- a pair's distance and a row's list depend on that pair and row alone.
        idx / dist: optional caller-owned outputs (contiguous [Q, k]); want_dist=False: the indices alone, dist is None."""
        q = self.queries(queries)
        k, Q, N = self.check_k(k), q.size(0), self.n
        rows = min(Q, int(workspace_bytes) // (8 * N))
        if rows < 1:
            raise SubgcError(f"neighbours: workspace_bytes = {workspace_bytes} holds no row of {N} distances ({8 * N} bytes)")
        if self._ws is None or self._ws.numel() < rows * N:
            self._ws = torch.empty(rows * N, device=self.device, dtype=torch.float64)
        ws = self._ws[:rows * N].view(rows, N)
        idx = torch.empty(Q, k, device=self.device, dtype=torch.int32) if idx is None else idx
        dist = torch.empty(Q, k, device=self.device, dtype=torch.float64) if (dist is None and want_dist) else dist
        if any(t is not None and (tuple(t.shape) != (Q, k) or not t.is_contiguous()) for t in (idx, dist)):
            raise SubgcError(f"neighbours: idx / dist must be contiguous [{Q}, {k}] tensors")
        for a in range(0, Q, rows):
            n = min(rows, Q - a)
            ops.nn_dist(q[a:a + n], self.d_features, ws[:n])
            ops.nn_select(ws[:n], N, k, idx[a:a + n], None if dist is None else dist[a:a + n])
        return idx, dist

    def find_nn(self, queries, k=NUM_NNIMG, workspace_bytes=WORKSPACE_BYTES):
        """The drop-in for `self.NNimg_list` (consensus_reranking.py:108, :114-117): per query a list of Python ints; `np.save` writes it
        as the reference writes NNimg_list_*.npy.  One host copy."""
        idx, _ = self.search(queries, k, workspace_bytes)
        return idx.cpu().numpy().tolist()
