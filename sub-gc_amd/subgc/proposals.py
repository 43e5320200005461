"""Sub-graph proposals on the device: candidate sub-graphs drawn from a raw scene graph.

The reference reads every image's candidate sub-graphs from downloaded files (`COCO_graph_mask_1000_rm_duplicate/`, data/README.md:6:
"store the sampled sub-graphs"; dataloader_test.py:216-235, dataloader.py:229-270) and publishes no sampler.  This module draws them:
seed sets -> the neighbour expansion `test.py:132` describes ("greedily find the sub-graphs with neighbors and same-cls nodes",
dataloader_test_sct.py:314-355 = `control_input.extract_greedy`) -> removal of candidates whose node set an earlier candidate already
has -> the two-half item of the plain test loader (`control_input._items`), plus the node-IoU table the training loader's
`choose_subgraphs` reads.  No kernel of its own: `subgc_uniform_f32`, `subgc_row_topk_f32`, `subgc_sct_extract_greedy`,
`subgc_row_count_f32`, `subgc_subgraph_nms_batched`, `subgc_gather_rows_multi_i64`, `subgc_mask_compact` and `subgc_pad_rows_*` do the
work; what is left is integer arithmetic on [sets] / [sets, n_obj] tensors in ATen (DESIGN 4.Z lists the ops), once per image and
outside every token loop.

Seed contract (`restate_seeds` is the same in numpy).  An image has a key k, a non-negative integer below 2^43 (default: its position
in the call; `eval_glue.caption_scene_graphs` derives it from the image id).  Candidate j < n of that image reads the counter-based
stream of `subgc_uniform_f32` under the sampler's `seed` at the offsets

    offset(k, j, c) = k * KEY_STRIDE + j * ROW_PITCH + c        KEY_STRIDE = 2^20, ROW_PITCH = 128

    U[j, c] = uniform(offset(k, j, c))         c < n_obj        (n_obj <= 64)
    w[j]    = uniform(offset(k, j, W_COLUMN))  W_COLUMN = 64

so KEY_STRIDE = 8192 * 128 exceeds n (n_obj + 1) for every n <= 8192 and two keys never share an offset.  With (s_lo, s_hi) = `seeds`:

    s_j   = s_lo + min(floor(float32(w_j) * float32(s_hi - s_lo + 1)), s_hi - s_lo)
    seeds = the s_j columns of U[j] with the largest values, in `subgc_row_topk_f32`'s order (value descending, ties to the lower column)
    seed_mask[j] = OR of 1 << column over them (uint64)

The `min` never binds on the stream's own values (at most 1 - 2^-24, whose product with r <= 32 rounds below r); it guards an injected
w = 1.  The draw of an image is a function of (seed, k) alone: not of the batch, its order, `group` or the rank.

Duplicates: two candidates of an image whose final NODE sets are equal (the relation lists are not compared: the model reads the
node lists, and the test-time NMS compares node sets as well); the first in draw order stays.  One `subgc_subgraph_nms_batched`
launch with score[j] = -j, max_keep = n and thres = 1 - 1 / (2 n_obj): two distinct subsets of n_obj nodes have IoU <=
1 - 1 / n_obj < thres, equal sets have IoU 1 > thres, and the kernel compares in double -- the threshold is derived, not tuned.  The
survivors come back ascending in draw order; an odd last survivor is not used by the item (`assemble_test_batch`, dataloader_test.py:224).

Not claimed: the released weights were trained on candidates of the authors' unpublished sampler, and no caption score on the
candidates of this one has been measured.  The node-IoU formula is `cal_node_iou`'s (models/lib/gpn.py:140-150) by analogy: the
offline files' own formula is not published.  Limits (ValueError with the number): n even, 2 <= n <= 8192 (`subgc_rank_desc_f32`
downstream), 1 <= s_lo <= s_hi <= min(32, obj_num - 1) (`subgc_row_topk_f32`), obj_num - 1 <= 64 objects (one lane each,
subgc_control_input_hip.h), keys below 2^43, relation endpoints inside [0, obj_num - 1).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import call
from .assemble import subgraph_indices
from .control_input import GT_LISTS, MAX_OBJ, _graph_part, _host_offsets, _items, extract_greedy, restate_greedy
from .ops import _ptr, _stream

KEY_STRIDE, ROW_PITCH, W_COLUMN = 1 << 20, 128, 64
MAX_N, MAX_SEEDS, MAX_KEY = 8192, 32, 1 << 43


# ---- numpy restatements of the contracts -----------------------------------------------------------------------------------------------

def restate_uniform(seed, offsets):
    """subgc_uniform_f32's value at every absolute stream offset (Philox-4x32-10: counter = offset // 4, word = offset % 4, key = seed;
    the top 24 bits of the word, scaled by 2^-24) -> float32, shaped like `offsets`."""
    off = np.asarray(offsets, np.uint64)
    ctr, lane = off >> np.uint64(2), (off & np.uint64(3)).astype(np.int64)
    m32 = np.uint64(0xFFFFFFFF)
    c = [ctr & m32, ctr >> np.uint64(32), np.zeros_like(ctr), np.zeros_like(ctr)]
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    word = np.choose(lane, c)
    return ((word >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def stream_offsets(key, n, n_obj):
    """-> (offsets of U [n, n_obj], offsets of w [n]) of image key `key` (the module docstring's formula), uint64."""
    j = np.arange(n, dtype=np.uint64)[:, None]
    base = np.uint64(int(key)) * np.uint64(KEY_STRIDE) + j * np.uint64(ROW_PITCH)
    return base + np.arange(n_obj, dtype=np.uint64)[None, :], (base + np.uint64(W_COLUMN))[:, 0]


def restate_seeds(n, n_obj, seeds, seed, key, U=None, w=None):
    """One image's draw -> (seed_mask [n] uint64, s [n] int64, U [n, n_obj] f32, w [n] f32); `U` / `w` injected or the stream's own."""
    s_lo, s_hi = seeds
    off_u, off_w = stream_offsets(key, n, n_obj)
    U = restate_uniform(seed, off_u) if U is None else np.asarray(U, np.float32).reshape(n, n_obj)
    w = restate_uniform(seed, off_w) if w is None else np.asarray(w, np.float32).reshape(n)
    r = s_hi - s_lo + 1
    s = s_lo + np.minimum(np.floor(w * np.float32(r)).astype(np.int64), s_hi - s_lo)
    mask = np.zeros(n, np.uint64)
    for j in range(n):
        order = sorted(range(n_obj), key=lambda c: (-float(U[j, c]), c))           # value descending, ties to the lower column
        for c in order[:int(s[j])]:
            mask[j] |= np.uint64(1) << np.uint64(c)
    return mask, s, U, w


def restate_extract(seed_mask, object_dist, rel_ind, obj_num, rel_num):
    """The expansion of one image's seed masks: `control_input.restate_greedy` with every status OK, plus the node masks as uint64."""
    rows = restate_greedy(seed_mask, np.zeros(len(seed_mask), np.int32), np.asarray(object_dist), rel_ind, obj_num, rel_num)
    node = np.zeros(len(seed_mask), np.uint64)
    for j in range(len(seed_mask)):
        for v in rows["gpn_obj_ind"][j][rows["att_masks"][j] > 0]:
            node[j] |= np.uint64(1) << np.uint64(v)
    rows["node_mask"] = node
    return rows


def restate_dedup(node_mask):
    """-> (kept: the first candidate of every distinct node set, ascending in draw order; used = 2 * (len(kept) // 2))."""
    seen, kept = set(), []
    for j, m in enumerate(np.asarray(node_mask, np.uint64).tolist()):
        if m not in seen:
            seen.add(m)
            kept.append(j)
    return np.asarray(kept, np.int64), 2 * (len(kept) // 2)


def restate_node_iou(gt_node_mask, node_mask):
    """gt_node_mask [5, n_obj] 0/1 (the sentences' own sub-graphs), node_mask [kept] uint64 -> (inter, union int64 [5, 5 + kept],
    iou float64): |A & B| / |A | B| (gpn.py:149), 0 where both sets are empty (the reference divides by zero there)."""
    gt = np.asarray(gt_node_mask).astype(bool)
    n_obj = gt.shape[1]
    cand = ((np.asarray(node_mask, np.uint64)[:, None] >> np.arange(n_obj, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    cols = np.concatenate([gt, cand.reshape(-1, n_obj)])
    inter = (gt[:, None, :] & cols[None, :, :]).sum(-1).astype(np.int64)
    union = (gt[:, None, :] | cols[None, :, :]).sum(-1).astype(np.int64)
    return inter, union, _quotient(inter, union)


def _quotient(inter, union):
    out = np.zeros(inter.shape, np.float64)
    np.divide(inter.astype(np.float64), union.astype(np.float64), out=out, where=union > 0)
    return out


# ---- the device path -------------------------------------------------------------------------------------------------------------------

class Proposals:
    """What `ProposalSampler.sample` returns.  items: one plain-test-loader item per image (`assemble_test_batch`'s).  table (host,
    numpy): "seed_mask" / "node_mask" uint64 [sum kept], "draw" int64 [sum kept] (the candidate's position among the image's n
    draws), "kept" / "used" int64 [B] (survivors; the even number of them the item holds) and "off" [B + 1] (image b's rows of the
    table are off[b] .. off[b+1]); candidate c of an item (first half, then second half) is row off[b] + c -- the entry
    misc/grd_utils.py:41-42 reads from the mask file as subgraph_mask_list[5 + c].  keys: the images' keys."""

    def __init__(self, items, table, keys, dev):
        self.items, self.table, self.keys, self._dev = items, table, keys, dev


class ProposalSampler:
    """ProposalSampler(n, seeds=(1, 3), seed=2019, obj_num=37, rel_num=65): n candidates per image, each from s_lo .. s_hi seed nodes
    (the module docstring states the draw)."""

    def __init__(self, n, seeds=(1, 3), seed=2019, obj_num=37, rel_num=65):
        n, obj_num, rel_num, seed = int(n), int(obj_num), int(rel_num), int(seed)
        if obj_num - 1 > MAX_OBJ or obj_num < 2:
            raise ValueError(f"ProposalSampler: 1 <= obj_num - 1 <= {MAX_OBJ} objects per image (one lane each), got obj_num = {obj_num}")
        if n < 2 or n > MAX_N or n % 2:
            raise ValueError(f"ProposalSampler: n must be even with 2 <= n <= {MAX_N} (the ranking kernel downstream takes {MAX_N} rows), got {n}")
        if len(tuple(seeds)) != 2:
            raise ValueError(f"ProposalSampler: seeds = (s_lo, s_hi), got {seeds!r}")
        s_lo, s_hi = int(seeds[0]), int(seeds[1])
        top = min(MAX_SEEDS, obj_num - 1)
        if not 1 <= s_lo <= s_hi <= top:
            raise ValueError(f"ProposalSampler: 1 <= s_lo <= s_hi <= {top} = min({MAX_SEEDS}, obj_num - 1) (the top-k kernel serves k <= {MAX_SEEDS}), "
                             f"got ({s_lo}, {s_hi})")
        if not 2 <= rel_num <= 1024:
            raise ValueError(f"ProposalSampler: 2 <= rel_num <= 1024, got {rel_num}")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"ProposalSampler: 0 <= seed < 2^64, got {seed}")
        self.n, self.seeds, self.seed, self.obj_num, self.rel_num = n, (s_lo, s_hi), seed, obj_num, rel_num

    # -- validation, before any launch
    def _check_raw(self, raw):
        fmap = raw["object_fmap"]
        B, n_obj = int(fmap.size(0)), int(fmap.size(1))
        if B < 1:
            raise ValueError(f"ProposalSampler: at least one image, got {B}")
        if n_obj != self.obj_num - 1:
            raise ValueError(f"ProposalSampler: the sampler was built for {self.obj_num - 1} objects per image (obj_num - 1), got {n_obj}")
        rel = raw["rel_ind"]
        if rel.numel():
            lo, hi = (int(v) for v in torch.stack(torch.aminmax(rel)).tolist())
            if lo < 0 or hi >= n_obj:
                raise ValueError(f"ProposalSampler: relation endpoints must lie in [0, {n_obj}), got values from {lo} to {hi}")
        return B, n_obj

    def _keys(self, keys, B):
        keys = list(range(B)) if keys is None else [k for k in keys]
        if len(keys) != B:
            raise ValueError(f"ProposalSampler: {len(keys)} keys for {B} images")
        for k in keys:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < MAX_KEY:
                raise ValueError(f"ProposalSampler: an image key is an integer with 0 <= key < 2^43 = {MAX_KEY}, got {k!r}")
        return [int(k) for k in keys]

    def draw_seeds(self, B, n_obj, keys, device, uniforms=None):
        """-> (seed_mask int64 [B n] holding the 64-bit masks, U [B n, n_obj] f32 view, w [B n] f32 view), nothing is read back."""
        n, (s_lo, s_hi) = self.n, self.seeds
        if uniforms is None:
            buf = torch.empty(B * n, ROW_PITCH, device=device, dtype=torch.float32)
            for b, k in enumerate(keys):                                            # one stream segment per image: the key fixes its offset
                call("subgc_uniform_f32", _ptr(buf[b * n:]), n * ROW_PITCH, self.seed, k * KEY_STRIDE, _stream())
            U, w = buf[:, :n_obj], buf[:, W_COLUMN]
        else:
            U, w = (torch.as_tensor(np.asarray(v.cpu() if torch.is_tensor(v) else v, np.float32)) for v in uniforms)
            if tuple(U.shape) != (B, n, n_obj) or tuple(w.shape) != (B, n):
                raise ValueError(f"ProposalSampler: injected uniforms are U [{B}, {n}, {n_obj}] and w [{B}, {n}], got {tuple(U.shape)} and {tuple(w.shape)}")
            if not bool(torch.isfinite(U).all()) or not bool(((w >= 0) & (w <= 1)).all()):
                raise ValueError("ProposalSampler: injected uniforms must be finite, w within [0, 1]")
            U, w = U.reshape(B * n, n_obj).to(device), w.reshape(B * n).to(device)
        vals = torch.empty(B * n, s_hi, device=device, dtype=torch.float32)
        col = torch.empty(B * n, s_hi, device=device, dtype=torch.int32)
        ops.row_topk(U, s_hi, vals, col, log_softmax=False)
        r = s_hi - s_lo + 1
        s = torch.floor(w * float(r)).to(torch.int64).clamp_(max=r - 1).add_(s_lo)                      # fp32 product, as the contract states it
        live = torch.arange(s_hi, device=device).unsqueeze(0) < s.unsqueeze(1)
        bits = torch.bitwise_left_shift(torch.ones((), device=device, dtype=torch.int64), col.to(torch.int64))
        return (bits * live).sum(1), U, w

    def extract(self, raw, seed_masks, set_off, want_pool_mtx=True):
        """The expansion step for seeds the caller supplies: seed_masks [n_sets] (uint64 numpy, or int64 holding the bits) with set_off
        [B + 1] -> {"object_cls" [B, n_obj] int32, "gpn_obj_ind" [n_sets, obj_num], "att_masks", "gpn_pool_mtx" (unless refused),
        "gpn_pred_ind" [n_sets, rel_num], "gpn_nrel_ind" [n_sets, rel_num, 2]} on the device (`control_input.extract_greedy`, status 0)."""
        B, n_obj = self._check_raw(raw)
        dev = raw["object_fmap"].device
        if not torch.is_tensor(seed_masks):
            seed_masks = torch.from_numpy(np.ascontiguousarray(np.asarray(seed_masks).astype(np.uint64)).view(np.int64))
        seed = seed_masks.to(device=dev, dtype=torch.int64).contiguous()
        seg = _host_offsets(set_off, "set_off", int(seed.numel()))
        if len(seg) != B + 1:
            raise ValueError(f"ProposalSampler.extract: set_off holds {len(seg)} entries for {B} images")
        _host_offsets(raw["rel_off"], "rel_off", int(raw["rel_ind"].size(0)))
        d_off = torch.tensor(seg, dtype=torch.int64, device=dev)
        status = ops.zero_(torch.empty(max(int(seed.numel()), 1), device=dev, dtype=torch.int32))
        cls, obj, att, pool, pred, nrel = extract_greedy(raw["object_dist"], raw["rel_ind"], raw["rel_off"].to(device=dev, dtype=torch.int64), d_off, seed,
                                                         status, self.obj_num, self.rel_num, want_pool_mtx=want_pool_mtx)
        out = {"object_cls": cls, "gpn_obj_ind": obj, "att_masks": att, "gpn_pred_ind": pred, "gpn_nrel_ind": nrel}
        if pool is not None:
            out["gpn_pool_mtx"] = pool
        return out

    def sample(self, raw, keys=None, uniforms=None, seq_per_img=5, materialize=False, want_pool_mtx=True):
        """raw (on the device): the scene-graph entries of `assemble_train_batch` -- object_fmap [B, obj_num-1, D] f32, object_dist
             [B, obj_num-1, C] f32, rel_ind [sum_k, 2] i64, pred_dist [sum_k, P] f32, rel_off [B+1] i64 (of an image's relation rows the
             first rel_num - 1 exist for the model, as in the plain test loader) -- and optionally captions [B * seq_per_img, seq_length].
           keys: one non-negative integer per image (default 0 .. B-1); uniforms: (U [B, n, n_obj], w [B, n]) injected in place of the
             stream (tests).
           -> Proposals.  An image left with fewer than 2 distinct candidates raises ValueError naming its key and the count."""
        B, n_obj = self._check_raw(raw)
        keys = self._keys(keys, B)
        n, dev = self.n, raw["object_fmap"].device
        total = B * n
        graph, _, d_rel_off = _graph_part(raw, self.obj_num, self.rel_num, raw.get("captions"), seq_per_img)
        seed, _, _ = self.draw_seeds(B, n_obj, keys, dev, uniforms)
        d_off = torch.arange(B + 1, device=dev, dtype=torch.int64) * n
        status = ops.zero_(torch.empty(total, device=dev, dtype=torch.int32))
        _, obj, att, _, pred, nrel = extract_greedy(raw["object_dist"], raw["rel_ind"], d_rel_off, d_off, seed, status, self.obj_num, self.rel_num,
                                                    want_pool_mtx=False)
        lens = ops.row_count(att)
        score = -(torch.arange(total, device=dev) % n).to(torch.float32)                                   # -j: exact, distinct, the earliest wins
        keep_all, n_keep, _ = ops.subgraph_nms_batched(score, obj, lens, [n] * B, 1.0 - 1.0 / (2.0 * n_obj), n)
        nodes = (torch.bitwise_left_shift(torch.ones((), device=dev, dtype=torch.int64), obj.clamp(max=63)) * att.to(torch.int64)).sum(1)
        # the chain's one host read: survivor counts and lists, and the table's two masks
        h_keep, h_all, h_seed, h_node = n_keep.cpu().numpy().astype(np.int64), keep_all.cpu().numpy(), seed.cpu().numpy(), nodes.cpu().numpy()
        if int(h_keep.min()) < 2:
            b = int(np.flatnonzero(h_keep < 2)[0])
            raise ValueError(f"ProposalSampler: image key {keys[b]} is left with {int(h_keep[b])} distinct candidate(s) of {n} draws; the test "
                             "loader's item needs at least 2 (one per half)")
        draw = np.concatenate([h_all[b * n:b * n + int(c)] for b, c in enumerate(h_keep)])
        glob = draw + np.repeat(np.arange(B, dtype=np.int64) * n, h_keep)
        off = np.concatenate([[0], np.cumsum(h_keep)]).astype(np.int64)
        table = {"seed_mask": h_seed[glob].view(np.uint64), "node_mask": h_node[glob].view(np.uint64), "draw": draw, "kept": h_keep,
                 "used": 2 * (h_keep // 2), "off": off}
        K = int(glob.size)
        d_glob = torch.from_numpy(glob).to(dev)
        k_node, k_pred, k_nrel = (torch.empty(K, *t.shape[1:], device=dev, dtype=torch.int64) for t in (nodes, pred, nrel))
        ops.take_rows([(nodes, k_node), (pred, k_pred), (nrel.view(total, -1), k_nrel.view(K, -1))], d_glob)
        node_u8 = ((k_node.unsqueeze(1) >> torch.arange(n_obj, device=dev)) & 1).to(torch.uint8)
        k_obj, k_att, k_pool = subgraph_indices(node_u8, self.obj_num, want_pool_mtx=want_pool_mtx)
        rows = {"gpn_obj_ind": (k_obj, True), "att_masks": (k_att, True), "gpn_pred_ind": (k_pred, True), "gpn_nrel_ind": (k_nrel, True)}
        if k_pool is not None:
            rows["gpn_pool_mtx"] = (k_pool, True)
        items = _items(graph, rows, off.tolist(), seq_per_img, materialize)
        return Proposals(items, table, keys, {"node_u8": node_u8, "pred": k_pred, "nrel": k_nrel, "n_obj": n_obj})

    def train_candidates(self, proposals):
        """The kept candidates packed as `assemble_test_batch` takes them (and as the training loader's callers index them: entry 5 + c of
        an image's `subgraph_mask_list` is row cand_off[b] + c) -> {cand_node_mask [K, obj_num-1] u8, cand_pred_mask [K, rel_num-1] u8,
        cand_off [B+1] (host list), cand_nrel [sum, 2] i64, cand_nrel_off [K+1] i64} on the device.  One host read (the relation total)."""
        d, rel_num = proposals._dev, self.rel_num
        pred, nrel = d["pred"], d["nrel"]
        K, dev = int(pred.size(0)), pred.device
        real = pred != rel_num - 1
        pmask = torch.zeros(K, rel_num, device=dev, dtype=torch.uint8).scatter_(1, pred, 1)[:, :rel_num - 1].contiguous()
        noff = torch.zeros(K + 1, device=dev, dtype=torch.int64)
        noff[1:] = real.sum(1).cumsum(0)
        return {"cand_node_mask": d["node_u8"], "cand_pred_mask": pmask, "cand_off": [int(v) for v in proposals.table["off"]],
                "cand_nrel": nrel[real].reshape(-1, 2), "cand_nrel_off": noff}

    def node_iou(self, proposals, gt_node_mask, counts=False):
        """gt_node_mask [B, 5, obj_num-1] 0/1 on the device (the five sentence sub-graphs' node masks, inputs as they are today) ->
        one float64 array [5, 5 + kept_b] per image for `assemble.choose_subgraphs`: columns 0..4 the sentences' own sets, column 5 + c
        kept candidate c.  Intersection and union are integer counts formed on the device; the quotient is formed once, in float64, on
        the host (0 where both sets are empty).  counts=True: -> (iou, inter, union), the int64 counts per image as well."""
        d = proposals._dev
        cand, n_obj, kept = d["node_u8"], d["n_obj"], proposals.table["kept"]
        B, dev = len(kept), cand.device
        if tuple(gt_node_mask.shape) != (B, GT_LISTS, n_obj):
            raise ValueError(f"node_iou: gt_node_mask [{B}, {GT_LISTS}, {n_obj}], got {tuple(gt_node_mask.shape)}")
        gt = (gt_node_mask.to(dev) != 0).to(torch.uint8)
        own_i = (gt.unsqueeze(2) & gt.unsqueeze(1)).sum(-1, dtype=torch.int64)                            # [B, 5, 5]
        own_u = (gt.unsqueeze(2) | gt.unsqueeze(1)).sum(-1, dtype=torch.int64)
        mine = torch.repeat_interleave(gt, torch.from_numpy(kept).to(dev), dim=0, output_size=int(kept.sum()))   # [K, 5, n_obj]: the candidate's image
        c_i = (mine & cand.unsqueeze(1)).sum(-1, dtype=torch.int64)                                       # [K, 5]
        c_u = (mine | cand.unsqueeze(1)).sum(-1, dtype=torch.int64)
        own_i, own_u, c_i, c_u = (t.cpu().numpy() for t in (own_i, own_u, c_i, c_u))
        off = proposals.table["off"]
        inter = [np.concatenate([own_i[b], c_i[off[b]:off[b + 1]].T], 1) for b in range(B)]
        union = [np.concatenate([own_u[b], c_u[off[b]:off[b + 1]].T], 1) for b in range(B)]
        iou = [_quotient(i, u) for i, u in zip(inter, union)]
        return (iou, inter, union) if counts else iou
