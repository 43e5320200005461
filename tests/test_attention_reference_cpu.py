"""The fp64 restatement of the attention contract (attention_reference.py), pinned without a GPU:
  * it is torch fp64 autograd of the reference project's own formulation (softmax over n_max, mask, renormalise) to 1e-12;
  * its shared-set forms equal its per-sentence forms on sets replicated g times;
  * its tolerance resolves the ways a kernel goes subtly wrong (a dropped tail node, a dropped float4 column chunk, the neighbouring
    sentence's query, a plane left out) by at least 10x, for every output, at the largest shape of each family;
  * the GPU file's case lists reach every reachable template instantiation of csrc/attention_vec.hip and csrc/attention_group.hip."""
import os

import pytest
import torch

import attention_reference as AR
import test_attention_variants_gpu as GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def d64(c, *names):
    return [c[n].double() if torch.is_tensor(c[n]) else c[n] for n in names]


# ----------------------------------------------------------------------------- the reference is the reference project's formulation
def test_reference_equals_autograd_of_softmax_mask_renormalise():
    c = AR.sentence_case(24, 48, lens=[1, 2, 5, 11, 7, 3, 36, 4, 9], n_stride=37, dctx_planes=3)
    S, A, R, lens, off = c["S"], 24, 48, c["lens"], c["off"]
    u, v, q, w_a, b_a = [t.clone().requires_grad_() for t in d64(c, "u", "v", "q", "w_a", "b_a")]
    n_max = max(lens)
    # the padded layout (AttModel.py:461-466): softmax over n_max, mask, renormalise
    up, vp, mk = torch.zeros(S, n_max, A, dtype=D), torch.zeros(S, n_max, R, dtype=D), torch.zeros(S, n_max, dtype=D)
    rows = []
    for s in range(S):
        rows += [(s, i, off[s] + i) for i in range(lens[s])]
    si, ii, mi = (torch.tensor(x) for x in zip(*rows))
    up = up.index_put((si, ii), u[mi]); vp = vp.index_put((si, ii), v[mi]); mk[si, ii] = 1
    e = torch.tanh(up + q.unsqueeze(1)) @ w_a + b_a
    wgt = torch.softmax(e, 1) * mk
    wgt = wgt / wgt.sum(1, keepdim=True)
    ctx = torch.bmm(wgt.unsqueeze(1), vp).squeeze(1)
    f = AR.attn_fwd(*d64(c, "u", "v", "q", "w_a", "b_a"), off, lens, c["n_stride"])
    assert rel(f["alpha"][:, :n_max], wgt.detach()) < 1e-12 and rel(f["ctx"], ctx.detach()) < 1e-12
    assert float(f["alpha"][:, n_max:].abs().max()) == 0
    planes = c["dctx_planes"].double()
    (ctx * planes.sum(0)).sum().backward()
    # the backward takes alpha as an input: the exact one here
    b = AR.attn_bwd(*d64(c, "u", "v", "q", "w_a"), off, lens, f["alpha"], planes)
    assert rel(b["dah"], q.grad) < 1e-12 and rel(b["du"], u.grad) < 1e-12 and rel(b["dv"], v.grad) < 1e-12
    assert rel(b["dw_a"].sum(0), w_a.grad) < 1e-12
    assert abs(float(b["db_a"].sum()) - float(b_a.grad)) < 1e-12          # d(b_a) is zero up to rounding: softmax is shift-invariant
    assert rel(b["dctx_keep"], planes.sum(0)) < 1e-15
    # de_keep is the gradient of the scores: d(loss)/d(e) through the masked, renormalised softmax
    e2 = e.detach().clone().requires_grad_()
    w2 = torch.softmax(e2, 1) * mk
    ((w2 / w2.sum(1, keepdim=True)).unsqueeze(1) @ vp.detach()).squeeze(1).mul(planes.sum(0)).sum().backward()
    assert rel(b["de_keep"][:, :n_max], e2.grad * mk) < 1e-12


def test_empty_set_and_query_planes():
    c = AR.sentence_case(8, 12, lens=[0, 3], n_stride=5, q_planes=9)
    f = AR.attn_fwd(*d64(c, "u", "v", "q", "w_a", "b_a"), c["off"], c["lens"], 5)
    assert float(f["alpha"][0].abs().max()) == 0 and float(f["ctx"][0].abs().max()) == 0 and abs(float(f["alpha"][1].sum()) - 1) < 1e-15
    q = AR.attn_query(c["q_planes"].double(), c["q_bias"].double())
    assert rel(q, c["q_planes"].double().sum(0) + c["q_bias"].double()) < 1e-15


def test_accumulators_equal_the_sum_of_per_step_backwards():
    """du_accum / dv_accum over the packed step layout == adding the per-step backward's increments step by step."""
    c = AR.accum_case(12, 8, [0, 1, 4, 7, 3], 6, 9)
    u, w_a, ah, de, alpha, dctx = d64(c, "u", "w_a", "ah", "de", "alpha", "dctx")
    so, off, lens = c["step_off"], c["off"], c["lens"]
    du = AR.attn_du_accum(u, ah, de, so, off, lens, w_a)["du"]
    dv = AR.attn_dv_accum(alpha, dctx, so, off, lens, c["rows"])["dv"]
    du2, dv2 = torch.zeros_like(du), torch.zeros_like(dv)
    g = torch.Generator().manual_seed(5)
    v = torch.randn(c["rows"], 8, generator=g, dtype=D)
    for t in range(c["T"]):
        o, m = so[t], so[t + 1] - so[t]
        b = AR.attn_bwd(u, v, ah[o:o + m], w_a, off[:m], lens[:m], alpha[o:o + m], dctx[None, o:o + m])
        dv2 += b["dv"]
        # d(u) from the FILED d(e) rows: the same formula with de in place of the step's own
        for s in range(m):
            l, m0 = lens[s], off[s]
            tt = torch.tanh(u[m0:m0 + l] + ah[o + s])
            du2[m0:m0 + l] += de[o + s, :l, None] * w_a * (1 - tt * tt)
    assert rel(dv, dv2) < 1e-12 and rel(du, du2) < 1e-12


@pytest.mark.parametrize("g,Nn", [(1, 5), (3, 7), (5, 37), (8, 13)])
def test_grouped_reference_equals_per_sentence_reference_on_replicated_sets(g, Nn):
    c = AR.group_case(12, 16, g, Nn, n_stride=Nn + 1, dctx_planes=2)
    live = AR.group_live(c["rows"], c["lens"], c["m"], c["B"], g, Nn)
    assert len(live) == c["m"] and sorted(r for _b, r, _l in live) == list(range(c["m"]))
    # the image's rows once per live sentence, in row order: what the reference project feeds its attention
    order = sorted(live, key=lambda x: x[1])
    lens = [l for _b, _r, l in order]
    off = [sum(lens[:i]) for i in range(len(lens))]
    take = torch.cat([torch.arange(b * Nn, b * Nn + l) for b, _r, l in order]) if sum(lens) else torch.zeros(0, dtype=torch.long)
    u, v, q, w_a, b_a, alpha = d64(c, "u", "v", "q", "w_a", "b_a", "alpha")
    planes = c["dctx_planes"].double()
    fg = AR.attn_fwd_group(u, v, q, w_a, b_a, c["rows"], c["lens"], c["m"], c["B"], g, Nn, Nn + 1)
    fs = AR.attn_fwd(u[take], v[take], q[:c["m"]], w_a, b_a, off, lens, Nn + 1)
    assert torch.equal(fg["alpha"], fs["alpha"]) and torch.equal(fg["ctx"], fs["ctx"])
    bg = AR.attn_bwd_group(u, v, q, w_a, c["rows"], c["lens"], c["m"], c["B"], g, Nn, alpha.double(), planes)
    bs = AR.attn_bwd(u[take], v[take], q[:c["m"]], w_a, off, lens, alpha.double(), planes[:, :c["m"]])
    for name in ("dah", "dw_a", "db_a", "dctx_keep"):
        assert torch.equal(bg[name], bs[name]), name
    du = torch.zeros_like(u).index_add_(0, take, bs["du"])                  # the copies' gradients land on the one shared row
    assert rel(bg["du"], du) < 1e-13
    a = AR.group_accum_case(16, g, Nn, 6, Nn + 1)
    dvg = AR.attn_dv_accum_group(a["alpha"].double(), a["dctx"].double(), a["step_off"], a["rows"], a["B"], g, Nn)["dv"]
    want = torch.zeros_like(dvg)
    for t in range(a["T"]):
        o, cnt = a["step_off"][t], a["step_off"][t + 1] - a["step_off"][t]
        for b in range(a["B"]):
            for j in range(g):
                r = a["rows"][b * g + j]
                if 0 <= r < cnt:
                    want[b * Nn:(b + 1) * Nn] += a["alpha"][o + r, :Nn, None].double() * a["dctx"][o + r].double()
    assert rel(dvg, want) < 1e-13
    assert float(dvg[2 * Nn:].abs().max()) == 0                            # the image without a live sentence: zero rows


def test_layout_has_the_edges_the_issue_names():
    for g in GPU.G_SWEEP:
        rows, lens, m, B = AR.group_layout(g, 37)
        img = [rows[b * g:(b + 1) * g] for b in range(B)]
        assert all(0 <= r < m for r in img[0]) and not any(0 <= r < m for r in img[2])
        assert lens[img[0][0]] == 0
        assert any(0 <= r < m for r in img[1])
        if g >= 2:
            assert img[1][0] == -1
        if g >= 3:
            assert img[1][-1] >= m
        if g >= 4:                                          # the dead slot >= m lies in the second workgroup's share: it starts at slot G
            assert g - 1 >= group_G(g) and 2 * group_G(g) >= g
        live_lens = [lens[r] for r in img[1] if 0 <= r < m]
        assert len(set(lens[r] for r in img[0])) > 1 or g == 1, "lens differ inside an image"
        assert all(l <= 35 for l in live_lens)              # image 1 leaves rows past its longest set


# ----------------------------------------------------------------------------- resolving power
RESOLVE = 10.0


def _zero_cols(t, chunk, dim=-1):
    t = t.clone()
    t.narrow(dim, 4 * chunk, 4).zero_()
    return t


def _resolves(fn, args, variants, outputs, bf16_out=()):
    """Every (variant, output) pair listed moves the fp64 reference by >= RESOLVE x that output's tolerance; every output is listed once.
    A variant is (changed inputs, post, outputs it must move).  `post` is NOT an input perturbation: a kernel that skips a column chunk also
    leaves that chunk of the column-wise outputs (q_out, dw_a) unwritten, which no change of an input reproduces, so the hook blanks those
    columns of the result itself -- for them the check says only that the tolerance is far below the values."""
    ref, tol, _ = AR.tolerance(fn, args, bf16_out=bf16_out)
    assert set(outputs) == set(ref), (outputs, list(ref))
    seen = set()
    for name, (changed, post, moves) in variants.items():
        got = fn(**AR.cast(dict(args, **changed), D), tanh=torch.tanh)
        if post:
            post(got)
        for out in moves:
            dev, t = (got[out] - ref[out]).abs(), tol[out]
            ratio = float((dev / t.clamp_min(1e-300)).max())
            assert ratio >= RESOLVE, f"{name} moves {out} by only {ratio:.2f} x its tolerance"
            seen.add(out)
    assert seen == set(outputs), f"no variant moves {set(outputs) - seen}"


def _set(t, idx, val):
    t = t.clone()
    t[idx] = val
    return t


def _dec(lens, i):
    lens = list(lens)
    lens[i] -= 1
    return lens


def _zero(name, chunk):
    def post(got):
        got[name][..., 4 * chunk:4 * chunk + 4] = 0
    return post


def test_tolerance_resolves_subtle_faults_forward():
    """Largest forward shape, query from 9 planes.  Chunks: the last (partial group) one and the first of the second per-lane chunk
    (fwd: 64 float4 of a score row per wave pass, 256 of a value row per workgroup pass)."""
    c = AR.sentence_case(512, 2048, q_planes=9)
    fn, args = AR.fwd_planes(c)
    s = c["lens"].index(130)
    v = {"drop_last_node": ({"lens": _dec(c["lens"], s)}, None, ("alpha", "ctx")),
         "neighbour_query": ({"q_planes": _set(c["q_planes"].transpose(0, 1), s, c["q_planes"][:, s - 1]).transpose(0, 1)}, None, ("alpha", "ctx", "q_out")),
         "drop_plane": ({"q_planes": c["q_planes"][:-1]}, None, ("alpha", "ctx", "q_out"))}
    for ch in (512 // 4 - 1, 64):
        v[f"drop_a_chunk{ch}"] = ({"w_a": _zero_cols(c["w_a"], ch)}, _zero("q_out", ch), ("alpha", "ctx", "q_out"))
    for ch in (2048 // 4 - 1, 256):
        v[f"drop_r_chunk{ch}"] = ({"v": _zero_cols(c["v"], ch)}, None, ("ctx",))
    _resolves(fn, args, v, ("alpha", "ctx", "q_out"))
    _resolves(fn, args, v, ("alpha", "ctx", "q_out"), bf16_out=("ctx",))      # the bound widened by one bf16 rounding of ctx still resolves them


def test_tolerance_resolves_subtle_faults_backward():
    """Largest backward shape, d(ctx) from 5 planes.  db_a = sum_i de_i vanishes identically while the alpha row sums to one, so only a
    fault that breaks the row sum (a dropped node) can move it; a wrong query or a dropped hidden chunk cannot move what does not pass
    through tanh (dv, dctx_keep, de_keep: alpha is an input)."""
    c = AR.sentence_case(1024, 2048, dctx_planes=5)
    args = AR.bwd_args(c)
    s = c["lens"].index(130)
    thru = ("dah", "dw_a", "du")
    v = {"drop_last_node": ({"lens": _dec(c["lens"], s)}, None, ("dah", "dw_a", "db_a", "du", "dv", "de_keep")),
         "neighbour_query": ({"q": _set(c["q"], s, c["q"][s - 1])}, None, thru),
         "drop_plane": ({"dctx_planes": c["dctx_planes"][:-1]}, None, thru + ("dv", "dctx_keep", "de_keep"))}
    for ch in (1024 // 4 - 1, 128):
        v[f"drop_a_chunk{ch}"] = ({"w_a": _zero_cols(c["w_a"], ch)}, _zero("dw_a", ch), thru)
    for ch in (2048 // 4 - 1, 64):
        v[f"drop_r_chunk{ch}"] = ({"dctx_planes": _zero_cols(c["dctx_planes"], ch)}, None, thru + ("dv", "dctx_keep", "de_keep"))
    _resolves(AR.attn_bwd, args, v, ("dah", "dw_a", "db_a", "du", "dv", "dctx_keep", "de_keep"))
    _resolves(AR.attn_bwd, args, v, ("dah", "dw_a", "db_a", "du", "dv", "dctx_keep", "de_keep"), bf16_out=("dah",))


def test_tolerance_resolves_subtle_faults_accumulators():
    """The accumulators' planes are the steps: the variant that leaves one out drops a step."""
    c = AR.accum_case(1024, 260, AR.SENT_LENS, 20, 130)
    s, so = c["lens"].index(130), c["step_off"]
    step3 = slice(so[3], so[4])
    args = {k: c[k] for k in ("u", "ah", "de", "step_off", "off", "lens", "w_a")}
    v = {"drop_last_node": ({"lens": _dec(c["lens"], s)}, None, ("du",)),
         "neighbour_query": ({"ah": _set(c["ah"], so[0] + 3, c["ah"][so[0] + 2])}, None, ("du",)),
         "drop_step": ({"de": _set(c["de"], step3, 0.0)}, None, ("du",))}
    for ch in (1024 // 4 - 1, 128):
        v[f"drop_a_chunk{ch}"] = ({"w_a": _zero_cols(c["w_a"], ch)}, None, ("du",))
    _resolves(AR.attn_du_accum, args, v, ("du",))
    args = {k: c[k] for k in ("alpha", "dctx", "step_off", "off", "lens", "rows")}
    v = {"drop_last_node": ({"lens": _dec(c["lens"], s)}, None, ("dv",)),
         "drop_step": ({"alpha": _set(c["alpha"], step3, 0.0)}, None, ("dv",))}
    for ch in (260 // 4 - 1, 64):
        v[f"drop_r_chunk{ch}"] = ({"dctx": _zero_cols(c["dctx"], ch)}, None, ("dv",))
    _resolves(AR.attn_dv_accum, args, v, ("dv",))
    c = AR.accum_case(8, 2048, AR.SENT_LENS, 20, 130)        # the widest value row subgc_attn_dv_accum serves
    args = {k: c[k] for k in ("alpha", "dctx", "step_off", "off", "lens", "rows")}
    step3 = slice(c["step_off"][3], c["step_off"][4])
    v = {"drop_last_node": ({"lens": _dec(c["lens"], s)}, None, ("dv",)),
         "drop_step": ({"alpha": _set(c["alpha"], step3, 0.0)}, None, ("dv",))}
    for ch in (2048 // 4 - 1, 64):
        v[f"drop_r_chunk{ch}"] = ({"dctx": _zero_cols(c["dctx"], ch)}, None, ("dv",))
    _resolves(AR.attn_dv_accum, args, v, ("dv",))
    a = AR.group_accum_case(1024, 8, 37, 20, 128)
    args = {k: a[k] for k in ("alpha", "dctx", "step_off", "rows", "B", "g", "Nn")}
    so = a["step_off"]
    v = {"drop_last_node": ({"alpha": _set(a["alpha"].t(), 36, 0.0).t()}, None, ("dv",)),
         "drop_step": ({"alpha": _set(a["alpha"], slice(so[3], so[4]), 0.0)}, None, ("dv",))}
    for ch in (1024 // 4 - 1, 64):
        v[f"drop_r_chunk{ch}"] = ({"dctx": _zero_cols(a["dctx"], ch)}, None, ("dv",))
    _resolves(AR.attn_dv_accum_group, args, v, ("dv",))


def test_tolerance_resolves_subtle_faults_shared_sets():
    c = AR.group_case(512, 2048, 8, 37, q_planes=9)
    fn, args = AR.group_fwd_planes(c)
    r = c["rows"][7]                                         # image 0's last slot: all 37 nodes
    assert c["lens"][r] == 37
    other = c["rows"][6]
    v = {"drop_last_node": ({"lens": _dec(c["lens"], r)}, None, ("alpha", "ctx")),
         "neighbour_query": ({"q_planes": _set(c["q_planes"].transpose(0, 1), r, c["q_planes"][:, other]).transpose(0, 1)}, None, ("alpha", "ctx", "q_out")),
         "drop_plane": ({"q_planes": c["q_planes"][:-1]}, None, ("alpha", "ctx", "q_out"))}
    for ch in (512 // 4 - 1, 64):
        v[f"drop_a_chunk{ch}"] = ({"w_a": _zero_cols(c["w_a"], ch)}, _zero("q_out", ch), ("alpha", "ctx", "q_out"))
    for ch in (2048 // 4 - 1, 256):
        v[f"drop_r_chunk{ch}"] = ({"v": _zero_cols(c["v"], ch)}, None, ("ctx",))
    _resolves(fn, args, v, ("alpha", "ctx", "q_out"))
    _resolves(fn, args, v, ("alpha", "ctx", "q_out"), bf16_out=("ctx",))
    c = AR.group_case(1024, 1024, 8, 37, dctx_planes=3)
    r, other = c["rows"][7], c["rows"][6]
    thru = ("dah", "dw_a", "du")
    v = {"drop_last_node": ({"lens": _dec(c["lens"], r)}, None, ("dah", "dw_a", "db_a", "du")),
         "neighbour_query": ({"q": _set(c["q"], r, c["q"][other])}, None, thru),
         "drop_plane": ({"dctx_planes": c["dctx_planes"][:-1]}, None, thru + ("dctx_keep",))}
    for ch in (1024 // 4 - 1, 128):
        v[f"drop_a_chunk{ch}"] = ({"w_a": _zero_cols(c["w_a"], ch)}, _zero("dw_a", ch), thru)
    for ch in (1024 // 4 - 1, 64):
        v[f"drop_r_chunk{ch}"] = ({"dctx_planes": _zero_cols(c["dctx_planes"], ch)}, None, thru + ("dctx_keep",))
    _resolves(AR.attn_bwd_group, AR.group_bwd_args(c), v, ("dah", "dw_a", "db_a", "du", "dctx_keep"))
    _resolves(AR.attn_bwd_group, AR.group_bwd_args(c), v, ("dah", "dw_a", "db_a", "du", "dctx_keep"), bf16_out=("dah",))


# ----------------------------------------------------------------------------- coverage: the dispatch thresholds, mirrored
def ceil_div(a, b):
    return (a + b - 1) // b


def pow2_arm(cr, arms):
    return next(a for a in arms if cr <= a)


# each entry: the expression as it stands in the source, cited so that a changed threshold breaks this table and not silently the coverage
DISPATCH_SOURCE = {
    "sub-gc_amd/csrc/attention_vec.hip": [
        "const int ca = (A / 4 + 63) / 64, cr = (R / 4 + 255) / 256;",          # attn_fwd_vec: line 469
        "if (ca > 2 || cr > 2) return -100;",                                    # line 470
        "const int ca = (A / 4 + 127) / 128, cr = (R / 4 + 63) / 64;",          # attn_bwd_vec: line 493
        "if (ca > 2 || cr > 8) return -100;",                                    # line 494
        "const bool lean = !du && !dv;",                                         # line 495
        "if (cr <= 1) SUBGC_ATT_BWD(1, 1); else if (cr <= 2) SUBGC_ATT_BWD(1, 2); else if (cr <= 4) SUBGC_ATT_BWD(1, 4); else SUBGC_ATT_BWD(1, 8);",   # 505
        "if (lean) SUBGC_ATT_BWD2(attn_bwd_vec_b16_kernel, CA_, CR_);",          # line 501: bf16 sets + lean = the register-capped kernel
        "if (cr <= 1) SUBGC_ATT_DV(1); else if (cr <= 2) SUBGC_ATT_DV(2); else if (cr <= 4) SUBGC_ATT_DV(4); else SUBGC_ATT_DV(8);",                   # 529
        "const int ca = (A / 4 + 127) / 128;",                                   # attn_du_accum_vec: line 538
    ],
    "sub-gc_amd/csrc/attention_group.hip": [
        "inline int group_splits(int g) { return g >= 4 ? 2 : 1; }",            # line 410
        "const int per = (g + splits - 1) / splits;",                            # line 413
        "if (per <= 2) { CALL(2); } else if (per <= 3) { CALL(3); } else if (per <= 5) { CALL(5); } else { CALL(8); }",                               # 414
        "g >= 1 && g <= 8",                                                      # lines 423, 471
        "const int ca = (A / 4 + 63) / 64, cr = (R / 4 + 255) / 256;",          # attn_fwd_group_any: line 427
        "const int ca = (A / 4 + 127) / 128, cr = (R / 4 + 63) / 64;",          # subgc_attn_bwd_group: line 477
        "SUBGC_REQUIRE(ca <= 2 && cr <= 4,",                                     # line 478
        "if (ca == 1 && cr <= 2) hipLaunchKernelGGL((attn_bwd_group_kernel<1, 2, true, G_>)",                                                          # 488
    ],
}


def test_dispatch_table_matches_the_source():
    for path, lines in DISPATCH_SOURCE.items():
        src = open(os.path.join(ROOT, path)).read()
        for line in lines:
            assert line in src, f"{path} no longer holds `{line}`: update the dispatch mirror below"


def fwd_inst(k):
    return ("attn_fwd_vec_kernel", ceil_div(k["A"] // 4, 64), ceil_div(k["R"] // 4, 256), k["uv16"])


def bwd_inst(k):
    ca, cr, lean = ceil_div(k["A"] // 4, 128), pow2_arm(ceil_div(k["R"] // 4, 64), (1, 2, 4, 8)), k["mode"] == "lean"
    return ("attn_bwd_vec_b16_kernel", ca, cr) if k["uv16"] and lean else ("attn_bwd_vec_kernel", ca, cr, k["uv16"], lean)


def group_G(g):
    splits = 2 if g >= 4 else 1
    return pow2_arm(ceil_div(g, splits), (2, 3, 5, 8))


def gfwd_inst(k):
    return ("attn_fwd_group_kernel", ceil_div(k["A"] // 4, 64), ceil_div(k["R"] // 4, 256), k["uv16"], group_G(k["g"]))


def gbwd_inst(k):
    return ("attn_bwd_group_kernel", ceil_div(k["A"] // 4, 128), 2 if ceil_div(k["R"] // 4, 64) <= 2 else 4, k["uv16"], group_G(k["g"]))


BOOL = (False, True)
# G = 8 is instantiated but unreachable: g <= 8 and two workgroups from g = 4 on leave at most ceil(8 / 2) = 4 sentences per workgroup
REACHABLE_G = (2, 3, 5)
REACHABLE = {
    "fwd": {("attn_fwd_vec_kernel", ca, cr, uv) for ca in (1, 2) for cr in (1, 2) for uv in BOOL},
    "bwd": {("attn_bwd_vec_kernel", ca, cr, uv, lean) for ca in (1, 2) for cr in (1, 2, 4, 8) for uv, lean in ((False, False), (False, True), (True, False))}
           | {("attn_bwd_vec_b16_kernel", ca, cr) for ca in (1, 2) for cr in (1, 2, 4, 8)},
    "du_accum": {("attn_du_accum_kernel", ca, uv) for ca in (1, 2) for uv in BOOL},
    "dv_accum": {("attn_dv_accum_kernel", cr) for cr in (1, 2, 4, 8)},
    "group_fwd": {("attn_fwd_group_kernel", ca, cr, uv, G) for ca in (1, 2) for cr in (1, 2) for uv in BOOL for G in REACHABLE_G},
    "group_bwd": {("attn_bwd_group_kernel", ca, cr, uv, G) for ca in (1, 2) for cr in (2, 4) for uv in BOOL for G in REACHABLE_G},
}
# test_kernels_gpu.py::test_deferred_dv_equals_the_per_step_accumulation already runs these R (CR64 = 1, 4, 8); the new file adds R = 260 (2)
EXISTING_DV_ACCUM_R = (48, 1000, 2048)


def test_case_lists_reach_every_reachable_instantiation():
    assert {group_G(g) for g in range(1, 9)} == set(REACHABLE_G) and 8 not in {group_G(g) for g in range(1, 9)}
    src = open(os.path.join(ROOT, "tests", "test_kernels_gpu.py")).read()
    assert "[(9, 48, 5, 7), (40, 1000, 17, 37), (6, 2048, 20, 12)]" in src, "the deferred-d(v) shapes the dv_accum coverage counts on"
    reached = {
        "fwd": {fwd_inst(k) for k in GPU.FWD_CASES},
        "bwd": {bwd_inst(k) for k in GPU.BWD_CASES},
        "du_accum": {("attn_du_accum_kernel", ceil_div(k["A"] // 4, 128), k["uv16"]) for k in GPU.DU_ACCUM_CASES},
        "dv_accum": {("attn_dv_accum_kernel", pow2_arm(ceil_div(R // 4, 64), (1, 2, 4, 8))) for R in EXISTING_DV_ACCUM_R + tuple(k["R"] for k in GPU.DV_ACCUM_CASES)},
        "group_fwd": {gfwd_inst(k) for k in GPU.G_FWD_CASES},
        "group_bwd": {gbwd_inst(k) for k in GPU.G_BWD_CASES},
    }
    for fam, want in REACHABLE.items():
        assert reached[fam] == want, f"{fam}: not reached {sorted(want - reached[fam])}, not reachable {sorted(reached[fam] - want)}"


def test_case_lists_hold_what_the_issue_lists():
    """The shapes, modes, plane counts and sweeps the issue names are all in the lists (the lists may hold more, never less)."""
    has = lambda cases, **kv: any(all(k[a] == b for a, b in kv.items()) for k in cases)
    for A, R in [(4, 4), (252, 1020), (256, 1024), (260, 1028), (512, 2048)]:
        assert all(has(GPU.FWD_CASES, A=A, R=R, uv16=uv) for uv in BOOL)
    assert has(GPU.FWD_CASES, A=24, R=48, pitched=True) and sum(k["ctx16"] for k in GPU.FWD_CASES) >= 2
    assert all(has(GPU.FWD_CASES, qn=n) for n in (1, 3, 8, 9, 16))
    assert all(n in (130, 132) for n in (k["n_stride"] for k in GPU.FWD_CASES + GPU.BWD_CASES))
    assert {k["n_stride"] for k in GPU.FWD_CASES} == {130, 132} == {k["n_stride"] for k in GPU.BWD_CASES}
    for A, R in [(4, 4), (512, 256), (516, 260), (512, 512), (516, 516), (1024, 1024), (24, 1028), (1024, 2048)]:
        assert all(has(GPU.BWD_CASES, A=A, R=R, mode=mode, uv16=uv) for mode in GPU.BWD_MODES for uv in BOOL)
    assert all(has(GPU.BWD_CASES, n=n) for n in (1, 2, 4, 5)) and sum(k["dah16"] for k in GPU.BWD_CASES) >= 2
    assert all(has(GPU.DU_ACCUM_CASES, A=A, uv16=uv) for A in (4, 512, 516, 1024) for uv in BOOL)
    assert has(GPU.DV_ACCUM_CASES, R=260, dead_last=True)
    for cases in (GPU.G_FWD_CASES, GPU.G_BWD_CASES):
        assert all(has(cases, A=256, R=512, Nn=37, g=g) for g in (1, 2, 3, 4, 5, 7, 8))
        assert all(has(cases, g=5, Nn=Nn, n_stride=Nn) for Nn in (1, 2, 13, 14, 25, 37, 128)) and has(cases, n_stride=130)
        assert all(has(cases, uv16=uv) for uv in BOOL)
    for A, R in [(4, 4), (256, 1024), (260, 1028), (512, 2048)]:
        assert all(has(GPU.G_FWD_CASES, A=A, R=R, g=g, uv16=uv) for g in (5, 8) for uv in BOOL)
    for A, R in [(4, 4), (512, 512), (516, 516), (1024, 1024)]:
        assert all(has(GPU.G_BWD_CASES, A=A, R=R, g=g, uv16=uv) for g in (5, 8) for uv in BOOL)
    assert all(has(GPU.G_FWD_CASES, qn=n) for n in (1, 9)) and has(GPU.G_FWD_CASES, ctx16=True)
    assert all(has(GPU.G_BWD_CASES, n=n) for n in (1, 3)) and has(GPU.G_BWD_CASES, dah16=True)
    assert has(GPU.G_BWD_CASES, keep=True) and has(GPU.G_BWD_CASES, keep=False)
    assert [k["R"] for k in GPU.G_DV_CASES] == [4, 260, 1024]
    # sizes: at most 12 sentences / 3 images and about 270 node rows
    assert len(AR.SENT_LENS) == 12 and sum(AR.SENT_LENS) <= 270
