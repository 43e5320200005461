"""Pins tests/lstm_reference.py on the CPU (no GPU, no kernel): agreement with torch.nn.LSTMCell and autograd in fp64, and the mutation
table -- for every case of the GPU variant tables (test_lstm_cell_gpu.py, test_lstm_planes_gpu.py), built by the same calls, every way the
kernels could be subtly wrong must move the affected output by more than 100 x the tolerance the GPU test allows it.  A case whose inputs
cannot see a mutation that applies to it fails here.

`python tests/test_lstm_reference_cpu.py` prints the CPU-float32 error and the bound of every case and output (the table in the docstring of
test_lstm_cell_gpu.py)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "sub-gc_amd")):        # what conftest.py adds under pytest; needed when run as a script
    if p not in sys.path:
        sys.path.insert(0, p)
import lstm_reference as LR  # noqa: E402
import test_lstm_cell_gpu as CELL  # noqa: E402
import test_lstm_planes_gpu as PLANES  # noqa: E402

F64 = torch.float64


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ----------------------------------------------------------------------------- agreement with torch
@pytest.mark.parametrize("keep,dc", [(True, True), (False, True), (True, False)], ids=["dropout-dc", "dc", "dropout"])
def test_cell_matches_lstmcell_and_autograd(keep, dc):
    S, R, scale = 13, 10, 2.0
    torch.manual_seed(3)
    cell = torch.nn.LSTMCell(R, R).double()
    g = torch.Generator().manual_seed(5)
    x, h0 = (torch.randn(S, R, generator=g, dtype=F64, requires_grad=True) for _ in range(2))
    c0 = torch.randn(S, R, generator=g, dtype=F64, requires_grad=True)
    kp = (torch.rand(S, R, generator=g) > 0.5).to(torch.uint8) if keep else None
    dh, dhd, dcn = (torch.randn(S, R, generator=g, dtype=F64) for _ in range(3))
    h1, c1 = cell(x, (h0, c0))
    ga, gb = (x @ cell.weight_ih.t()).detach(), (h0 @ cell.weight_hh.t()).detach()
    f = LR.cell_fwd(ga[None], gb, None, cell.bias_ih.detach(), cell.bias_hh.detach(), c0.detach(), kp, scale)
    assert rel(f["h"], h1.detach()) < 1e-12 and rel(f["c"], c1.detach()) < 1e-12 and rel(f["h2"], h1.detach()) < 1e-12
    hdrop = h1 * kp.double() * scale if keep else h1
    assert rel(f["hdrop"], hdrop.detach()) < 1e-12
    pre = ga + gb + cell.bias_ih.detach() + cell.bias_hh.detach()
    assert rel(f["gates"], torch.cat([torch.sigmoid(pre[:, :R]), torch.sigmoid(pre[:, R:2 * R]), torch.tanh(pre[:, 2 * R:3 * R]),
                                      torch.sigmoid(pre[:, 3 * R:])], 1)) < 1e-12
    loss = (h1 * dh).sum() + (hdrop * dhd).sum() + ((c1 * dcn).sum() if dc else 0.0)
    loss.backward()
    b = LR.cell_bwd(f["gates"], c0.detach(), f["c"], [dh[None]], dhd, kp, scale, dcn if dc else None)
    assert rel(b["dc_prev"], c0.grad) < 1e-12
    # d(pre) is not a leaf of the LSTMCell graph; its images under the two weight matrices are
    assert rel(b["dpre"] @ cell.weight_ih.detach(), x.grad) < 1e-12 and rel(b["dpre"] @ cell.weight_hh.detach(), h0.grad) < 1e-12
    assert rel(b["dpre"].sum(0), cell.bias_ih.grad) < 1e-12


def test_cell_bwd_is_autograd_of_cell_fwd_element_by_element():
    """d(pre) itself (not its image under a weight matrix), with and without c_prev, through the explicit formula as an autograd graph."""
    k = LR.cast(LR.case(7, 6, n_pre=3, sources=((2, 7, 12, 6), (3, 4, 6, 0)), seed=9), F64)
    for cp in (k["c_prev"], None):
        planes = k["pre_planes"].clone().requires_grad_()
        f = LR.cell_fwd(planes, k["g1"], k["g2"], k["b0"], k["b1"], cp, k["keep"], k["scale"])
        src = LR.windows(k)
        dh = LR.sum_sources(src, 7, 6, k["c"])
        ((f["h2"] * dh).sum() + (f["hdrop"] * k["dh_drop"]).sum() + (f["c"] * k["dc"]).sum()).backward()
        b = LR.cell_bwd(f["gates"].detach(), cp, f["c"].detach(), src, k["dh_drop"], k["keep"], k["scale"], k["dc"])
        for p in range(3):                                   # every plane of the sum receives the whole gradient
            assert rel(b["dpre"], planes.grad[p]) < 1e-12
        if cp is None:
            assert float(b["dpre"][:, 6:12].abs().max()) == 0.0


def test_plane_form_equals_summed_form():
    k = LR.cast(LR.case(9, 8, n_pre=5, sources=((3, 9, 24, 8), (8, 4, 8, 0), (2, 0, 16, 8)), rows_h=5, rows_h2=2, seed=11), F64)
    a = LR.cell_fwd(**LR.fwd_args(k))
    b = LR.cell_fwd(**dict(LR.fwd_args(k), pre_planes=LR.sum_planes(k["pre_planes"])[None]))
    for key in a:
        assert torch.equal(torch.isnan(a[key]), torch.isnan(b[key])) and rel(torch.nan_to_num(a[key]), torch.nan_to_num(b[key])) < 1e-12
    assert bool(torch.isnan(a["h"][5:]).all()) and not bool(torch.isnan(a["h"][:5]).any()) and bool(torch.isnan(a["h2"][2:]).all())
    src = LR.windows(k)
    summed = [LR.sum_planes(s)[None] if s.shape[0] and s.shape[1] else s for s in src]
    x, y = LR.cell_bwd(**LR.bwd_args(k)), LR.cell_bwd(**dict(LR.bwd_args(k), sources=summed))
    assert rel(x["dpre"], y["dpre"]) < 1e-12 and rel(x["dc_prev"], y["dc_prev"]) < 1e-12
    one = torch.zeros(9, 8, dtype=F64)
    one[:9] += summed[0][0]
    one[:4] += summed[1][0]
    z = LR.cell_bwd(**dict(LR.bwd_args(k), sources=[one[None]]))
    assert rel(x["dpre"], z["dpre"]) < 1e-12


def test_bf16_round_is_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8, 2.0 ** -133], dtype=F64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 2.0 ** -133], dtype=F64)
    assert torch.equal(LR.bf16_round(x), want) and LR.bf16_round(x).dtype == F64
    y = torch.randn(1000, generator=torch.Generator().manual_seed(1))
    assert float(((LR.bf16_round(y) - y).abs() / y.abs()).max()) <= LR.BF16_ULP          # eight significand bits: at most 2^-8 of the value


def test_streaming_references():
    src = torch.arange(24, dtype=F64).view(12, 2)
    got = LR.packed_time_sum(src, [0, 3, 6, 8, 8], 3)                        # live 3, 3, 2, 0
    assert torch.equal(got, src[0:3] + src[3:6] + torch.cat([src[6:8], torch.zeros(1, 2, dtype=F64)]))
    y = torch.tensor([0.0, -0.0, 2.0 ** -133, -1.0, 2.0])
    assert LR.relu_bwd(torch.ones(5), y, 3.0).tolist() == [0.0, 0.0, 3.0, 0.0, 3.0]
    rows = torch.tensor([1, -1, 1, 0], dtype=torch.int32)
    keep = torch.tensor([[1, 0], [1, 1], [0, 1], [1, 1]], dtype=torch.uint8)
    g = LR.gather_rows_keep(src[:2], rows, keep, 2.0)
    assert g.tolist() == [[4.0, 0.0], [0.0, 0.0], [0.0, 6.0], [0.0, 2.0]]
    assert torch.equal(LR.gather_rows_keep(src[:2], rows, None, 2.0), torch.stack([src[1], torch.zeros(2, dtype=F64), src[1], src[0]]))
    cls = torch.tensor([2, 0, 2, -1, 3, 1], dtype=torch.int32)
    s = LR.class_sum(src[:6], cls, 3)                                        # ids -1 and 3 fall outside [0, 3)
    assert torch.equal(s, torch.stack([src[1], src[5], src[0] + src[2]]))


# ----------------------------------------------------------------------------- the mutation table
FAMILIES = {
    "lstm_fwd": (CELL.FWD_CASES, CELL.fwd_case, "fwd"),
    "lstm_fwd_gemm": (CELL.GEMM_CASES, CELL.gemm_case, "fwd"),
    "lstm_bwd": (CELL.BWD_CASES, CELL.bwd_case, "bwd"),
    "lstm_bwd_planes": (CELL.PLANES_CASES, CELL.planes_case, "bwd"),
    "hand-over": (PLANES.HANDOVER_CASES, PLANES.handover_case, "bwd"),
}
TABLE = [(fam, c) for fam, (cases, _b, _k) in FAMILIES.items() for c in cases]


def bounds(fam, c, k):
    """(fp64 reference, {output: fp32 bound}, {output: CPU-float32 error}) exactly as the GPU test of the family computes them."""
    kind = FAMILIES[fam][2]
    if kind == "fwd":
        ref, err = LR.fp32_error(LR.cell_fwd, LR.fwd_args(k))
        extra = LR.GEMM_RTOL * float(LR.sum_planes(k["pre_planes"]).abs().max()) if fam == "lstm_fwd_gemm" else 0.0
        return ref, {o: LR.bound(err[o], LR.FWD_ATOL, extra) for o in ref}, err
    ref, err = LR.fp32_error(LR.cell_bwd, LR.bwd_args(k))
    extra = LR.GEMM_RTOL * float(LR.sum_planes(k["stacks"][0]["stack"]).abs().max()) if fam == "hand-over" else 0.0
    return ref, {o: LR.bound(err[o], LR.BWD_ATOL, extra) for o in ref}, err


def moved(mut, ref, b, b16):
    """max over the elements both hold of |mutated - reference| / the GPU test's tolerance."""
    ok = ~torch.isnan(ref) & ~torch.isnan(mut)
    return float(((mut - ref).abs() / LR.tol_of(ref, b, b16))[ok].max()) if bool(ok.any()) else 0.0


def with_stack(k, i, **over):
    k2 = dict(k)
    k2["stacks"] = [dict(s, **over) if j == i else s for j, s in enumerate(k["stacks"])]
    return k2


def wrong_stride_window(s, R):
    """What a kernel reads when it steps from plane to plane by rows_i * R instead of the buffer's stride."""
    flat, (n, rows, N, col0) = s["stack"].reshape(-1), (s["n"], s["rows"], s["N"], s["col0"])
    idx = (torch.arange(n)[:, None, None] * rows * R + torch.arange(rows)[None, :, None] * N + col0 + torch.arange(R)[None, None, :])
    return flat[idx]


def fwd_mutations(c, k):
    """(mutation, output, mutated fp64 output) for every mutation that applies to a forward case."""
    a = LR.cast(LR.fwd_args(k), F64)
    S = k["S"]
    out = []
    run = lambda **over: LR.cell_fwd(**dict(a, **over))
    if a["pre_planes"].shape[0] > 1:
        out.append(("drop the last plane", "c", run(pre_planes=a["pre_planes"][:-1])["c"]))
    if a["keep"] is not None and "hdrop" not in c["absent"]:
        out.append(("ignore keep", "hdrop", run(keep=None)["hdrop"]))
        out.append(("ignore scale", "hdrop", run(scale=1.0)["hdrop"]))
    if a["c_prev"] is not None:
        out.append(("c_prev as zero", "c", run(c_prev=None)["c"]))
    if LR.row_limit(c["rows_h"], S) < S:
        out.append(("write h past rows_h", "h", run(rows_h=0)["h"]))
    if LR.row_limit(c["rows_h2"], S) < S and "h2" not in c["absent"]:
        out.append(("write h2 past rows_h2", "h2", run(rows_h2=0)["h2"]))
    return out


def bwd_mutations(c, k):
    a = LR.cast(LR.bwd_args(k), F64)
    S, R = k["S"], k["R"]
    out = []
    run = lambda **over: LR.cell_bwd(**dict(a, **over))["dpre"]
    srcs = lambda k2: LR.cast({"s": LR.windows(k2)}, F64)["s"]
    for i, s in enumerate(k["stacks"]):
        n, rows, N, col0 = s["n"], s["rows"], s["N"], s["col0"]
        if n > 0 and rows > 0:
            out.append((f"drop the last plane of source {i}", "dpre", run(sources=srcs(with_stack(k, i, n=n - 1)))))
        if n > 0 and rows < S and s["stack"].shape[1] >= S:
            out.append((f"add source {i} to rows >= rows_i", "dpre", run(sources=srcs(with_stack(k, i, rows=S)))))
        if n > 0 and rows > 0 and N >= 2 * R:
            off = col0 + R if col0 + 2 * R <= N else col0 - R
            out.append((f"window of source {i} one gate off", "dpre", run(sources=srcs(with_stack(k, i, col0=off)))))
        if n > 1 and rows > 0 and rows * R != s["stack"].shape[1] * N:
            wrong = [wrong_stride_window(s, R).double() if j == i else w for j, w in enumerate(srcs(k))]
            out.append((f"plane stride rows_i R for source {i}", "dpre", run(sources=wrong)))
    if a["dh_drop"] is not None and a["keep"] is not None:
        out.append(("ignore keep", "dpre", run(keep=None)))
        out.append(("ignore scale", "dpre", run(scale=1.0)))
    if a["dc"] is not None:
        out.append(("omit dc", "dpre", run(dc=None)))
    if a["c_prev"] is not None:
        out.append(("c_prev as zero", "dpre", run(c_prev=None)))
    # f and g derivative factors swapped: d(pre_f) takes (1 - g^2), d(pre_g) takes f (1 - f); dct = dc_prev / f
    good = LR.cell_bwd(**a)
    i_, f_, g_ = a["gates"][:, :R], a["gates"][:, R:2 * R], a["gates"][:, 2 * R:3 * R]
    dct = good["dc_prev"] / f_
    cp = torch.zeros_like(dct) if a["c_prev"] is None else a["c_prev"]
    swapped = good["dpre"].clone()
    swapped[:, R:2 * R], swapped[:, 2 * R:3 * R] = dct * cp * (1 - g_ * g_), dct * i_ * f_ * (1 - f_)
    out.append(("swap the f and g derivative factors", "dpre", swapped))
    return out


@pytest.mark.parametrize("fam,c", TABLE, ids=[f"{fam}-{CELL._id(c)}" for fam, c in TABLE])
def test_case_inputs_see_every_mutation(fam, c):
    _cases_, build, kind = FAMILIES[fam]
    k = build(c)
    ref, b, _err = bounds(fam, c, k)
    muts = fwd_mutations(c, k) if kind == "fwd" else bwd_mutations(c, k)      # none for the forward case that leaves every optional term out
    for name, o, mut in muts:
        b16 = c.get("dpre16", False) if o == "dpre" else (c.get("h16", False) if o in ("h", "h2", "hdrop") else False)
        if name.startswith("write h"):
            # the GPU test wants those rows bit-unchanged from UNWRITTEN: the mutation is seen when it writes there, and what it writes is not
            # the value the rows start from
            past = torch.isnan(ref[o])
            assert bool(past.any()) and not bool(torch.isnan(mut[past]).any()), (name, "writes nothing past the limit")
            assert float((mut[past] - CELL.UNWRITTEN).abs().min()) > 100 * b[o], name
            continue
        m = moved(mut, ref[o], b[o], b16)
        assert m > 100.0, f"{fam} {CELL._id(c)}: '{name}' moves {o} by only {m:.1f} x its tolerance"


def test_every_mutation_meets_a_case():
    """Each mutation of the issue's list applies to at least one case of the tables (none is tested vacuously)."""
    seen = set()
    for fam, c in TABLE:
        k = FAMILIES[fam][1](c)
        for name, _o, _m in (fwd_mutations if FAMILIES[fam][2] == "fwd" else bwd_mutations)(c, k):
            seen.add(" ".join(w for w in name.split() if not w.isdigit()))
    for want in ("drop the last plane", "drop the last plane of source", "add source to rows >= rows_i", "window of source one gate off",
                 "plane stride rows_i R for source", "ignore keep", "ignore scale", "omit dc", "c_prev as zero",
                 "swap the f and g derivative factors", "write h past rows_h", "write h2 past rows_h2"):
        assert want in seen, want


def test_variant_tables_cover_what_the_issue_lists():
    fwd, bwd, pl, gm = CELL.FWD_CASES, CELL.BWD_CASES, CELL.PLANES_CASES, CELL.GEMM_CASES
    for cases in (fwd, bwd, pl):
        assert {c["form"] for c in cases} == {"vec", "scalar"}
    assert {c["h16"] for c in fwd} == {False, True} and {c["dpre16"] for c in bwd} == {False, True} == {c["dpre16"] for c in pl}
    for name in ("g1", "g2", "b0", "b1", "c_prev", "keep", "hdrop", "gates", "h2"):
        assert any(name in c["absent"] for c in fwd), name
    for name in ("dh_a", "dh_b", "dh_drop", "keep", "dc", "c_prev"):
        assert any(name in c["absent"] for c in bwd), name
    assert any("dh_drop" not in c["absent"] and "keep" in c["absent"] for c in bwd) and any(not c["absent"] for c in bwd)
    assert any(0 < c["rows_h"] < c["S"] for c in fwd) and any(0 < c["rows_h2"] < c["S"] for c in fwd)
    assert {c["layout"] for c in fwd} >= {"one", "apart", "g1off"}
    ns = {s[0] for c in pl for s in c["sources"]}
    assert ns >= {0, 1, 2, 3, 8} and {len(c["sources"]) for c in pl} == {1, 2, 3}
    assert any(s[1] == 0 for c in pl for s in c["sources"]) and any(0 < s[1] < c["S"] for c in pl for s in c["sources"])
    assert any(len(c["sources"]) == 3 and c["sources"][1][0] == 0 and c["sources"][0][0] > 0 and c["sources"][2][0] > 0 for c in pl)
    for c in pl:                                             # col0 in {0, R, 2R} of a [n, rows, 3R] stack, and one that breaks alignment
        assert all(s[3] + c["R"] <= s[2] for s in c["sources"])
    assert {s[3] // c["R"] for c in pl for s in c["sources"] if s[2] == 3 * c["R"]} == {0, 1, 2}
    assert any(c["R"] % 4 == 0 and (4 * s[3]) % 16 for c in pl for s in c["sources"])
    assert {c["parts"] for c in gm if not c["x16"]} >= {1, 2, 3, 4} and {c["parts"] for c in gm if not c["x16"]} & {5, 6, 8}
    assert {(c["x16"], c["h16"]) for c in gm} == {(False, False), (True, False), (True, True)}
    assert any(0 < c["rows_h"] < c["S"] for c in gm) and all(2.0 * c["S"] * 4 * c["R"] * c["K"] < 4e9 for c in gm)
    gp = PLANES.GEMM_PLANES_CASES
    for b16 in (False, True):
        assert {c["n"] for c in gp if c["b16"] == b16} >= {1, 2, 8} and {c["mode"] for c in gp if c["b16"] == b16} == {"nt", "nn", "tn"}
        assert any(c["strided"] for c in gp if c["b16"] == b16)
    assert all(c["n"] > 1 for c in PLANES.HANDOVER_CASES) and len(PLANES.HANDOVER_CASES) == 2


if __name__ == "__main__":
    for fam, c in TABLE:
        _ref, b, err = bounds(fam, c, FAMILIES[fam][1](c))
        print(f"{fam:16s} {CELL._id(c):90s} " + "  ".join(f"{o} e32 {err[o]:.2e} bound {b[o]:.2e}" for o in b))
