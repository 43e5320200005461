"""Every form of the GCN aggregation behind the seven `ops.gcn_*` wrappers -- nodes <- relations and relations <- nodes, forward and backward;
fp32 or bf16-stored unit outputs, with or without the normalise-on-load triple `aff`, with or without the residual and the bf16 copy of the
result; the float4 kernels, the scalar fallbacks (L % 4 != 0, misaligned rows) and a node loop that strides over gridDim.z -- against the
dense-incidence arithmetic of the reference (graph_conv_unit.py:34-36, graph_conv.py:26,33) restated in fp64.

Tolerances: atol = 1e-5 on fp32 outputs and gradients (that of test_kernels_gpu.py::test_gcn_nodes_and_edges_fwd_bwd); the bf16 copy of a
result equals the rounded result and bf16 gradients equal the rounded fp32 gradients exactly; a scalar kernel equals the float4 kernel on
the same numbers exactly (same summation order)."""
import functools

import pytest
import torch

from subgc import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BFT = torch.bfloat16
N, K = 5, 11
# (subject, object) per relation.  Subject degrees of nodes 0..4: 5, 4, 1, 0, 1; object degrees: 0, 1, 4, 5, 1 -- a full round of four,
# a round and its tail, a lone row and an empty list in each role; the last relation carries the pad id N - 1 (gcn_backbone.py:55-67).
# The second image swaps the roles; both list their relations out of node order.
_REL0 = [(0, 3), (1, 2), (0, 3), (2, 1), (1, 2), (0, 3), (1, 2), (0, 3), (1, 2), (0, 3), (N - 1, N - 1)]
REL = torch.tensor([_REL0, [(o, s) for s, o in _REL0]], dtype=torch.int64)
FORMS = {  # name: (bf16-stored inputs, aff, want16)
    "f32": (False, False, False), "f32_w16": (False, False, True), "f32_aff": (False, True, False),
    "b16": (True, False, False), "b16_aff": (True, True, False), "b16_aff_w16": (True, True, True)}


@functools.lru_cache(maxsize=None)
def _case(L, b16, aff, B=2):
    """Inputs (on the CPU; the fp32 values the device sees) and the fp64 results of one shape; computed once, never written to."""
    g = torch.Generator().manual_seed(L * 4 + b16 * 2 + aff)
    rn = lambda *s: torch.randn(*s, generator=g)
    store = (lambda t: t.to(BFT).float()) if b16 else (lambda t: t)
    rel = REL.repeat(B // 2, 1, 1)
    c = dict(B=B, L=L, b16=b16, rel=rel, y=[store(rn(B, K, L)), store(rn(B, K, L)), store(rn(B, N, L)), store(rn(B, N, L))],
             skx=rn(B, N, L), skp=rn(B, K, L), gx=rn(B, N, L), gp=rn(B, K, L),
             aff=[torch.stack([rn(L) * 0.5, torch.rand(L, generator=g) + 0.5, rn(L) * 0.5]) if aff else None for _ in range(4)])
    ms, mo = torch.zeros(B, N, K, dtype=torch.float64), torch.zeros(B, N, K, dtype=torch.float64)
    for b in range(B):
        for k in range(K):
            ms[b, rel[b, k, 0], k] = 1.0
            mo[b, rel[b, k, 1], k] = 1.0
    # the (normalised) unit outputs: what the gradients of the aggregation kernels are gradients of
    f = [((y.double() - a[0].double()) * a[1].double() + a[2].double()) if aff else y.double() for y, a in zip(c["y"], c["aff"])]
    f = [t.requires_grad_() for t in f]
    unit = lambda adj, x: torch.relu(torch.bmm(adj, x) / (adj.sum(2, keepdim=True) + 1e-7))
    X = (unit(ms, f[0]) + unit(mo, f[1])) / 2
    P = (unit(ms.transpose(1, 2), f[2]) + unit(mo.transpose(1, 2), f[3])) / 2
    (X * c["gx"].double()).sum().backward()
    (P * c["gp"].double()).sum().backward()
    c["X"], c["P"], c["df"] = X.detach(), P.detach(), [t.grad for t in f]
    return c


def _close(got, want, what):
    err = float((got.double().cpu() - want).abs().max())
    print(f"{what}: max |error| {err:.3e}")
    assert err <= 1e-5, (what, err)


def _off1(t):
    """The same numbers in a view that starts one element into its buffer: rows 4 (fp32) or 2 (bf16) bytes off every wider alignment."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def _run(c, skip, want16=False, plain=False, place=lambda t: t, dirs=("nf", "nb", "ef", "eb")):
    """The requested directions through the `ops` wrappers: the plain four (`plain`: fp32 storage, no aff) or the `_bn` ones.  `place`
    puts every floating-point input where the case wants it (aligned as allocated, or one element off)."""
    B, L, b16 = c["B"], c["L"], c["b16"]
    dev = lambda t: None if t is None else place(t.to(DEV))
    rel = c["rel"].to(DEV)
    ptr, edges = ops.csr_build(rel, N)
    y = [dev(t.to(BFT) if b16 else t) for t in c["y"]]
    aff = [None if a is None else a.to(DEV) for a in c["aff"]]
    skx, skp = (dev(c["skx"]), dev(c["skp"])) if skip else (None, None)
    r = {}
    if "nf" in dirs or "nb" in dirs:
        if plain:
            r["X"], act = ops.gcn_nodes_fwd(y[0], y[1], ptr, edges, skx, B, N, K, L)
        else:
            r["X"], r["X16"], act = ops.gcn_nodes_fwd_bn(y[0], y[1], aff[0], aff[1], ptr, edges, skx, B, N, K, L, want16)
    if "nb" in dirs:
        r["df0"], r["df1"] = ops.gcn_nodes_bwd(dev(c["gx"]), act, rel, ptr, B, N, K, L)
        if b16:
            r["df0_16"], r["df1_16"] = ops.gcn_nodes_bwd(dev(c["gx"]), act, rel, ptr, B, N, K, L, bf16=True)
    if "ef" in dirs:
        if plain:
            r["P"] = ops.gcn_edges_fwd(y[2], y[3], rel, skp, B, N, K, L)
        else:
            r["P"], r["P16"] = ops.gcn_edges_fwd_bn(y[2], y[3], aff[2], aff[3], rel, skp, B, N, K, L, want16)
    if "eb" in dirs:
        if plain:
            r["df2"], r["df3"] = ops.gcn_edges_bwd(dev(c["gp"]), y[2], y[3], ptr, edges, B, N, K, L)
        else:
            r["df2"], r["df3"] = ops.gcn_edges_bwd_bn(dev(c["gp"]), y[2], y[3], aff[2], aff[3], ptr, edges, B, N, K, L)
            if b16:
                r["df2_16"], r["df3_16"] = ops.gcn_edges_bwd_bn(dev(c["gp"]), y[2], y[3], aff[2], aff[3], ptr, edges, B, N, K, L, bf16=True)
    torch.cuda.synchronize()
    return r


def _check(c, r, skip, want16=False):
    """Everything `_run` returned against the fp64 results of the case."""
    for name, sk in (("X", "skx"), ("P", "skp")):
        if name in r:
            _close(r[name], c[name] + (c[sk].double() if skip else 0.0), name)
            if want16:
                assert r[name + "16"].dtype == BFT and torch.equal(r[name + "16"], r[name].to(BFT)), name + "16"
            else:
                assert r.get(name + "16") is None
    for i in range(4):
        if f"df{i}" in r:
            assert r[f"df{i}"].dtype == torch.float32
            _close(r[f"df{i}"], c["df"][i], f"df{i}")
        if f"df{i}_16" in r:
            assert r[f"df{i}_16"].dtype == BFT and torch.equal(r[f"df{i}_16"], r[f"df{i}"].to(BFT)), f"df{i}_16"


@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", [4, 132])          # one live lane | a second 128-column edges tile that holds four columns
def test_float4_forms_match_the_dense_reference(L, form, skip):
    b16, aff, want16 = FORMS[form]
    c = _case(L, b16, aff)
    _check(c, _run(c, skip, want16, plain=form == "f32"), skip, want16)


@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
def test_scalar_kernels_when_L_is_no_multiple_of_4(skip):
    """L = 6: nodes-fwd, nodes-bwd and edges-bwd run their one-column-per-thread kernels; edges-fwd has none and refuses."""
    c = _case(6, False, False)
    _check(c, _run(c, skip, plain=True, dirs=("nf", "nb", "eb")), skip)
    with pytest.raises(ops.SubgcError):
        _run(c, skip, plain=True, dirs=("ef",))


@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
def test_scalar_kernels_on_misaligned_rows_equal_the_float4_kernels(skip):
    """L = 8 with every floating-point input one float into a larger buffer: the scalar kernels (and, with a skip, the VEC = false
    edges-fwd) -- bit for bit the float4 results on aligned copies of the same numbers."""
    c = _case(8, False, False)
    aligned, shifted = _run(c, skip, plain=True), _run(c, skip, plain=True, place=_off1)
    _check(c, aligned, skip)
    for k, v in aligned.items():
        assert torch.equal(v, shifted[k]), k


@pytest.mark.parametrize("form", ["f32", "b16_aff"])
def test_node_loop_strides_over_the_z_slices(form):
    """B = 600 images of one column group: gcn_zsplit gives 4 slices for the 5 nodes (3 for the backward's relation quads), so a workgroup
    takes more than one node."""
    b16, aff, want16 = FORMS[form]
    c = _case(4, b16, aff, 600)
    _check(c, _run(c, True, want16, plain=form == "f32"), True, want16)
