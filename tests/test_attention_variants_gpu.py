"""Every reachable variant of the per-step attention kernels (csrc/attention_vec.hip, csrc/attention_group.hip) against the fp64 restatement
of their contract (attention_reference.py), on the MI355X.  The case lists below are plain data: test_attention_reference_cpu.py maps each
case to the template instantiation the dispatch picks for it and asserts that every reachable one is reached.

Bounds: |device - fp64| <= 8 floor + 4 sens per output, both computed from the reference alone (attention_reference.tolerance), plus one
bf16 rounding where the destination is bf16.  Outputs the contract says are overwritten start as NaN, accumulated ones from a known
non-zero pattern, and everything around a view (guard columns, guard rows) from a sentinel that must come back untouched.  Every check
prints `RATIO <family> <output> <error / tolerance>`; DESIGN 3.4.1 tabulates the largest per family."""
import pytest
import torch

import attention_reference as AR
from subgc import ops
from subgc._lib import SubgcError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 777.0
B16_DST = "(bf16-dst)"      # family suffix of the cases whose ctx / dah destination is bf16: their ratio is one bf16 rounding, listed apart


# ----------------------------------------------------------------------------- case lists (read by the CPU coverage test)
def _cases(keys, rows):
    return [dict(zip(keys, r)) for r in rows]


FWD_SHAPES = [(4, 4), (252, 1020), (256, 1024), (260, 1028), (512, 2048), (260, 1020), (252, 1028)]   # the last two: <2,1> and <1,2>
FWD_KEYS = ("A", "R", "uv16", "ctx16", "qn", "n_stride", "pitched")
FWD_CASES = _cases(FWD_KEYS,
                   [(A, R, uv, False, 0, 130 + 2 * ((i + uv) % 2), False) for i, (A, R) in enumerate(FWD_SHAPES) for uv in (False, True)]
                   + [(24, 48, False, False, 0, 130, True), (24, 48, True, False, 0, 132, True)]
                   + [(252, 1020, False, True, 0, 132, False), (512, 2048, True, True, 0, 130, False), (24, 48, False, True, 0, 130, True)]
                   + [(256, 1024, n % 2 == 0, False, n, 130, False) for n in (1, 3, 8, 9, 16)]
                   + [(260, 1028, False, False, 9, 132, False), (4, 4, True, False, 3, 130, False)])

BWD_SHAPES = [(4, 4), (512, 256), (516, 260), (512, 512), (516, 516), (1024, 1024), (24, 1028), (1024, 2048),
              (516, 252), (508, 1020)]                                                                 # the last two: <2,1> and <1,4>
BWD_MODES = ("rmw", "defer_dv", "lean")
BWD_KEYS = ("A", "R", "mode", "uv16", "dah16", "n", "n_stride")
BWD_CASES = _cases(BWD_KEYS,
                   [(A, R, mode, uv, False, (1, 2, 4, 5)[(i + k + uv) % 4], 130 + 2 * ((i + k) % 2))
                    for i, (A, R) in enumerate(BWD_SHAPES) for k, mode in enumerate(BWD_MODES) for uv in (False, True)]
                   + [(512, 512, "rmw", False, True, 1, 130), (1024, 2048, "lean", True, True, 4, 132)])

DU_ACCUM_CASES = _cases(("A", "uv16"), [(A, uv) for A in (4, 512, 516, 1024) for uv in (False, True)])
DV_ACCUM_CASES = _cases(("R", "dead_last"), [(260, False), (260, True)])

G_FWD_SHAPES = [(4, 4), (256, 1024), (260, 1028), (512, 2048), (260, 1020), (252, 1028)]
G_BWD_SHAPES = [(4, 4), (512, 512), (516, 516), (1024, 1024), (516, 256), (512, 1024)]
G_SWEEP = (1, 2, 3, 4, 5, 7, 8)
NN_SWEEP = (1, 2, 13, 14, 25, 37, 128)
GF_KEYS = ("A", "R", "g", "Nn", "n_stride", "uv16", "ctx16", "qn")
G_FWD_CASES = _cases(GF_KEYS,
                     [(256, 512, g, 37, 37, g % 2 == 0, False, 9 if g in (3, 8) else 0) for g in G_SWEEP]
                     + [(256, 512, 5, Nn, Nn, Nn % 2 == 0, False, 0) for Nn in NN_SWEEP] + [(256, 512, 5, 128, 130, False, False, 1)]
                     # every (A, R) at g = 5 and 8 as the issue asks, and at g = 2 so that the G = 2 arm meets every (CA, CR) too
                     + [(A, R, g, 37, 37, uv, False, (0, 1, 9)[(i + g) % 3]) for i, (A, R) in enumerate(G_FWD_SHAPES) for g in (2, 5, 8)
                        for uv in (False, True)]
                     + [(512, 2048, 8, 37, 37, False, True, 0)])
GB_KEYS = ("A", "R", "g", "Nn", "n_stride", "uv16", "dah16", "n", "keep")
G_BWD_CASES = _cases(GB_KEYS,
                     [(256, 512, g, 37, 37, g % 2 == 1, False, 1 + 2 * (g % 2), g % 3 != 0) for g in G_SWEEP]
                     + [(256, 512, 5, Nn, Nn, Nn % 2 == 1, False, 1, True) for Nn in NN_SWEEP] + [(256, 512, 5, 128, 130, False, False, 3, False)]
                     + [(A, R, g, 37, 37, uv, False, (1, 3)[(i + g + uv) % 2], (i + g) % 2 == 0) for i, (A, R) in enumerate(G_BWD_SHAPES)
                        for g in (2, 5, 8) for uv in (False, True)]
                     + [(1024, 1024, 8, 37, 37, True, True, 3, True)])
G_DV_CASES = _cases(("R",), [(4,), (260,), (1024,)])


def _id(c):
    return "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in c.items())


# ----------------------------------------------------------------------------- helpers
def dv_(x, b16=False):
    t = x.to(DEV).contiguous()
    return t.to(torch.bfloat16) if b16 else t


def ints(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def full(shape, val, b16=False):
    return torch.full(shape, val, device=DEV, dtype=torch.bfloat16 if b16 else torch.float32)


def pitched(rows, cols, b16=False, pad=8):
    """A [rows, cols] NaN view inside a [rows, cols + 2 pad] buffer of GUARD (pad elements each side: 16- or 32-byte aligned starts)."""
    buf = full((rows, cols + 2 * pad), GUARD, b16)
    view = buf[:, pad:pad + cols]
    view.fill_(NAN)
    return buf, view


def guards_untouched(buf, cols, pad=8):
    return bool((buf[:, :pad] == GUARD).all()) and bool((buf[:, pad + cols:] == GUARD).all())


def pattern(rows, cols):
    """A known non-zero start value of an accumulated buffer: multiples of 0.25 in [-0.75, 0.75], never zero."""
    i = torch.arange(rows * cols, dtype=torch.float32).view(rows, cols)
    return ((i % 6) - 2.5).sign() * (0.25 + 0.25 * (i % 3))


def plane_window(planes, pad=4):
    """planes [n, rows, cols] fp32 -> the device plane stack [n, rows, cols + 2 pad] (GUARD around) and the window tuple ops.attn_bwd takes."""
    n, rows, cols = planes.shape
    buf = full((n, rows, cols + 2 * pad), GUARD)
    buf[:, :, pad:pad + cols] = planes.to(DEV)
    return buf, (buf, cols + 2 * pad, pad, n, rows * (cols + 2 * pad), rows)


def check(family, ref, tol, got, name, where=None):
    """|got - ref| <= tol element by element (no NaN may be left), `where`: a row / element selection applied to all three."""
    g, r, t = got.double().cpu(), ref[name], tol[name]
    if where is not None:
        g, r, t = g[where], r[where], t[where]
    assert g.shape == r.shape, (name, g.shape, r.shape)
    assert not bool(torch.isnan(g).any()), f"{family} {name}: NaN left in an output the contract says is written"
    err = (g - r).abs()
    bad = err > t
    ratio = float((err / t.clamp_min(1e-300)).max()) if err.numel() and float(err.max()) > 0 else 0.0
    print(f"RATIO {family} {name} {ratio:.3f}")
    assert not bool(bad.any()), f"{family} {name}: max error {float(err.max()):.3e} against tolerance {float(t.min()):.3e} (ratio {ratio:.2f}, {int(bad.sum())} elements)"


# ----------------------------------------------------------------------------- per-sentence family
def run_fwd(c, k):
    S, A, R = c["S"], c["A"], c["R"]
    u, v = dv_(c["u"], k["uv16"]), dv_(c["v"], k["uv16"])
    cbuf, ctx = pitched(S, R, k["ctx16"]) if k["pitched"] else (None, full((S, R), NAN, k["ctx16"]))
    alpha = full((S, c["n_stride"]), NAN)
    w_a, b_a, off, lens = dv_(c["w_a"]).view(1, A), dv_(c["b_a"]), ints(c["off"]), ints(c["lens"])
    out = {"ctx": ctx, "alpha": alpha, "cbuf": cbuf}
    if k["qn"]:
        out["q_out"] = full((S, A), NAN)
        ops.attn_fwd(u, v, out["q_out"], w_a, b_a, off, lens, ctx, alpha, S, A, R, q=(dv_(c["q_planes"]), k["qn"], S * A, dv_(c["q_bias"])))
    else:
        ops.attn_fwd(u, v, dv_(c["q"]), w_a, b_a, off, lens, ctx, alpha, S, A, R)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("k", FWD_CASES, ids=_id)
def test_forward_variants(k):
    c = AR.sentence_case(k["A"], k["R"], n_stride=k["n_stride"], q_planes=k["qn"], bf16_sets=k["uv16"])
    fn, args = AR.fwd_planes(c) if k["qn"] else (AR.attn_fwd, AR.fwd_args(c))
    ref, tol, _ = AR.tolerance(fn, args, bf16_out=("ctx",) if k["ctx16"] else ())
    out = run_fwd(c, k)
    for name in ref:
        check("fwd" + B16_DST * k["ctx16"], ref, tol, out[name], name)
    for s, l in enumerate(c["lens"]):                       # the columns from len on are exact zeros, the empty set gives exact zero rows
        assert l == c["n_stride"] or float(out["alpha"][s, l:].abs().max()) == 0.0
    assert float(out["ctx"][0].float().abs().max()) == 0.0 and c["lens"][0] == 0
    if k["pitched"]:
        assert guards_untouched(out["cbuf"], k["R"])


def run_bwd(c, k, du0=None, dv0=None):
    S, A, R, mode = c["S"], c["A"], c["R"], k["mode"]
    u, v = dv_(c["u"], k["uv16"]), dv_(c["v"], k["uv16"])
    w_a, off, lens = dv_(c["w_a"]).view(1, A), ints(c["off"]), ints(c["lens"])
    out = {"dah": full((S, A), NAN, k["dah16"]), "dw_a": full((S, A), NAN), "db_a": full((S,), NAN)}
    if k["n"] == 1 and mode != "lean":
        out["gbuf"], dctx = pitched(S, R)
        dctx.copy_(c["dctx_planes"][0].to(DEV))
    else:
        out["gbuf"], dctx = plane_window(c["dctx_planes"])
    keep = de = None
    if mode != "lean":
        out["du"] = du0.to(DEV)
    if mode == "rmw":
        out["dv"] = dv0.to(DEV)
    else:
        out["kbuf"], keep = pitched(S, R)
        out["dctx_keep"] = keep
    if mode == "lean":
        de = out["de_keep"] = full((S, c["n_stride"]), GUARD)
    ops.attn_bwd(u, v, dv_(c["q"]), w_a, off, lens, dv_(c["alpha"]), dctx, out["dah"], out.get("du"), out.get("dv"), out["dw_a"], out["db_a"], S, A, R,
                 dctx_keep=keep, de_keep=de)
    torch.cuda.synchronize()
    return out


BWD_OUT = {"rmw": ("dah", "dw_a", "db_a", "du", "dv"), "defer_dv": ("dah", "dw_a", "db_a", "du", "dctx_keep"),
           "lean": ("dah", "dw_a", "db_a", "dctx_keep", "de_keep")}


@pytest.mark.parametrize("k", BWD_CASES, ids=_id)
def test_backward_variants(k):
    c = AR.sentence_case(k["A"], k["R"], n_stride=k["n_stride"], dctx_planes=k["n"], bf16_sets=k["uv16"])
    du0, dv0 = pattern(c["rows"], k["A"]), pattern(c["rows"], k["R"])
    ref, tol, _ = AR.tolerance(AR.attn_bwd, dict(AR.bwd_args(c), du0=du0, dv0=dv0), bf16_out=("dah",) if k["dah16"] else ())
    out = run_bwd(c, k, du0, dv0)
    for name in BWD_OUT[k["mode"]]:
        if name == "de_keep":                                # entries from len on are left alone
            inside = torch.arange(c["n_stride"]).view(1, -1) < torch.tensor(c["lens"]).view(-1, 1)
            check("bwd" + B16_DST * k["dah16"], ref, tol, out[name], name, where=inside)
            assert bool((out[name].cpu()[~inside] == GUARD).all())
        else:
            check("bwd" + B16_DST * k["dah16"], ref, tol, out[name], name)
    assert guards_untouched(out["gbuf"].view(-1, out["gbuf"].shape[-1]), k["R"], pad=8 if out["gbuf"].dim() == 2 else 4)
    if k["mode"] != "rmw":
        assert guards_untouched(out["kbuf"], k["R"])


def _per_step(c, fn):
    for t in range(c["T"]):
        o, m = c["step_off"][t], c["step_off"][t + 1] - c["step_off"][t]
        fn(slice(o, o + m), m)


@pytest.mark.parametrize("k", DU_ACCUM_CASES, ids=_id)
def test_du_accum_variants(k):
    """subgc_attn_du_accum over T = 20 packed, shrinking steps (A = 1024: more than one LDS pass) from the d(e) rows the deferred backward
    files, against the reference and against the per-step read-modify-write of d(u), both at the reference's tolerance."""
    A, R = k["A"], 8
    c = AR.accum_case(A, R, AR.SENT_LENS, 20, 130, bf16_u=k["uv16"])
    S, tot, n = c["S"], c["tot"], c["n_stride"]
    g = torch.Generator().manual_seed(A)
    v = torch.randn(c["rows"], R, generator=g)
    u, vd, ah, w_a = dv_(c["u"], k["uv16"]), dv_(AR.bf16_round(v) if k["uv16"] else v, k["uv16"]), dv_(c["ah"]), dv_(c["w_a"]).view(1, A)
    alpha, dctx, off, lens = dv_(c["alpha"]), dv_(c["dctx"]), ints(c["off"]), ints(c["lens"])
    de, keep = full((tot, n), 0.0), full((tot, R), NAN)
    du_rmw = torch.zeros(c["rows"], A, device=DEV)
    dah, dwa, dba = full((tot, A), NAN), full((tot, A), NAN), full((tot,), NAN)

    def step(sl, m):
        ops.attn_bwd(u, vd, ah[sl], w_a, off, lens, alpha[sl], dctx[sl], dah[sl], du_rmw, None, dwa[sl], dba[sl], m, A, R, dctx_keep=keep[sl])
        ops.attn_bwd(u, vd, ah[sl], w_a, off, lens, alpha[sl], dctx[sl], dah[sl], None, None, dwa[sl], dba[sl], m, A, R, dctx_keep=keep[sl], de_keep=de[sl])
    _per_step(c, step)
    du = full((c["rows"], A), NAN)
    ops.attn_du_accum(u, ah, de, ints(c["step_off"]), c["T"], off, lens, w_a, du, S, A)
    torch.cuda.synchronize()
    args = {"u": c["u"], "ah": c["ah"], "de": de.cpu(), "step_off": c["step_off"], "off": c["off"], "lens": c["lens"], "w_a": c["w_a"]}
    ref, tol, _ = AR.tolerance(AR.attn_du_accum, args)
    check("du_accum", ref, tol, du, "du")
    check("du_accum(per-step)", ref, tol, du_rmw, "du")
    check("du_accum(vs per-step)", {"du": du_rmw.double().cpu()}, tol, du, "du")


@pytest.mark.parametrize("k", DV_ACCUM_CASES, ids=_id)
def test_dv_accum_variants(k):
    c = AR.accum_case(8, k["R"], AR.SENT_LENS, 20, 132, dead_last=k["dead_last"])
    kbuf, keep = pitched(c["tot"], k["R"])
    keep.copy_(c["dctx"].to(DEV))
    dv = full((c["rows"], k["R"]), NAN)
    ops.attn_dv_accum(dv_(c["alpha"]), keep, ints(c["step_off"]), c["T"], ints(c["off"]), ints(c["lens"]), dv, c["S"], k["R"])
    torch.cuda.synchronize()
    args = {"alpha": c["alpha"], "dctx": c["dctx"], "step_off": c["step_off"], "off": c["off"], "lens": c["lens"], "rows": c["rows"]}
    ref, tol, _ = AR.tolerance(AR.attn_dv_accum, args)
    check("dv_accum", ref, tol, dv, "dv")
    if k["dead_last"]:                                       # live at no step: its rows are written, as zeros
        assert float(dv[c["off"][-1]:].abs().max()) == 0.0


def _small():
    c = AR.sentence_case(24, 48, lens=[3, 5, 2], n_stride=8)
    return c, dict(uv16=False, ctx16=False, qn=0, pitched=False, mode="rmw", dah16=False, n=1)


def test_refusals_name_the_sizes():
    """What the float4 kernels cannot serve is an error that carries the numbers, never another path."""
    with pytest.raises(SubgcError, match=r"A=22 R=48"):
        c = AR.sentence_case(22, 48, lens=[3, 5, 2], n_stride=8)
        run_fwd(c, _small()[1])
    with pytest.raises(SubgcError, match=r"A=516 R=48"):
        run_fwd(AR.sentence_case(516, 48, lens=[3, 5, 2], n_stride=8), _small()[1])
    with pytest.raises(SubgcError, match=r"A=24 R=2052"):
        c = AR.sentence_case(24, 2052, lens=[3, 5, 2], n_stride=8)
        run_bwd(c, _small()[1], pattern(c["rows"], 24), pattern(c["rows"], 2052))
    c, k = _small()
    S, A, R = c["S"], 24, 48
    buf = full((S, R + 8), 0.0)
    with pytest.raises(SubgcError, match=r"A=24 R=48"):      # a view that starts 4 bytes past a 16-byte boundary
        ops.attn_fwd(dv_(c["u"]), dv_(c["v"]), dv_(c["q"]), dv_(c["w_a"]).view(1, A), dv_(c["b_a"]), ints(c["off"]), ints(c["lens"]), buf[:, 1:1 + R],
                     full((S, 8), 0.0), S, A, R)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- shared-set family
def rows_by(ma, m, cols, b16=False):
    """[ma, cols]: rows < m NaN (every one of them is some live sentence's and must be written), the guard rows GUARD."""
    t = full((ma, cols) if cols else (ma,), GUARD, b16)
    t[:m] = NAN
    return t


def poison_sets(c, u, v):
    """NaN in the node rows at or beyond each image's longest live set (the kernels may not read them)."""
    for b in range(c["B"]):
        lo = b * c["Nn"] + AR.image_lmax(c, b)
        u[lo:(b + 1) * c["Nn"]] = NAN
        v[lo:(b + 1) * c["Nn"]] = NAN
    return u, v


def run_gfwd(c, k, u=None, v=None):
    A, R, m, ma = c["A"], c["R"], c["m"], c["ma"]
    if u is None:
        u, v = poison_sets(c, dv_(c["u"], k["uv16"]), dv_(c["v"], k["uv16"]))
    out = {"ctx": rows_by(ma, m, R, k["ctx16"]), "alpha": rows_by(ma, m, c["n_stride"])}
    w_a, b_a, rows, lens = dv_(c["w_a"]).view(1, A), dv_(c["b_a"]), ints(c["rows"]), ints(c["lens"] + [0, 0])
    if k["qn"]:
        out["q_out"] = rows_by(ma, m, A)
        q = (dv_(c["q_planes"]), k["qn"], ma * A, dv_(c["q_bias"]))
        ops.attn_fwd_group(u, v, out["q_out"], w_a, b_a, rows, lens, m, c["B"], c["g"], c["Nn"], out["ctx"], out["alpha"], A, R, q=q)
    else:
        ops.attn_fwd_group(u, v, dv_(c["q"]), w_a, b_a, rows, lens, m, c["B"], c["g"], c["Nn"], out["ctx"], out["alpha"], A, R)
    torch.cuda.synchronize()
    return out


def check_rows(family, c, ref, tol, out, names):
    m = c["m"]
    for name in names:
        check(family, ref, tol, out[name][:m], name)
        assert bool((out[name][m:] == GUARD).all()), f"{family} {name}: a row at or beyond m was written"


@pytest.mark.parametrize("k", G_FWD_CASES, ids=_id)
def test_group_forward_variants(k):
    c = AR.group_case(k["A"], k["R"], k["g"], k["Nn"], n_stride=k["n_stride"], q_planes=k["qn"], bf16_sets=k["uv16"])
    fn, args = AR.group_fwd_planes(c) if k["qn"] else (AR.attn_fwd_group, AR.group_fwd_args(c))
    ref, tol, _ = AR.tolerance(fn, args, bf16_out=("ctx",) if k["ctx16"] else ())
    out = run_gfwd(c, k)
    check_rows("group_fwd" + B16_DST * k["ctx16"], c, ref, tol, out, list(ref))
    for r, l in enumerate(c["lens"]):
        tail = out["alpha"][r, l:]
        assert tail.numel() == 0 or float(tail.abs().max()) == 0.0


def run_gbwd(c, k, bases, u=None, v=None):
    A, R, m, ma, BN = c["A"], c["R"], c["m"], c["ma"], c["B"] * c["Nn"]
    if u is None:
        u, v = poison_sets(c, dv_(c["u"], k["uv16"]), dv_(c["v"], k["uv16"]))
    out = {"dah": rows_by(ma, m, A, k["dah16"]), "dw_a": rows_by(ma, m, A), "db_a": rows_by(ma, m, 0), "du_planes": bases.to(DEV)}
    if k["keep"]:
        out["kbuf"], keep = pitched(ma, R)
        keep[m:] = GUARD
        out["dctx_keep"] = keep
    out["gbuf"], dctx = plane_window(c["dctx_planes"])
    alpha = torch.cat([c["alpha"], torch.full((2, c["n_stride"]), NAN)]).to(DEV)
    ops.attn_bwd_group(u, v, dv_(c["q"]), dv_(c["w_a"]).view(1, A), ints(c["rows"]), ints(c["lens"] + [0, 0]), m, c["B"], c["g"], c["Nn"], alpha, dctx,
                       out["dah"], out["du_planes"], out["dw_a"], out["db_a"], A, R, out.get("dctx_keep"))
    torch.cuda.synchronize()
    out["du"] = out["du_planes"].double().sum(0)            # the planes are added by the caller
    return out


def du_bases(c):
    """Start values of the d(u) planes: one pattern per plane (the second shifted) so that `+=` is visible in each."""
    planes, BN = ops.attn_group_du_planes(c["g"]), c["B"] * c["Nn"]
    assert planes == (2 if c["g"] >= 4 else 1)
    p = pattern(BN, c["A"])
    return torch.stack([p if i == 0 else -2 * p for i in range(planes)])


@pytest.mark.parametrize("k", G_BWD_CASES, ids=_id)
def test_group_backward_variants(k):
    c = AR.group_case(k["A"], k["R"], k["g"], k["Nn"], n_stride=k["n_stride"], dctx_planes=k["n"], bf16_sets=k["uv16"])
    bases = du_bases(c)
    ref, tol, _ = AR.tolerance(AR.attn_bwd_group, dict(AR.group_bwd_args(c), du0=bases.sum(0)), bf16_out=("dah",) if k["dah16"] else ())
    out = run_gbwd(c, k, bases)
    check_rows("group_bwd" + B16_DST * k["dah16"], c, ref, tol, out, ["dah", "dw_a", "db_a"] + (["dctx_keep"] if k["keep"] else []))
    check("group_bwd", ref, tol, out["du"], "du")
    if k["keep"]:
        assert guards_untouched(out["kbuf"], k["R"])
    assert guards_untouched(out["gbuf"].view(-1, out["gbuf"].shape[-1]), k["R"], pad=4)


@pytest.mark.parametrize("k", G_DV_CASES, ids=_id)
def test_group_dv_accum(k):
    """T = 20, g = 8, n_stride = 128: T g = 160 live-pair slots exceed one LDS pass; the image without a live sentence gets zero rows."""
    c = AR.group_accum_case(k["R"], 8, 37, 20, 128)
    kbuf, keep = pitched(c["tot"], k["R"])
    keep.copy_(c["dctx"].to(DEV))
    dv = full((c["B"] * c["Nn"], k["R"]), NAN)
    ops.attn_dv_accum_group(dv_(c["alpha"]), keep, ints(c["step_off"]), c["T"], ints(c["rows"]), c["B"], c["g"], c["Nn"], dv, k["R"])
    torch.cuda.synchronize()
    args = {key: c[key] for key in ("alpha", "dctx", "step_off", "rows", "B", "g", "Nn")}
    ref, tol, _ = AR.tolerance(AR.attn_dv_accum_group, args)
    check("group_dv_accum", ref, tol, dv, "dv")
    assert float(dv[2 * c["Nn"]:].abs().max()) == 0.0


@pytest.mark.parametrize("uv16", [False, True], ids=["f32", "bf16"])
def test_group_results_do_not_depend_on_rows_beyond_the_sentence(uv16):
    """Rows [len_j, lmax) of an image belong to its longer sentences: sentence j's outputs are bit for bit the same whatever (finite) values
    they hold.  (They must be finite: the forward weights them with an exact zero and does not skip them.)"""
    k = dict(uv16=uv16, ctx16=False, qn=0, dah16=False, n=1, keep=True)
    c = AR.group_case(256, 512, 5, 37, bf16_sets=uv16)
    j = 1                                                    # image 0, slot 1: a live sentence shorter than the image's longest (37 nodes)
    r = c["rows"][j]
    l = c["lens"][r]
    assert 0 < l < 37 and AR.image_lmax(c, 0) == 37
    u1, v1 = poison_sets(c, dv_(c["u"], uv16), dv_(c["v"], uv16))
    u2, v2 = u1.clone(), v1.clone()
    u2[l:37] = (u2[l:37].float() * -1.5 + 0.25).to(u2.dtype)
    v2[l:37] = (v2[l:37].float() * 2.0 - 1.0).to(v2.dtype)
    f1, f2 = run_gfwd(c, k, u1, v1), run_gfwd(c, k, u2, v2)
    assert torch.equal(f1["alpha"][r], f2["alpha"][r]) and torch.equal(f1["ctx"][r], f2["ctx"][r])
    assert not torch.equal(f1["ctx"][c["rows"][4]], f2["ctx"][c["rows"][4]])          # the 37-node sentence does see them
    b1, b2 = run_gbwd(c, k, du_bases(c), u1, v1), run_gbwd(c, k, du_bases(c), u2, v2)
    for name in ("dah", "dw_a", "db_a", "dctx_keep"):
        assert torch.equal(b1[name][r], b2[name][r]), name
