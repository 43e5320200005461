"""Companion of test_lstm_cell_gpu.py: the producers of split-K planes (ops.gemm_planes: subgc_gemm_f32_planes / subgc_gemm_bf16_planes), their
hand-over to ops.lstm_bwd_planes, and the four streaming kernels of the train step that no test called directly (ops.packed_time_sum,
ops.relu_bwd, ops.gather_rows_keep, ops.class_sum), each against lstm_reference.py in fp64 on the MI355X.

  entry point        shapes                                   variants
  gemm_planes        64^3; 256x1024x256; 256x256x1024 (fp32)  modes nt nn tn, fp32 and bf16 operands, observed n = 1 / 2 / 8 (64x64 split form),
                     256x256x3072 (bf16); 250x260x1000;       257x1152x3072: n = 8 from the 128x128 form, 1030x256x768: the eight-phase form;
                     257x1152x3072; 1030x256x768              buffers of M N, 3 M N and 8 M N + tail floats; a strided `a` (ld != K)
  hand-over          256x768x1024 -> cell 256x256, 300x256    the tuple (buf, N, col0, n, M N, M) of functions.py, n = 8 (fp32) and n = 2 (bf16)
  packed_time_sum    S 5 / 1 / 70, C 4 / 52                   fp32 and bf16 src; live counts with equal neighbours and a 0 tail
  relu_bwd           n 1 / 1000 / 8192 x 256 + 77             y, dz each fp32 / bf16; +0, -0, the smallest positive bf16; scale 1.7
  gather_rows_keep   11 x 52, 11 x 300 from 7 rows            src, dst each fp32 / bf16; -1 and repeated rows; keep absent / ldk != L; m_dev < M
  class_sum          M 1 63 64 130 8200, L 4 300              C 5 and 64 (slab partials, ids outside [0, C) dropped), C 65 (atomics)

Bounds: GEMM parts 2e-5 x max |reference| (the project's GEMM bound); the cell outputs of the hand-over get that added to the cell bound of
test_lstm_cell_gpu.py; sums 2^-23 x (number of addends) x max |addend|; a copy or one multiply into fp32 is bit-exact; a bf16 destination is
compared with the rounded reference, one bf16 ulp allowed."""
import gc

import pytest
import torch

import lstm_reference as LR
import test_lstm_cell_gpu as CELL
from subgc import ops
from test_lstm_cell_gpu import DEV, GUARD, UNWRITTEN, Dest, _cases, _id, check, dev, full, inside

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EPS23 = 2.0 ** -23


# ----------------------------------------------------------------------------- ops.gemm_planes
# n is what the dispatch must report for a buffer of 8 M N floats (kt = ceil(K / 32), read from pick_tile in csrc/gemm_f32.hip and from
# run<..>(partials_only) in csrc/gemm_bf16.hip):
#   fp32, M <= 256: 64x64 tiles, small = ceil(M / 64) ceil(N / 64); parts grow while small (s + 1) <= 768, kt / (s + 1) >= 4, s < 8; split only
#   if small s >= 128:   64^3: kt 2 -> 1;   256 x 1024 x 256: small 64, kt 8 -> 2 (128 workgroups);   256 x 256 x 1024: small 16, kt 32 -> 8 (128);
#   250 x 260 x 1000: small 4 x 5 = 20, kt 32 -> 8 (160), ragged tiles in M, N and K
#   fp32, M > 256: 128x128 tiles, big = 3 x 9 = 27 >= 16, kt 96: choose_splits -> 8 (ceil(96 / 8) = 12 K-tiles a part), 216 >= 200 workgroups
#   bf16: s in 2..8 with ceil(kt / s) >= 12 minimising ceil(tiles s / 512) (ceil(kt / s) + 8) + 0.8 s:   64^3: kt 2 -> 1;   256 x 256 x 1024:
#   kt 32 -> 2 (s = 3 leaves 11);   256 x 256 x 3072: kt 96 -> 8 (12 + 8 + 6.4 is the least);   1030 x 256 x 768: kt 24 -> 2, and from 1024 rows
#   on the eight-phase form with 12 sixty-four-deep K-tiles -> 2
PLANES_KEYS = ("M", "N", "K", "mode", "b16", "n", "strided")
GEMM_PLANES_CASES = _cases(PLANES_KEYS,
                           [(M, N, K, mode, False, n, False) for M, N, K, n in ((64, 64, 64, 1), (256, 1024, 256, 2), (256, 256, 1024, 8))
                            for mode in ("nt", "nn", "tn")]
                           + [(250, 260, 1000, "nt", False, 8, False), (257, 1152, 3072, "nt", False, 8, False), (256, 1024, 256, "nt", False, 2, True)]
                           + [(M, N, K, mode, True, n, False) for M, N, K, n in ((64, 64, 64, 1), (256, 256, 1024, 2), (256, 256, 3072, 8))
                              for mode in ("nt", "nn", "tn")]
                           + [(1030, 256, 768, "nt", True, 2, False), (256, 256, 1024, "nn", True, 2, True)])


_OPERANDS = {}


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """As in test_lstm_cell_gpu.py: no cached operands, no cached device blocks once the module is done."""
    yield
    _OPERANDS.clear()
    CELL._BUILT.clear()
    gc.collect()
    torch.cuda.empty_cache()


def gemm_operands(c):
    if _id(c) not in _OPERANDS:
        _OPERANDS[_id(c)] = _gemm_operands(c)
    return _OPERANDS[_id(c)]


def _gemm_operands(c):
    """CPU operands as stored (bf16 ones rounded), laid out for the mode: a [M, K] (tn: [K, M]), b [N, K] (nn, tn: [K, N]); the fp64 product."""
    M, N, K = c["M"], c["N"], c["K"]
    g = torch.Generator().manual_seed(M + 3 * N + 5 * K)
    a, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * K ** -0.5
    if c["b16"]:
        a, b = LR.bf16_round(a), LR.bf16_round(b)
    ref = a.double() @ b.double()
    return (a.t().contiguous() if c["mode"] == "tn" else a), (b.t().contiguous() if c["mode"] == "nt" else b), ref


def put(x, b16, strided=False):
    """Device copy of an operand; strided: the middle third of a three times wider buffer (the H2[t][:, R:2R] view of functions.py)."""
    x = x.to(BF16) if b16 else x
    if not strided:
        return x.to(DEV).contiguous()
    buf = full((x.shape[0], 3 * x.shape[1]), GUARD, b16)
    buf[:, x.shape[1]:2 * x.shape[1]] = x.to(DEV)
    return buf[:, x.shape[1]:2 * x.shape[1]]


def run_planes(c, floats, tail=0):
    a, b, ref = gemm_operands(c)
    buf = full((floats + tail,), GUARD)
    n, stride = ops.gemm_planes(put(a, c["b16"], c["strided"]), put(b, c["b16"]), buf[:floats], ta=c["mode"] == "tn", tb=c["mode"] == "nt")
    torch.cuda.synchronize()
    assert stride == c["M"] * c["N"] and 1 <= n <= floats // stride
    planes = buf[:n * stride].view(n, c["M"], c["N"]).double().cpu()
    return n, planes, buf, ref


def check_product(tag, planes, ref):
    tol = LR.GEMM_RTOL * float(ref.abs().max())
    err = float((planes.sum(0) - ref).abs().max())
    print(f"RATIO gemm_planes {tag} sum {err / tol:.3f}")
    assert err <= tol, f"gemm_planes {tag}: |sum of planes - fp64 product| = {err:.3g} > {tol:.3g}"
    return tol


@pytest.mark.parametrize("c", GEMM_PLANES_CASES, ids=_id)
def test_gemm_planes(c):
    M, N = c["M"], c["N"]
    n, planes, buf, ref = run_planes(c, 8 * M * N, tail=64)
    tol = check_product(_id(c), planes, ref)
    assert n == c["n"], f"the dispatch left {n} planes, the parameter list says {c['n']}"
    assert bool((buf[n * M * N:] == GUARD).all()), "a plane at index >= n or the guard tail was written"
    if n > 1:          # the planes are real partial sums: a consumer that drops the last one is far off
        moved = float(planes[-1].abs().max())
        assert moved > 100 * tol, f"the last plane holds at most {moved:.3g}: not a partial sum the tests could miss"


@pytest.mark.parametrize("c", [c for c in GEMM_PLANES_CASES if c["mode"] == "nt" and c["n"] > 1 and c["M"] <= 257], ids=_id)
def test_gemm_planes_buffer_bound(c):
    """The plane count is bounded by the caller's buffer: M N floats leave one plane, 3 M N at most three, and the product stays right."""
    M, N = c["M"], c["N"]
    n, planes, buf, ref = run_planes(c, M * N, tail=64)
    assert n == 1 and bool((buf[M * N:] == GUARD).all())
    check_product(_id(c) + "-MN", planes, ref)
    n, planes, buf, ref = run_planes(c, 3 * M * N, tail=64)
    assert n <= 3 and bool((buf[n * M * N:] == GUARD).all())
    check_product(_id(c) + "-3MN", planes, ref)


# ----------------------------------------------------------------------------- gemm_planes -> lstm_bwd_planes
# dy [M, 4R'] . W [4R', 3R] (mode nn: the d(h) product of the language cell, PA in functions.py) left as planes, a [*, R] window of which
# the next cell reads.  256 x 768 x 1024: fp32 small = 4 x 12 = 48, kt 32 -> 8 planes (384 workgroups); bf16 kt 32 -> 2 planes.
# In the second case the consuming step has more rows than the producing one (S = 300 > M): rows past M take nothing from the planes.
# d(pre) is fp32 in both.  A bf16 d(pre) cannot be held to the one-ulp rule here: with the GEMM part the fp32 value may sit 1e-4 from the
# reference, which carries about one element in a thousand across a bf16 rounding boundary, and a crossing costs a whole grid step -- up to
# 2^-7 |ref|, twice what 2^-8 |ref| + 1e-4 admits from |ref| ~ 0.03 on (measured with such a case: 1.26 x the tolerance at the worst of
# 307 200 elements).  The bf16 store itself is pinned where the fp32 bound is 1e-5: PLANES_CASES of test_lstm_cell_gpu.py.
HANDOVER_KEYS = ("M", "S", "R", "K", "b16", "col0", "n", "dpre16", "absent")
HANDOVER_CASES = _cases(HANDOVER_KEYS, [
    (256, 256, 256, 1024, False, 256, 8, False, ("dh_drop", "keep")),
    (256, 300, 256, 1024, True, 512, 2, False, ("dc",)),
])


@CELL.cached
def handover_case(c):
    """LR.case whose one source is the window [:, col0:col0 + R] of the fp64 K-part products of dy . W (their sum: the product)."""
    M, S, R, K, N = c["M"], c["S"], c["R"], c["K"], 3 * c["R"]
    k = LR.case(S, R, absent=c["absent"], seed=4)
    g = torch.Generator().manual_seed(5 + M + K)
    dy, w = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * K ** -0.5
    if c["b16"]:
        dy, w = LR.bf16_round(dy), LR.bf16_round(w)
    parts = torch.stack([dy[:, a:b].double() @ w[a:b].double() for a, b in CELL.k_parts(K, c["n"])])
    k["dy"], k["w"] = dy, w
    k["stacks"] = [{"stack": parts, "n": parts.shape[0], "rows": M, "N": N, "col0": c["col0"]}]
    return k


@pytest.mark.parametrize("c", HANDOVER_CASES, ids=_id)
def test_planes_hand_over(c):
    M, S, R, N = c["M"], c["S"], c["R"], 3 * c["R"]
    k = handover_case(c)
    buf = full((8 * M * N,), GUARD)
    n, stride = ops.gemm_planes(put(k["dy"], c["b16"]), put(k["w"], c["b16"]), buf)
    assert n == c["n"] and stride == M * N
    gates, cp, cc, dhd, keep, dc = CELL.bwd_inputs(k)
    d = Dest()
    dpre, dcp = d.flat(S, 4 * R, c["dpre16"]), d.flat(S, R)
    d.snapshot()
    ops.lstm_bwd_planes(gates, cp, cc, [(buf, N, c["col0"], n, stride, M)], dhd, keep, k["scale"], dc, dpre, dcp, S, R)
    torch.cuda.synchronize()
    d.untouched()
    ref, err = LR.fp32_error(LR.cell_bwd, LR.bwd_args(k))
    extra = LR.GEMM_RTOL * float(LR.sum_planes(k["stacks"][0]["stack"]).abs().max())
    check("hand-over", _id(c), "dpre", dpre, ref["dpre"], LR.bound(err["dpre"], LR.BWD_ATOL, extra), c["dpre16"])
    check("hand-over", _id(c), "dc_prev", dcp, ref["dc_prev"], LR.bound(err["dc_prev"], LR.BWD_ATOL, extra))


# ----------------------------------------------------------------------------- ops.packed_time_sum
@pytest.mark.parametrize("b16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("S,C,live", [(5, 4, (5, 5, 3, 1, 0, 0)), (1, 52, (1, 1, 1)), (70, 52, (70, 70, 33, 33, 9, 1, 0)), (9, 4, (9,))],
                         ids=["S5-C4", "S1-C52", "S70-C52", "S9-C4-T1"])
def test_packed_time_sum(S, C, live, b16):
    off = [0]
    for m in live:
        off.append(off[-1] + m)
    g = torch.Generator().manual_seed(S + C)
    src = torch.randn(off[-1] + 2, C, generator=g)                       # two rows behind the last step: never read
    if b16:
        src = LR.bf16_round(src)
    ref = LR.packed_time_sum(src.double(), off, S)
    d = Dest()
    dst = d.flat(S, C)
    d.snapshot()
    ops.packed_time_sum(put(src, b16), torch.tensor(off, dtype=torch.int32, device=DEV), len(live), S, dst)
    torch.cuda.synchronize()
    d.untouched()
    check("packed_time_sum", f"S{S}-C{C}-b16{int(b16)}", "dst", dst, ref, EPS23 * len(live) * float(src.abs().max()))


# ----------------------------------------------------------------------------- ops.relu_bwd
@pytest.mark.parametrize("y16", [False, True], ids=["y32", "y16"])
@pytest.mark.parametrize("dz16", [False, True], ids=["dz32", "dz16"])
@pytest.mark.parametrize("n", [1, 1000, 8192 * 256 + 77])               # the last: more elements than the grid has threads
def test_relu_bwd(n, dz16, y16):
    scale = 1.7
    g = torch.Generator().manual_seed(n)
    y = LR.bf16_round(torch.randn(n, generator=g))
    tiny = 2.0 ** -133                                                   # the smallest positive bf16 (a subnormal), exact in fp32
    edge = torch.tensor([0.0, -0.0, tiny, -tiny, 1.0, -1.0])
    if n >= 8:
        y[1:7] = edge
        y[-6:] = edge
    else:
        y[0] = tiny
    dy = torch.randn(n, generator=g)
    want = LR.relu_bwd(dy, y, torch.tensor(scale))                       # one fp32 multiply: exact in torch's fp32 too
    d = Dest()
    dz = d.flat(1, n, dz16)
    d.snapshot()
    ops.relu_bwd(dev(dy), put(y, y16), scale, out=dz.view(n))
    torch.cuda.synchronize()
    d.untouched()
    if dz16:
        check("relu_bwd", f"n{n}-y16{int(y16)}", "dz", dz.view(n), want.double(), 0.0, True)
    else:
        assert torch.equal(dz.view(n).cpu().view(torch.int32), want.view(torch.int32)), "relu_bwd into fp32 is one multiply: bit-exact"


# ----------------------------------------------------------------------------- ops.gather_rows_keep
@pytest.mark.parametrize("src16", [False, True], ids=["s32", "s16"])
@pytest.mark.parametrize("dst16", [False, True], ids=["d32", "d16"])
@pytest.mark.parametrize("L,keep,scale,m_dev", [(52, False, 1.0, None), (52, True, 4.0, 8), (300, True, 1.0, None), (300, False, 2.5, 11)],
                         ids=["L52", "L52-keep-m8", "L300-keep", "L300-scale"])
def test_gather_rows_keep(L, keep, scale, m_dev, dst16, src16):
    M, rows_src = 11, 7
    g = torch.Generator().manual_seed(L + M)
    src = torch.randn(rows_src, L, generator=g)
    if src16:
        src = LR.bf16_round(src)
    rows = torch.tensor([3, -1, 3, 0, 6, 6, -1, 2, 5, 1, 3], dtype=torch.int32)
    kp = (torch.rand(M, L, generator=g) < 0.5).to(torch.uint8) if keep else None
    ref = LR.gather_rows_keep(src.double(), rows, kp, scale)
    s_dev = inside(src.to(BF16) if src16 else src, col=8, extra=16)      # strided source
    k_dev = None
    if keep:
        k_dev = torch.zeros(M, L + 12, dtype=torch.uint8, device=DEV)    # ldk != L
        k_dev[:, :L] = kp.to(DEV)
        k_dev = k_dev[:, :L]
    live = M if m_dev is None else m_dev
    d = Dest()
    dst = d.window(M, L, dst16, rows=live)                               # strided destination; rows >= m_dev stay as they are
    d.snapshot()
    ops.gather_rows_keep(s_dev, rows.to(DEV), k_dev, scale, dst, m_dev=None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    d.untouched()
    tag = f"L{L}-s16{int(src16)}-d16{int(dst16)}"
    if not dst16 and scale == 1.0:
        assert torch.equal(dst[:live].cpu().view(torch.int32), ref[:live].float().view(torch.int32)), "a copy (times 0 or 1) is bit-exact"
    else:
        check("gather_rows_keep", tag, "dst", dst, ref, 2.0 ** -24 * float(ref.abs().max()), dst16, live)


# ----------------------------------------------------------------------------- ops.class_sum
@pytest.mark.parametrize("L", [4, 300])
@pytest.mark.parametrize("M", [1, 63, 64, 130, 8200])                    # slabs = max(1, min(128, M // 64)) = 1, 1, 1, 2, 128 (65 rows each: a ragged last)
@pytest.mark.parametrize("C", [5, 64, 65])                               # <= 64: per-slab partials + a column sum; 65: atomics
def test_class_sum(C, M, L):
    g = torch.Generator().manual_seed(C + M + L)
    x = torch.randn(M, L, generator=g)
    cls = torch.randint(0, C, (M,), generator=g).to(torch.int32)
    if C <= 64 and M >= 63:                                              # ids outside [0, C): dropped by the slab form
        cls[5], cls[17], cls[M - 1], cls[M // 2] = -1, C, C + 3, -7
    ref = LR.class_sum(x.double(), cls, C)
    x_dev = inside(x, col=4, extra=8) if (M + L) % 2 == 0 else dev(x)    # a strided x in half of the cases
    got = ops.class_sum(x_dev, cls.to(DEV), C)
    torch.cuda.synchronize()
    assert got.shape == (C, L)
    ok = (cls >= 0) & (cls < C)
    addends = int(torch.bincount(cls[ok].long(), minlength=C).max()) if bool(ok.any()) else 1
    check("class_sum", f"C{C}-M{M}-L{L}", "sum", got, ref, EPS23 * max(addends, 1) * float(x.abs().max()))
    if C <= 64:
        again = ops.class_sum(x_dev, cls.to(DEV), C)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "the slab form adds in a fixed order: two calls, the same bits"
