"""The LSTM cell kernels (csrc/decoder.hip: lstm_fwd_kernel<VW, PARTS>, lstm_bwd_kernel<VW>) through every entry point that launches them
-- ops.lstm_fwd, ops.lstm_bwd, ops.lstm_bwd_planes, ops.lstm_fwd_gemm -- against the fp64 restatement in lstm_reference.py, on the MI355X.
The case lists are plain data: test_lstm_reference_cpu.py builds every case with the same calls and shows that its inputs can see each
mutation of the reference (a dropped plane, a source added past rows_i, a window one gate off, ...).

Variant table (one list per entry point; `form` is what the wrapper's alignment test must pick, asserted from the pointers):

  entry point       S, R                         form            storage              absent                    row limits          planes
  lstm_fwd          70x48 9x52 1x48 20x52        vec (float4)    h fp32 and bf16      each of g1 g2 b0 b1       rows_h 50 / 4 / 69  -
                    70x46 9x46 1x46, 70x52+1     scalar          one buffer / apart   c_prev keep hdrop gates   rows_h2 33 / 1
                                                                                       h2 in at least one case
  lstm_bwd          70x48 9x52 1x48 20x52        vec             dpre fp32 and bf16   dh_a dh_b dh_drop keep    -                   -
                    70x46 9x46, 20x52+1          scalar                               dc c_prev
  lstm_bwd_planes   70x48 9x52 1x48              vec             dpre fp32 and bf16   dh_drop keep dc c_prev    rows_i 50 33 5 0    1 2 3 8, n = 0
                    70x46, 70x48 at col0 R+1     scalar                                                                             between two live
  lstm_fwd_gemm     641x640 ... 257x288          vec, PARTS      x/w fp32 and bf16,   g1 g2 c_prev keep         rows_h < S          2 3 4 5 8, none
                    70x48 1030x64 100x48         2 3 4 5 8, 1    h fp32 and bf16

Every destination lives in a wider buffer: GUARD around it (columns beside a window, two rows past S), UNWRITTEN inside it; after the call
everything but the elements the contract names must be bit-unchanged -- guard columns, guard rows, and the rows of h / h2 past rows_h / rows_h2.

Bounds.  fp32 outputs: |device - fp64| <= max(project constant, 8 x e32), e32 = max |lstm_reference in fp32 on the CPU - fp64| on the same
case; the constants are the existing cell test's (1e-6 forward, 1e-5 backward).  bf16 outputs: |device - bf16_round(fp64)| <= 2^-8 |fp64| + that
bound.  lstm_fwd_gemm adds 2e-5 x max |x W^T| (the project's GEMM bound; every gate function has slope <= 1).  Measured e32, the largest
over the cases of a family (CPU; `python tests/test_lstm_reference_cpu.py` prints the row of every case), and the largest bound that results:

  family            output: e32 -> bound
  lstm_fwd          c 3.6e-07 -> 2.9e-06   h, h2 1.3e-07 -> 1.0e-06   hdrop (scale 4) 4.2e-07 -> 3.4e-06   gates 1.4e-07 -> 1.1e-06
  lstm_fwd_gemm     c 4.9e-07   h, h2 1.9e-07   hdrop 6.7e-07   gates 4.1e-07; all -> 1.1e-04 to 1.2e-04 (the GEMM part, max |x W^T| ~ 5.5, decides)
  lstm_bwd          dpre 5.1e-07 -> 1.0e-05   dc_prev 7.1e-07 -> 1.0e-05
  lstm_bwd_planes   dpre 8.2e-07 -> 1.0e-05   dc_prev 9.2e-07 -> 1.0e-05   (up to 3 + 8 + 2 planes: 8 e32 stays below the constant)
  hand-over         dpre 8.9e-07   dc_prev 6.3e-07; both -> 1.0e-04 (GEMM part)     (test_lstm_planes_gpu.py)

So the project's constants decide everywhere but for c and hdrop (= 4 h) of the forward, where 8 e32 reaches 2.9e-6 and 3.4e-6.

Every check prints `RATIO <family> <case> <output> <error / tolerance>` (pytest -s)."""
import gc

import pytest
import torch

import lstm_reference as LR
from subgc import ops
from subgc._lib import SubgcError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 777.0           # around every destination
UNWRITTEN = 555.0       # inside every destination before the call (both exact in bf16)
PAD = 8                 # guard columns beside a window: 32 bytes fp32, 16 bytes bf16 -- windows keep 16-byte alignment
INPUTS = ("g1", "g2", "b0", "b1", "c_prev", "keep", "dh_drop", "dc")


def _cases(keys, rows):
    return [dict(zip(keys, r)) for r in rows]


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """The case cache and the device blocks torch keeps for reuse go when the module is done: the tests that follow in the same process
    find it as they would without this file."""
    yield
    _BUILT.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _id(c):
    def one(v):
        if isinstance(v, bool):
            return str(int(v))
        if isinstance(v, (tuple, list)):
            return "+".join(one(x) for x in v) or "none"
        return str(v)
    return "-".join(f"{k}{one(v)}" for k, v in c.items())


# ----------------------------------------------------------------------------- case lists (read by the CPU mutation test)
# layout: "one" = h, h2, hdrop are column windows of ONE buffer; "apart" = three allocations; "g1off" / "aoff" = the g1 / dh_a view starts one
# float past a 16-byte boundary, which must send a float4-capable shape to the scalar kernel.  S R / 4 = 840, 117, 12, 260 threads: the last
# workgroup is partial in every case and 20 x 52 straddles 256.
FWD_KEYS = ("S", "R", "form", "h16", "absent", "rows_h", "rows_h2", "layout")
FWD_CASES = _cases(FWD_KEYS, [
    (70, 48, "vec", False, (), 0, 0, "one"),
    (70, 48, "vec", True, (), 50, 33, "one"),
    (70, 48, "vec", False, ("hdrop",), 69, 70, "apart"),
    (9, 52, "vec", False, ("g1", "b0", "keep"), 0, 4, "apart"),
    (1, 48, "vec", True, ("g2", "b1", "c_prev"), 0, 0, "apart"),
    (20, 52, "vec", True, ("gates", "h2"), 4, 0, "one"),
    (70, 46, "scalar", False, (), 69, 1, "one"),
    (9, 46, "scalar", True, ("hdrop", "gates", "h2"), 5, 0, "apart"),
    (1, 46, "scalar", False, ("g1", "g2", "b0", "b1", "c_prev", "keep"), 0, 0, "apart"),
    (70, 52, "scalar", False, ("c_prev",), 33, 50, "g1off"),
    (70, 52, "scalar", True, ("g2",), 0, 33, "g1off"),
])

# sources of ops.lstm_bwd: dh_a a [S, R] window at column 4 of an [S, R + 8] buffer (column 5: "aoff"), dh_b a plain [S, R] tensor
BWD_KEYS = ("S", "R", "form", "dpre16", "absent", "layout")
BWD_CASES = _cases(BWD_KEYS, [
    (70, 48, "vec", False, (), "plain"),
    (70, 48, "vec", True, ("dh_b", "keep", "dc"), "plain"),
    (9, 52, "vec", False, ("dh_a", "dh_drop", "keep", "c_prev"), "plain"),
    (1, 48, "vec", True, ("dh_b", "c_prev"), "plain"),
    (20, 52, "vec", False, ("dh_a", "dh_b", "dc"), "plain"),
    (70, 46, "scalar", False, (), "plain"),
    (9, 46, "scalar", True, ("dh_b", "keep", "dc", "c_prev"), "plain"),
    (20, 52, "scalar", False, ("dh_b",), "aoff"),
    (20, 52, "scalar", True, ("dc",), "aoff"),
])

# sources of ops.lstm_bwd_planes: (n, rows_i, N, col0) -- the window [:n, :rows_i, col0:col0 + R] of a stack [n, S, N] (plane stride S N).
# [n, rows, 3R] with col0 in {0, R, 2R} is the layout of PA in functions.py, [n, rows, 2R] that of PC, [n, rows, R] that of PB.
PLANES_KEYS = ("S", "R", "form", "dpre16", "absent", "sources")
PLANES_CASES = _cases(PLANES_KEYS, [
    (70, 48, "vec", False, (), ((2, 70, 144, 0),)),
    (70, 48, "vec", False, ("dh_drop", "keep"), ((3, 70, 144, 48), (8, 50, 48, 0))),
    (70, 48, "vec", True, ("dc",), ((1, 70, 144, 96), (0, 70, 48, 0), (3, 33, 96, 48))),
    (9, 52, "vec", True, ("c_prev", "keep"), ((8, 9, 156, 52), (2, 0, 104, 0), (3, 5, 52, 0))),
    (1, 48, "vec", False, ("dh_drop", "keep", "dc"), ((8, 1, 144, 0), (3, 1, 144, 48), (2, 1, 144, 96))),
    (70, 46, "scalar", False, (), ((3, 70, 138, 46), (2, 40, 138, 92), (1, 70, 138, 0))),
    (70, 46, "scalar", True, ("dc", "c_prev"), ((8, 33, 92, 46), (2, 70, 46, 0))),
    (70, 48, "scalar", False, ("keep",), ((2, 70, 148, 49), (3, 50, 48, 0))),          # col0 = R + 1: the window is 4 bytes past alignment
    (70, 48, "scalar", True, ("dh_drop", "keep"), ((8, 70, 148, 97), (1, 0, 48, 0), (2, 70, 96, 48))),
])

# ops.lstm_fwd_gemm: x [S, K] (a window of an [S, K + 8] buffer), w [4R, K].  `parts` is what the dispatch must choose; it cannot be
# observed from Python, so a wrong derivation only loses coverage.  kt = ceil(K / 32) K-tiles, big = ceil(S / 128) ceil(4R / 128) tiles.
#   fp32 operands (gemm_nt_partials, csrc/gemm_f32.hip): splits only for S > 256, 16 <= big < 384, big parts >= 200; choose_splits takes the
#   part count s <= 8 with ceil(kt / s) >= 12 that minimises rounds (ceil(kt / s) + 3) + 0.6 (s + 1), rounds = ceil(big s / 512) = 1 in all of
#   these, so the largest admissible s wins:
#     641 x 640, K 1024: big 6 x 20 = 120, kt 32 -> s = 2 (s = 3 leaves 11 K-tiles a part); 240 workgroups
#     513 x 544, K 1152: big 5 x 17 = 85, kt 36 -> s = 3 (s = 4 leaves 9); 255
#     385 x 544, K 1536: big 4 x 17 = 68, kt 48 -> s = 4 (s = 5 leaves 10); 272
#     385 x 448, K 1920: big 4 x 14 = 56, kt 60 -> s = 5 (s = 6 leaves 10); 280
#     257 x 288, K 3072: big 3 x 9 = 27, kt 96 -> s = 8; 216
#     300 x 512, K 1024: big 3 x 16 = 48, kt 32 -> s = 2, but 96 workgroups < 200: no split (gemm, then the plain cell kernel)
#     100 x 48, K 96: S <= 256: no split (the case test_decode_fastpaths_gpu.py lists)
#   bf16 operands (run<..>(partials_only), csrc/gemm_bf16.hip): s in 2..8 with ceil(kt / s) >= 12 minimising
#   ceil(tiles s / 512) (ceil(kt / s) + 8) + 0.8 s, any S; from 1024 rows on the eight-phase form, s in 2..8 with ceil(ceil(K / 64) / s) >= 6:
#     70 x 48, K 768: kt 24 -> s = 2 only;   70 x 48, K 1152: kt 36 -> s = 3 (15 + 8 + 2.4 < 18 + 8 + 1.6);   300 x 64, K 3072: kt 96 -> s = 8
#     1030 x 64, K 768: 128 x 128 form s = 2, then 12 sixty-four-deep K-tiles -> eight-phase s = 2;   100 x 48, K 96: kt 3: no split
GEMM_KEYS = ("S", "R", "K", "x16", "h16", "parts", "absent", "rows_h", "rows_h2")
GEMM_CASES = _cases(GEMM_KEYS, [
    (641, 640, 1024, False, False, 2, ("g2",), 600, 0),
    (513, 544, 1152, False, False, 3, (), 0, 500),
    (385, 544, 1536, False, False, 4, ("g1", "g2", "keep"), 300, 300),
    (385, 448, 1920, False, False, 5, ("c_prev",), 0, 0),
    (257, 288, 3072, False, False, 8, ("g1", "g2"), 256, 129),
    (300, 512, 1024, False, False, 1, ("g2",), 299, 0),
    (100, 48, 96, False, False, 1, (), 70, 0),
    (70, 48, 768, True, False, 2, (), 50, 0),
    (70, 48, 1152, True, True, 3, ("g1", "g2", "c_prev"), 0, 33),
    (300, 64, 3072, True, True, 8, ("keep",), 257, 0),
    (1030, 64, 768, True, False, 2, ("g2",), 1000, 1029),
    (100, 48, 96, True, True, 1, (), 70, 0),
])


_BUILT = {}


def cached(fn):
    """One build per case and process: the references are computed once and shared (nothing writes into them)."""
    def wrap(c):
        key = (fn.__name__, _id(c))
        if key not in _BUILT:
            _BUILT[key] = fn(c)
        return _BUILT[key]
    wrap.__name__, wrap.__doc__ = fn.__name__, fn.__doc__
    return wrap


@cached
def fwd_case(c):
    return LR.case(c["S"], c["R"], absent=[a for a in c["absent"] if a in INPUTS], rows_h=c["rows_h"], rows_h2=c["rows_h2"])


@cached
def bwd_case(c):
    S, R = c["S"], c["R"]
    src = []
    if "dh_a" not in c["absent"]:
        src.append((1, S, R + 8, 5 if c["layout"] == "aoff" else 4))
    if "dh_b" not in c["absent"]:
        src.append((1, S, R, 0))
    return LR.case(S, R, absent=[a for a in c["absent"] if a in INPUTS], sources=src, seed=1)


@cached
def planes_case(c):
    return LR.case(c["S"], c["R"], absent=[a for a in c["absent"] if a in INPUTS], sources=c["sources"], seed=2)


def k_parts(K, parts):
    """The K ranges of the split-K workgroups: `parts` runs of ceil(kt / parts) 32-deep K-tiles."""
    kt = (K + 31) // 32
    per = (kt + parts - 1) // parts
    return [(p * per * 32, min(K, (p + 1) * per * 32)) for p in range(parts) if p * per * 32 < K]


@cached
def gemm_case(c):
    """LR.case with the pre-activation planes replaced by the fp64 partial products of x W^T over the K ranges the split form uses (their
    fp64 sum is the product); x, w are the stored operand values (bf16 ones widened)."""
    S, R, K = c["S"], c["R"], c["K"]
    k = LR.case(S, R, absent=[a for a in c["absent"] if a in INPUTS], rows_h=c["rows_h"], rows_h2=c["rows_h2"], seed=3)
    g = torch.Generator().manual_seed(77 + S + K)
    x, w = torch.randn(S, K, generator=g), torch.randn(4 * R, K, generator=g) * K ** -0.5
    if c["x16"]:
        x, w = LR.bf16_round(x), LR.bf16_round(w)
    k["x"], k["w"] = x, w
    k["pre_planes"] = torch.stack([x[:, a:b].double() @ w[:, a:b].double().t() for a, b in k_parts(K, c["parts"])])
    return k


# ----------------------------------------------------------------------------- helpers
def full(shape, val, b16=False):
    return torch.full(shape, val, device=DEV, dtype=torch.bfloat16 if b16 else torch.float32)


def dev(x, b16=False):
    if x is None:
        return None
    t = x.to(DEV).contiguous()
    return t.to(torch.bfloat16) if b16 else t


def inside(x, col=4, extra=8):
    """The device copy of an input [S, C] as a window at column `col` of an [S, C + extra] buffer (ld != C; col = 4: 16-byte aligned)."""
    if x is None:
        return None
    buf = full((x.shape[0], x.shape[1] + extra), GUARD, x.dtype == torch.bfloat16)
    buf[:, col:col + x.shape[1]] = x.to(DEV)
    return buf[:, col:col + x.shape[1]]


class Dest:
    """Destinations inside guarded buffers.  window() hands out an [S, cols] view filled with UNWRITTEN and records which elements the call
    may write; untouched() then asserts that every other element of every buffer is bit-unchanged."""

    def __init__(self):
        self.bufs = []

    def buffer(self, rows, cols, b16=False):
        buf = full((rows, cols), GUARD, b16)
        self.bufs.append([buf, torch.zeros(rows, cols, dtype=torch.bool, device=DEV), None])
        return len(self.bufs) - 1

    def window(self, S, cols, b16=False, rows=None, buf=None, col=PAD):
        if buf is None:
            buf = self.buffer(S + 2, cols + 2 * PAD, b16)
        b, m, _ = self.bufs[buf]
        v = b[:S, col:col + cols]
        v.fill_(UNWRITTEN)
        m[:S if rows is None else rows, col:col + cols] = True
        return v

    def flat(self, S, cols, b16=False):
        """A contiguous [S, cols] destination (no leading dimension in the call): two guard rows behind it."""
        buf = self.buffer(S + 2, cols, b16)
        return self.window(S, cols, b16, buf=buf, col=0)

    def snapshot(self):
        for e in self.bufs:
            e[2] = e[0].clone()

    def untouched(self):
        for b, m, snap in self.bufs:
            assert torch.equal(b[~m], snap[~m]), "a guard column, a guard row or a row past the row limit was written"


def expect_vec(R, tensors, keep):
    """The wrappers' test for the float4 form: R % 4, every leading dimension % 4, every pointer 16-byte aligned, keep 4-byte aligned."""
    ok = R % 4 == 0 and (keep is None or keep.data_ptr() % 4 == 0)
    for t in tensors:
        if t is not None:
            ok = ok and t.data_ptr() % 16 == 0 and (t.dim() < 2 or t.stride(0) % 4 == 0)
    return ok


def check(family, tag, name, got, ref, b, b16=False, rows=None):
    """|got - ref| <= b element by element on rows < rows (a bf16 destination: against the rounded reference, one more ulp allowed)."""
    g, r = got.double().cpu(), ref
    if rows is not None:
        g, r = g[:rows], r[:rows]
    assert g.shape == r.shape, (name, g.shape, r.shape)
    assert not bool(torch.isnan(g).any()) and not bool(torch.isnan(r).any()), f"{family} {tag} {name}: NaN"
    want = LR.bf16_round(r) if b16 else r
    err, tol = (g - want).abs(), LR.tol_of(r, b, b16)
    ratio = float((err / tol.clamp_min(1e-300)).max()) if r.numel() else 0.0
    print(f"RATIO {family}{'(bf16)' if b16 else ''} {tag} {name} {ratio:.3f}  (bound {b:.3g})")
    assert bool((err <= tol).all()), f"{family} {tag} {name}: error / tolerance = {ratio:.3f} (bound {b:.3g})"


def h_dests(d, c, S, R):
    """h, h2, hdrop destinations of a forward case (None where absent) in the case's layout."""
    b16, r1, r2 = c["h16"], LR.row_limit(c["rows_h"], S), LR.row_limit(c["rows_h2"], S)
    one = d.buffer(S + 2, 3 * R + 4 * PAD, b16) if c["layout"] == "one" else None
    col = (lambda j: PAD + j * (R + PAD)) if one is not None else (lambda j: PAD)
    h = d.window(S, R, b16, r1, one, col(0))
    h2 = None if "h2" in c["absent"] else d.window(S, R, b16, r2, one, col(1))
    hd = None if "hdrop" in c["absent"] else d.window(S, R, b16, None, one, col(2))
    return h, h2, hd, r1, r2


def check_fwd(family, tag, c, ref, err, extra, outs, r1, r2):
    cc, h, h2, hd, gates = outs
    b = {k: LR.bound(err[k], LR.FWD_ATOL, extra) for k in ref}
    check(family, tag, "c", cc, ref["c"], b["c"])
    check(family, tag, "h", h, ref["h"], b["h"], c["h16"], r1)
    if h2 is not None:
        check(family, tag, "h2", h2, ref["h2"], b["h2"], c["h16"], r2)
    if hd is not None:
        check(family, tag, "hdrop", hd, ref["hdrop"], b["hdrop"], c["h16"])
    if gates is not None:
        check(family, tag, "gates", gates, ref["gates"], b["gates"])


# ----------------------------------------------------------------------------- ops.lstm_fwd
@pytest.mark.parametrize("c", FWD_CASES, ids=_id)
def test_lstm_fwd(c):
    S, R = c["S"], c["R"]
    k = fwd_case(c)
    ref, err = LR.fp32_error(LR.cell_fwd, LR.fwd_args(k))
    g0 = inside(k["pre_planes"][0])
    g1 = inside(k["g1"], col=5) if c["layout"] == "g1off" else inside(k["g1"])
    g2, b0, b1, cp, keep = inside(k["g2"]), dev(k["b0"]), dev(k["b1"]), dev(k["c_prev"]), dev(k["keep"])
    d = Dest()
    cc = d.flat(S, R)
    h, h2, hd, r1, r2 = h_dests(d, c, S, R)
    gates = None if "gates" in c["absent"] else d.flat(S, 4 * R)
    assert expect_vec(R, [g0, g1, g2, b0, b1, cp, cc, h, h2, hd, gates], keep) == (c["form"] == "vec")
    d.snapshot()
    ops.lstm_fwd(g0, g1, g2, b0, b1, cp, cc, h, h2, keep, k["scale"], hd, gates, S, R, c["rows_h"], c["rows_h2"])
    torch.cuda.synchronize()
    d.untouched()
    check_fwd("lstm_fwd", _id(c), c, ref, err, 0.0, (cc, h, h2, hd, gates), r1, r2)


def test_lstm_fwd_rejects_mixed_h_storage():
    """h, h2 and hdrop share one bf16 flag in the C call: the wrapper refuses fp32 next to bf16 instead of picking one."""
    S, R = 4, 8
    z = lambda b16=False: full((S, R), 0.0, b16)
    with pytest.raises(SubgcError):
        ops.lstm_fwd(full((S, 4 * R), 0.0), None, None, None, None, None, z(), z(), z(True), None, 1.0, None, None, S, R)
    with pytest.raises(SubgcError):
        ops.lstm_fwd(full((S, 4 * R), 0.0), None, None, None, None, None, z(), z(True), None, None, 1.0, z(), None, S, R)


# ----------------------------------------------------------------------------- ops.lstm_bwd / ops.lstm_bwd_planes
def bwd_inputs(k):
    return dev(k["gates"]), dev(k["c_prev"]), dev(k["c"]), inside(k["dh_drop"]), dev(k["keep"]), dev(k["dc"])


def check_bwd(family, tag, k, dpre16, dpre, dcp):
    ref, err = LR.fp32_error(LR.cell_bwd, LR.bwd_args(k))
    check(family, tag, "dpre", dpre, ref["dpre"], LR.bound(err["dpre"], LR.BWD_ATOL), dpre16)
    check(family, tag, "dc_prev", dcp, ref["dc_prev"], LR.bound(err["dc_prev"], LR.BWD_ATOL))


@pytest.mark.parametrize("c", BWD_CASES, ids=_id)
def test_lstm_bwd(c):
    S, R = c["S"], c["R"]
    k = bwd_case(c)
    gates, cp, cc, dhd, keep, dc = bwd_inputs(k)
    views = [dev(s["stack"])[0][:, s["col0"]:s["col0"] + R] for s in k["stacks"]]
    dh_a = None if "dh_a" in c["absent"] else views.pop(0)
    dh_b = None if "dh_b" in c["absent"] else views.pop(0)
    d = Dest()
    dpre, dcp = d.flat(S, 4 * R, c["dpre16"]), d.flat(S, R)
    assert expect_vec(R, [gates, cp, cc, dh_a, dh_b, dhd, dc, dpre, dcp], keep) == (c["form"] == "vec")
    d.snapshot()
    ops.lstm_bwd(gates, cp, cc, dh_a, dh_b, dhd, keep, k["scale"], dc, dpre, dcp, S, R)
    torch.cuda.synchronize()
    d.untouched()
    check_bwd("lstm_bwd", _id(c), k, c["dpre16"], dpre, dcp)


@pytest.mark.parametrize("c", PLANES_CASES, ids=_id)
def test_lstm_bwd_planes(c):
    S, R = c["S"], c["R"]
    k = planes_case(c)
    gates, cp, cc, dhd, keep, dc = bwd_inputs(k)
    stacks = [dev(s["stack"]) for s in k["stacks"]]
    srcs = [(t, s["N"], s["col0"], s["n"], S * s["N"], s["rows"]) for t, s in zip(stacks, k["stacks"])]
    live = [t[0][:, s["col0"]:s["col0"] + R] for t, s in zip(stacks, k["stacks"]) if s["n"] > 0]
    d = Dest()
    dpre, dcp = d.flat(S, 4 * R, c["dpre16"]), d.flat(S, R)
    assert expect_vec(R, [gates, cp, cc, dhd, dc, dpre, dcp] + live, keep) == (c["form"] == "vec")
    d.snapshot()
    ops.lstm_bwd_planes(gates, cp, cc, srcs, dhd, keep, k["scale"], dc, dpre, dcp, S, R)
    torch.cuda.synchronize()
    d.untouched()
    check_bwd("lstm_bwd_planes", _id(c), k, c["dpre16"], dpre, dcp)
    # the kernel adds the planes one after the other into a zero start, source by source: the same fp32 adds done by torch on the device and
    # handed to lstm_bwd as its one d(h) term must give the same bits (rows past rows_i take no add at all)
    acc = torch.zeros(S, R, device=DEV)
    for t, s in zip(stacks, k["stacks"]):
        for q in range(s["n"]):
            acc[:s["rows"]] += t[q, :s["rows"], s["col0"]:s["col0"] + R]
    dpre2, dcp2 = torch.empty_like(dpre), torch.empty_like(dcp)
    ops.lstm_bwd(gates, cp, cc, acc, None, dhd, keep, k["scale"], dc, dpre2, dcp2, S, R)
    torch.cuda.synchronize()
    assert torch.equal(dpre.view(torch.int16 if c["dpre16"] else torch.int32), dpre2.view(torch.int16 if c["dpre16"] else torch.int32))
    assert torch.equal(dcp.view(torch.int32), dcp2.view(torch.int32))


# ----------------------------------------------------------------------------- ops.lstm_fwd_gemm against fp64
@pytest.mark.parametrize("c", GEMM_CASES, ids=_id)
def test_lstm_fwd_gemm(c):
    S, R, K = c["S"], c["R"], c["K"]
    k = gemm_case(c)
    ref, err = LR.fp32_error(LR.cell_fwd, LR.fwd_args(k))
    pre_max = float(LR.sum_planes(k["pre_planes"]).abs().max())
    ops.ensure_workspace(DEV)
    x, w = inside(k["x"].to(torch.bfloat16) if c["x16"] else k["x"], col=8, extra=16), dev(k["w"], c["x16"])
    pre = full((S, 4 * R), UNWRITTEN)
    g1, g2, b0, b1, cp, keep = inside(k["g1"]), inside(k["g2"]), dev(k["b0"]), dev(k["b1"]), dev(k["c_prev"]), dev(k["keep"])
    d = Dest()
    cc = d.flat(S, R)
    h, h2, hd, r1, r2 = h_dests(d, dict(c, layout="one"), S, R)
    gates = d.flat(S, 4 * R)
    assert expect_vec(R, [g1, g2, b0, b1, cp, cc, h, h2, hd, gates, x, w], keep)
    d.snapshot()
    ops.lstm_fwd_gemm(x, w, pre, g1, g2, b0, b1, cp, cc, h, h2, keep, k["scale"], hd, gates, S, R, c["rows_h"], c["rows_h2"])
    torch.cuda.synchronize()
    d.untouched()
    check_fwd("lstm_fwd_gemm", _id(c), c, ref, err, LR.GEMM_RTOL * pre_max, (cc, h, h2, hd, gates), r1, r2)
