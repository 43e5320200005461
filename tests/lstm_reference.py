"""Plain restatement of the LSTM cell kernels and of the "plane" protocol around them (include/subgc_hip.h: subgc_lstm_fwd / _fwd_gemm /
_bwd / _bwd_planes, subgc_gemm_*_planes) and of four streaming kernels (subgc_packed_time_sum, subgc_relu_bwd, subgc_gather_rows_keep,
subgc_class_partials), written from the header comments and not from the kernels.  A helper, not a test: tests/test_lstm_reference_cpu.py
pins it against torch.nn.LSTMCell + autograd, tests/test_lstm_cell_gpu.py and tests/test_lstm_planes_gpu.py compare the kernels with it.

Every function computes in the dtype of the tensors it is given (torch, CPU, no subgc import): with float64 inputs it is the reference, with
float32 inputs the same formulas give the rounding floor of the operation (`fp32_error`).

  forward   pre = sum of the planes (+ g1 + g2 + b0 + b1), column blocks of R in the order i, f, g, o;
            i, f, o = sigmoid, g = tanh;  c = f c_prev + i g (c_prev absent: zero);  h = o tanh(c);  hdrop = h keep scale (keep absent: h);
            h is written to rows < rows_h, its second copy h2 to rows < rows_h2 (0: all rows); c, hdrop and the gates to every row
  backward  dh = sum over the sources i of (sum of its planes) on rows < rows_i  +  dh_drop keep scale (keep absent: dh_drop);
            dct = dh o (1 - tanh(c)^2) + dc;  dpre = [dct g i(1-i) | dct c_prev f(1-f) | dct i (1-g^2) | dh tanh(c) o(1-o)];  dc_prev = dct f"""
import torch

NOT_WRITTEN = float("nan")      # marks the rows of h / h2 the kernel must leave alone
FWD_ATOL = 1e-6                 # what the project's cell test allows with O(1) inputs (test_lstm_gates_fwd_bwd)
BWD_ATOL = 1e-5
FLOOR_FACTOR = 8.0              # device tanhf / expf differ from the host's by a few ulp
BF16_ULP = 2.0 ** -8            # one bf16 rounding, relative
GEMM_RTOL = 2e-5                # of max |product|: test_gemm_f32_row_cut_shapes, test_gemm_bf16_mode_rounds_operands_only


def bf16_round(x):
    """Round to nearest even onto the bf16 grid; the result keeps the input's dtype (exact in fp32 and fp64)."""
    return x.to(torch.bfloat16).to(x.dtype)


def sum_planes(planes):
    """[n, rows, cols] -> [rows, cols]: the planes added one after the other into a zero start (the order the kernels add in)."""
    acc = torch.zeros_like(planes[0]) if planes.shape[0] else planes.new_zeros(planes.shape[1:])
    for p in range(planes.shape[0]):
        acc = acc + planes[p]
    return acc


def row_limit(r, S):
    return S if r is None or r <= 0 or r > S else int(r)


def cell_fwd(pre_planes, g1, g2, b0, b1, c_prev, keep, scale, rows_h=0, rows_h2=0):
    """pre_planes [n, S, 4R]; g1, g2 [S, 4R]; b0, b1 [4R]; c_prev [S, R]; keep [S, R] (0 / non-zero); absent terms are None.
    -> dict(c, h, h2, hdrop [S, R], gates [S, 4R]); h rows >= rows_h and h2 rows >= rows_h2 hold NOT_WRITTEN."""
    pre = sum_planes(pre_planes)
    S, R = pre.shape[0], pre.shape[1] // 4
    for t in (g1, g2, b0, b1):
        if t is not None:
            pre = pre + t
    i, f, o = torch.sigmoid(pre[:, :R]), torch.sigmoid(pre[:, R:2 * R]), torch.sigmoid(pre[:, 3 * R:])
    g = torch.tanh(pre[:, 2 * R:3 * R])
    c = i * g if c_prev is None else f * c_prev + i * g
    hn = o * torch.tanh(c)
    hdrop = hn if keep is None else hn * (keep != 0).to(hn.dtype) * scale
    h, h2 = hn.clone(), hn.clone()
    h[row_limit(rows_h, S):] = NOT_WRITTEN
    h2[row_limit(rows_h2, S):] = NOT_WRITTEN
    return {"c": c, "h": h, "h2": h2, "hdrop": hdrop, "gates": torch.cat([i, f, g, o], 1)}


def sum_sources(sources, S, R, like):
    """sources: at most three plane stacks [n_i, rows_i, R]; source i adds the sum of its planes to rows < rows_i, nothing to the rest."""
    assert len(sources) <= 3
    dh = like.new_zeros(S, R)
    for p in sources:
        if p is None or p.shape[0] == 0 or p.shape[1] == 0:
            continue
        dh[:p.shape[1]] = dh[:p.shape[1]] + sum_planes(p)
    return dh


def cell_bwd(gates, c_prev, c, sources, dh_drop, keep, scale, dc):
    """gates [S, 4R] (i, f, g, o as saved by the forward), c [S, R]; c_prev, dh_drop, keep, dc may be None.  -> dict(dpre [S, 4R], dc_prev [S, R])"""
    S, R = c.shape
    i, f, g, o = gates[:, :R], gates[:, R:2 * R], gates[:, 2 * R:3 * R], gates[:, 3 * R:]
    dh = sum_sources(sources, S, R, c)
    if dh_drop is not None:
        dh = dh + (dh_drop if keep is None else dh_drop * (keep != 0).to(c.dtype) * scale)
    tc = torch.tanh(c)
    dct = dh * o * (1 - tc * tc)
    if dc is not None:
        dct = dct + dc
    cp = torch.zeros_like(c) if c_prev is None else c_prev
    dpre = torch.cat([dct * g * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return {"dpre": dpre, "dc_prev": dct * f}


# ----------------------------------------------------------------------------- the streaming kernels
def packed_time_sum(src, offsets, S):
    """dst[s] = sum over the steps t with s < offsets[t+1] - offsets[t] of src[offsets[t] + s]."""
    dst = src.new_zeros(S, src.shape[1])
    for t in range(len(offsets) - 1):
        dst[:offsets[t + 1] - offsets[t]] += src[offsets[t]:offsets[t + 1]]
    return dst


def relu_bwd(dy, y, scale):
    return torch.where(y > 0, dy * scale, torch.zeros_like(dy))


def gather_rows_keep(src, rows, keep, scale):
    """dst[m] = src[rows[m]] (a zero row for rows[m] < 0), times keep[m] scale where a mask is given."""
    x = torch.where((rows >= 0)[:, None], src[rows.clamp(min=0).long()], src.new_zeros(()))
    return x if keep is None else torch.where(keep != 0, x * scale, torch.zeros_like(x))


def class_sum(x, cls, C):
    """[C, L]: the rows of x added per class id; ids outside [0, C) add nothing."""
    ok = (cls >= 0) & (cls < C)
    return x.new_zeros(C, x.shape[1]).index_add_(0, cls[ok].long(), x[ok])


# ----------------------------------------------------------------------------- inputs (shared by the CPU and the GPU tests)
def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def case(S, R, n_pre=1, absent=(), scale=4.0, rows_h=0, rows_h2=0, sources=(), seed=0):
    """fp32 CPU inputs of one cell case, forward and backward.
    absent: names among g1 g2 b0 b1 c_prev keep dh_drop dc (outputs a call leaves out are the GPU test's business).
    sources: up to three (n, rows_i, N, col0) -- a stack [max(n, 1), S, N] of unit-sum-scale planes of which the cell reads the window
    [:n, :rows_i, col0:col0 + R].  Every stack has S rows whatever rows_i is, so its plane stride is S * N and what lies past rows_i is
    valid memory holding values that must not be added.
    The backward's gates and c are the fp64 forward's, rounded to fp32."""
    g = torch.Generator().manual_seed(100003 * S + 101 * R + 7 * n_pre + seed)
    c = {"S": S, "R": R, "scale": float(scale), "rows_h": rows_h, "rows_h2": rows_h2}
    c["pre_planes"] = _randn(g, n_pre, S, 4 * R, scale=n_pre ** -0.5)
    c["g1"], c["g2"] = _randn(g, S, 4 * R, scale=0.5), _randn(g, S, 4 * R, scale=0.5)
    c["b0"], c["b1"] = _randn(g, 4 * R, scale=0.3), _randn(g, 4 * R, scale=0.3)
    c["c_prev"] = _randn(g, S, R)
    c["keep"] = (torch.rand(S, R, generator=g) < 1.0 / scale).to(torch.uint8)
    c["dh_drop"], c["dc"] = _randn(g, S, R), _randn(g, S, R)
    c["stacks"] = []
    for n, rows, N, col0 in sources:
        assert 0 <= rows <= S and 0 <= col0 and col0 + R <= N
        c["stacks"].append({"stack": _randn(g, max(n, 1), S, N, scale=max(n, 1) ** -0.5), "n": n, "rows": rows, "N": N, "col0": col0})
    for k in absent:
        assert k in ("g1", "g2", "b0", "b1", "c_prev", "keep", "dh_drop", "dc"), k
        c[k] = None
    f = cell_fwd(**cast(fwd_args(c), torch.float64))
    c["gates"], c["c"] = f["gates"].float(), f["c"].float()
    return c


def cast(args, dtype):
    def one(x):
        if isinstance(x, (list, tuple)):
            return [one(y) for y in x]
        return x.to(dtype) if torch.is_tensor(x) and x.is_floating_point() else x
    return {k: one(x) for k, x in args.items()}


def fwd_args(c):
    return {k: c[k] for k in ("pre_planes", "g1", "g2", "b0", "b1", "c_prev", "keep", "scale", "rows_h", "rows_h2")}


def windows(c):
    """The plane windows of the case's stacks: [n_i, rows_i, R] each."""
    R = c["R"]
    return [s["stack"][:s["n"], :s["rows"], s["col0"]:s["col0"] + R] for s in c["stacks"]]


def bwd_args(c):
    return dict({k: c[k] for k in ("gates", "c_prev", "c", "dh_drop", "keep", "scale", "dc")}, sources=windows(c))


def fp32_error(fn, args):
    """fn(**args) in fp64 (the reference) and in fp32; -> (ref, {output: max |fp32 - fp64| over the written elements})."""
    ref = fn(**cast(args, torch.float64))
    low = fn(**cast(args, torch.float32))
    err = {}
    for k, x in ref.items():
        d = (low[k].double() - x).abs()
        d = d[~torch.isnan(x)]
        err[k] = float(d.max()) if d.numel() else 0.0
    return ref, err


def bound(err32, atol, extra=0.0):
    """The fp32 bound of one output: the larger of the project's constant and FLOOR_FACTOR x the reference's own fp32 error (+ a GEMM part)."""
    return max(atol, FLOOR_FACTOR * err32) + extra


def tol_of(ref, b, bf16):
    """Element-wise tolerance: the fp32 bound, plus one bf16 ulp of the reference where the destination is bf16."""
    t = torch.full_like(ref, b)
    return t + ref.abs() * BF16_ULP if bf16 else t
