"""Plain restatement of the attention kernels' contract (include/subgc_hip.h: subgc_attn_fwd / _fwd_q / _bwd / _bwd_planes / _bwd_planes_de /
_du_accum / _dv_accum and the shared-set forms subgc_attn_*_group), written from the header comments and not from the kernels.  A helper, not
a test: tests/test_attention_reference_cpu.py pins it, tests/test_attention_variants_gpu.py compares every kernel variant with it.

Every function computes in the dtype of the tensors it is given (torch, CPU): with float64 inputs it is the reference, with float32 inputs the
same formulas give the rounding floor of the operation.  `tanh` is the activation; ShiftedTanh moves every tanh value by +-TANH_EPS with
random signs (the absolute error bound of the device's tanh), which measures how far an output may move for that reason alone.
`tolerance()` turns the two into the bound the GPU tests assert and the CPU tests check for resolving power: nothing in it is measured on
the kernels.

For a sentence s with node rows m0 .. m0 + len - 1:
  forward   e_i = sum_a w_a[a] tanh(u[m0+i, a] + q[s, a]) + b_a;  alpha = softmax(e) over i < len, zero from len on;  ctx = sum_i alpha_i v[m0+i]
            (len = 0: a zero alpha row and a zero ctx row);  a query from planes is q[s] = bias + sum_p planes[p][s]
  backward  (alpha is an INPUT)  dctx = sum of its planes;  dalpha_i = <dctx, v_i>;  de_i = alpha_i (dalpha_i - sum_k alpha_k dalpha_k);
            db_a[s] = sum_i de_i;  dah[s, a] = sum_i de_i w_a (1 - t^2);  dw_a[s, a] = sum_i de_i t;  du[m0+i, a] += de_i w_a (1 - t^2);
            dv[m0+i] += alpha_i dctx;  dctx_keep[s] = dctx;  de_keep[s, i] = de_i
du / dv accumulate: the functions take what the buffers held before the call (du0 / dv0)."""
import torch

TANH_EPS = 5e-7
FLOOR_FACTOR = 8.0      # the kernels sum in another order (wave trees, four-way unrolled sums) than torch does
SENS_FACTOR = 4.0       # a random-sign shift understates a correlated one
BF16_ULP = 2.0 ** -8    # one bf16 rounding, relative


class ShiftedTanh:
    """tanh(x) +- TANH_EPS, the signs drawn from a seeded generator (the same sequence for the same sequence of calls)."""

    def __init__(self, seed=1234, eps=TANH_EPS):
        self.g = torch.Generator().manual_seed(seed)
        self.eps = eps

    def __call__(self, x):
        sign = torch.randint(0, 2, x.shape, generator=self.g).to(x.dtype) * 2 - 1
        return torch.tanh(x) + self.eps * sign


def bf16_round(x):
    """The values a bf16 tensor holds, as the input's dtype (exact in fp32 and fp64)."""
    return x.to(torch.bfloat16).to(x.dtype)


def attn_query(planes, bias):
    """planes [n, S, A], bias [A] -> q [S, A] = bias + sum of the planes (added in plane order)."""
    q = planes[0].clone()
    for p in range(1, planes.shape[0]):
        q = q + planes[p]
    return q + bias


def _sentence_fwd(ur, vr, q, w_a, b_a, tanh):
    e = tanh(ur + q) @ w_a + b_a
    a = torch.softmax(e, 0)
    return a, a @ vr


def _sentence_bwd(ur, vr, q, w_a, al, g, tanh):
    t = tanh(ur + q)
    dal = vr @ g
    de = al * (dal - (al * dal).sum())
    gu = de[:, None] * w_a * (1 - t * t)
    return de, gu, (de[:, None] * t).sum(0), al[:, None] * g


def _sum_planes(planes):
    g = planes[0].clone()
    for p in range(1, planes.shape[0]):
        g = g + planes[p]
    return g


def attn_fwd(u, v, q, w_a, b_a, off, lens, n_stride, tanh=torch.tanh):
    """u [rows, A], v [rows, R], q [S, A], w_a [A], b_a [1]; off / lens: S ints.  -> alpha [S, n_stride], ctx [S, R]."""
    S, R = len(lens), v.shape[1]
    alpha, ctx = u.new_zeros(S, n_stride), u.new_zeros(S, R)
    for s in range(S):
        m0, l = int(off[s]), int(lens[s])
        if l > 0:
            alpha[s, :l], ctx[s] = _sentence_fwd(u[m0:m0 + l], v[m0:m0 + l], q[s], w_a, b_a, tanh)
    return {"alpha": alpha, "ctx": ctx}


def attn_bwd(u, v, q, w_a, off, lens, alpha, dctx_planes, du0=None, dv0=None, tanh=torch.tanh):
    """alpha [S, n_stride] (input), dctx_planes [n, S, R]; du0 / dv0: what the accumulated buffers hold before the call (None: zeros).
    -> dah, dw_a [S, A], db_a [S], du [rows, A] and dv [rows, R] after the call, dctx_keep [S, R], de_keep [S, n_stride] (zero from len on:
    the kernel leaves those entries alone)."""
    S, A = len(lens), u.shape[1]
    g = _sum_planes(dctx_planes)
    out = {"dah": u.new_zeros(S, A), "dw_a": u.new_zeros(S, A), "db_a": u.new_zeros(S), "du": torch.zeros_like(u) if du0 is None else du0.clone(),
           "dv": torch.zeros_like(v) if dv0 is None else dv0.clone(), "dctx_keep": g, "de_keep": torch.zeros_like(alpha)}
    for s in range(S):
        m0, l = int(off[s]), int(lens[s])
        if l == 0:
            continue
        de, gu, dw, dv = _sentence_bwd(u[m0:m0 + l], v[m0:m0 + l], q[s], w_a, alpha[s, :l], g[s], tanh)
        out["de_keep"][s, :l] = de
        out["db_a"][s] = de.sum()
        out["dah"][s] = gu.sum(0)
        out["dw_a"][s] = dw
        out["du"][m0:m0 + l] += gu
        out["dv"][m0:m0 + l] += dv
    return out


def live_steps(step_off, s):
    """The flat rows step_off[t] + s of the steps t at which sentence s is live (s < step_off[t+1] - step_off[t])."""
    return [int(step_off[t]) + s for t in range(len(step_off) - 1) if s < int(step_off[t + 1]) - int(step_off[t])]


def attn_du_accum(u, ah, de, step_off, off, lens, w_a, tanh=torch.tanh):
    """ah [rows_t, A], de [rows_t, n_stride] in the packed step layout.  -> du [rows, A] (every row of every sentence is written)."""
    du = torch.zeros_like(u)
    for s in range(len(lens)):
        m0, l = int(off[s]), int(lens[s])
        for f in live_steps(step_off, s):
            t = tanh(u[m0:m0 + l] + ah[f])
            du[m0:m0 + l] += de[f, :l, None] * w_a * (1 - t * t)
    return {"du": du}


def attn_dv_accum(alpha, dctx, step_off, off, lens, rows, tanh=None):
    """alpha [rows_t, n_stride], dctx [rows_t, R] in the packed step layout.  -> dv [rows, R]."""
    dv = dctx.new_zeros(rows, dctx.shape[1])
    for s in range(len(lens)):
        m0, l = int(off[s]), int(lens[s])
        for f in live_steps(step_off, s):
            dv[m0:m0 + l] += alpha[f, :l, None] * dctx[f]
    return {"dv": dv}


# ----------------------------------------------------------------------------- shared sets: u [B*Nn, A], v [B*Nn, R] once per image
def group_live(rows, lens, m, B, g, Nn):
    """(image, row, valid nodes) of every sentence that takes part: 0 <= rows[b*g + j] < m; lens is indexed by row."""
    out = []
    for b in range(B):
        for j in range(g):
            r = int(rows[b * g + j])
            if 0 <= r < m:
                out.append((b, r, min(int(lens[r]), Nn)))
    return out


def attn_fwd_group(u, v, q, w_a, b_a, rows, lens, m, B, g, Nn, n_stride, tanh=torch.tanh):
    """q [>= m, A] by row.  -> alpha [m, n_stride], ctx [m, R] (rows no live sentence maps to stay zero here and untouched on the device)."""
    alpha, ctx = u.new_zeros(m, n_stride), u.new_zeros(m, v.shape[1])
    for b, r, l in group_live(rows, lens, m, B, g, Nn):
        if l > 0:
            alpha[r, :l], ctx[r] = _sentence_fwd(u[b * Nn:b * Nn + l], v[b * Nn:b * Nn + l], q[r], w_a, b_a, tanh)
    return {"alpha": alpha, "ctx": ctx}


def attn_bwd_group(u, v, q, w_a, rows, lens, m, B, g, Nn, alpha, dctx_planes, du0=None, tanh=torch.tanh):
    """-> dah, dw_a [m, A], db_a [m], dctx_keep [m, R] by row; du [B*Nn, A] = du0 (None: zeros) + the increments of all of the image's
    sentences (the device spreads them over subgc_attn_group_du_planes(g) planes that the caller adds)."""
    A = u.shape[1]
    g_ = _sum_planes(dctx_planes)[:m]
    out = {"dah": u.new_zeros(m, A), "dw_a": u.new_zeros(m, A), "db_a": u.new_zeros(m), "du": torch.zeros_like(u) if du0 is None else du0.clone(),
           "dctx_keep": g_}
    for b, r, l in group_live(rows, lens, m, B, g, Nn):
        if l == 0:
            continue
        de, gu, dw, _ = _sentence_bwd(u[b * Nn:b * Nn + l], v[b * Nn:b * Nn + l], q[r], w_a, alpha[r, :l], g_[r], tanh)
        out["db_a"][r] = de.sum()
        out["dah"][r] = gu.sum(0)
        out["dw_a"][r] = dw
        out["du"][b * Nn:b * Nn + l] += gu
    return out


def attn_dv_accum_group(alpha, dctx, step_off, rows, B, g, Nn, tanh=None):
    """dv [B*Nn, R] = sum over steps t and the image's sentences j with 0 <= rows[b*g+j] < step_off[t+1] - step_off[t] of
    alpha[step_off[t] + row, i] * dctx[step_off[t] + row]: every one of the image's Nn rows is written (zeros where nothing attends)."""
    dv = dctx.new_zeros(B * Nn, dctx.shape[1])
    l = min(Nn, alpha.shape[1])
    for b in range(B):
        for j in range(g):
            r = int(rows[b * g + j])
            for t in range(len(step_off) - 1):
                if 0 <= r < int(step_off[t + 1]) - int(step_off[t]):
                    f = int(step_off[t]) + r
                    dv[b * Nn:b * Nn + l] += alpha[f, :l, None] * dctx[f]
    return {"dv": dv}


# ----------------------------------------------------------------------------- tolerance: from the reference alone
def cast(args, dtype):
    return {k: (x.to(dtype) if torch.is_tensor(x) and x.is_floating_point() else x) for k, x in args.items()}


def tolerance(fn, args, bf16_out=(), seed=1234):
    """fn(**args, tanh=...) -> dict of tensors; args hold fp32-representable tensors.  Returns (ref, tol, parts):
    ref  = fn in fp64;  floor(X) = max |fn in fp32 - ref|;  sens(X) = max |fn in fp64 with every tanh shifted by +-TANH_EPS - ref|;
    tol(X) = FLOOR_FACTOR floor(X) + SENS_FACTOR sens(X), plus |ref| 2^-8 element by element where the destination is bf16."""
    a64 = cast(args, torch.float64)
    ref = fn(**a64, tanh=torch.tanh)
    low = fn(**cast(args, torch.float32), tanh=torch.tanh)
    shf = fn(**a64, tanh=ShiftedTanh(seed))
    tol, parts = {}, {}
    for k, x in ref.items():
        floor = float((low[k].double() - x).abs().max()) if x.numel() else 0.0
        sens = float((shf[k] - x).abs().max()) if x.numel() else 0.0
        parts[k] = (floor, sens)
        t = torch.full_like(x, FLOOR_FACTOR * floor + SENS_FACTOR * sens)
        tol[k] = t + x.abs() * BF16_ULP if k in bf16_out else t
    return ref, tol, parts


# ----------------------------------------------------------------------------- inputs (shared by the CPU and the GPU tests)
SENT_LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 33, 37, 130]


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def sentence_case(A, R, lens=SENT_LENS, n_stride=130, q_planes=0, dctx_planes=1, bf16_sets=False, seed=0):
    """fp32 CPU inputs of one per-sentence case: u, v, q (and, q_planes > 0, the planes and bias it is the sum of), w_a scaled by 1/sqrt(A)
    (unit-scale scores whatever A is: every perturbation of the resolving-power test then moves every output), b_a, d(ctx) planes whose sum
    is unit scale, off / lens, and `alpha`: the fp64 reference's weights rounded to fp32 (the backward's input)."""
    g = torch.Generator().manual_seed(1000 * A + R + seed)
    lens = list(lens)
    S, rows = len(lens), sum(lens)
    off = [sum(lens[:s]) for s in range(S)]
    c = {"A": A, "R": R, "S": S, "rows": rows, "lens": lens, "off": off, "n_stride": n_stride}
    c["u"], c["v"] = _randn(g, rows, A), _randn(g, rows, R)
    if bf16_sets:
        c["u"], c["v"] = bf16_round(c["u"]), bf16_round(c["v"])
    c["w_a"], c["b_a"] = _randn(g, A, scale=A ** -0.5), torch.tensor([0.2])
    if q_planes:
        c["q_planes"], c["q_bias"] = _randn(g, q_planes, S, A, scale=q_planes ** -0.5), _randn(g, A, scale=0.1)
        c["q"] = attn_query(c["q_planes"].double(), c["q_bias"].double()).float()      # what q_out should hold, to fp32
    else:
        c["q"] = _randn(g, S, A)
    c["dctx_planes"] = _randn(g, dctx_planes, S, R, scale=dctx_planes ** -0.5)
    f = attn_fwd(c["u"].double(), c["v"].double(), c["q"].double(), c["w_a"].double(), c["b_a"].double(), off, lens, n_stride)
    c["alpha"] = f["alpha"].float()
    return c


def fwd_args(c):
    return {k: c[k] for k in ("u", "v", "q", "w_a", "b_a", "off", "lens", "n_stride")}


def fwd_planes(c):
    """The forward from query planes as one function: q_out is an output."""
    def fn(u, v, q_planes, q_bias, w_a, b_a, off, lens, n_stride, tanh):
        q = attn_query(q_planes, q_bias)
        return dict(attn_fwd(u, v, q, w_a, b_a, off, lens, n_stride, tanh), q_out=q)
    return fn, {k: c[k] for k in ("u", "v", "q_planes", "q_bias", "w_a", "b_a", "off", "lens", "n_stride")}


def bwd_args(c):
    return {k: c[k] for k in ("u", "v", "q", "w_a", "off", "lens", "alpha", "dctx_planes")}


def packed_steps(S, T, seed=0):
    """step_off [T+1] of a packed layout whose live count shrinks from S (non-increasing) so that the last sentences are live at few steps."""
    g = torch.Generator().manual_seed(seed)
    live = sorted(torch.randint(1, S + 1, (T,), generator=g).tolist(), reverse=True)
    live[0] = S
    off = [0]
    for m in live:
        off.append(off[-1] + m)
    return off


def accum_case(A, R, lens, T, n_stride, bf16_u=False, seed=0, dead_last=False):
    """Inputs of the two per-sentence accumulators: T packed steps of query rows, d(e) rows, alpha rows and d(ctx) rows.
    dead_last: one more sentence (the last) that is live at no step."""
    lens = list(lens)
    S = len(lens)
    step_off = packed_steps(S, T, seed + A + R)
    if dead_last:
        lens = lens + [7]
    g = torch.Generator().manual_seed(7000 + 13 * A + R + seed)
    rows, tot = sum(lens), step_off[-1]
    c = {"A": A, "R": R, "S": len(lens), "T": T, "rows": rows, "lens": lens, "off": [sum(lens[:s]) for s in range(len(lens))],
         "step_off": step_off, "tot": tot, "n_stride": n_stride}
    c["u"] = _randn(g, rows, A)
    if bf16_u:
        c["u"] = bf16_round(c["u"])
    c["w_a"] = _randn(g, A, scale=A ** -0.5)
    c["ah"], c["de"] = _randn(g, tot, A), _randn(g, tot, n_stride, scale=0.1)
    c["alpha"], c["dctx"] = torch.rand(tot, n_stride, generator=g), _randn(g, tot, R)
    return c


def group_layout(g, Nn, seed=0):
    """B = 3 images of g sentence slots: image 0 all live (slot 0 over an EMPTY set, the last slot over all Nn nodes), image 1 with dead slots
    of both kinds (-1 in slot 0 from g = 2 on, a position >= m in the last slot from g = 3 on: from g = 4 on that one lies in the image's second
    workgroup) and the live positions of all images permuted, image 2 without a live sentence.  -> rows [3g], lens [m] by row, m."""
    gen = torch.Generator().manual_seed(31 * g + Nn + seed)
    B = 3
    live = [(0, j) for j in range(g)] + [(1, j) for j in range(g) if not (g >= 2 and j == 0) and not (g >= 3 and j == g - 1)]
    m = len(live)
    pos = torch.randperm(m, generator=gen).tolist()
    rows = [-1 if k % 2 == 0 else m + k for k in range(B * g)]
    lens = [0] * m
    for (b, j), r in zip(live, pos):
        rows[b * g + j] = r
        lens[r] = int(torch.randint(1, Nn + 1, (1,), generator=gen)) if Nn > 1 else 1
        if b == 0 and j == 0:
            lens[r] = 0
        elif b == 0 and j == g - 1:
            lens[r] = Nn
        elif b == 1 and Nn > 2:
            lens[r] = min(lens[r], Nn - 2)                  # image 1 leaves node rows past its longest set (NaN on the device)
    if g >= 3:
        rows[g + g - 1] = m + 1
    if g >= 2:
        rows[g] = -1
    return rows, lens, m, B


def group_case(A, R, g, Nn, n_stride=None, q_planes=0, dctx_planes=1, bf16_sets=False, seed=0):
    """fp32 CPU inputs of one shared-set case; arrays by row have m + 2 rows (two guard rows the kernels must not touch)."""
    rows, lens, m, B = group_layout(g, Nn, seed)
    gen = torch.Generator().manual_seed(500 * A + 3 * R + 17 * g + Nn + seed)
    n_stride = n_stride or Nn
    c = {"A": A, "R": R, "g": g, "Nn": Nn, "B": B, "m": m, "ma": m + 2, "rows": rows, "lens": lens, "n_stride": n_stride}
    c["u"], c["v"] = _randn(gen, B * Nn, A), _randn(gen, B * Nn, R)
    if bf16_sets:
        c["u"], c["v"] = bf16_round(c["u"]), bf16_round(c["v"])
    c["w_a"], c["b_a"] = _randn(gen, A, scale=A ** -0.5), torch.tensor([0.2])
    if q_planes:
        c["q_planes"], c["q_bias"] = _randn(gen, q_planes, m + 2, A, scale=q_planes ** -0.5), _randn(gen, A, scale=0.1)
        c["q"] = attn_query(c["q_planes"].double(), c["q_bias"].double()).float()
    else:
        c["q"] = _randn(gen, m + 2, A)
    c["dctx_planes"] = _randn(gen, dctx_planes, m + 2, R, scale=dctx_planes ** -0.5)
    f = attn_fwd_group(c["u"].double(), c["v"].double(), c["q"].double(), c["w_a"].double(), c["b_a"].double(), rows, lens, m, B, g, Nn, n_stride)
    c["alpha"] = f["alpha"].float()
    return c


def image_lmax(c, b):
    """Valid nodes of image b's longest live sentence (0: none live, or only empty sets)."""
    return max([l for bb, _r, l in group_live(c["rows"], c["lens"], c["m"], c["B"], c["g"], c["Nn"]) if bb == b] + [0])


def group_fwd_args(c):
    return {k: c[k] for k in ("u", "v", "q", "w_a", "b_a", "rows", "lens", "m", "B", "g", "Nn", "n_stride")}


def group_fwd_planes(c):
    def fn(u, v, q_planes, q_bias, w_a, b_a, rows, lens, m, B, g, Nn, n_stride, tanh):
        q = attn_query(q_planes, q_bias)
        return dict(attn_fwd_group(u, v, q, w_a, b_a, rows, lens, m, B, g, Nn, n_stride, tanh), q_out=q[:m])
    return fn, {k: c[k] for k in ("u", "v", "q_planes", "q_bias", "w_a", "b_a", "rows", "lens", "m", "B", "g", "Nn", "n_stride")}


def group_bwd_args(c):
    return {k: c[k] for k in ("u", "v", "q", "w_a", "rows", "lens", "m", "B", "g", "Nn", "alpha", "dctx_planes")}


def group_accum_case(R, g, Nn, T, n_stride, seed=0):
    """Inputs of subgc_attn_dv_accum_group: the layout of group_layout, the positions live while < the step's shrinking live count."""
    rows, _lens, m, B = group_layout(g, Nn, seed)
    step_off = packed_steps(m, T, seed + R)
    gen = torch.Generator().manual_seed(9000 + R + g + seed)
    tot = step_off[-1]
    return {"R": R, "g": g, "Nn": Nn, "B": B, "T": T, "rows": rows, "step_off": step_off, "tot": tot, "n_stride": n_stride,
            "alpha": torch.rand(tot, n_stride, generator=gen), "dctx": _randn(gen, tot, R)}
