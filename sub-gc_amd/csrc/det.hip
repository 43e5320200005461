// Deterministic-mode forms of the scatter-adds of the training step (subgc_deterministic(1), see include/subgc_hip.h).
//
// Scatter-add without float atomics: an inverted index (destination -> its source items in ASCENDING order) is built in the caller's
// workspace, then every destination sums its items in that order and adds the total to its row ONCE (cdna_hip_programming.md,
// Appendix B 'Scatter / gather / embedding').  Long lists are cut into chunks of DCHK items summed by separate workgroups; the chunk
// sums are added in chunk order by a finish pass (the skewed-word pitfall of the same section: pad / end tokens reach thousands of
// rows per word).  Index build: integer counts (order-free) -> one-workgroup scans -> placement through an integer cursor -> a per-list
// sort that restores ascending order (one wave per list of <= DCHK items, an LDS bitmap for longer ones: at most 262144 items
// per call).  The layout and the chunk plan depend on (items, destinations, columns) alone.
//
// sumsq: fixed grid of per-workgroup partials and one ordered finish pass; the float4 and scalar loads run the same arithmetic.
#include "common.h"

#include <algorithm>

namespace subgc {
namespace {

constexpr int DCHK = 64;             // items per chunk of one destination's list
constexpr int BITMAP_WORDS = 8192;   // 32 KB of LDS for the long-list sort: at most 262144 items per call

inline size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }

struct IndexLayout {
    int* cnt; int* cursor; int* start; int* ustart; int* pstart; int* lstart; int* list; float* part;
    int64_t unit_bound, long_bound, pslots;
    size_t bytes;
};
// shape-only layout: D destinations, n items, E columns per row
inline IndexLayout index_layout(void* ws, int64_t n, int64_t D, int64_t E) {
    IndexLayout l{};
    l.pslots = 2 * cdiv(n, DCHK);                       // sum over lists longer than DCHK of ceil(len / DCHK) <= 2 n / DCHK
    l.long_bound = std::max<int64_t>(1, cdiv(n, DCHK));
    l.unit_bound = std::max<int64_t>(1, std::min(n, D) + l.pslots);
    const size_t ints = (size_t)2 * D + 4 * (D + 1) + n;
    l.bytes = al16(ints * sizeof(int)) + (size_t)l.pslots * E * sizeof(float);
    int* p = static_cast<int*>(ws);
    l.cnt = p; l.cursor = p + D; l.start = p + 2 * D; l.ustart = l.start + (D + 1); l.pstart = l.ustart + (D + 1); l.lstart = l.pstart + (D + 1);
    l.list = l.lstart + (D + 1);
    l.part = reinterpret_cast<float*>(static_cast<char*>(ws) + al16(ints * sizeof(int)));
    return l;
}

// ---- keys: destination of item i, or -1 (skipped) ----
struct EmbedKey {
    const int64_t* tok; int64_t stride; int rows;
    __device__ int operator()(int i) const {
        int64_t w = tok[(int64_t)i * stride];
        return (int)(w < 0 ? 0 : (w >= rows ? rows - 1 : w));           // the clamp of embed_bwd_kernel
    }
};
struct RowKey {
    const int32_t* rows; const int32_t* m_dev; int D;
    __device__ int operator()(int m) const {
        if (m_dev && m >= *m_dev) return -1;
        const int r = rows[m];
        return r >= 0 && r < D ? r : -1;
    }
};
struct PoolKey {                     // item = g * N + i
    const int64_t* idx; int64_t idx_stride; const float* w; int64_t w_g, w_i; const int32_t* img; int N, D;
    __device__ int operator()(int p) const {
        const int g = p / N, i = p - g * N;
        if (w[(int64_t)g * w_g + (int64_t)i * w_i] == 0.f) return -1;
        int64_t n = idx[(int64_t)g * idx_stride + i];
        n = n < 0 ? 0 : (n >= N ? N - 1 : n);
        const int64_t r = (int64_t)img[g] * N + n;
        return r >= 0 && r < D ? (int)r : -1;
    }
};

// ---- values: column c of item i; commit: add a destination's total to its row ----
struct EmbedVal {
    const float* table; const uint8_t* keep; float scale; const float* dout; float* dtable; int E;
    __device__ float operator()(int i, int c) const {
        const float g = dout[(int64_t)i * E + c];
        return keep ? (keep[(int64_t)i * E + c] ? g * scale : 0.f) : g;
    }
    __device__ void commit(int d, int c, float s) const {
        if (table[(int64_t)d * E + c] > 0.f) dtable[(int64_t)d * E + c] += s;    // ReLU mask of the embedding (AttModel.py embed)
    }
};
struct RowVal {
    const float* src; int64_t lds; float* dX; int64_t ldx;
    __device__ float operator()(int m, int c) const { return src[(int64_t)m * lds + c]; }
    __device__ void commit(int d, int c, float s) const { dX[(int64_t)d * ldx + c] += s; }
};
struct PoolVal {
    const float* dout; const float* denom; const int32_t* argmax; const float* w; int64_t w_g, w_i; float* dX; int N, L;
    __device__ float operator()(int p, int c) const {
        const int g = p / N, i = p - g * N;
        const float wi = w[(int64_t)g * w_g + (int64_t)i * w_i];
        const float dmean = dout[(int64_t)g * 2 * L + L + c] / denom[g];
        const float dmax = argmax[(int64_t)g * L + c] == i ? dout[(int64_t)g * 2 * L + c] : 0.f;
        return wi * (dmean + dmax);                                       // the expression of pool_bwd_kernel
    }
    __device__ void commit(int d, int c, float s) const { dX[(int64_t)d * L + c] += s; }
};

template <class K>
__global__ __launch_bounds__(256) void det_count_kernel(K key, int n, int* __restrict__ cnt) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int d = key(i);
        if (d >= 0) atomicAdd(cnt + d, 1);                                // integer: the counts do not depend on the order
    }
}
// exclusive scans over D destinations of: list length, work units (max(1, chunks) of a non-empty list), partial slots (chunks of a
// list longer than DCHK), long lists.  One workgroup of 1024 threads, each a contiguous range of destinations.
__global__ __launch_bounds__(1024) void det_scan_kernel(const int* __restrict__ cnt, int D, int* __restrict__ start, int* __restrict__ ustart,
                                                        int* __restrict__ pstart, int* __restrict__ lstart) {
    __shared__ int sm[4][1024];
    const int t = threadIdx.x, per = (D + 1023) / 1024, a = min(D, t * per), b = min(D, a + per);
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int d = a; d < b; ++d) {
        const int c = cnt[d], ch = (c + DCHK - 1) / DCHK;
        s0 += c; s1 += c > 0 ? max(1, ch) : 0; s2 += c > DCHK ? ch : 0; s3 += c > DCHK ? 1 : 0;
    }
    sm[0][t] = s0; sm[1][t] = s1; sm[2][t] = s2; sm[3][t] = s3;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                        // Hillis-Steele inclusive scan
        int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        if (t >= off) { v0 = sm[0][t - off]; v1 = sm[1][t - off]; v2 = sm[2][t - off]; v3 = sm[3][t - off]; }
        __syncthreads();
        sm[0][t] += v0; sm[1][t] += v1; sm[2][t] += v2; sm[3][t] += v3;
        __syncthreads();
    }
    int e0 = sm[0][t] - s0, e1 = sm[1][t] - s1, e2 = sm[2][t] - s2, e3 = sm[3][t] - s3;
    for (int d = a; d < b; ++d) {
        start[d] = e0; ustart[d] = e1; pstart[d] = e2; lstart[d] = e3;
        const int c = cnt[d], ch = (c + DCHK - 1) / DCHK;
        e0 += c; e1 += c > 0 ? max(1, ch) : 0; e2 += c > DCHK ? ch : 0; e3 += c > DCHK ? 1 : 0;
    }
    if (t == 1023) { start[D] = sm[0][t]; ustart[D] = sm[1][t]; pstart[D] = sm[2][t]; lstart[D] = sm[3][t]; }
}
template <class K>
__global__ __launch_bounds__(256) void det_fill_kernel(K key, int n, const int* __restrict__ start, int* __restrict__ cursor, int* __restrict__ list) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int d = key(i);
        if (d >= 0) list[start[d] + atomicAdd(cursor + d, 1)] = i;     // any order inside the list: the sort kernels fix it
    }
}
// largest d in [0, D) with x[d] <= q (x non-decreasing, x[0] = 0 <= q)
__device__ __forceinline__ int det_find(const int* __restrict__ x, int D, int q) {
    int lo = 0, hi = D - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (x[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// lists of at most DCHK items: one wave per destination ranks its list in LDS and writes it back ascending (256 B of LDS per wave)
__global__ __launch_bounds__(256) void det_sort_small_kernel(const int* __restrict__ start, int* __restrict__ list, int D) {
    __shared__ int sv[4][DCHK];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, d = blockIdx.x * 4 + w;
    int a = 0, len = 0, v = 0;
    if (d < D) { a = start[d]; len = start[d + 1] - a; }
    const bool mine = len > 1 && len <= DCHK && lane < len;
    if (mine) { v = list[a + lane]; sv[w][lane] = v; }
    __syncthreads();
    if (mine) {
        int r = 0;
        for (int j = 0; j < len; ++j) r += sv[w][j] < v;
        list[a + r] = v;
    }
}
// lists longer than DCHK (at most n / DCHK of them; grid = that bound, the lists found through lstart): a bitmap of the item range in LDS,
// set bits emitted in ascending order
__global__ __launch_bounds__(256) void det_sort_long_kernel(const int* __restrict__ start, const int* __restrict__ lstart, int* __restrict__ list,
                                                            int D, int n) {
    __shared__ unsigned bm[BITMAP_WORDS];
    __shared__ int wsum[256];
    const int q = blockIdx.x, t = threadIdx.x;
    if (q >= lstart[D]) return;
    const int d = det_find(lstart, D, q);
    const int a = start[d], len = start[d + 1] - a;
    const int words = (n + 31) / 32;
    for (int k = t; k < words; k += 256) bm[k] = 0u;
    __syncthreads();
    for (int k = t; k < len; k += 256) {
        const int v = list[a + k];
        atomicOr(&bm[v >> 5], 1u << (v & 31));                        // set bits: the result does not depend on the order
    }
    __syncthreads();
    const int per = (words + 255) / 256, w0 = min(words, t * per), w1 = min(words, w0 + per);
    int c = 0;
    for (int k = w0; k < w1; ++k) c += __popc(bm[k]);
    wsum[t] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = t >= off ? wsum[t - off] : 0;
        __syncthreads();
        wsum[t] += v;
        __syncthreads();
    }
    int o = a + wsum[t] - c;
    for (int k = w0; k < w1; ++k) {
        unsigned m = bm[k];
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            list[o++] = k * 32 + b;
        }
    }
}
// grid (unit_bound, E / 256): one chunk of one list per workgroup, a column per thread, items added in list order; a list of at most
// DCHK items is committed here, the chunks of a longer one go to its partial slots
template <class V>
__global__ __launch_bounds__(256) void det_sum_kernel(V val, const int* __restrict__ start, const int* __restrict__ ustart,
                                                      const int* __restrict__ pstart, const int* __restrict__ list, float* __restrict__ part,
                                                      int D, int E) {
#pragma clang fp contract(off)
    const int q = blockIdx.x;
    if (q >= ustart[D]) return;
    const int d = det_find(ustart, D, q), j = q - ustart[d];
    const int a = start[d], len = start[d + 1] - a;
    const int k0 = a + j * DCHK, k1 = min(a + len, k0 + DCHK);
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= E) return;
    float s = 0.f;
    int k = k0;
    for (; k + 4 <= k1; k += 4) {                                     // four items requested before the first is added (order kept)
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = val(list[k + u], c);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += x[u];
    }
    for (; k < k1; ++k) s += val(list[k], c);
    if (len <= DCHK) val.commit(d, c, s);
    else part[(int64_t)(pstart[d] + j) * E + c] = s;
}
// grid (long_bound, E / 256): a long list's chunk sums added in chunk order, then committed
template <class V>
__global__ __launch_bounds__(256) void det_finish_kernel(V val, const int* __restrict__ start, const int* __restrict__ pstart,
                                                         const int* __restrict__ lstart, const float* __restrict__ part, int D, int E) {
#pragma clang fp contract(off)
    const int q = blockIdx.x;
    if (q >= lstart[D]) return;
    const int d = det_find(lstart, D, q);
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= E) return;
    const int nch = (start[d + 1] - start[d] + DCHK - 1) / DCHK, p0 = pstart[d];
    float s = 0.f;
    for (int j = 0; j < nch; ++j) s += part[(int64_t)(p0 + j) * E + c];
    val.commit(d, c, s);
}

inline int ew_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 256), 2048)); }

template <class K, class V>
int det_scatter(K key, V val, int64_t n, int64_t D, int E, void* workspace, size_t ws_bytes, hipStream_t s, const char* what) {
    SUBGC_REQUIRE(n <= (int64_t)BITMAP_WORDS * 32 && D < (1ll << 30), "%s: deterministic mode supports up to %d items (got %lld)", what,
                  BITMAP_WORDS * 32, (long long)n);
    const IndexLayout l = index_layout(workspace, n, D, E);
    SUBGC_REQUIRE(workspace && ws_bytes >= l.bytes && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "%s: deterministic mode needs %zu bytes of 16-byte aligned workspace (got %zu)", what, l.bytes, workspace ? ws_bytes : (size_t)0);
    if (hipMemsetAsync(l.cnt, 0, (size_t)2 * D * sizeof(int), s) != hipSuccess) return check_launch(what);
    const int nb = ew_blocks(n);
    hipLaunchKernelGGL(det_count_kernel<K>, dim3(nb), dim3(256), 0, s, key, (int)n, l.cnt);
    hipLaunchKernelGGL(det_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)l.cnt, (int)D, l.start, l.ustart, l.pstart, l.lstart);
    hipLaunchKernelGGL(det_fill_kernel<K>, dim3(nb), dim3(256), 0, s, key, (int)n, (const int*)l.start, l.cursor, l.list);
    hipLaunchKernelGGL(det_sort_small_kernel, dim3((unsigned)cdiv(D, 4)), dim3(256), 0, s, (const int*)l.start, l.list, (int)D);
    hipLaunchKernelGGL(det_sort_long_kernel, dim3((unsigned)l.long_bound), dim3(256), 0, s, (const int*)l.start, (const int*)l.lstart, l.list, (int)D,
                       (int)n);
    const unsigned cg = (unsigned)cdiv(E, 256);
    hipLaunchKernelGGL(det_sum_kernel<V>, dim3((unsigned)l.unit_bound, cg), dim3(256), 0, s, val, (const int*)l.start, (const int*)l.ustart,
                       (const int*)l.pstart, (const int*)l.list, l.part, (int)D, E);
    if (l.pslots > 0)
        hipLaunchKernelGGL(det_finish_kernel<V>, dim3((unsigned)l.long_bound, cg), dim3(256), 0, s, val, (const int*)l.start, (const int*)l.pstart,
                           (const int*)l.lstart, (const float*)l.part, (int)D, E);
    return check_launch(what);
}

// ---- sumsq: a thread owns groups of four consecutive elements (float4 loads when aligned; the same sums, contraction off, either way) ----
constexpr int SQ_BLOCKS = 512;
inline int sumsq_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), SQ_BLOCKS)); }
template <bool VEC>
__global__ __launch_bounds__(256) void det_sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ float sm[16];
    float acc = 0.f;
    const int64_t groups = (n + 3) / 4, stride = (int64_t)gridDim.x * blockDim.x;
#pragma unroll 4
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
        float4 x;
        if (VEC && 4 * q + 4 <= n) x = *reinterpret_cast<const float4*>(g + 4 * q);
        else {
            const int64_t e = 4 * q;
            x.x = g[e];
            x.y = e + 1 < n ? g[e + 1] : 0.f;
            x.z = e + 2 < n ? g[e + 2] : 0.f;
            x.w = e + 3 < n ? g[e + 3] : 0.f;
        }
        acc += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void det_sumsq_finish_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ float sm[16];
    float acc = 0.f;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) acc += part[b];
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) out[0] += acc;
}

}  // namespace

int det_embed_bwd(const float* table, const int64_t* tok, int64_t tok_stride, const uint8_t* keep, float keep_scale, const float* dout,
                  float* dtable, int n, int E, int vocab_rows, void* workspace, size_t ws_bytes, hipStream_t s) {
    return det_scatter(EmbedKey{tok, tok_stride, vocab_rows}, EmbedVal{table, keep, keep_scale, dout, dtable, E}, n, vocab_rows, E, workspace,
                       ws_bytes, s, "subgc_embed_bwd_ws");
}
int det_scatter_add_rows(const float* src, int64_t lds, const int32_t* rows, float* dX, int64_t ldx, int M, int L, const int32_t* m_dev,
                         int x_rows, void* workspace, size_t ws_bytes, hipStream_t s) {
    return det_scatter(RowKey{rows, m_dev, x_rows}, RowVal{src, lds, dX, ldx}, M, x_rows, L, workspace, ws_bytes, s, "subgc_scatter_add_rows_ws");
}
int det_pool_bwd(const float* dout, const int64_t* idx, int64_t idx_stride, const float* w, int64_t w_g, int64_t w_i, const float* denom,
                 const int32_t* img, const int32_t* argmax, float* dX, int G, int N, int L, int x_rows, void* workspace, size_t ws_bytes,
                 hipStream_t s) {
    return det_scatter(PoolKey{idx, idx_stride, w, w_g, w_i, img, N, x_rows}, PoolVal{dout, denom, argmax, w, w_g, w_i, dX, N, L}, (int64_t)G * N,
                       x_rows, L, workspace, ws_bytes, s, "subgc_subgraph_pool_bwd_ws");
}
int det_sumsq(const float* g, int64_t n, float* sumsq, void* workspace, size_t ws_bytes, hipStream_t s) {
    const int nb = sumsq_blocks(n);
    const size_t need = (size_t)nb * sizeof(float);
    SUBGC_REQUIRE(workspace && ws_bytes >= need, "subgc_sumsq_f32_ws: deterministic mode needs %zu bytes of workspace (got %zu)", need,
                  workspace ? ws_bytes : (size_t)0);
    float* part = static_cast<float*>(workspace);
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) hipLaunchKernelGGL(det_sumsq_kernel<true>, dim3(nb), dim3(256), 0, s, g, n, part);
    else hipLaunchKernelGGL(det_sumsq_kernel<false>, dim3(nb), dim3(256), 0, s, g, n, part);
    hipLaunchKernelGGL(det_sumsq_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)part, nb, sumsq);
    return check_launch("subgc_sumsq_f32_ws");
}

}  // namespace subgc
