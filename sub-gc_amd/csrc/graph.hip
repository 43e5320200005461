// Scene-graph kernels: class arg-max, CSR build, the unfused BatchNorm, the aggregate-first pair (the GCN neighbour aggregation
// itself: gcn.hip).  All are HBM-bound streaming kernels: threads run along the feature dimension (coalesced rows), indices live in LDS.
//
// Reference op sites: AttModel.py:376,383,385 (argmax); gcn_backbone.py:55-67 (make_map, replaced
// by CSR); graph_conv_unit.py:28-36 (BatchNorm).
#include "common.h"
#include "bf16_util.h"
#include "gcn_lists.h"

#include <algorithm>

namespace {

// ------------------------------------------------------------------ row arg-max (first max)
__global__ __launch_bounds__(256) void row_argmax_kernel(const float* __restrict__ X, int64_t ldx, int rows,
                                                         int cols, int skip, int64_t* __restrict__ idx,
                                                         float* __restrict__ val, int32_t* __restrict__ idx32) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* x = X + (int64_t)row * ldx;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = skip + lane; c < cols; c += 64) {
        const float v = x[c];
        if (v > best || bi == 0x7fffffff) { best = v; bi = c; }   // strict >: first max inside a lane
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    if (lane == 0) {
        if (idx) idx[row] = bi;
        if (idx32) idx32[row] = bi;
        if (val) val[row] = best;
    }
}

// ------------------------------------------------------------------ CSR by subject / by object
// grid (B, 2 roles); thread n owns node n: counts its relations, then lists them in ascending k.
__global__ __launch_bounds__(256) void csr_build_kernel(const int64_t* __restrict__ rel_ind, int B, int K, int N,
                                                        int32_t* __restrict__ ptr, int32_t* __restrict__ edges) {
    extern __shared__ int sm_i[];
    int* node_of = sm_i;          // [K]
    int* start = sm_i + K;        // [N+1]
    const int b = blockIdx.x, role = blockIdx.y;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        int64_t v = rel_ind[((int64_t)b * K + k) * 2 + role];
        node_of[k] = (int)(v < 0 ? 0 : (v >= N ? N - 1 : v));
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        int c = 0;
        for (int k = 0; k < K; ++k) c += node_of[k] == n;
        start[n + 1] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        start[0] = 0;
        for (int n = 0; n < N; ++n) start[n + 1] += start[n];
    }
    __syncthreads();
    int32_t* p = ptr + ((int64_t)role * B + b) * (N + 1);
    int32_t* e = edges + ((int64_t)role * B + b) * K;
    for (int n = threadIdx.x; n <= N; n += blockDim.x) p[n] = start[n];
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        int pos = start[n];
        for (int k = 0; k < K; ++k)
            if (node_of[k] == n) e[pos++] = k;
    }
}

// ------------------------------------------------------------------ BatchNorm1d over rows
// column statistics: grid (C/64, slabs); 4 waves stride rows; atomics merge slabs.
__global__ __launch_bounds__(256) void bn_colsum_kernel(const float* __restrict__ X, int M, int C, const float* __restrict__ center,
                                                        float* __restrict__ sum, int square, int rows_per_block) {
    __shared__ float sm[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    const float mu = (center && col < C) ? center[col] : 0.f;
    float acc = 0.f;
    if (col < C)
        for (int r = r0 + w; r < r1; r += 4) {
            const float d = X[(int64_t)r * C + col] - mu;
            acc += square ? d * d : d;
        }
    sm[w][lane] = acc;
    __syncthreads();
    if (w == 0 && col < C) atomicAdd(sum + col, sm[0][lane] + sm[1][lane] + sm[2][lane] + sm[3][lane]);
}
// float4 form (C % 4 == 0, 16-byte aligned rows): a wave covers 256 columns of a row per load instruction (1 KB) instead of 64
// (the scalar form moved 68 MB in 39.5 us = 1.7 TB/s on the [16640, 1024] relation features of Full-GC); grid (C/256, slabs)
// part != NULL: the slab's column sums go to part[blockIdx.y][C] with plain stores and bn_finalize_kernel adds the slabs in a
// fixed order -- no zero-fill launches, no atomics (256 same-address float atomics per column from 8 XCDs were most of the
// 32 us the pass still took), and bit-reproducible statistics
__global__ __launch_bounds__(256) void bn_colsum_vec_kernel(const float* __restrict__ X, int M, int C, const float* __restrict__ center,
                                                            float* __restrict__ sum, int square, int rows_per_block, float* __restrict__ part) {
    __shared__ float4 sm[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = (blockIdx.x * 64 + lane) * 4;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < C) {
        const float4 mu = center ? *reinterpret_cast<const float4*>(center + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        int r = r0 + w;
        for (; r + 12 < r1; r += 16) {                                  // four rows in flight per wave
            float4 x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const float4*>(X + (int64_t)(r + 4 * q) * C + col);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d0 = x[q].x - mu.x, d1 = x[q].y - mu.y, d2 = x[q].z - mu.z, d3 = x[q].w - mu.w;
                if (square) { acc.x += d0 * d0; acc.y += d1 * d1; acc.z += d2 * d2; acc.w += d3 * d3; }
                else { acc.x += d0; acc.y += d1; acc.z += d2; acc.w += d3; }
            }
        }
        for (; r < r1; r += 4) {
            const float4 x = *reinterpret_cast<const float4*>(X + (int64_t)r * C + col);
            const float d0 = x.x - mu.x, d1 = x.y - mu.y, d2 = x.z - mu.z, d3 = x.w - mu.w;
            if (square) { acc.x += d0 * d0; acc.y += d1 * d1; acc.z += d2 * d2; acc.w += d3 * d3; }
            else { acc.x += d0; acc.y += d1; acc.z += d2; acc.w += d3; }
        }
    }
    sm[w][lane] = acc;
    __syncthreads();
    if (w == 0 && col < C) {
        const float4 a = sm[0][lane], b = sm[1][lane], c = sm[2][lane], d = sm[3][lane];
        const float4 t = make_float4(a.x + b.x + c.x + d.x, a.y + b.y + c.y + d.y, a.z + b.z + c.z + d.z, a.w + b.w + c.w + d.w);
        if (part) *reinterpret_cast<float4*>(part + (int64_t)blockIdx.y * C + col) = t;
        else { atomicAdd(sum + col, t.x); atomicAdd(sum + col + 1, t.y); atomicAdd(sum + col + 2, t.z); atomicAdd(sum + col + 3, t.w); }
    }
}
__global__ __launch_bounds__(256) void bn_bwd_reduce_vec_kernel(const float* __restrict__ dY, const float* __restrict__ X, int M, int C,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta, int rows_per_block,
                                                                float* __restrict__ part) {
    // part != NULL: slab sums to part[blockIdx.y][2][C] (dgamma row, dbeta row); bn_sum_slabs_kernel adds them
    __shared__ float4 sg[4][64], sb[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = (blockIdx.x * 64 + lane) * 4;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float4 ag = make_float4(0.f, 0.f, 0.f, 0.f), ab = ag;
    if (col < C) {
        const float4 mu = *reinterpret_cast<const float4*>(mean + col), rs = *reinterpret_cast<const float4*>(rstd + col);
        for (int r = r0 + w; r < r1; r += 4) {
            const float4 dy = *reinterpret_cast<const float4*>(dY + (int64_t)r * C + col);
            const float4 x = *reinterpret_cast<const float4*>(X + (int64_t)r * C + col);
            ab.x += dy.x; ab.y += dy.y; ab.z += dy.z; ab.w += dy.w;
            ag.x += dy.x * (x.x - mu.x) * rs.x; ag.y += dy.y * (x.y - mu.y) * rs.y;
            ag.z += dy.z * (x.z - mu.z) * rs.z; ag.w += dy.w * (x.w - mu.w) * rs.w;
        }
    }
    sg[w][lane] = ag; sb[w][lane] = ab;
    __syncthreads();
    if (w == 0 && col < C) {
        const float4 g0 = sg[0][lane], g1 = sg[1][lane], g2 = sg[2][lane], g3 = sg[3][lane];
        const float4 b0 = sb[0][lane], b1 = sb[1][lane], b2 = sb[2][lane], b3 = sb[3][lane];
        const float4 tg = make_float4(g0.x + g1.x + g2.x + g3.x, g0.y + g1.y + g2.y + g3.y, g0.z + g1.z + g2.z + g3.z, g0.w + g1.w + g2.w + g3.w);
        const float4 tb = make_float4(b0.x + b1.x + b2.x + b3.x, b0.y + b1.y + b2.y + b3.y, b0.z + b1.z + b2.z + b3.z, b0.w + b1.w + b2.w + b3.w);
        if (part) {
            *reinterpret_cast<float4*>(part + ((int64_t)blockIdx.y * 2 + 0) * C + col) = tg;
            *reinterpret_cast<float4*>(part + ((int64_t)blockIdx.y * 2 + 1) * C + col) = tb;
        } else {
            atomicAdd(dgamma + col, tg.x); atomicAdd(dgamma + col + 1, tg.y); atomicAdd(dgamma + col + 2, tg.z); atomicAdd(dgamma + col + 3, tg.w);
            atomicAdd(dbeta + col, tb.x); atomicAdd(dbeta + col + 1, tb.y); atomicAdd(dbeta + col + 2, tb.z); atomicAdd(dbeta + col + 3, tb.w);
        }
    }
}
// column c of vector j: sum over slabs of part[slab][j][c] in a fixed order.  256 threads = 64 columns x 4 waves, wave w adds
// slabs w, w+4, ... eight loads at a time, LDS combines the four; every thread of the column's lane gets the total.
__device__ __forceinline__ float bn_slab_sum(const float* __restrict__ part, int slabs, int nvec, int j, int C, int c, float (*sm)[64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float s = 0.f;
    if (c < C) {
        int k = w;
        for (; k + 28 < slabs; k += 32) {
            float x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = part[((int64_t)(k + 4 * q) * nvec + j) * C + c];
#pragma unroll
            for (int q = 0; q < 8; ++q) s += x[q];
        }
        for (; k < slabs; k += 4) s += part[((int64_t)k * nvec + j) * C + c];
    }
    __syncthreads();
    sm[w][lane] = s;
    __syncthreads();
    return sm[0][lane] + sm[1][lane] + sm[2][lane] + sm[3][lane];
}
// grid C/64 x 256 threads: out0 / out1 [C] = the two summed vectors of the backward (dgamma, dbeta)
__global__ __launch_bounds__(256) void bn_sum_slabs_kernel(const float* __restrict__ part, int slabs, int C, float* __restrict__ out0,
                                                           float* __restrict__ out1) {
    __shared__ float sm[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const float a = bn_slab_sum(part, slabs, 2, 0, C, c, sm), b = bn_slab_sum(part, slabs, 2, 1, C, c, sm);
    if (threadIdx.x < 64 && c < C) { out0[c] = a; out1[c] = b; }
}
// finalise: mean = s/M (pass 0)  |  var -> rstd, running stats (pass 1)
__global__ __launch_bounds__(256) void bn_finalize_kernel(float* __restrict__ mean_or_var, int M, int C, int pass, float* __restrict__ save_mean,
                                                          float* __restrict__ save_rstd, float* __restrict__ running_mean,
                                                          float* __restrict__ running_var, float momentum, float eps,
                                                          const float* __restrict__ part, int slabs) {
    // part == NULL: grid C/256, thread per column, the sums are in mean_or_var (atomic path)
    // part != NULL: grid C/64, 64 columns x 4 waves: the column sums arrive as per-slab partials (bn_slab_sum)
    __shared__ float sm[4][64];
    int c;
    if (part) {
        c = blockIdx.x * 64 + (threadIdx.x & 63);
        const float tot = bn_slab_sum(part, slabs, 1, 0, C, c, sm);
        if (threadIdx.x >= 64 || c >= C) return;
        mean_or_var[c] = tot;
    } else {
        c = blockIdx.x * blockDim.x + threadIdx.x;
        if (c >= C) return;
    }
    if (pass == 0) {
        const float m = mean_or_var[c] / (float)M;
        save_mean[c] = m;
        if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    } else {
        const float ss = mean_or_var[c];
        const float var_b = ss / (float)M;
        save_rstd[c] = 1.f / sqrtf(var_b + eps);
        if (running_var) {
            const float var_u = M > 1 ? ss / (float)(M - 1) : var_b;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * var_u;
        }
    }
}
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ X, float* __restrict__ Y, int64_t total, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ rvar, float eps,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float rs = rstd ? rstd[c] : 1.f / sqrtf(rvar[c] + eps);
        Y[i] = (X[i] - mean[c]) * rs * gamma[c] + beta[c];
    }
}
// backward pass 1: dbeta = sum dy, dgamma = sum dy * xhat
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ dY, const float* __restrict__ X, int M, int C,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            int rows_per_block) {
    __shared__ float sg[4][64], sb[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float ag = 0.f, ab = 0.f;
    if (col < C) {
        const float mu = mean[col], rs = rstd[col];
        for (int r = r0 + w; r < r1; r += 4) {
            const float dy = dY[(int64_t)r * C + col];
            ab += dy;
            ag += dy * (X[(int64_t)r * C + col] - mu) * rs;
        }
    }
    sg[w][lane] = ag; sb[w][lane] = ab;
    __syncthreads();
    if (w == 0 && col < C) {
        atomicAdd(dgamma + col, sg[0][lane] + sg[1][lane] + sg[2][lane] + sg[3][lane]);
        atomicAdd(dbeta + col, sb[0][lane] + sb[1][lane] + sb[2][lane] + sb[3][lane]);
    }
}
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dY, const float* __restrict__ X, float* __restrict__ dX,
                                                           int64_t total, int M, int C, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ dgamma, const float* __restrict__ dbeta) {
    const float invM = 1.f / (float)M;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float xh = (X[i] - mean[c]) * rstd[c];
        dX[i] = gamma[c] * rstd[c] * (dY[i] - dbeta[c] * invM - xh * dgamma[c] * invM);
    }
}
// deterministic mode: the two column reductions in ONE source for every alignment -- VEC = a lane owns four adjacent columns (float4 loads),
// otherwise one; each column's arithmetic is the same scalar code with contraction off (no FMA in either form), rows in the order wave w:
// r0 + w, r0 + w + 4, ..., waves added 0 + 1 + 2 + 3; the slab sums go to the partials bn_finalize_kernel / bn_sum_slabs_kernel add in order
template <bool VEC>
__global__ __launch_bounds__(256) void bn_colsum_det_kernel(const float* __restrict__ X, int M, int C, const float* __restrict__ center, int square,
                                                            int rows_per_block, float* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 4 : 1;
    __shared__ float sm[4][64][V];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = (blockIdx.x * 64 + lane) * V;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float acc[V], mu[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { acc[k] = 0.f; mu[k] = (center && col < C) ? center[col + k] : 0.f; }
    if (col < C)
        for (int r = r0 + w; r < r1; r += 4) {
            float x[V];
            if (VEC) { const float4 t = *reinterpret_cast<const float4*>(X + (int64_t)r * C + col); x[0] = t.x; x[1 % V] = t.y; x[2 % V] = t.z; x[3 % V] = t.w; }
            else x[0] = X[(int64_t)r * C + col];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float d = x[k] - mu[k];
                acc[k] = square ? acc[k] + d * d : acc[k] + d;
            }
        }
#pragma unroll
    for (int k = 0; k < V; ++k) sm[w][lane][k] = acc[k];
    __syncthreads();
    if (w == 0 && col < C)
#pragma unroll
        for (int k = 0; k < V; ++k) part[(int64_t)blockIdx.y * C + col + k] = sm[0][lane][k] + sm[1][lane][k] + sm[2][lane][k] + sm[3][lane][k];
}
template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_reduce_det_kernel(const float* __restrict__ dY, const float* __restrict__ X, int M, int C,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd, int rows_per_block,
                                                                float* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 4 : 1;
    __shared__ float sg[4][64][V], sb[4][64][V];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = (blockIdx.x * 64 + lane) * V;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float ag[V], ab[V], mu[V], rs[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { ag[k] = 0.f; ab[k] = 0.f; mu[k] = col < C ? mean[col + k] : 0.f; rs[k] = col < C ? rstd[col + k] : 0.f; }
    if (col < C)
        for (int r = r0 + w; r < r1; r += 4) {
            float dy[V], x[V];
            if (VEC) {
                const float4 a = *reinterpret_cast<const float4*>(dY + (int64_t)r * C + col), b = *reinterpret_cast<const float4*>(X + (int64_t)r * C + col);
                dy[0] = a.x; dy[1 % V] = a.y; dy[2 % V] = a.z; dy[3 % V] = a.w;
                x[0] = b.x; x[1 % V] = b.y; x[2 % V] = b.z; x[3 % V] = b.w;
            } else { dy[0] = dY[(int64_t)r * C + col]; x[0] = X[(int64_t)r * C + col]; }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                ab[k] = ab[k] + dy[k];
                const float t = dy[k] * (x[k] - mu[k]);
                ag[k] = ag[k] + t * rs[k];
            }
        }
#pragma unroll
    for (int k = 0; k < V; ++k) { sg[w][lane][k] = ag[k]; sb[w][lane][k] = ab[k]; }
    __syncthreads();
    if (w == 0 && col < C)
#pragma unroll
        for (int k = 0; k < V; ++k) {
            part[((int64_t)blockIdx.y * 2 + 0) * C + col + k] = sg[0][lane][k] + sg[1][lane][k] + sg[2][lane][k] + sg[3][lane][k];
            part[((int64_t)blockIdx.y * 2 + 1) * C + col + k] = sb[0][lane][k] + sb[1][lane][k] + sb[2][lane][k] + sb[3][lane][k];
        }
}
__global__ void zero_f32_kernel(float* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0.f;
}

inline bool bn_vec_ok(int C, const void* a, const void* b, const void* c) {
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return C % 4 == 0 && al(a) && al(b) && al(c);
}
// rows per workgroup of the float4 column reductions: ~512 workgroups (2 per CU) however tall the matrix is
inline int bn_rows_per_block(int M, int C) {
    const int col_groups = (C + 255) / 256;
    const int slabs = std::max(1, 512 / col_groups);
    return std::max(16, (M + slabs - 1) / slabs);
}

}  // namespace

SUBGC_API int subgc_row_argmax_f32(const float* X, int64_t ldx, int rows, int cols, int skip, int64_t* idx, float* val,
                                   void* stream) {
    SUBGC_REQUIRE(rows >= 0 && cols > skip && skip >= 0 && ldx >= cols, "row_argmax: bad sizes rows=%d cols=%d skip=%d", rows, cols, skip);
    if (rows == 0) return SUBGC_OK;
    SUBGC_REQUIRE(X && idx, "row_argmax: null pointer");
    hipLaunchKernelGGL(row_argmax_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, ldx, rows, cols, skip, idx, val, (int32_t*)nullptr);
    return subgc::check_launch("subgc_row_argmax_f32");
}
SUBGC_API int subgc_row_argmax_i32(const float* X, int64_t ldx, int rows, int cols, int skip, int32_t* idx, void* stream) {
    SUBGC_REQUIRE(rows >= 0 && cols > skip && skip >= 0 && ldx >= cols, "row_argmax: bad sizes rows=%d cols=%d skip=%d", rows, cols, skip);
    if (rows == 0) return SUBGC_OK;
    SUBGC_REQUIRE(X && idx, "row_argmax: null pointer");
    hipLaunchKernelGGL(row_argmax_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, ldx, rows, cols, skip, (int64_t*)nullptr,
                       (float*)nullptr, idx);
    return subgc::check_launch("subgc_row_argmax_i32");
}

SUBGC_API int subgc_csr_build(const int64_t* rel_ind, int B, int K, int N, int32_t* ptr, int32_t* edges, void* stream) {
    SUBGC_REQUIRE(B >= 0 && K > 0 && N > 0, "csr_build: bad sizes");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(rel_ind && ptr && edges, "csr_build: null pointer");
    SUBGC_DEBUG_RANGE(rel_ind, 8, (int64_t)B * K, 2, 2, 0, N - 1, -1, "csr_build: rel_ind (node ids of the relations)", stream);
    const size_t lds = sizeof(int) * (K + N + 1);
    hipLaunchKernelGGL(csr_build_kernel, dim3(B, 2), dim3(128), lds, (hipStream_t)stream, rel_ind, B, K, N, ptr, edges);
    return subgc::check_launch("subgc_csr_build");
}

SUBGC_API int subgc_bn_fwd(const float* X, float* Y, int M, int C, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float* save_mean, float* save_rstd, int training, float momentum, float eps,
                           void* workspace, size_t ws_bytes, void* stream) {
    SUBGC_REQUIRE(M > 0 && C > 0, "bn_fwd: bad sizes");
    SUBGC_REQUIRE(X && Y && gamma && beta, "bn_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)M * C;
    const int ew_blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
    if (!training) {
        SUBGC_REQUIRE(running_mean && running_var, "bn_fwd(eval): running stats required");
        hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_blocks), dim3(256), 0, s, X, Y, total, C, running_mean, (const float*)nullptr,
                           running_var, eps, gamma, beta);
        return subgc::check_launch("subgc_bn_fwd");
    }
    SUBGC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "bn_fwd: workspace must be 16-byte aligned");
    SUBGC_REQUIRE(save_mean && save_rstd, "bn_fwd(train): save buffers required");
    const bool vec = bn_vec_ok(C, X, save_mean, save_rstd);
    const bool det = subgc::deterministic();         // slabs from the shape alone, always summed in order (no atomics)
    const int rpb = vec || det ? bn_rows_per_block(M, C) : 512;
    dim3 g(vec ? (C + 255) / 256 : (C + 63) / 64, (M + rpb - 1) / rpb);
    float* part = vec && workspace && ws_bytes >= (size_t)g.y * C * sizeof(float) ? static_cast<float*>(workspace) : nullptr;
    if (det) {
        const size_t need = (size_t)g.y * C * sizeof(float);
        SUBGC_REQUIRE(workspace && ws_bytes >= need, "subgc_bn_fwd: deterministic mode needs %zu bytes of workspace (got %zu)", need,
                      workspace ? ws_bytes : (size_t)0);
        part = static_cast<float*>(workspace);
    }
    if (!part) {
        hipLaunchKernelGGL(zero_f32_kernel, dim3((C + 255) / 256), dim3(256), 0, s, save_mean, (int64_t)C);
        hipLaunchKernelGGL(zero_f32_kernel, dim3((C + 255) / 256), dim3(256), 0, s, save_rstd, (int64_t)C);
    }
    if (det && vec) hipLaunchKernelGGL(bn_colsum_det_kernel<true>, g, dim3(256), 0, s, X, M, C, (const float*)nullptr, 0, rpb, part);
    else if (det) hipLaunchKernelGGL(bn_colsum_det_kernel<false>, g, dim3(256), 0, s, X, M, C, (const float*)nullptr, 0, rpb, part);
    else if (vec) hipLaunchKernelGGL(bn_colsum_vec_kernel, g, dim3(256), 0, s, X, M, C, (const float*)nullptr, save_mean, 0, rpb, part);
    else hipLaunchKernelGGL(bn_colsum_kernel, g, dim3(256), 0, s, X, M, C, (const float*)nullptr, save_mean, 0, rpb);
    const dim3 fg(part ? (C + 63) / 64 : (C + 255) / 256);
    hipLaunchKernelGGL(bn_finalize_kernel, fg, dim3(256), 0, s, save_mean, M, C, 0, save_mean, save_rstd,
                       running_mean, running_var, momentum, eps, (const float*)part, (int)g.y);
    if (det && vec) hipLaunchKernelGGL(bn_colsum_det_kernel<true>, g, dim3(256), 0, s, X, M, C, (const float*)save_mean, 1, rpb, part);
    else if (det) hipLaunchKernelGGL(bn_colsum_det_kernel<false>, g, dim3(256), 0, s, X, M, C, (const float*)save_mean, 1, rpb, part);
    else if (vec) hipLaunchKernelGGL(bn_colsum_vec_kernel, g, dim3(256), 0, s, X, M, C, (const float*)save_mean, save_rstd, 1, rpb, part);
    else hipLaunchKernelGGL(bn_colsum_kernel, g, dim3(256), 0, s, X, M, C, (const float*)save_mean, save_rstd, 1, rpb);
    hipLaunchKernelGGL(bn_finalize_kernel, fg, dim3(256), 0, s, save_rstd, M, C, 1, save_mean, save_rstd,
                       running_mean, running_var, momentum, eps, (const float*)part, (int)g.y);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_blocks), dim3(256), 0, s, X, Y, total, C, (const float*)save_mean,
                       (const float*)save_rstd, (const float*)nullptr, eps, gamma, beta);
    return subgc::check_launch("subgc_bn_fwd");
}

SUBGC_API int subgc_bn_bwd(const float* dY, const float* X, const float* gamma, const float* save_mean, const float* save_rstd,
                           float* dX, float* dgamma, float* dbeta, int M, int C, void* workspace, size_t ws_bytes, void* stream) {
    SUBGC_REQUIRE(M > 0 && C > 0, "bn_bwd: bad sizes");
    SUBGC_REQUIRE(dY && X && gamma && save_mean && save_rstd && dX && dgamma && dbeta, "bn_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)M * C;
    const bool det = subgc::deterministic();
    const bool vec = bn_vec_ok(C, X, dY, save_mean) && bn_vec_ok(C, save_rstd, dgamma, dbeta) &&
                     (!det || (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
    const int rpb = vec || det ? bn_rows_per_block(M, C) : 512;
    dim3 g(vec ? (C + 255) / 256 : (C + 63) / 64, (M + rpb - 1) / rpb);
    float* part = vec && workspace && ws_bytes >= (size_t)g.y * 2 * C * sizeof(float) ? static_cast<float*>(workspace) : nullptr;
    if (det) {
        const size_t need = (size_t)g.y * 2 * C * sizeof(float);
        SUBGC_REQUIRE(workspace && ws_bytes >= need, "subgc_bn_bwd: deterministic mode needs %zu bytes of workspace (got %zu)", need,
                      workspace ? ws_bytes : (size_t)0);
        part = static_cast<float*>(workspace);
    }
    if (!part) {
        hipLaunchKernelGGL(zero_f32_kernel, dim3((C + 255) / 256), dim3(256), 0, s, dgamma, (int64_t)C);
        hipLaunchKernelGGL(zero_f32_kernel, dim3((C + 255) / 256), dim3(256), 0, s, dbeta, (int64_t)C);
    }
    if (det && vec) hipLaunchKernelGGL(bn_bwd_reduce_det_kernel<true>, g, dim3(256), 0, s, dY, X, M, C, save_mean, save_rstd, rpb, part);
    else if (det) hipLaunchKernelGGL(bn_bwd_reduce_det_kernel<false>, g, dim3(256), 0, s, dY, X, M, C, save_mean, save_rstd, rpb, part);
    else if (vec) hipLaunchKernelGGL(bn_bwd_reduce_vec_kernel, g, dim3(256), 0, s, dY, X, M, C, save_mean, save_rstd, dgamma, dbeta, rpb, part);
    else hipLaunchKernelGGL(bn_bwd_reduce_kernel, g, dim3(256), 0, s, dY, X, M, C, save_mean, save_rstd, dgamma, dbeta, rpb);
    if (part) hipLaunchKernelGGL(bn_sum_slabs_kernel, dim3((C + 63) / 64), dim3(256), 0, s, (const float*)part, (int)g.y, C, dgamma, dbeta);
    const int ew_blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_blocks), dim3(256), 0, s, dY, X, dX, total, M, C, save_mean, save_rstd, gamma,
                       (const float*)dgamma, (const float*)dbeta);
    return subgc::check_launch("subgc_bn_bwd");
}

// ------------------------------------------------------------------ aggregate first (include/subgc_gcn_agg_hip.h)
// Collection units without BatchNorm are linear in front of their ReLU, so the 0/1 map is applied to the SOURCE rows and the two Linear
// layers run on the (fewer) target rows.  gcn_agg_fwd_kernel is the gather of gcn_nodes_fwd_f4_kernel (CSR lists in LDS, float4 rows, four
// rows of each role requested at a time) without its ReLU / role-average / residual epilogue: both roles read the SAME source X.
#include "../../include/subgc_gcn_agg_hip.h"

namespace {

__global__ __launch_bounds__(256) void gcn_agg_fwd_kernel(const float* __restrict__ X, const int32_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ edges, float* __restrict__ A0, float* __restrict__ A1,
                                                          float* __restrict__ s0, float* __restrict__ s1, int B, int N, int K, int L) {
    extern __shared__ int sm_i[];
    int *ps, *po, *es, *eo;
    const int b = blockIdx.y;
    gcn_stage_csr(sm_i, ptr, edges, b, B, N, K, ps, po, es, eo);
    __syncthreads();
    const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
    const float* x = X + (int64_t)b * K * L + col;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const int c0 = ps[n + 1] - ps[n], c1 = po[n + 1] - po[n];
        const float d0 = (float)c0 + 1e-7f, d1 = (float)c1 + 1e-7f;
        if (blockIdx.x == 0 && threadIdx.x == 0) {                        // the bias scale of the row: rowsum(A) under the same normalisation
            s0[(int64_t)b * N + n] = 0.5f * (float)c0 / d0;
            s1[(int64_t)b * N + n] = 0.5f * (float)c1 / d1;
        }
        if (col >= L) continue;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
        auto row = [&](int e) { return *reinterpret_cast<const float4*>(x + (int64_t)e * L); };
        gather_pair(es, ps[n], ps[n + 1], row, eo, po[n], po[n + 1], row, a, c);
        const int64_t o = ((int64_t)b * N + n) * L + col;
        *reinterpret_cast<float4*>(A0 + o) = make_float4(a.x / d0 * 0.5f, a.y / d0 * 0.5f, a.z / d0 * 0.5f, a.w / d0 * 0.5f);
        *reinterpret_cast<float4*>(A1 + o) = make_float4(c.x / d1 * 0.5f, c.y / d1 * 0.5f, c.z / d1 * 0.5f, c.w / d1 * 0.5f);
    }
}

// dX[b,k,:] (+)= w0[s_k] dA0[b,s_k,:] + w1[o_k] dA1[b,o_k,:]: one subject and one object per relation -- a gather, no atomics
__global__ __launch_bounds__(256) void gcn_agg_bwd_kernel(const float* __restrict__ dA0, const float* __restrict__ dA1,
                                                          const int64_t* __restrict__ rel_ind, const int32_t* __restrict__ ptr,
                                                          float* __restrict__ dX, int accumulate, int B, int N, int K, int L) {
    extern __shared__ int sm_i[];
    int* ns = sm_i; int* no = ns + K;
    float* w0 = reinterpret_cast<float*>(no + K); float* w1 = w0 + N;
    const int b = blockIdx.y;
    gcn_stage_rel_nodes(rel_ind, ptr, b, B, N, K, ns, no, w0, w1);         // w = cnt + 1e-7, each thread its own nodes ...
    for (int n = threadIdx.x; n < N; n += blockDim.x) {                    // ... which it turns into the weights 0.5 / (cnt + 1e-7)
        w0[n] = 0.5f / w0[n];
        w1[n] = 0.5f / w1[n];
    }
    __syncthreads();
    const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (col >= L) return;
    const int kz = gridDim.z;
    for (int k0 = blockIdx.z; k0 < K; k0 += 4 * kz) {                      // four relations' target rows requested before the first is used
        float4 xs[4], xo[4], old[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * kz;
            if (k < K) {
                xs[u] = *reinterpret_cast<const float4*>(dA0 + ((int64_t)b * N + ns[k]) * L + col);
                xo[u] = *reinterpret_cast<const float4*>(dA1 + ((int64_t)b * N + no[k]) * L + col);
                if (accumulate) old[u] = *reinterpret_cast<const float4*>(dX + ((int64_t)b * K + k) * L + col);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * kz;
            if (k < K) {
                const float a = w0[ns[k]], c = w1[no[k]];
                float4 v = make_float4(a * xs[u].x + c * xo[u].x, a * xs[u].y + c * xo[u].y, a * xs[u].z + c * xo[u].z, a * xs[u].w + c * xo[u].w);
                if (accumulate) { v.x += old[u].x; v.y += old[u].y; v.z += old[u].z; v.w += old[u].w; }
                *reinterpret_cast<float4*>(dX + ((int64_t)b * K + k) * L + col) = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void gcn_agg_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y0, const float* __restrict__ y1,
                                                               float* __restrict__ dz0, float* __restrict__ dz1, int64_t n, int vec) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        for (int64_t i = i0; i < n / 4; i += step) {
            const float4 g = reinterpret_cast<const float4*>(dy)[i], a = reinterpret_cast<const float4*>(y0)[i], c = reinterpret_cast<const float4*>(y1)[i];
            reinterpret_cast<float4*>(dz0)[i] = make_float4(a.x > 0.f ? g.x : 0.f, a.y > 0.f ? g.y : 0.f, a.z > 0.f ? g.z : 0.f, a.w > 0.f ? g.w : 0.f);
            reinterpret_cast<float4*>(dz1)[i] = make_float4(c.x > 0.f ? g.x : 0.f, c.y > 0.f ? g.y : 0.f, c.z > 0.f ? g.z : 0.f, c.w > 0.f ? g.w : 0.f);
        }
        return;
    }
    for (int64_t i = i0; i < n; i += step) {
        dz0[i] = y0[i] > 0.f ? dy[i] : 0.f;
        dz1[i] = y1[i] > 0.f ? dy[i] : 0.f;
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

SUBGC_API int subgc_gcn_agg_fwd(const float* X, const int32_t* ptr, const int32_t* edges, float* Xagg0, float* Xagg1, float* s0, float* s1,
                                int B, int N, int K, int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0 && L % 4 == 0, "gcn_agg_fwd: bad sizes (L must be a multiple of 4)");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(X && ptr && edges && Xagg0 && Xagg1 && s0 && s1, "gcn_agg_fwd: null pointer");
    SUBGC_REQUIRE(al16(X) && al16(Xagg0) && al16(Xagg1), "gcn_agg_fwd: rows must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    subgc::ProfScope prof(SUBGC_FAM_GCN, s, 4.0 * B * L * (2.0 * K + 2.0 * N));
    const size_t lds = sizeof(int) * (2 * (N + 1) + 2 * K);
    const int cg = (L / 4 + 255) / 256;
    hipLaunchKernelGGL(gcn_agg_fwd_kernel, dim3(cg, B, subgc::gcn_zsplit(cg, B, N)), dim3(256), lds, s, X, ptr, edges, Xagg0, Xagg1, s0, s1, B, N, K, L);
    return subgc::check_launch("subgc_gcn_agg_fwd");
}

SUBGC_API int subgc_gcn_agg_bwd(const float* dXagg0, const float* dXagg1, const int64_t* rel_ind, const int32_t* ptr, float* dX, int accumulate,
                                int B, int N, int K, int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0 && L % 4 == 0, "gcn_agg_bwd: bad sizes (L must be a multiple of 4)");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(dXagg0 && dXagg1 && rel_ind && ptr && dX, "gcn_agg_bwd: null pointer");
    SUBGC_REQUIRE(al16(dXagg0) && al16(dXagg1) && al16(dX), "gcn_agg_bwd: rows must be 16-byte aligned");
    SUBGC_DEBUG_RANGE(rel_ind, 8, (int64_t)B * K, 2, 2, 0, N - 1, -1, "gcn_agg_bwd: rel_ind", stream);
    hipStream_t s = (hipStream_t)stream;
    subgc::ProfScope prof(SUBGC_FAM_GCN, s, 4.0 * B * L * (2.0 * K + (accumulate ? 2.0 : 1.0) * K));
    const size_t lds = sizeof(int) * (2 * K) + sizeof(float) * 2 * N;
    const int cg = (L / 4 + 255) / 256;
    hipLaunchKernelGGL(gcn_agg_bwd_kernel, dim3(cg, B, subgc::gcn_zsplit(cg, B, (K + 3) / 4)), dim3(256), lds, s, dXagg0, dXagg1, rel_ind, ptr, dX,
                       accumulate ? 1 : 0, B, N, K, L);
    return subgc::check_launch("subgc_gcn_agg_bwd");
}

SUBGC_API int subgc_gcn_agg_relu_bwd(const float* dy, const float* y0, const float* y1, float* dz0, float* dz1, int64_t n, void* stream) {
    SUBGC_REQUIRE(n >= 0, "gcn_agg_relu_bwd: bad size");
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(dy && y0 && y1 && dz0 && dz1, "gcn_agg_relu_bwd: null pointer");
    const int vec = n % 4 == 0 && al16(dy) && al16(y0) && al16(y1) && al16(dz0) && al16(dz1);
    const int64_t items = vec ? n / 4 : n;
    hipLaunchKernelGGL(gcn_agg_relu_bwd_kernel, dim3((unsigned)std::min<int64_t>((items + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, dy, y0, y1,
                       dz0, dz1, n, vec);
    return subgc::check_launch("subgc_gcn_agg_relu_bwd");
}
