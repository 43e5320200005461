// BatchNorm1d of the Full-GC collection units (graph_conv_unit.py:31-32, nn.BatchNorm1d(dim) on the [rows, L] unit outputs)
// FUSED into the GCN aggregation kernels that consume it (gcn.hip; graph_conv_unit.py:34-36, graph_conv.py:26,33):
//   forward   ONE pass over the raw unit output y computes the batch statistics (per-slab shifted sums, merged with Chan's
//             formula in double), a finishing launch turns them into the per-column triple {mean, gamma * rstd, beta} and updates
//             the running statistics; the aggregation kernels apply (y - mean) * scale + beta ON LOAD -- the normalised tensor is
//             never written (was: two statistics passes + normalise = 3 reads + 1 write of y and 5 launches);
//   backward  the aggregation backward yields d(normalised); ONE reduce launch leaves per-slab {sum dy * xhat, sum dy}, ONE apply
//             launch adds the slabs in a fixed order and writes d(y) in y's storage type (bf16 when y is a bf16 GEMM result, so the
//             producing Linear's backward needs no cast pass) and d(gamma), d(beta) straight into their gradient slots.
// y may be fp32 or bf16 (SRC16): under compute_dtype = bf16 the unit's second GEMM writes bf16 only.
// All kernels are HBM-bound streams over [rows, L] with L % 4 == 0: a lane owns four adjacent columns (16-byte / 8-byte accesses).
#include "common.h"
#include "bf16_util.h"

#include <algorithm>

namespace {

// ------------------------------------------------------------------ statistics
// grid (C/256, slabs): part[slab][{sum (x - p), sum (x - p)^2, p}][C], p = the slab's first row (shifted-data sums)
template <bool SRC16>
__device__ __forceinline__ void bn_stats_body(const void* __restrict__ X, int M, int C, int rpb, float* __restrict__ part) {
    __shared__ float4 ss[4][64], sq[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = (blockIdx.x * 64 + lane) * 4;
    const int r0 = blockIdx.y * rpb, r1 = min(M, r0 + rpb);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s, p = s;
    if (col < C) {
        p = subgc_load4<SRC16>(X, (int64_t)r0 * C + col);
        int r = r0 + w;
        for (; r + 12 < r1; r += 16) {
            float4 x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = subgc_load4<SRC16>(X, (int64_t)(r + 4 * k) * C + col);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d0 = x[k].x - p.x, d1 = x[k].y - p.y, d2 = x[k].z - p.z, d3 = x[k].w - p.w;
                s.x += d0; s.y += d1; s.z += d2; s.w += d3;
                q.x += d0 * d0; q.y += d1 * d1; q.z += d2 * d2; q.w += d3 * d3;
            }
        }
        for (; r < r1; r += 4) {
            const float4 x = subgc_load4<SRC16>(X, (int64_t)r * C + col);
            const float d0 = x.x - p.x, d1 = x.y - p.y, d2 = x.z - p.z, d3 = x.w - p.w;
            s.x += d0; s.y += d1; s.z += d2; s.w += d3;
            q.x += d0 * d0; q.y += d1 * d1; q.z += d2 * d2; q.w += d3 * d3;
        }
    }
    ss[w][lane] = s; sq[w][lane] = q;
    __syncthreads();
    if (w == 0 && col < C) {
        const float4 a0 = ss[0][lane], a1 = ss[1][lane], a2 = ss[2][lane], a3 = ss[3][lane];
        const float4 b0 = sq[0][lane], b1 = sq[1][lane], b2 = sq[2][lane], b3 = sq[3][lane];
        float* o = part + (int64_t)blockIdx.y * 3 * C + col;
        *reinterpret_cast<float4*>(o) = make_float4(a0.x + a1.x + a2.x + a3.x, a0.y + a1.y + a2.y + a3.y, a0.z + a1.z + a2.z + a3.z, a0.w + a1.w + a2.w + a3.w);
        *reinterpret_cast<float4*>(o + C) = make_float4(b0.x + b1.x + b2.x + b3.x, b0.y + b1.y + b2.y + b3.y, b0.z + b1.z + b2.z + b3.z, b0.w + b1.w + b2.w + b3.w);
        *reinterpret_cast<float4*>(o + 2 * C) = p;
    }
}
template <bool SRC16>
__global__ __launch_bounds__(256) void bn_stats_kernel(const void* __restrict__ X, int M, int C, int rpb, float* __restrict__ part) {
    bn_stats_body<SRC16>(X, M, C, rpb, part);
}
// the two units of a GCN pair in one launch (blockIdx.z = unit; its slab partials at part + z * slabs * 3 C)
struct BnPair { const void* X[2]; const float* gamma[2]; const float* beta[2]; float* rmean[2]; float* rvar[2]; float* aff[2]; float* rstd[2]; };
template <bool SRC16>
__global__ __launch_bounds__(256) void bn_stats_pair_kernel(BnPair a, int M, int C, int rpb, float* __restrict__ part, int slabs) {
    bn_stats_body<SRC16>(a.X[blockIdx.z], M, C, rpb, part + (size_t)blockIdx.z * slabs * 3 * C);
}
// grid C/64 x 1024 threads: wave w takes slabs w, w+16, ...  Two sweeps over the (L2-resident) partials, no division in the loops:
// the batch mean from the slab means, then M2 = sum_k [M2_k + n_k (mean_k - mean)^2] (Chan's formula for many groups), in double.
// A sweep requests FIN_U slabs' partials before it consumes any: with one load in flight per wave the kernel was a chain of L2
// latencies (128 slabs, 4 waves: 23.7 us -- 3.5 x the pass over the data it finishes).
constexpr int FIN_WAVES = 16, FIN_U = 8;
__device__ __forceinline__ void bn_stats_finish_body(const float* __restrict__ part, int slabs, int rpb, int M, int C,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* __restrict__ running_mean, float* __restrict__ running_var,
                                                              float* __restrict__ aff, float* __restrict__ rstd_out, float momentum, float eps) {
    __shared__ double sacc[FIN_WAVES][64];
    __shared__ double smean[64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = min(blockIdx.x * 64 + lane, C - 1);
    const int n_last = M - (slabs - 1) * rpb;
    const double inv_full = 1.0 / (double)rpb, inv_last = 1.0 / (double)n_last;
    double acc = 0.0;
    for (int k0 = w; k0 < slabs; k0 += FIN_WAVES * FIN_U) {                // sum_k n_k mean_k = sum_k (n_k p_k + s_k)
        float s_[FIN_U], p_[FIN_U];
#pragma unroll
        for (int u = 0; u < FIN_U; ++u) {
            const int k = min(k0 + u * FIN_WAVES, slabs - 1);
            const float* o = part + (int64_t)k * 3 * C + c;
            s_[u] = o[0]; p_[u] = o[2 * C];
        }
#pragma unroll
        for (int u = 0; u < FIN_U; ++u) {
            const int k = k0 + u * FIN_WAVES;
            if (k < slabs) acc += (double)(k == slabs - 1 ? n_last : rpb) * (double)p_[u] + (double)s_[u];
        }
    }
    sacc[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < FIN_WAVES; ++i) t += sacc[i][lane];
        smean[lane] = t / (double)M;
    }
    __syncthreads();
    const double mean = smean[lane];
    acc = 0.0;
    for (int k0 = w; k0 < slabs; k0 += FIN_WAVES * FIN_U) {
        float s_[FIN_U], q_[FIN_U], p_[FIN_U];
#pragma unroll
        for (int u = 0; u < FIN_U; ++u) {
            const int k = min(k0 + u * FIN_WAVES, slabs - 1);
            const float* o = part + (int64_t)k * 3 * C + c;
            s_[u] = o[0]; q_[u] = o[C]; p_[u] = o[2 * C];
        }
#pragma unroll
        for (int u = 0; u < FIN_U; ++u) {
            const int k = k0 + u * FIN_WAVES;
            if (k < slabs) {
                const bool last = k == slabs - 1;
                const double n = last ? (double)n_last : (double)rpb, inv = last ? inv_last : inv_full;
                const double s = s_[u], q = q_[u], p = p_[u];
                const double d = p + s * inv - mean;
                acc += (q - s * s * inv) + n * d * d;
            }
        }
    }
    __syncthreads();
    sacc[w][lane] = acc;
    __syncthreads();
    if (w != 0 || blockIdx.x * 64 + lane >= C) return;
    double m2 = 0.0;
#pragma unroll
    for (int i = 0; i < FIN_WAVES; ++i) m2 += sacc[i][lane];
    const float meanf = (float)mean, var_b = (float)(m2 / (double)M);
    const float rs = 1.f / sqrtf(var_b + eps);
    aff[c] = meanf; aff[C + c] = gamma[c] * rs; aff[2 * C + c] = beta[c];
    rstd_out[c] = rs;
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (M > 1 ? (float)(m2 / (double)(M - 1)) : var_b);
}
__global__ __launch_bounds__(FIN_WAVES * 64) void bn_stats_finish_kernel(const float* __restrict__ part, int slabs, int rpb, int M, int C,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* __restrict__ running_mean, float* __restrict__ running_var,
                                                              float* __restrict__ aff, float* __restrict__ rstd_out, float momentum, float eps) {
    bn_stats_finish_body(part, slabs, rpb, M, C, gamma, beta, running_mean, running_var, aff, rstd_out, momentum, eps);
}
__global__ __launch_bounds__(FIN_WAVES * 64) void bn_stats_finish_pair_kernel(const float* __restrict__ part, int slabs, int rpb, int M, int C, BnPair a,
                                                                   float momentum, float eps) {
    const int z = blockIdx.y;
    bn_stats_finish_body(part + (size_t)z * slabs * 3 * C, slabs, rpb, M, C, a.gamma[z], a.beta[z], a.rmean[z], a.rvar[z], a.aff[z], a.rstd[z], momentum, eps);
}
__global__ __launch_bounds__(256) void bn_eval_aff_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                                          float* __restrict__ aff, float* __restrict__ rstd_out, float eps) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float rs = 1.f / sqrtf(running_var[c] + eps);
    aff[c] = running_mean[c]; aff[C + c] = gamma[c] * rs; aff[2 * C + c] = beta[c];
    if (rstd_out) rstd_out[c] = rs;
}

// ------------------------------------------------------------------ BatchNorm backward
// grid (C/256, slabs): part[slab][{sum dy * xhat, sum dy}][C]
template <bool SRC16>
__device__ __forceinline__ void bn_bwd_reduce2_body(const float* __restrict__ dY, const void* __restrict__ X, int M, int C,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, int rpb,
                                                             float* __restrict__ part) {
    __shared__ float4 sg[4][64], sb[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = (blockIdx.x * 64 + lane) * 4;
    const int r0 = blockIdx.y * rpb, r1 = min(M, r0 + rpb);
    float4 ag = make_float4(0.f, 0.f, 0.f, 0.f), ab = ag;
    if (col < C) {
        const float4 mu = *reinterpret_cast<const float4*>(mean + col), rs = *reinterpret_cast<const float4*>(rstd + col);
        int r = r0 + w;
        for (; r + 4 < r1; r += 8) {
            const float4 d0 = *reinterpret_cast<const float4*>(dY + (int64_t)r * C + col), d1 = *reinterpret_cast<const float4*>(dY + (int64_t)(r + 4) * C + col);
            const float4 x0 = subgc_load4<SRC16>(X, (int64_t)r * C + col), x1 = subgc_load4<SRC16>(X, (int64_t)(r + 4) * C + col);
            ab.x += d0.x + d1.x; ab.y += d0.y + d1.y; ab.z += d0.z + d1.z; ab.w += d0.w + d1.w;
            ag.x += d0.x * (x0.x - mu.x) * rs.x + d1.x * (x1.x - mu.x) * rs.x; ag.y += d0.y * (x0.y - mu.y) * rs.y + d1.y * (x1.y - mu.y) * rs.y;
            ag.z += d0.z * (x0.z - mu.z) * rs.z + d1.z * (x1.z - mu.z) * rs.z; ag.w += d0.w * (x0.w - mu.w) * rs.w + d1.w * (x1.w - mu.w) * rs.w;
        }
        for (; r < r1; r += 4) {
            const float4 dy = *reinterpret_cast<const float4*>(dY + (int64_t)r * C + col);
            const float4 x = subgc_load4<SRC16>(X, (int64_t)r * C + col);
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
        float* o = part + (int64_t)blockIdx.y * 2 * C + col;
        *reinterpret_cast<float4*>(o) = make_float4(g0.x + g1.x + g2.x + g3.x, g0.y + g1.y + g2.y + g3.y, g0.z + g1.z + g2.z + g3.z, g0.w + g1.w + g2.w + g3.w);
        *reinterpret_cast<float4*>(o + C) = make_float4(b0.x + b1.x + b2.x + b3.x, b0.y + b1.y + b2.y + b3.y, b0.z + b1.z + b2.z + b3.z, b0.w + b1.w + b2.w + b3.w);
    }
}
// grid (C/256, row slabs): every workgroup first adds the reduce pass's slab partials of ITS columns (wave w: slabs w, w+4, ...;
// the four waves combined in a fixed order, so every workgroup gets the same totals), then streams its rows
template <bool SRC16, bool DX16>
__device__ __forceinline__ void bn_bwd_apply2_body(const float* __restrict__ dY, const void* __restrict__ X, void* __restrict__ dX,
                                                            int M, int C, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ part, int slabs,
                                                            int rpb, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate) {
    __shared__ float4 sg[4][64], sb[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = (blockIdx.x * 64 + lane) * 4;
    float4 tg = make_float4(0.f, 0.f, 0.f, 0.f), tb = tg;
    if (col < C)
        for (int k0 = w; k0 < slabs; k0 += 4 * 8) {                        // eight slabs requested before any is added (else: a chain of L2 latencies)
            float4 g[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = min(k0 + 4 * u, slabs - 1);
                g[u] = *reinterpret_cast<const float4*>(part + (int64_t)k * 2 * C + col);
                b[u] = *reinterpret_cast<const float4*>(part + ((int64_t)k * 2 + 1) * C + col);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + 4 * u < slabs) {
                    tg.x += g[u].x; tg.y += g[u].y; tg.z += g[u].z; tg.w += g[u].w;
                    tb.x += b[u].x; tb.y += b[u].y; tb.z += b[u].z; tb.w += b[u].w;
                }
        }
    sg[w][lane] = tg; sb[w][lane] = tb;
    __syncthreads();
    if (col >= C) return;
    {
        const float4 g0 = sg[0][lane], g1 = sg[1][lane], g2 = sg[2][lane], g3 = sg[3][lane];
        const float4 b0 = sb[0][lane], b1 = sb[1][lane], b2 = sb[2][lane], b3 = sb[3][lane];
        tg = make_float4(g0.x + g1.x + g2.x + g3.x, g0.y + g1.y + g2.y + g3.y, g0.z + g1.z + g2.z + g3.z, g0.w + g1.w + g2.w + g3.w);
        tb = make_float4(b0.x + b1.x + b2.x + b3.x, b0.y + b1.y + b2.y + b3.y, b0.z + b1.z + b2.z + b3.z, b0.w + b1.w + b2.w + b3.w);
    }
    if (blockIdx.y == 0 && w == 0) {
        float4 og = tg, ob = tb;
        if (accumulate) {
            const float4 pg = *reinterpret_cast<const float4*>(dgamma + col), pb = *reinterpret_cast<const float4*>(dbeta + col);
            og.x += pg.x; og.y += pg.y; og.z += pg.z; og.w += pg.w;
            ob.x += pb.x; ob.y += pb.y; ob.z += pb.z; ob.w += pb.w;
        }
        *reinterpret_cast<float4*>(dgamma + col) = og;
        *reinterpret_cast<float4*>(dbeta + col) = ob;
    }
    const float invM = 1.f / (float)M;
    const float4 mu = *reinterpret_cast<const float4*>(mean + col), rs = *reinterpret_cast<const float4*>(rstd + col);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + col);
    const float kx = ga.x * rs.x, ky = ga.y * rs.y, kz = ga.z * rs.z, kw = ga.w * rs.w;
    const int r0 = blockIdx.y * rpb, r1 = min(M, r0 + rpb);
    auto one = [&](int64_t o, const float4& dy, const float4& x) {
        const float out[4] = {kx * (dy.x - tb.x * invM - (x.x - mu.x) * rs.x * tg.x * invM), ky * (dy.y - tb.y * invM - (x.y - mu.y) * rs.y * tg.y * invM),
                              kz * (dy.z - tb.z * invM - (x.z - mu.z) * rs.z * tg.z * invM), kw * (dy.w - tb.w * invM - (x.w - mu.w) * rs.w * tg.w * invM)};
        subgc_store_act<4>(dX, o, out, DX16 ? 1 : 0);
    };
    int r = r0 + w;
    for (; r + 12 < r1; r += 16) {                                         // four rows requested before the first is used
        float4 dy[4], x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t o = (int64_t)(r + 4 * u) * C + col;
            dy[u] = *reinterpret_cast<const float4*>(dY + o);
            x[u] = subgc_load4<SRC16>(X, o);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) one((int64_t)(r + 4 * u) * C + col, dy[u], x[u]);
    }
    for (; r < r1; r += 4) {
        const int64_t o = (int64_t)r * C + col;
        one(o, *reinterpret_cast<const float4*>(dY + o), subgc_load4<SRC16>(X, o));
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline int stat_rows_per_block(int M, int C) {
    const int col_groups = (C + 255) / 256;
    const int slabs = std::max(1, 512 / col_groups);
    return std::max(16, (M + slabs - 1) / slabs);
}

template <bool SRC16>
__global__ __launch_bounds__(256) void bn_bwd_reduce2_kernel(const float* __restrict__ dY, const void* __restrict__ X, int M, int C,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, int rpb,
                                                             float* __restrict__ part) {
    bn_bwd_reduce2_body<SRC16>(dY, X, M, C, mean, rstd, rpb, part);
}
template <bool SRC16, bool DX16>
__global__ __launch_bounds__(256) void bn_bwd_apply2_kernel(const float* __restrict__ dY, const void* __restrict__ X, void* __restrict__ dX,
                                                            int M, int C, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ part, int slabs,
                                                            int rpb, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate) {
    bn_bwd_apply2_body<SRC16, DX16>(dY, X, dX, M, C, mean, rstd, gamma, part, slabs, rpb, dgamma, dbeta, accumulate);
}
// both units of a GCN pair (blockIdx.z = unit; partials at part + z * slabs * 2 C)
struct BnPairBwd { const float* dY[2]; const void* X[2]; void* dX[2]; const float* mean[2]; const float* rstd[2]; const float* gamma[2]; float* dgamma[2]; float* dbeta[2]; };
template <bool SRC16>
__global__ __launch_bounds__(256) void bn_bwd_reduce2_pair_kernel(BnPairBwd a, int M, int C, int rpb, float* __restrict__ part, int slabs) {
    const int z = blockIdx.z;
    bn_bwd_reduce2_body<SRC16>(a.dY[z], a.X[z], M, C, a.mean[z], a.rstd[z], rpb, part + (size_t)z * slabs * 2 * C);
}
template <bool SRC16, bool DX16>
__global__ __launch_bounds__(256) void bn_bwd_apply2_pair_kernel(BnPairBwd a, int M, int C, const float* __restrict__ part, int slabs, int rpb, int accumulate) {
    const int z = blockIdx.z;
    bn_bwd_apply2_body<SRC16, DX16>(a.dY[z], a.X[z], a.dX[z], M, C, a.mean[z], a.rstd[z], a.gamma[z], part + (size_t)z * slabs * 2 * C, slabs, rpb, a.dgamma[z],
                                    a.dbeta[z], accumulate);
}

}  // namespace

SUBGC_API int subgc_bn_stats_workspace_bytes(int M, int C, size_t* bytes) {
    SUBGC_REQUIRE(M > 0 && C > 0 && bytes, "bn_stats_workspace_bytes: bad arguments");
    const int rpb = stat_rows_per_block(M, C);
    *bytes = (size_t)((M + rpb - 1) / rpb) * 3 * C * sizeof(float);
    return SUBGC_OK;
}

SUBGC_API int subgc_bn_stats(const void* X, int x_bf16, int M, int C, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, float* aff, float* rstd, int training, float momentum, float eps, void* workspace,
                             size_t ws_bytes, void* stream) {
    SUBGC_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "bn_stats: M > 0 and C a positive multiple of 4 (got M=%d C=%d)", M, C);
    SUBGC_REQUIRE(gamma && beta && aff, "bn_stats: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!training) {
        SUBGC_REQUIRE(running_mean && running_var, "bn_stats(eval): running statistics required");
        hipLaunchKernelGGL(bn_eval_aff_kernel, dim3((C + 255) / 256), dim3(256), 0, s, C, gamma, beta, (const float*)running_mean,
                           (const float*)running_var, aff, rstd, eps);
        return subgc::check_launch("subgc_bn_stats");
    }
    SUBGC_REQUIRE(X && rstd, "bn_stats(train): null pointer");
    SUBGC_REQUIRE(x_bf16 ? al8(X) : al16(X), "bn_stats: X must be 16-byte (fp32) / 8-byte (bf16) aligned");
    const int rpb = stat_rows_per_block(M, C), slabs = (M + rpb - 1) / rpb;
    SUBGC_REQUIRE(workspace && al16(workspace) && ws_bytes >= (size_t)slabs * 3 * C * sizeof(float),
                  "bn_stats: workspace of %zu bytes required", (size_t)slabs * 3 * C * sizeof(float));
    float* part = static_cast<float*>(workspace);
    const dim3 g((C + 255) / 256, slabs);
    if (x_bf16) hipLaunchKernelGGL((bn_stats_kernel<true>), g, dim3(256), 0, s, X, M, C, rpb, part);
    else hipLaunchKernelGGL((bn_stats_kernel<false>), g, dim3(256), 0, s, X, M, C, rpb, part);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 63) / 64), dim3(FIN_WAVES * 64), 0, s, (const float*)part, slabs, rpb, M, C, gamma, beta, running_mean,
                       running_var, aff, rstd, momentum, eps);
    return subgc::check_launch("subgc_bn_stats");
}

SUBGC_API int subgc_bn_bwd_fused(const float* dY, const void* X, int x_bf16, int M, int C, const float* gamma, const float* mean,
                                 const float* rstd, void* dX, int dx_bf16, float* dgamma, float* dbeta, int accumulate, void* workspace,
                                 size_t ws_bytes, void* stream) {
    SUBGC_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "bn_bwd_fused: M > 0 and C a positive multiple of 4");
    SUBGC_REQUIRE(dY && X && gamma && mean && rstd && dX && dgamma && dbeta, "bn_bwd_fused: null pointer");
    SUBGC_REQUIRE(al16(dY) && (x_bf16 ? al8(X) : al16(X)) && (dx_bf16 ? al8(dX) : al16(dX)) && al16(dgamma) && al16(dbeta) && al16(mean) && al16(rstd) &&
                      al16(gamma), "bn_bwd_fused: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const int rpb = stat_rows_per_block(M, C), slabs = (M + rpb - 1) / rpb;
    SUBGC_REQUIRE(workspace && al16(workspace) && ws_bytes >= (size_t)slabs * 2 * C * sizeof(float), "bn_bwd_fused: workspace of %zu bytes required",
                  (size_t)slabs * 2 * C * sizeof(float));
    float* part = static_cast<float*>(workspace);
    const dim3 g((C + 255) / 256, slabs);
    if (x_bf16) hipLaunchKernelGGL((bn_bwd_reduce2_kernel<true>), g, dim3(256), 0, s, dY, X, M, C, mean, rstd, rpb, part);
    else hipLaunchKernelGGL((bn_bwd_reduce2_kernel<false>), g, dim3(256), 0, s, dY, X, M, C, mean, rstd, rpb, part);
    const int col_groups = (C + 255) / 256;
    const int rpb2 = std::max(8, (int)(((int64_t)M * col_groups + 1023) / 1024));
    const dim3 g2(col_groups, (M + rpb2 - 1) / rpb2);
#define SUBGC_BN_APPLY(S16, D16) \
    hipLaunchKernelGGL((bn_bwd_apply2_kernel<S16, D16>), g2, dim3(256), 0, s, dY, X, dX, M, C, mean, rstd, gamma, (const float*)part, slabs, rpb2, dgamma, dbeta, accumulate)
    if (x_bf16) { if (dx_bf16) SUBGC_BN_APPLY(true, true); else SUBGC_BN_APPLY(true, false); }
    else { if (dx_bf16) SUBGC_BN_APPLY(false, true); else SUBGC_BN_APPLY(false, false); }
#undef SUBGC_BN_APPLY
    return subgc::check_launch("subgc_bn_bwd_fused");
}

// The two units of a GCN pair (same M, C, storage type) through subgc_bn_stats in two launches instead of four
SUBGC_API int subgc_bn_stats_pair(const void* X0, const void* X1, int x_bf16, int M, int C, const float* gamma0, const float* gamma1, const float* beta0,
                                  const float* beta1, float* rmean0, float* rmean1, float* rvar0, float* rvar1, float* aff0, float* aff1, float* rstd0,
                                  float* rstd1, float momentum, float eps, void* workspace, size_t ws_bytes, void* stream) {
    SUBGC_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "bn_stats_pair: M > 0 and C a positive multiple of 4 (got M=%d C=%d)", M, C);
    SUBGC_REQUIRE(X0 && X1 && gamma0 && gamma1 && beta0 && beta1 && aff0 && aff1 && rstd0 && rstd1, "bn_stats_pair: null pointer");
    SUBGC_REQUIRE(x_bf16 ? (al8(X0) && al8(X1)) : (al16(X0) && al16(X1)), "bn_stats_pair: X must be 16-byte (fp32) / 8-byte (bf16) aligned");
    hipStream_t s = (hipStream_t)stream;
    const int rpb = stat_rows_per_block(M, C), slabs = (M + rpb - 1) / rpb;
    SUBGC_REQUIRE(workspace && al16(workspace) && ws_bytes >= (size_t)2 * slabs * 3 * C * sizeof(float), "bn_stats_pair: workspace of %zu bytes required",
                  (size_t)2 * slabs * 3 * C * sizeof(float));
    float* part = static_cast<float*>(workspace);
    BnPair a{{X0, X1}, {gamma0, gamma1}, {beta0, beta1}, {rmean0, rmean1}, {rvar0, rvar1}, {aff0, aff1}, {rstd0, rstd1}};
    const dim3 g((C + 255) / 256, slabs, 2);
    if (x_bf16) hipLaunchKernelGGL((bn_stats_pair_kernel<true>), g, dim3(256), 0, s, a, M, C, rpb, part, slabs);
    else hipLaunchKernelGGL((bn_stats_pair_kernel<false>), g, dim3(256), 0, s, a, M, C, rpb, part, slabs);
    hipLaunchKernelGGL(bn_stats_finish_pair_kernel, dim3((C + 63) / 64, 2), dim3(FIN_WAVES * 64), 0, s, (const float*)part, slabs, rpb, M, C, a, momentum, eps);
    return subgc::check_launch("subgc_bn_stats_pair");
}

// ... and through subgc_bn_bwd_fused in two launches instead of four
SUBGC_API int subgc_bn_bwd_fused_pair(const float* dY0, const float* dY1, const void* X0, const void* X1, int x_bf16, int M, int C, const float* gamma0,
                                      const float* gamma1, const float* mean0, const float* mean1, const float* rstd0, const float* rstd1, void* dX0,
                                      void* dX1, int dx_bf16, float* dgamma0, float* dgamma1, float* dbeta0, float* dbeta1, int accumulate,
                                      void* workspace, size_t ws_bytes, void* stream) {
    SUBGC_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "bn_bwd_fused_pair: M > 0 and C a positive multiple of 4");
    SUBGC_REQUIRE(dY0 && dY1 && X0 && X1 && gamma0 && gamma1 && mean0 && mean1 && rstd0 && rstd1 && dX0 && dX1 && dgamma0 && dgamma1 && dbeta0 && dbeta1,
                  "bn_bwd_fused_pair: null pointer");
    SUBGC_REQUIRE(al16(dY0) && al16(dY1) && (x_bf16 ? (al8(X0) && al8(X1)) : (al16(X0) && al16(X1))) && (dx_bf16 ? (al8(dX0) && al8(dX1)) : (al16(dX0) && al16(dX1))) &&
                      al16(dgamma0) && al16(dgamma1) && al16(dbeta0) && al16(dbeta1) && al16(mean0) && al16(mean1) && al16(rstd0) && al16(rstd1) && al16(gamma0) &&
                      al16(gamma1), "bn_bwd_fused_pair: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const int rpb = stat_rows_per_block(M, C), slabs = (M + rpb - 1) / rpb;
    SUBGC_REQUIRE(workspace && al16(workspace) && ws_bytes >= (size_t)2 * slabs * 2 * C * sizeof(float), "bn_bwd_fused_pair: workspace of %zu bytes required",
                  (size_t)2 * slabs * 2 * C * sizeof(float));
    float* part = static_cast<float*>(workspace);
    BnPairBwd a{{dY0, dY1}, {X0, X1}, {dX0, dX1}, {mean0, mean1}, {rstd0, rstd1}, {gamma0, gamma1}, {dgamma0, dgamma1}, {dbeta0, dbeta1}};
    const dim3 g((C + 255) / 256, slabs, 2);
    if (x_bf16) hipLaunchKernelGGL((bn_bwd_reduce2_pair_kernel<true>), g, dim3(256), 0, s, a, M, C, rpb, part, slabs);
    else hipLaunchKernelGGL((bn_bwd_reduce2_pair_kernel<false>), g, dim3(256), 0, s, a, M, C, rpb, part, slabs);
    const int col_groups = (C + 255) / 256;
    const int rpb2 = std::max(8, (int)(((int64_t)M * col_groups + 1023) / 1024));
    const dim3 g2(col_groups, (M + rpb2 - 1) / rpb2, 2);
#define SUBGC_BN_APPLY(S16, D16) hipLaunchKernelGGL((bn_bwd_apply2_pair_kernel<S16, D16>), g2, dim3(256), 0, s, a, M, C, (const float*)part, slabs, rpb2, accumulate)
    if (x_bf16) { if (dx_bf16) SUBGC_BN_APPLY(true, true); else SUBGC_BN_APPLY(true, false); }
    else { if (dx_bf16) SUBGC_BN_APPLY(false, true); else SUBGC_BN_APPLY(false, false); }
#undef SUBGC_BN_APPLY
    return subgc::check_launch("subgc_bn_bwd_fused_pair");
}
