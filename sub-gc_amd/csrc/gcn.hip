// GCN neighbour aggregation, forward and backward (graph_conv_unit.py:34-36 bmm + normalise + ReLU, graph_conv.py:24-33 average of the two
// roles, gcn_backbone.py:43-47 residual): nodes <- relations through the CSR lists, relations <- nodes through LDS-staged node tiles.
// HBM-bound streaming kernels: threads run along the feature dimension L, the image's index lists live in LDS (gcn_lists.h).
//
// Each direction has ONE float4 kernel (L % 4 == 0, 16-byte / 8-byte aligned rows; a lane owns four adjacent columns), templated on
//   SRC16  the unit outputs are bf16 GEMM results (compute_dtype = bf16) instead of fp32
//   AFF    the BatchNorm1d of the units (graph_conv_unit.py:31-32) is applied ON LOAD from the per-column triple {mean, gamma * rstd, beta}
//          that subgc_bn_stats leaves (gcn_bn.hip) -- the normalised tensor is never written
// and serves the plain entry points as <false, false> and the `_bn` ones in every form.  nodes-fwd, nodes-bwd and edges-bwd keep a scalar
// form (a thread = one column) for L % 4 != 0 or misaligned rows: every element is summed in the same order, so its results are bit-identical.
#include "common.h"
#include "bf16_util.h"
#include "gcn_lists.h"

#include <type_traits>

namespace {

struct Aff4 { float4 mu, sc, be; };
template <bool AFF>
__device__ __forceinline__ Aff4 load_aff(const float* __restrict__ aff, int L, int col) {
    Aff4 a{};
    if (AFF) {
        a.mu = *reinterpret_cast<const float4*>(aff + col);
        a.sc = *reinterpret_cast<const float4*>(aff + L + col);
        a.be = *reinterpret_cast<const float4*>(aff + 2 * L + col);
    }
    return a;
}
template <bool AFF>
__device__ __forceinline__ float4 apply_aff(const Aff4& a, float4 x) {
    if (!AFF) return x;
    return make_float4((x.x - a.mu.x) * a.sc.x + a.be.x, (x.y - a.mu.y) * a.sc.y + a.be.y, (x.z - a.mu.z) * a.sc.z + a.be.z,
                       (x.w - a.mu.w) * a.sc.w + a.be.w);
}

// A relation row between its request and its addition (gather_pair holds eight of them): a bf16 row stays packed, two registers instead of
// four, and is unpacked and normalised when it is added; an fp32 row is normalised in place when it arrives
template <bool SRC16, bool AFF>
__device__ __forceinline__ auto row_request(const void* F, int64_t i, const Aff4& A) {
    if constexpr (SRC16) return *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(F) + i);
    else return apply_aff<AFF>(A, subgc_load4<false>(F, i));
}
template <bool AFF> __device__ __forceinline__ float4 row_value(uint2 r, const Aff4& A) { return apply_aff<AFF>(A, subgc_unpack4(r)); }
template <bool AFF> __device__ __forceinline__ float4 row_value(float4 r, const Aff4&) { return r; }

// ------------------------------------------------------------------ nodes <- relations
// grid (L/256, B); thread = one feature column; CSR lists of the image in LDS.
__global__ __launch_bounds__(256) void gcn_nodes_fwd_kernel(const float* __restrict__ F0, const float* __restrict__ F1,
                                                            const int32_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ edges,
                                                            const float* __restrict__ skip, float* __restrict__ Xout,
                                                            uint8_t* __restrict__ act, int B, int N, int K, int L) {
    extern __shared__ int sm_i[];
    int *ps, *po, *es, *eo;
    const int b = blockIdx.y;
    gcn_stage_csr(sm_i, ptr, edges, b, B, N, K, ps, po, es, eo);
    __syncthreads();
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= L) return;
    const float* f0 = F0 + (int64_t)b * K * L + col;
    const float* f1 = F1 + (int64_t)b * K * L + col;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {           // node chunks over gridDim.z: shorter dependent chains, 4x the loads in flight
        float a = 0.f, c = 0.f;
        const int s0 = ps[n], s1 = ps[n + 1], o0 = po[n], o1 = po[n + 1];
        for (int j = s0; j < s1; ++j) a += f0[(int64_t)es[j] * L];
        for (int j = o0; j < o1; ++j) c += f1[(int64_t)eo[j] * L];
        a = a / ((float)(s1 - s0) + 1e-7f);
        c = c / ((float)(o1 - o0) + 1e-7f);
        const uint8_t bits = (a > 0.f ? 1 : 0) | (c > 0.f ? 2 : 0);
        float v = (fmaxf(a, 0.f) + fmaxf(c, 0.f)) / 2.f;
        const int64_t o = ((int64_t)b * N + n) * L + col;
        if (skip) v += skip[o];
        Xout[o] = v;
        if (act) act[o] = bits;
    }
}

// float4 form: a wave reads 1 KB of a relation row per instruction instead of 256 B (the scalar form ran at 2.3 TB/s on Full-GC's
// 65 x 1024 relation rows).  Xout16: also a bf16 copy of the result (the next layer's GEMM operand under compute_dtype = bf16)
template <bool SRC16, bool AFF>
__global__ __launch_bounds__(256) void gcn_nodes_fwd_f4_kernel(const void* __restrict__ F0, const void* __restrict__ F1,
                                                               const float* __restrict__ aff0, const float* __restrict__ aff1,
                                                               const int32_t* __restrict__ ptr, const int32_t* __restrict__ edges,
                                                               const float* __restrict__ skip, float* __restrict__ Xout,
                                                               uint16_t* __restrict__ Xout16, uint8_t* __restrict__ act, int B, int N, int K, int L) {
    extern __shared__ int sm_i[];
    int *ps, *po, *es, *eo;
    const int b = blockIdx.y;
    gcn_stage_csr(sm_i, ptr, edges, b, B, N, K, ps, po, es, eo);
    __syncthreads();
    const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (col >= L) return;
    const Aff4 A0 = load_aff<AFF>(aff0, L, col), A1 = load_aff<AFF>(aff1, L, col);
    const int64_t base = (int64_t)b * K * L + col;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
        const int s0 = ps[n], s1 = ps[n + 1], o0 = po[n], o1 = po[n + 1];
        gather_pair(es, s0, s1, [&](int e) { return row_request<SRC16, AFF>(F0, base + (int64_t)e * L, A0); },
                    eo, o0, o1, [&](int e) { return row_request<SRC16, AFF>(F1, base + (int64_t)e * L, A1); }, a, c,
                    [&](auto r) { return row_value<AFF>(r, A0); }, [&](auto r) { return row_value<AFF>(r, A1); });
        const float da = (float)(s1 - s0) + 1e-7f, dc = (float)(o1 - o0) + 1e-7f;
        const float av[4] = {a.x / da, a.y / da, a.z / da, a.w / da}, cv[4] = {c.x / dc, c.y / dc, c.z / dc, c.w / dc};
        const int64_t o = ((int64_t)b * N + n) * L + col;
        float4 sk = make_float4(0.f, 0.f, 0.f, 0.f);
        if (skip) sk = *reinterpret_cast<const float4*>(skip + o);
        const float skv[4] = {sk.x, sk.y, sk.z, sk.w};
        float v[4];
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bits |= (uint32_t)((av[e] > 0.f ? 1 : 0) | (cv[e] > 0.f ? 2 : 0)) << (8 * e);
            v[e] = (fmaxf(av[e], 0.f) + fmaxf(cv[e], 0.f)) / 2.f;
            if (skip) v[e] += skv[e];
        }
        *reinterpret_cast<float4*>(Xout + o) = make_float4(v[0], v[1], v[2], v[3]);
        if (Xout16) *reinterpret_cast<uint2*>(Xout16 + o) = subgc_pack4(v[0], v[1], v[2], v[3]);
        if (act) *reinterpret_cast<uint32_t*>(act + o) = bits;
    }
}

// dF0[b,k,:] = 1/2 [bit0](b,s_k,:) dX[b,s_k,:] / (cnt_s[s_k] + 1e-7);  dF1 likewise with o_k / bit1
__global__ __launch_bounds__(256) void gcn_nodes_bwd_kernel(const float* __restrict__ dX, const uint8_t* __restrict__ act,
                                                            const int64_t* __restrict__ rel_ind,
                                                            const int32_t* __restrict__ ptr, float* __restrict__ dF0,
                                                            float* __restrict__ dF1, int B, int N, int K, int L) {
    extern __shared__ int sm_i[];
    int* ns = sm_i;            // [K] subject node of k
    int* no = ns + K;          // [K] object node of k
    float* ds = reinterpret_cast<float*>(no + K);   // [N] cnt_s + 1e-7 denominators
    float* dn_o = ds + N;
    const int b = blockIdx.y;
    gcn_stage_rel_nodes(rel_ind, ptr, b, B, N, K, ns, no, ds, dn_o);
    __syncthreads();
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= L) return;
    for (int k = blockIdx.z; k < K; k += gridDim.z) {
        const int s = ns[k], o = no[k];
        const int64_t is = ((int64_t)b * N + s) * L + col, io = ((int64_t)b * N + o) * L + col;
        const float gs = (act[is] & 1) ? dX[is] * 0.5f / ds[s] : 0.f;
        const float go = (act[io] & 2) ? dX[io] * 0.5f / dn_o[o] : 0.f;
        const int64_t ok = ((int64_t)b * K + k) * L + col;
        dF0[ok] = gs;
        dF1[ok] = go;
    }
}

// o16: dF0 / dF1 are bf16 (the unit outputs they are gradients of were bf16 GEMM results: compute_dtype = bf16 without BatchNorm)
__global__ __launch_bounds__(256) void gcn_nodes_bwd_vec_kernel(const float* __restrict__ dX, const uint8_t* __restrict__ act,
                                                                const int64_t* __restrict__ rel_ind, const int32_t* __restrict__ ptr,
                                                                void* __restrict__ dF0, void* __restrict__ dF1, int B, int N, int K, int L, int o16) {
    extern __shared__ int sm_i[];
    int* ns = sm_i; int* no = ns + K;
    float* ds = reinterpret_cast<float*>(no + K); float* dn_o = ds + N;
    const int b = blockIdx.y;
    gcn_stage_rel_nodes(rel_ind, ptr, b, B, N, K, ns, no, ds, dn_o);
    __syncthreads();
    const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (col >= L) return;
    const int kz = gridDim.z;
    for (int k0 = blockIdx.z; k0 < K; k0 += 4 * kz) {                      // four relations' node rows requested before the first is used
        int sn[4], on[4];
        uint32_t as[4], ao[4];
        float4 xs[4], xo[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * kz;
            if (k < K) {
                sn[u] = ns[k]; on[u] = no[k];
                const int64_t is = ((int64_t)b * N + sn[u]) * L + col, io = ((int64_t)b * N + on[u]) * L + col;
                as[u] = *reinterpret_cast<const uint32_t*>(act + is); ao[u] = *reinterpret_cast<const uint32_t*>(act + io);
                xs[u] = *reinterpret_cast<const float4*>(dX + is); xo[u] = *reinterpret_cast<const float4*>(dX + io);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * kz;
            if (k < K) {
                const float xsv[4] = {xs[u].x, xs[u].y, xs[u].z, xs[u].w}, xov[4] = {xo[u].x, xo[u].y, xo[u].z, xo[u].w};
                float gs[4], go[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    gs[e] = ((as[u] >> (8 * e)) & 1u) ? xsv[e] * 0.5f / ds[sn[u]] : 0.f;
                    go[e] = ((ao[u] >> (8 * e)) & 2u) ? xov[e] * 0.5f / dn_o[on[u]] : 0.f;
                }
                const int64_t ok = ((int64_t)b * K + k) * L + col;
                subgc_store_act<4>(dF0, ok, gs, o16);
                subgc_store_act<4>(dF1, ok, go, o16);
            }
        }
    }
}

// ------------------------------------------------------------------ relations <- nodes
// grid (L/TC, B), TC = 128 columns; the image's F2/F3 node tiles [N x TC] are staged in LDS (normalised while staging;
// each node row is consumed by ~K/N relations per role), then every relation gathers from LDS.
// VEC: Pout / skip / Pout16 rows are 16-byte (8-byte) aligned -- 16-byte LDS reads and stores; else a thread = one column
// OUT16: Pout16 is given (the pack of four results costs the float4 form nine registers, a wave per SIMD: only where it is asked for)
constexpr int TC = 128;
template <bool SRC16, bool AFF, bool VEC, bool OUT16>
__global__ __launch_bounds__(256) void gcn_edges_fwd_f4_kernel(const void* __restrict__ F2, const void* __restrict__ F3,
                                                               const float* __restrict__ aff2, const float* __restrict__ aff3,
                                                               const int64_t* __restrict__ rel_ind, const float* __restrict__ skip,
                                                               float* __restrict__ Pout, uint16_t* __restrict__ Pout16, int B, int N, int K, int L) {
    extern __shared__ __attribute__((aligned(16))) float sm_f[];
    float* t2 = sm_f;                    // [N][TC]
    float* t3 = sm_f + (size_t)N * TC;   // [N][TC]
    int* ns = reinterpret_cast<int*>(t3 + (size_t)N * TC);   // [K]
    int* no = ns + K;
    const int b = blockIdx.y, c0 = blockIdx.x * TC;
    const float cdiv1 = 1.f + 1e-7f;     // fp32(1 + 1e-7) = 1.00000012: rowsum of a 0/1 incidence row + 1e-7
    gcn_stage_rel_nodes(rel_ind, nullptr, b, B, N, K, ns, no, nullptr, nullptr);
    const int items = N * (TC / 4);
    for (int i0 = threadIdx.x; i0 < items; i0 += 4 * blockDim.x) {         // four node-row quads requested before the first is staged
        float4 a[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * blockDim.x;
            a[u] = make_float4(0.f, 0.f, 0.f, 0.f); c[u] = a[u];
            if (i < items) {
                const int n = i / (TC / 4), c4 = (i % (TC / 4)) * 4;
                if (c0 + c4 < L) {                                        // L % 4 == 0: a float4 is all in or all out
                    const int64_t g = ((int64_t)b * N + n) * L + c0 + c4;
                    a[u] = subgc_load4<SRC16>(F2, g);
                    c[u] = subgc_load4<SRC16>(F3, g);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * blockDim.x;
            if (i < items) {
                const int n = i / (TC / 4), c4 = (i % (TC / 4)) * 4;
                float4 x = a[u], y = c[u];
                if (AFF && c0 + c4 < L) {
                    x = apply_aff<AFF>(load_aff<AFF>(aff2, L, c0 + c4), x);
                    y = apply_aff<AFF>(load_aff<AFF>(aff3, L, c0 + c4), y);
                }
                // relu(x / c) is what every consumer needs: do it once per node element
                x.x = fmaxf(x.x / cdiv1, 0.f); x.y = fmaxf(x.y / cdiv1, 0.f); x.z = fmaxf(x.z / cdiv1, 0.f); x.w = fmaxf(x.w / cdiv1, 0.f);
                y.x = fmaxf(y.x / cdiv1, 0.f); y.y = fmaxf(y.y / cdiv1, 0.f); y.z = fmaxf(y.z / cdiv1, 0.f); y.w = fmaxf(y.w / cdiv1, 0.f);
                *reinterpret_cast<float4*>(t2 + n * TC + c4) = x;
                *reinterpret_cast<float4*>(t3 + n * TC + c4) = y;
            }
        }
    }
    __syncthreads();
    if (VEC) {                                                             // 8 relation streams x 32 lanes x 4 columns
        const int cl4 = (threadIdx.x & 31) * 4, st = threadIdx.x >> 5;
        if (c0 + cl4 >= L) return;
        for (int k0 = st; k0 < K; k0 += 32) {
            float4 v[4], sk[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 8 * u;
                if (k < K) {
                    const float4 x = *reinterpret_cast<const float4*>(t2 + ns[k] * TC + cl4), y = *reinterpret_cast<const float4*>(t3 + no[k] * TC + cl4);
                    v[u] = make_float4((x.x + y.x) / 2.f, (x.y + y.y) / 2.f, (x.z + y.z) / 2.f, (x.w + y.w) / 2.f);
                    if (skip) sk[u] = *reinterpret_cast<const float4*>(skip + ((int64_t)b * K + k) * L + c0 + cl4);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 8 * u;
                if (k < K) {
                    float4 r = v[u];
                    if (skip) { r.x += sk[u].x; r.y += sk[u].y; r.z += sk[u].z; r.w += sk[u].w; }
                    const int64_t o = ((int64_t)b * K + k) * L + c0 + cl4;
                    *reinterpret_cast<float4*>(Pout + o) = r;
                    if (OUT16) *reinterpret_cast<uint2*>(Pout16 + o) = subgc_pack4(r.x, r.y, r.z, r.w);
                }
            }
        }
        return;
    }
    const int cl = threadIdx.x & (TC - 1), half = threadIdx.x >> 7;   // 2 relation streams x 128 columns
    const int col = c0 + cl;
    if (col >= L) return;
    for (int k0 = half; k0 < K; k0 += 8) {                                 // four relations per round: LDS reads and skip loads in flight together
        float v[4], sk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 2 * u;
            if (k < K) {
                v[u] = (t2[ns[k] * TC + cl] + t3[no[k] * TC + cl]) / 2.f;
                sk[u] = skip ? skip[((int64_t)b * K + k) * L + col] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 2 * u;
            if (k < K) {
                const int64_t o = ((int64_t)b * K + k) * L + col;
                const float r = skip ? v[u] + sk[u] : v[u];
                Pout[o] = r;
                if (OUT16) Pout16[o] = (uint16_t)subgc_f2bf(r);
            }
        }
    }
}

// dF2[b,n,:] = 1/2 [F2>0] / c * sum_{k in CSR_s(n)} dP[b,k,:]   (and F3 / CSR_o)
__global__ __launch_bounds__(256) void gcn_edges_bwd_kernel(const float* __restrict__ dP, const float* __restrict__ F2,
                                                            const float* __restrict__ F3, const int32_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ edges, float* __restrict__ dF2,
                                                            float* __restrict__ dF3, int B, int N, int K, int L) {
    extern __shared__ int sm_i[];
    int *ps, *po, *es, *eo;
    const int b = blockIdx.y;
    gcn_stage_csr(sm_i, ptr, edges, b, B, N, K, ps, po, es, eo);
    __syncthreads();
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= L) return;
    const float cdiv1 = 1.f + 1e-7f;
    const float* dp = dP + (int64_t)b * K * L + col;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        float a = 0.f, c = 0.f;
        for (int j = ps[n]; j < ps[n + 1]; ++j) a += dp[(int64_t)es[j] * L];
        for (int j = po[n]; j < po[n + 1]; ++j) c += dp[(int64_t)eo[j] * L];
        const int64_t o = ((int64_t)b * N + n) * L + col;
        dF2[o] = (F2[o] / cdiv1 > 0.f) ? a * 0.5f / cdiv1 : 0.f;
        dF3[o] = (F3[o] / cdiv1 > 0.f) ? c * 0.5f / cdiv1 : 0.f;
    }
}

// o16: dF2 / dF3 are bf16 (see gcn_nodes_bwd_vec_kernel)
template <bool SRC16, bool AFF>
__global__ __launch_bounds__(256) void gcn_edges_bwd_f4_kernel(const float* __restrict__ dP, const void* __restrict__ F2,
                                                               const void* __restrict__ F3, const float* __restrict__ aff2,
                                                               const float* __restrict__ aff3, const int32_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ edges, void* __restrict__ dF2,
                                                               void* __restrict__ dF3, int B, int N, int K, int L, int o16) {
    extern __shared__ int sm_i[];
    int *ps, *po, *es, *eo;
    const int b = blockIdx.y;
    gcn_stage_csr(sm_i, ptr, edges, b, B, N, K, ps, po, es, eo);
    __syncthreads();
    const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (col >= L) return;
    const Aff4 A2 = load_aff<AFF>(aff2, L, col), A3 = load_aff<AFF>(aff3, L, col);
    const float cdiv1 = 1.f + 1e-7f;
    const float* dp = dP + (int64_t)b * K * L + col;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
        const int64_t o = ((int64_t)b * N + n) * L + col;
        const float4 f2 = apply_aff<AFF>(A2, subgc_load4<SRC16>(F2, o)), f3 = apply_aff<AFF>(A3, subgc_load4<SRC16>(F3, o));
        auto row = [&](int e) { return *reinterpret_cast<const float4*>(dp + (int64_t)e * L); };
        gather_pair(es, ps[n], ps[n + 1], row, eo, po[n], po[n + 1], row, a, c);
        float4 r2, r3;
        r2.x = (f2.x / cdiv1 > 0.f) ? a.x * 0.5f / cdiv1 : 0.f; r2.y = (f2.y / cdiv1 > 0.f) ? a.y * 0.5f / cdiv1 : 0.f;
        r2.z = (f2.z / cdiv1 > 0.f) ? a.z * 0.5f / cdiv1 : 0.f; r2.w = (f2.w / cdiv1 > 0.f) ? a.w * 0.5f / cdiv1 : 0.f;
        r3.x = (f3.x / cdiv1 > 0.f) ? c.x * 0.5f / cdiv1 : 0.f; r3.y = (f3.y / cdiv1 > 0.f) ? c.y * 0.5f / cdiv1 : 0.f;
        r3.z = (f3.z / cdiv1 > 0.f) ? c.z * 0.5f / cdiv1 : 0.f; r3.w = (f3.w / cdiv1 > 0.f) ? c.w * 0.5f / cdiv1 : 0.f;
        const float o2[4] = {r2.x, r2.y, r2.z, r2.w}, o3[4] = {r3.x, r3.y, r3.z, r3.w};
        subgc_store_act<4>(dF2, o, o2, o16);
        subgc_store_act<4>(dF3, o, o3, o16);
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool gcn_vec_ok(int L, const void* a, const void* b, const void* c, const void* d) {
    return L % 4 == 0 && al16(a) && al16(b) && al16(c) && al16(d);
}

// The float4 launches behind a plain entry point and its `_bn` twin, which has validated the arguments; `what` = the entry point's name.
// with_bool(b, f): f(std::true_type / std::false_type) -- a run-time choice as a template argument
template <class F>
int with_bool(bool b, F f) { return b ? f(std::true_type()) : f(std::false_type()); }
#define CT(x) decltype(x)::value

int nodes_fwd_f4(const char* what, const void* F0, const void* F1, int f_bf16, const float* aff0, const float* aff1, const int32_t* ptr,
                 const int32_t* edges, const float* skip, float* Xout, uint16_t* Xout16, uint8_t* act, int B, int N, int K, int L, hipStream_t s) {
    subgc::ProfScope prof(SUBGC_FAM_GCN, s, (f_bf16 ? 2.0 : 4.0) * B * L * 2.0 * K + 4.0 * B * L * (skip ? 2.0 : 1.0) * N);
    const size_t lds = sizeof(int) * (2 * (N + 1) + 2 * K);
    const dim3 g((L / 4 + 255) / 256, B, subgc::gcn_zsplit((L / 4 + 255) / 256, B, N));
    return with_bool(f_bf16, [&](auto s16) { return with_bool(aff0, [&](auto aff) {
        hipLaunchKernelGGL((gcn_nodes_fwd_f4_kernel<CT(s16), CT(aff)>), g, dim3(256), lds, s, F0, F1, aff0, aff1, ptr, edges, skip, Xout, Xout16, act, B, N, K, L);
        return subgc::check_launch(what);
    }); });
}

int edges_fwd_f4(const char* what, const void* F2, const void* F3, int f_bf16, const float* aff2, const float* aff3, const int64_t* rel_ind,
                 const float* skip, float* Pout, uint16_t* Pout16, int B, int N, int K, int L, hipStream_t s) {
    const size_t lds = sizeof(float) * 2 * (size_t)N * TC + sizeof(int) * 2 * K;
    const bool vec = al16(Pout) && al16(skip) && al8(Pout16);
    return with_bool(f_bf16, [&](auto s16) { return with_bool(aff2, [&](auto aff) { return with_bool(vec, [&](auto v) { return with_bool(Pout16, [&](auto o16) {
        const auto kernel = gcn_edges_fwd_f4_kernel<CT(s16), CT(aff), CT(v), CT(o16)>;
        if (int rc = subgc::raise_lds_cached((const void*)kernel, lds, what + 6)) return rc;     // the name without its "subgc_"
        subgc::ProfScope prof(SUBGC_FAM_GCN, s, (f_bf16 ? 2.0 : 4.0) * B * L * 2.0 * N + 4.0 * B * L * (skip ? 2.0 : 1.0) * K);
        hipLaunchKernelGGL(kernel, dim3((L + TC - 1) / TC, B), dim3(256), lds, s, F2, F3, aff2, aff3, rel_ind, skip, Pout, Pout16, B, N, K, L);
        return subgc::check_launch(what);
    }); }); }); });
}

int edges_bwd_f4(const char* what, const float* dP, const void* F2, const void* F3, int f_bf16, const float* aff2, const float* aff3,
                 const int32_t* ptr, const int32_t* edges, void* dF2, void* dF3, int out_bf16, int B, int N, int K, int L, hipStream_t s) {
    subgc::ProfScope prof(SUBGC_FAM_GCN, s, 4.0 * B * L * (2.0 * K + 2.0 * N) + (f_bf16 ? 2.0 : 4.0) * B * L * 2.0 * N);
    const size_t lds = sizeof(int) * (2 * (N + 1) + 2 * K);
    const dim3 g((L / 4 + 255) / 256, B, subgc::gcn_zsplit((L / 4 + 255) / 256, B, N));
    return with_bool(f_bf16, [&](auto s16) { return with_bool(aff2, [&](auto aff) {
        hipLaunchKernelGGL((gcn_edges_bwd_f4_kernel<CT(s16), CT(aff)>), g, dim3(256), lds, s, dP, F2, F3, aff2, aff3, ptr, edges, dF2, dF3, B, N, K, L, out_bf16);
        return subgc::check_launch(what);
    }); });
}
#undef CT

}  // namespace

SUBGC_API int subgc_gcn_nodes_fwd(const float* F0, const float* F1, const int32_t* ptr, const int32_t* edges, const float* skip,
                                  float* Xout, uint8_t* act, int B, int N, int K, int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0, "gcn_nodes_fwd: bad sizes");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(F0 && F1 && ptr && edges && Xout, "gcn_nodes_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (gcn_vec_ok(L, F0, F1, skip, Xout) && (reinterpret_cast<uintptr_t>(act) & 3) == 0)
        return nodes_fwd_f4("subgc_gcn_nodes_fwd", F0, F1, 0, nullptr, nullptr, ptr, edges, skip, Xout, nullptr, act, B, N, K, L, s);
    subgc::ProfScope prof(SUBGC_FAM_GCN, s, 4.0 * B * L * (2.0 * K + (skip ? 2.0 : 1.0) * N));
    const size_t lds = sizeof(int) * (2 * (N + 1) + 2 * K);
    hipLaunchKernelGGL(gcn_nodes_fwd_kernel, dim3((L + 255) / 256, B, subgc::gcn_zsplit((L + 255) / 256, B, N)), dim3(256), lds, s, F0, F1, ptr, edges, skip, Xout, act, B, N, K, L);
    return subgc::check_launch("subgc_gcn_nodes_fwd");
}

SUBGC_API int subgc_gcn_nodes_fwd_bn(const void* F0, const void* F1, int f_bf16, const float* aff0, const float* aff1, const int32_t* ptr,
                                     const int32_t* edges, const float* skip, float* Xout, uint16_t* Xout16, uint8_t* act, int B, int N, int K,
                                     int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0 && L % 4 == 0, "gcn_nodes_fwd_bn: bad sizes (L must be a multiple of 4)");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(F0 && F1 && ptr && edges && Xout, "gcn_nodes_fwd_bn: null pointer");
    SUBGC_REQUIRE(!aff0 == !aff1, "gcn_nodes_fwd_bn: aff0 and aff1 must both be given or both be null");
    SUBGC_REQUIRE((f_bf16 ? (al8(F0) && al8(F1)) : (al16(F0) && al16(F1))) && al16(skip) && al16(Xout) && al8(Xout16) && al16(aff0) && al16(aff1) &&
                      (reinterpret_cast<uintptr_t>(act) & 3) == 0, "gcn_nodes_fwd_bn: misaligned pointer");
    return nodes_fwd_f4("subgc_gcn_nodes_fwd_bn", F0, F1, f_bf16, aff0, aff1, ptr, edges, skip, Xout, Xout16, act, B, N, K, L, (hipStream_t)stream);
}

SUBGC_API int subgc_gcn_nodes_bwd(const float* dX, const uint8_t* act, const int64_t* rel_ind, const int32_t* ptr, void* dF0,
                                  void* dF1, int out_bf16, int B, int N, int K, int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0, "gcn_nodes_bwd: bad sizes");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(dX && act && rel_ind && ptr && dF0 && dF1, "gcn_nodes_bwd: null pointer");
    SUBGC_DEBUG_RANGE(rel_ind, 8, (int64_t)B * K, 2, 2, 0, N - 1, -1, "gcn_nodes_bwd: rel_ind", stream);
    hipStream_t s = (hipStream_t)stream;
    subgc::ProfScope prof(SUBGC_FAM_GCN, s, 4.0 * B * L * (2.0 * K + 2.0 * K));
    const size_t lds = sizeof(int) * (2 * K) + sizeof(float) * 2 * N;
    const bool vec = gcn_vec_ok(L, dX, nullptr, nullptr, nullptr) && (reinterpret_cast<uintptr_t>(act) & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(dF0) | reinterpret_cast<uintptr_t>(dF1)) & (out_bf16 ? 7 : 15)) == 0;
    SUBGC_REQUIRE(vec || !out_bf16, "gcn_nodes_bwd: bf16 gradients need L %% 4 == 0 and aligned rows");
    if (vec)
        hipLaunchKernelGGL(gcn_nodes_bwd_vec_kernel, dim3((L / 4 + 255) / 256, B, subgc::gcn_zsplit((L / 4 + 255) / 256, B, (K + 3) / 4)), dim3(256), lds, s, dX, act, rel_ind, ptr, dF0, dF1, B, N, K, L, out_bf16);
    else
        hipLaunchKernelGGL(gcn_nodes_bwd_kernel, dim3((L + 255) / 256, B, subgc::gcn_zsplit((L + 255) / 256, B, K)), dim3(256), lds, s, dX, act, rel_ind, ptr, static_cast<float*>(dF0), static_cast<float*>(dF1), B, N, K, L);
    return subgc::check_launch("subgc_gcn_nodes_bwd");
}

SUBGC_API int subgc_gcn_edges_fwd(const float* F2, const float* F3, const int64_t* rel_ind, const float* skip, float* Pout, int B,
                                  int N, int K, int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0, "gcn_edges_fwd: bad sizes");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(F2 && F3 && rel_ind && Pout, "gcn_edges_fwd: null pointer");
    SUBGC_DEBUG_RANGE(rel_ind, 8, (int64_t)B * K, 2, 2, 0, N - 1, -1, "gcn_edges_fwd: rel_ind", stream);
    SUBGC_REQUIRE(L % 4 == 0, "gcn_edges_fwd: L must be a multiple of 4 (got %d)", L);
    return edges_fwd_f4("subgc_gcn_edges_fwd", F2, F3, 0, nullptr, nullptr, rel_ind, skip, Pout, nullptr, B, N, K, L, (hipStream_t)stream);
}

SUBGC_API int subgc_gcn_edges_fwd_bn(const void* F2, const void* F3, int f_bf16, const float* aff2, const float* aff3, const int64_t* rel_ind,
                                     const float* skip, float* Pout, uint16_t* Pout16, int B, int N, int K, int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0 && L % 4 == 0, "gcn_edges_fwd_bn: bad sizes (L must be a multiple of 4)");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(F2 && F3 && rel_ind && Pout, "gcn_edges_fwd_bn: null pointer");
    SUBGC_REQUIRE(!aff2 == !aff3, "gcn_edges_fwd_bn: aff2 and aff3 must both be given or both be null");
    SUBGC_DEBUG_RANGE(rel_ind, 8, (int64_t)B * K, 2, 2, 0, N - 1, -1, "gcn_edges_fwd_bn: rel_ind", stream);
    SUBGC_REQUIRE((f_bf16 ? (al8(F2) && al8(F3)) : (al16(F2) && al16(F3))) && al16(aff2) && al16(aff3), "gcn_edges_fwd_bn: misaligned pointer");
    return edges_fwd_f4("subgc_gcn_edges_fwd_bn", F2, F3, f_bf16, aff2, aff3, rel_ind, skip, Pout, Pout16, B, N, K, L, (hipStream_t)stream);
}

SUBGC_API int subgc_gcn_edges_bwd(const float* dP, const float* F2, const float* F3, const int32_t* ptr, const int32_t* edges,
                                  float* dF2, float* dF3, int B, int N, int K, int L, void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0, "gcn_edges_bwd: bad sizes");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(dP && F2 && F3 && ptr && edges && dF2 && dF3, "gcn_edges_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (gcn_vec_ok(L, dP, F2, F3, dF2) && al16(dF3))
        return edges_bwd_f4("subgc_gcn_edges_bwd", dP, F2, F3, 0, nullptr, nullptr, ptr, edges, dF2, dF3, 0, B, N, K, L, s);
    subgc::ProfScope prof(SUBGC_FAM_GCN, s, 4.0 * B * L * (2.0 * K + 4.0 * N));
    const size_t lds = sizeof(int) * (2 * (N + 1) + 2 * K);
    hipLaunchKernelGGL(gcn_edges_bwd_kernel, dim3((L + 255) / 256, B, subgc::gcn_zsplit((L + 255) / 256, B, N)), dim3(256), lds, s, dP, F2, F3, ptr, edges, dF2, dF3, B, N, K, L);
    return subgc::check_launch("subgc_gcn_edges_bwd");
}

SUBGC_API int subgc_gcn_edges_bwd_bn(const float* dP, const void* F2, const void* F3, int f_bf16, const float* aff2, const float* aff3,
                                     const int32_t* ptr, const int32_t* edges, void* dF2, void* dF3, int out_bf16, int B, int N, int K, int L,
                                     void* stream) {
    SUBGC_REQUIRE(B >= 0 && N > 0 && K > 0 && L > 0 && L % 4 == 0, "gcn_edges_bwd_bn: bad sizes (L must be a multiple of 4)");
    if (B == 0) return SUBGC_OK;
    SUBGC_REQUIRE(dP && F2 && F3 && ptr && edges && dF2 && dF3, "gcn_edges_bwd_bn: null pointer");
    SUBGC_REQUIRE(!aff2 == !aff3, "gcn_edges_bwd_bn: aff2 and aff3 must both be given or both be null");
    SUBGC_REQUIRE(al16(dP) && (f_bf16 ? (al8(F2) && al8(F3)) : (al16(F2) && al16(F3))) && (out_bf16 ? (al8(dF2) && al8(dF3)) : (al16(dF2) && al16(dF3))) &&
                      al16(aff2) && al16(aff3), "gcn_edges_bwd_bn: misaligned pointer");
    return edges_bwd_f4("subgc_gcn_edges_bwd_bn", dP, F2, F3, f_bf16, aff2, aff3, ptr, edges, dF2, dF3, out_bf16, B, N, K, L, (hipStream_t)stream);
}
