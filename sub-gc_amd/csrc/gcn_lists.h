// The two LDS prologues of the per-image GCN kernels (gcn.hip, the aggregate-first pair of graph.hip): every workgroup of image b first
// copies that image's index lists into dynamic LDS.  Neither helper synchronises: the caller's __syncthreads() follows, after whatever
// else it stages.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

// CSR lists by subject / by object (csr_build_kernel): sm = [ps: N+1][po: N+1][es: K][eo: K]
__device__ __forceinline__ void gcn_stage_csr(int* sm, const int32_t* __restrict__ ptr, const int32_t* __restrict__ edges, int b, int B, int N, int K,
                                              int*& ps, int*& po, int*& es, int*& eo) {
    ps = sm; po = ps + (N + 1); es = po + (N + 1); eo = es + K;
    for (int i = threadIdx.x; i <= N; i += blockDim.x) {
        ps[i] = ptr[((int64_t)0 * B + b) * (N + 1) + i];
        po[i] = ptr[((int64_t)1 * B + b) * (N + 1) + i];
    }
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        es[i] = edges[((int64_t)0 * B + b) * K + i];
        eo[i] = edges[((int64_t)1 * B + b) * K + i];
    }
}

// ns / no [K]: subject and object node of every relation, clamped into [0, N - 1]; ds / dn_o [N] (both or neither; they need `ptr`): the
// per-node denominators cnt_s + 1e-7 and cnt_o + 1e-7
__device__ __forceinline__ void gcn_stage_rel_nodes(const int64_t* __restrict__ rel_ind, const int32_t* __restrict__ ptr, int b, int B, int N, int K,
                                                    int* ns, int* no, float* ds, float* dn_o) {
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        int64_t s = rel_ind[((int64_t)b * K + k) * 2 + 0], o = rel_ind[((int64_t)b * K + k) * 2 + 1];
        ns[k] = (int)(s < 0 ? 0 : (s >= N ? N - 1 : s));
        no[k] = (int)(o < 0 ? 0 : (o >= N ? N - 1 : o));
    }
    if (!ds) return;
    const int32_t* p0 = ptr + ((int64_t)0 * B + b) * (N + 1);
    const int32_t* p1 = ptr + ((int64_t)1 * B + b) * (N + 1);
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        ds[n] = (float)(p0[n + 1] - p0[n]) + 1e-7f;
        dn_o[n] = (float)(p1[n + 1] - p1[n]) + 1e-7f;
    }
}
