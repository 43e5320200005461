// The nearest-image search of consensus re-ranking (include/subgc_neighbours_hip.h): `find_NNimg` of
// misc/consensus_reranking/concensus_reranking_utils/consensus_reranking.py:59-119 -- a float64 euclidean cdist over image features and
// the argsort of every row, cut at num_NNimg.
//
//   distance  scipy's cdist is the sequential sum s = s + (a[d] - b[d])^2 over ascending d, every operation rounded on its own, and a
//             correctly rounded sqrt.  The kernel keeps exactly that chain per (query, train) pair -- the expansion |a|^2 + |b|^2 - 2ab
//             and the matrix pipe both sum in another order and give other bits -- and gets its speed from the register tile alone: a
//             workgroup of 256 lanes owns 64 x 64 pairs, a lane 4 x 4 of them (16 independent chains), both operands go through LDS
//             in chunks of 32 columns, column-major with a pitch of 66 doubles.  Read side: a lane reads 16 B at column-pair tx (train) or
//             ty (query) of one d; the 16 lanes of a ds_read_b128 group hold 16 different tx (256 contiguous bytes: every bank once) and
//             at most 2 different ty (adjacent 16 B), so no read conflicts.  Write side: a 16-lane ds_write_b64 group holds 4 d-pairs x 4
//             rows -> dword (2 d) * 132 + 2 row: banks 8 dq + 2 row (+4 for the odd d), all different mod 32.
//   select    per row an MSB-first radix select over the eight 8-bit digits of the 64-bit key (decode_sample.hip's scheme, widened), a
//             scan in ascending index order that keeps the smaller keys and the lowest-indexed equal ones, and a bitonic sort of the
//             kept (key, index) pairs in LDS.  Integer work only; its pure logic is nn_select_logic.h, shared with the host check.
#include "common.h"

#include <cmath>

#include "../../include/subgc_neighbours_hip.h"
#include "nn_select_logic.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 64;           // pairs per side of a workgroup's tile
constexpr int DK = 32;             // columns per LDS chunk
constexpr int PITCH = 66;          // doubles per staged column: 64 rows + 2 (see the head of this file)

// two consecutive columns d, d + 1 of row `r` (row < rows): one 16-byte read where the operand allows it; what lies outside the matrix is
// never read and comes back as zero (it is never summed or stored either: the loops stop at D, the stores at Q / N)
template <bool VEC>
__device__ __forceinline__ double2 load_pair(const double* __restrict__ p, int64_t ld, int64_t r, int64_t rows, int d, int D) {
    double2 v = make_double2(0.0, 0.0);
    if (r < rows) {
        const double* a = p + r * ld + d;
        if (d + 1 < D) {
            if (VEC) v = *reinterpret_cast<const double2*>(a);
            else { v.x = a[0]; v.y = a[1]; }
        } else if (d < D) v.x = a[0];
    }
    return v;
}

// VEC: both bases are 16-byte aligned and both pitches even, so every column pair of every row is one 16-byte read
template <bool VEC>
__global__ __launch_bounds__(256) void nn_dist_kernel(const double* __restrict__ q, int64_t ldq, int Q, const double* __restrict__ x, int64_t ldx,
                                                      int64_t N, int D, double* __restrict__ dist, int64_t ldd, int64_t q_tiles, int64_t tiles) {
    __shared__ __attribute__((aligned(16))) double sQ[DK * PITCH];
    __shared__ __attribute__((aligned(16))) double sX[DK * PITCH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    // staging: lane -> column pair dp (4 adjacent lanes = 64 contiguous bytes of a row) and rows r16, r16 + 16, + 32, + 48
    const int dp = (tid >> 6) * 4 + (tid & 3), r16 = (tid >> 2) & 15;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {          // query tiles fastest: the tiles that share train rows run together
        const int64_t i0 = (t % q_tiles) * TILE, j0 = (t / q_tiles) * TILE;
        double acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
        double2 rq[4], rx[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            rq[p] = load_pair<VEC>(q, ldq, i0 + r16 + 16 * p, Q, 2 * dp, D);
            rx[p] = load_pair<VEC>(x, ldx, j0 + r16 + 16 * p, N, 2 * dp, D);
        }
        for (int d0 = 0; d0 < D; d0 += DK) {
            __syncthreads();                                          // the previous chunk (or tile) is no longer read
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int r = r16 + 16 * p;
                sQ[(2 * dp) * PITCH + r] = rq[p].x; sQ[(2 * dp + 1) * PITCH + r] = rq[p].y;
                sX[(2 * dp) * PITCH + r] = rx[p].x; sX[(2 * dp + 1) * PITCH + r] = rx[p].y;
            }
            __syncthreads();
            if (d0 + DK < D) {                                         // the next chunk travels while this one is summed
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    rq[p] = load_pair<VEC>(q, ldq, i0 + r16 + 16 * p, Q, d0 + DK + 2 * dp, D);
                    rx[p] = load_pair<VEC>(x, ldx, j0 + r16 + 16 * p, N, d0 + DK + 2 * dp, D);
                }
            }
            const int dn = D - d0 < DK ? D - d0 : DK;                 // no column beyond D enters a sum
            auto step = [&](int d) {
                const double2 a0 = *reinterpret_cast<const double2*>(&sQ[d * PITCH + 2 * ty]);
                const double2 a1 = *reinterpret_cast<const double2*>(&sQ[d * PITCH + 32 + 2 * ty]);
                const double2 b0 = *reinterpret_cast<const double2*>(&sX[d * PITCH + 2 * tx]);
                const double2 b1 = *reinterpret_cast<const double2*>(&sX[d * PITCH + 32 + 2 * tx]);
                const double a[4] = {a0.x, a0.y, a1.x, a1.y}, b[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const double df = a[r] - b[c];
                        acc[r][c] = acc[r][c] + df * df;
                    }
            };
            if (dn == DK) {
#pragma unroll 8
                for (int d = 0; d < DK; ++d) step(d);
            } else {
                for (int d = 0; d < dn; ++d) step(d);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = i0 + (r < 2 ? 2 * ty + r : 32 + 2 * ty + (r - 2));
            if (i >= Q) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t j = j0 + (c < 2 ? 2 * tx + c : 32 + 2 * tx + (c - 2));
                if (j < N) dist[i * ldd + j] = sqrt(acc[r][c]);
            }
        }
    }
}

constexpr int SEL_THREADS = 1024;  // >= nnsel::MAX_K: one lane per slot of the bitonic network

__global__ __launch_bounds__(SEL_THREADS) void nn_select_kernel(const double* __restrict__ dist, int64_t ldd, int64_t N, int k,
                                                                int32_t* __restrict__ idx, double* __restrict__ val) {
    __shared__ int hist[nnsel::BINS];
    __shared__ uint64_t skey[nnsel::MAX_K];
    __shared__ int32_t sidx[nnsel::MAX_K];
    __shared__ int wcnt[2][SEL_THREADS / 64];
    __shared__ uint64_t s_prefix;
    __shared__ int s_need;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t* __restrict__ row = reinterpret_cast<const uint64_t*>(dist + (int64_t)blockIdx.x * ldd);
    // the k-th smallest key, digit by digit
    uint64_t prefix = 0;
    int need = k;
    for (int pass = 0; pass < nnsel::DIGITS; ++pass) {
        if (tid < nnsel::BINS) hist[tid] = 0;
        __syncthreads();
        for (int64_t j = tid; j < N; j += SEL_THREADS) {
            const uint64_t key = nnsel::key_of(row[j]);
            if (nnsel::follows(key, prefix, pass)) atomicAdd(&hist[nnsel::digit_of(key, pass)], 1);
        }
        __syncthreads();
        if (tid < nnsel::BINS) {
            int below = 0;
            for (int b = 0; b < tid; ++b) below += hist[b];
            if (nnsel::owns_rank(below, hist[tid], need)) {
                s_prefix = prefix | ((uint64_t)tid << nnsel::shift_of(pass));
                s_need = need - below;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
    }
    // prefix = the k-th key; k - need keys are smaller; of the equal ones the `need` lowest indices belong to the list
    const uint64_t kth = prefix;
    const int n_below = k - need;
    int base_lt = 0, base_eq = 0;
    for (int64_t j0 = 0; j0 < N; j0 += SEL_THREADS) {
        const int64_t j = j0 + tid;
        const uint64_t key = j < N ? nnsel::key_of(row[j]) : ~0ull;
        const bool lt = j < N && nnsel::is_below(key, kth), eq = j < N && key == kth;
        const uint64_t m_lt = __ballot(lt), m_eq = __ballot(eq), lower = (1ull << lane) - 1ull;
        if (lane == 0) { wcnt[0][w] = __popcll(m_lt); wcnt[1][w] = __popcll(m_eq); }
        __syncthreads();
        int off_lt = base_lt + __popcll(m_lt & lower), off_eq = base_eq + __popcll(m_eq & lower), tot_lt = 0, tot_eq = 0;
        for (int v = 0; v < SEL_THREADS / 64; ++v) {
            const int a = wcnt[0][v], b = wcnt[1][v];
            if (v < w) { off_lt += a; off_eq += b; }
            tot_lt += a; tot_eq += b;
        }
        int slot = -1;
        if (lt) slot = off_lt;
        else if (nnsel::keeps_tie(key, kth, off_eq, need) && eq) slot = n_below + off_eq;
        if (slot >= 0 && slot < k) { skey[slot] = key; sidx[slot] = (int32_t)j; }
        base_lt += tot_lt; base_eq += tot_eq;
        __syncthreads();
        if (base_lt >= n_below && base_eq >= need) break;             // uniform: every lane holds the same totals
    }
    int P = 1;
    while (P < k) P <<= 1;
    if (tid >= k && tid < P) { skey[tid] = ~0ull; sidx[tid] = 0x7FFFFFFF; }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int o = tid ^ stride;
            if (tid < P && o > tid) {
                const uint64_t ka = skey[tid], kb = skey[o];
                const int32_t ia = sidx[tid], ib = sidx[o];
                const bool up = (tid & size) == 0;
                if (up ? nnsel::pair_less(kb, ib, ka, ia) : nnsel::pair_less(ka, ia, kb, ib)) {
                    skey[tid] = kb; sidx[tid] = ib; skey[o] = ka; sidx[o] = ia;
                }
            }
            __syncthreads();
        }
    if (tid < k) {
        const int32_t j = sidx[tid];
        idx[(int64_t)blockIdx.x * k + tid] = j;
        if (val && j >= 0 && j < N) val[(int64_t)blockIdx.x * k + tid] = dist[(int64_t)blockIdx.x * ldd + j];      // the entry itself: its own bits, sign included
    }
}

}  // namespace

SUBGC_API int subgc_nn_dist_f64(const double* q, int64_t ldq, int Q, const double* x, int64_t ldx, int64_t N, int D, double* dist, int64_t ldd,
                                void* stream) {
    SUBGC_REQUIRE(q && x && dist, "nn_dist_f64: null pointer (q %p, x %p, dist %p)", (const void*)q, (const void*)x, (void*)dist);
    SUBGC_REQUIRE(Q >= 1 && N >= 1 && D >= 1, "nn_dist_f64: Q = %d, N = %lld, D = %d; each must be at least 1", Q, (long long)N, D);
    SUBGC_REQUIRE(N < ((int64_t)1 << 31), "nn_dist_f64: N = %lld train rows; the lists hold 32-bit indices (N < 2^31)", (long long)N);
    SUBGC_REQUIRE(ldq >= D && ldx >= D, "nn_dist_f64: ldq = %lld, ldx = %lld; a row pitch is at least D = %d", (long long)ldq, (long long)ldx, D);
    SUBGC_REQUIRE(ldd >= N, "nn_dist_f64: ldd = %lld; the pitch of dist is at least N = %lld", (long long)ldd, (long long)N);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (uintptr_t)q % 16 == 0 && ldq % 2 == 0 && (uintptr_t)x % 16 == 0 && ldx % 2 == 0;
    const int64_t q_tiles = subgc::cdiv(Q, TILE), tiles = q_tiles * subgc::cdiv(N, TILE);
    const unsigned grid = (unsigned)(tiles < 0x7FFFFFFF ? tiles : 0x7FFFFFFF);
    if (vec) hipLaunchKernelGGL(nn_dist_kernel<true>, dim3(grid), dim3(256), 0, s, q, ldq, Q, x, ldx, N, D, dist, ldd, q_tiles, tiles);
    else hipLaunchKernelGGL(nn_dist_kernel<false>, dim3(grid), dim3(256), 0, s, q, ldq, Q, x, ldx, N, D, dist, ldd, q_tiles, tiles);
    return subgc::check_launch("nn_dist_f64");
}

SUBGC_API int subgc_nn_select_f64(const double* dist, int64_t ldd, int Q, int64_t N, int k, int32_t* idx, double* val, void* stream) {
    SUBGC_REQUIRE(dist && idx, "nn_select_f64: null pointer (dist %p, idx %p)", (const void*)dist, (void*)idx);
    SUBGC_REQUIRE(Q >= 1 && N >= 1, "nn_select_f64: Q = %d, N = %lld; each must be at least 1", Q, (long long)N);
    SUBGC_REQUIRE(N < ((int64_t)1 << 31), "nn_select_f64: N = %lld entries per row; the lists hold 32-bit indices (N < 2^31)", (long long)N);
    SUBGC_REQUIRE(ldd >= N, "nn_select_f64: ldd = %lld; the pitch of dist is at least N = %lld", (long long)ldd, (long long)N);
    const int64_t k_max = N < nnsel::MAX_K ? N : nnsel::MAX_K;
    SUBGC_REQUIRE(k >= 1 && k <= k_max, "nn_select_f64: k = %d; 1 <= k <= min(N, %d) = %lld", k, nnsel::MAX_K, (long long)k_max);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nn_select_kernel, dim3((unsigned)Q), dim3(SEL_THREADS), 0, s, dist, ldd, N, k, idx, val);
    return subgc::check_launch("nn_select_f64");
}
