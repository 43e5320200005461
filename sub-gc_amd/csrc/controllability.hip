// Noun IoU of a decode batch (include/subgc_controllability_hip.h): NounIoU.score (misc/controllability/noun_iou.py:19-47) for every
// (generated caption, ground-truth caption of its group) pair and the group mean of controllability_score.py:47-52.  One launch: a
// workgroup of four waves per token row, the waves striding the group's captions.  A wave fills the similarity matrix of its pair in LDS
// (64 x 64 fp32 = 16 KB per wave, the smaller side as rows), solves the assignment by shortest augmenting paths with dual potentials --
// one lane per column, potentials and slacks in fp64 registers, the word lists in registers too -- and writes the pair's outputs; after a
// workgroup barrier wave 0 forms the group mean in caption order.  FMA contraction is off for the whole file and both divisions are
// correctly rounded.  No atomics: every output has one writer.
#include "common.h"

#include "../../include/subgc_controllability_hip.h"

#pragma clang fp contract(off)

#include "caption.h"      // after the pragma: its functions are compiled without contraction here

namespace {

constexpr int kWords = SUBGC_CTL_MAX_WORDS;
constexpr int kWaves = 4;

// the smallest value over the 64 lanes (all active)
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}

// Maximum-weight assignment of the nr x nc matrix M (row stride kWords, 1 <= nr <= nc <= 64) that matches every row: shortest augmenting
// paths on the costs -M with dual potentials u (rows) and v (columns).  Lane c owns column c (its v, its slack, its predecessor and the
// row matched to it) and, as row `lane`, that row's u; scalars of the search are wave-uniform.  -> the row matched to the lane's column,
// or -1.  Every loop is bounded by the shape alone, so the wave ends whatever the entries hold (a NaN entry gives some matching, not a hang).
__device__ __forceinline__ int solve_assignment(const float* __restrict__ M, int nr, int nc, int lane) {
    double u = 0.0, v = 0.0;
    int p = -1;
    const int col = lane < nc ? lane : nc - 1;
    for (int i = 0; i < nr; ++i) {                          // row i enters the matching
        double slack = INFINITY;
        int way = -1;                                       // the column before the lane's on the cheapest path; -1 = the root
        bool used = lane >= nc, rowin = false;
        int i0 = i, j0 = -1;
        for (int it = 0; it <= i; ++it) {                   // the tree gains one column per round: at most the i matched ones and a free one
            if (lane == i0) rowin = true;
            const double ui = __shfl(u, i0);
            const double cur = (-(double)M[i0 * kWords + col] - ui) - v;
            if (!used && cur < slack) { slack = cur; way = j0; }
            const double delta = wave_min_f64(used ? (double)INFINITY : slack);
            unsigned long long pick = __ballot(!used && slack == delta);      // ties: the lowest column index
            if (!pick) pick = __ballot(!used);
            if (!pick) break;
            const int j1 = __ffsll((long long)pick) - 1;
            if (rowin) u += delta;
            if (used) v -= delta; else slack -= delta;
            j0 = j1;
            if (lane == j0) used = true;
            i0 = __shfl(p, j0);
            if (i0 < 0) break;                              // a free column: the path is complete
        }
        for (int s = 0; s < kWords && j0 >= 0; ++s) {       // flip the path back to the root
            const int jp = __shfl(way, j0);
            const int pi = jp < 0 ? i : __shfl(p, jp);
            if (lane == j0) p = pi;
            j0 = jp;
        }
    }
    return lane < nc ? p : -1;
}

__global__ __launch_bounds__(kWaves * 64) void noun_iou_kernel(const void* __restrict__ tok, int tok64, int T, const uint8_t* __restrict__ bad, int bad_n,
                                                               const int32_t* __restrict__ tok_noun, int n_tok_noun, const float* __restrict__ vec,
                                                               const double* __restrict__ norm, int n_noun, int d, const int32_t* __restrict__ row_group,
                                                               int n_groups, const int32_t* __restrict__ pair_off, int n_pairs,
                                                               const int32_t* __restrict__ gcap_off, int n_caps, const int32_t* __restrict__ gn_off,
                                                               const int32_t* __restrict__ gn, int n_gn, float* __restrict__ iou,
                                                               float* __restrict__ pair_iou, int32_t* __restrict__ pair_mn, int8_t* __restrict__ assign) {
    __shared__ float sim[kWaves][kWords * kWords];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = clampi(pair_off[r], 0, n_pairs), p1 = clampi(pair_off[r + 1], p0, n_pairs);
    const int g = row_group[r];
    if (g < 0 || g >= n_groups || n_noun < 1) {             // no group: zeros, count 0
        for (int64_t q = p0 + wave; q < p1; q += kWaves) {
            if (lane == 0) { pair_iou[q] = 0.f; pair_mn[q * 2] = 0; pair_mn[q * 2 + 1] = 0; }
            assign[q * kWords + lane] = -1;
        }
        if (threadIdx.x == 0) iou[r] = 0.f;
        return;
    }
    const int c0 = clampi(gcap_off[g], 0, n_caps), c1 = clampi(gcap_off[g + 1], c0, n_caps);
    const int n_cap = c1 - c0 < p1 - p0 ? c1 - c0 : p1 - p0;
    // the predicted words: lane k ends up with the vector row of the k-th word that has one
    int64_t id;
    const int L = load_row(tok, tok64, T, r, bad, bad_n, lane, id);
    int mine = -1;
    if (lane < L && id > 0 && id < n_tok_noun) mine = tok_noun[id];
    if (mine >= n_noun) mine = -1;
    const unsigned long long have = __ballot(mine >= 0);
    const int n = __popcll(have);
    int src = 0;
    {
        unsigned long long left = have;
        for (int k = 0; k < n; ++k) {                       // the position of the k-th set bit
            const int t = __ffsll((long long)left) - 1;
            if (lane == k) src = t;
            left &= left - 1;
        }
    }
    int pw = __shfl(mine, src);
    if (lane >= n) pw = 0;
    float* M = sim[wave];
    for (int q = wave; q < p1 - p0; q += kWaves) {
        const int64_t p = p0 + q;
        if (q >= n_cap) {                                   // a slot beyond the group's captions
            if (lane == 0) { pair_iou[p] = 0.f; pair_mn[p * 2] = 0; pair_mn[p * 2 + 1] = 0; }
            assign[p * kWords + lane] = -1;
            continue;
        }
        const int c = c0 + q;
        const int g0 = clampi(gn_off[c], 0, n_gn), g1 = clampi(gn_off[c + 1], g0, n_gn);
        const int m = g1 - g0 < kWords ? g1 - g0 : kWords;
        const int gw = lane < m ? clampi(gn[g0 + lane], 0, n_noun - 1) : 0;
        if (lane == 0) { pair_mn[p * 2] = m; pair_mn[p * 2 + 1] = n; }
        if (m == 0 || n == 0) {
            if (lane == 0) pair_iou[p] = m == 0 ? 1.f : 0.f;
            assign[p * kWords + lane] = -1;
            continue;
        }
        // the matrix: the smaller side as rows, the lane's word of the larger side as its column
        const bool tr = m > n;                              // rows = predicted words, columns = ground-truth words
        const int nr = tr ? n : m, nc = tr ? m : n;
        const int cw = __shfl(tr ? gw : pw, lane < nc ? lane : nc - 1);
        const float* __restrict__ b = vec + (int64_t)cw * d;
        const double nb = norm[cw];
        for (int r0 = 0; r0 < nr; r0 += 4) {
            int rw[4];
            const float* a[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                rw[t] = __builtin_amdgcn_readfirstlane(__shfl(tr ? pw : gw, r0 + t < nr ? r0 + t : nr - 1));
                a[t] = vec + (int64_t)rw[t] * d;
            }
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < d; ++k) {
                const double bk = (double)b[k];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] += (double)a[t][k] * bk;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double den = norm[rw[t]] * nb;
                const float cs = (float)(acc[t] / (den > 1e-8 ? den : 1e-8));
                if (r0 + t < nr && lane < nc) M[(r0 + t) * kWords + lane] = (cs + 1.f) / 2.f;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int prow = solve_assignment(M, nr, nc, lane);
        // the lane as ground-truth word: the predicted word matched to it
        int hit = -1;
        if (tr) {
            hit = prow;
        } else {
            for (int j = 0; j < nc; ++j) {
                const int rr = __shfl(prow, j);
                if (rr == lane) hit = j;
            }
        }
        if (lane >= m) hit = -1;
        const float s = hit >= 0 ? (tr ? M[hit * kWords + lane] : M[lane * kWords + hit]) : 0.f;
        const unsigned long long matched = __ballot(hit >= 0);
        float I = 0.f;
        for (int i = 0; i < m; ++i) {
            const float x = __shfl(s, i);
            if ((matched >> i) & 1ull) I += x;
        }
        assign[p * kWords + lane] = (int8_t)hit;
        if (lane == 0) pair_iou[p] = __fdiv_rn(I, (float)(m + n) - I);
        __builtin_amdgcn_wave_barrier();                    // the next pair's matrix is written only after every lane has read this one
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        for (int q = 0; q < n_cap; ++q) sum += pair_iou[(int64_t)p0 + q];
        iou[r] = n_cap > 0 ? __fdiv_rn(sum, (float)n_cap) : 0.f;
    }
}

}  // namespace

SUBGC_API int subgc_control_noun_iou(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, int rows, const int32_t* tok_noun, int n_tok_noun,
                                     const float* vec, const double* norm, int n_noun, int d, const int32_t* row_group, int n_groups,
                                     const int32_t* pair_off, int n_pairs, const int32_t* gcap_off, int n_caps, const int32_t* gn_off,
                                     const int32_t* gn, int n_gn, float* iou, float* pair_iou, int32_t* pair_mn, int8_t* assign, void* stream) {
    SUBGC_REQUIRE(rows >= 0 && n_tok_noun >= 0 && n_noun >= 0 && n_groups >= 0 && n_pairs >= 0 && n_caps >= 0 && n_gn >= 0 && (!bad || bad_n >= 1),
                  "control_noun_iou: rows, n_tok_noun, n_noun, n_groups, n_pairs, n_caps, n_gn >= 0, bad_n >= 1 with a bad-endings table");
    SUBGC_REQUIRE(T >= 1 && T <= kWords, "control_noun_iou: token rows need 1 <= T <= %d (got %d)", kWords, T);
    SUBGC_REQUIRE(d >= 1, "control_noun_iou: vectors need d >= 1 (got %d)", d);
    SUBGC_REQUIRE(n_noun >= 1 || n_gn == 0, "control_noun_iou: %d ground-truth vector words without a vector table", n_gn);
    if (rows == 0) return SUBGC_OK;
    SUBGC_REQUIRE(tok && row_group && pair_off && iou && (n_tok_noun == 0 || tok_noun) && (n_noun == 0 || (vec && norm)) && (n_groups == 0 || gcap_off) &&
                      (n_caps == 0 || gn_off) && (n_gn == 0 || gn) && (n_pairs == 0 || (pair_iou && pair_mn && assign)),
                  "control_noun_iou: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_RANGE(row_group, 4, 1, rows, rows, 0, (int64_t)n_groups - 1, -1, "control_noun_iou: row_group (ground-truth group of every row)", s);
    SUBGC_DEBUG_MONO("control_noun_iou", "pair_off (pairs of the rows)", "position", pair_off, rows, n_pairs, s);
    SUBGC_DEBUG_MONO("control_noun_iou", "gcap_off (CSR caption offsets of the groups)", "position", gcap_off, n_groups, n_caps, s);
    SUBGC_DEBUG_MONO("control_noun_iou", "gn_off (CSR vector-word offsets of the captions)", "position", gn_off, n_caps, n_gn, s);
    SUBGC_DEBUG_RANGE(gn, 4, 1, n_gn, n_gn, 0, (int64_t)n_noun - 1, -1, "control_noun_iou: gn (vector rows of the ground-truth words)", s);
    SUBGC_DEBUG_RANGE(tok_noun, 4, 1, n_tok_noun, n_tok_noun, 0, (int64_t)n_noun - 1, -1, "control_noun_iou: tok_noun (vector row of every word id)", s);
    hipLaunchKernelGGL(noun_iou_kernel, dim3(rows), dim3(kWaves * 64), 0, s, tok, tok64, T, bad, bad_n, tok_noun, n_tok_noun, vec, norm, n_noun, d, row_group,
                       n_groups, pair_off, n_pairs, gcap_off, n_caps, gn_off, gn, n_gn, iou, pair_iou, pair_mn, assign);
    return subgc::check_launch("subgc_control_noun_iou");
}
