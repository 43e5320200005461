// The pointwise kernels of the bf16-batched decode step (include/subgc_decode_b16_hip.h): the LSTM cell whose h lands as bf16 inside
// the next products' operands, with the x->gates table row gathered in the cell, and the beam-search fork of the mixed bf16 / fp32 state.
// Both are pure streaming: a lane owns 16-byte pieces, no LDS, no atomics.
#include "../../include/subgc_decode_b16_hip.h"
#include "bf16_util.h"
#include "common.h"

namespace {

struct CellDst { uint16_t* p[SUBGC_DECODE_B16_MAX_DST]; int64_t ld[SUBGC_DECODE_B16_MAX_DST]; int n; };

__device__ __forceinline__ void add4(float (&a)[8], const float* __restrict__ p) {
    const float4 x = *reinterpret_cast<const float4*>(p), y = *reinterpret_cast<const float4*>(p + 4);
    a[0] += x.x; a[1] += x.y; a[2] += x.z; a[3] += x.w; a[4] += y.x; a[5] += y.y; a[6] += y.z; a[7] += y.w;
}

// one lane: 8 consecutive hidden units j .. j+7 of row s.  The additions keep subgc_lstm_fwd's order (g0, g1 = table row, g2, b0, b1) and
// the activations its expressions, so c is that kernel's c on the same pre-activations.
__global__ __launch_bounds__(256) void decode_cell_b16_kernel(const float* __restrict__ g0, int64_t ld0, const float* __restrict__ table,
                                                              int64_t ldt, const int64_t* __restrict__ tok, int64_t tok_stride,
                                                              int vocab_rows, const float* __restrict__ g2, int64_t ld2,
                                                              const float* __restrict__ b0, const float* __restrict__ b1,
                                                              const float* __restrict__ c_prev, float* __restrict__ c, CellDst d, int S,
                                                              int R) {
    const int R8 = R >> 3;
    const int64_t qv = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (qv >= (int64_t)S * R8) return;
    const int s = (int)(qv / R8), j = (int)(qv % R8) << 3;
    const float* trow = nullptr;
    if (table) {
        int64_t w = tok[(int64_t)s * tok_stride];
        w = w < 0 ? 0 : (w >= vocab_rows ? vocab_rows - 1 : w);
        trow = table + w * ldt;
    }
    float pre[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int col = k * R + j;
#pragma unroll
        for (int e = 0; e < 8; ++e) pre[k][e] = 0.f;
        add4(pre[k], g0 + (int64_t)s * ld0 + col);
        if (trow) add4(pre[k], trow + col);
        if (g2) add4(pre[k], g2 + (int64_t)s * ld2 + col);
        if (b0) add4(pre[k], b0 + col);
        if (b1) add4(pre[k], b1 + col);
    }
    const int64_t q = (int64_t)s * R + j;
    float cp[8], cn[8], hn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cp[e] = 0.f;
    if (c_prev) add4(cp, c_prev + q);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float ig = sigmoidf_(pre[0][e]), fg = sigmoidf_(pre[1][e]), gg = tanhf(pre[2][e]), og = sigmoidf_(pre[3][e]);
        cn[e] = fg * cp[e] + ig * gg;
        hn[e] = og * tanhf(cn[e]);
    }
    *reinterpret_cast<float4*>(c + q) = make_float4(cn[0], cn[1], cn[2], cn[3]);
    *reinterpret_cast<float4*>(c + q + 4) = make_float4(cn[4], cn[5], cn[6], cn[7]);
    const uint2 lo = subgc_pack4(hn[0], hn[1], hn[2], hn[3]), hi = subgc_pack4(hn[4], hn[5], hn[6], hn[7]);
    const uint4 h16 = make_uint4(lo.x, lo.y, hi.x, hi.y);
#pragma unroll
    for (int k = 0; k < SUBGC_DECODE_B16_MAX_DST; ++k)
        if (k < d.n) *reinterpret_cast<uint4*>(d.p[k] + (int64_t)s * d.ld[k] + j) = h16;
}

// rows as 16-byte pieces: tensor k of the fork is `pieces[k]` uint4 wide, pitches in uint4 units
struct ForkSet { const uint4* src[4]; uint4* dst[4]; int64_t lds[4]; int64_t ldd[4]; int pieces[4]; };

__global__ __launch_bounds__(256) void decode_fork_b16_kernel(ForkSet g, const int32_t* __restrict__ rows, int S) {
    const int m = blockIdx.x, k = blockIdx.y;
    if (m >= S) return;
    int r = rows[m];
    r = r < 0 ? 0 : (r >= S ? S - 1 : r);
    const uint4* __restrict__ src = g.src[k] + (int64_t)r * g.lds[k];
    uint4* __restrict__ dst = g.dst[k] + (int64_t)m * g.ldd[k];
    for (int c = threadIdx.x; c < g.pieces[k]; c += blockDim.x) dst[c] = src[c];
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

SUBGC_API int subgc_decode_cell_b16(const float* g0, int64_t ld0, const float* table, int64_t ldt, const int64_t* tok, int64_t tok_stride,
                                    int vocab_rows, const float* g2, int64_t ld2, const float* b0, const float* b1, const float* c_prev,
                                    float* c, uint16_t* hd0, int64_t ldh0, uint16_t* hd1, int64_t ldh1, uint16_t* hd2, int64_t ldh2, int n_dst,
                                    int S, int R, void* stream) {
    SUBGC_REQUIRE(S >= 1, "decode_cell_b16: S = %d rows (need >= 1)", S);
    SUBGC_REQUIRE(R >= 8 && R % 8 == 0, "decode_cell_b16: R = %d is not a positive multiple of 8 (16-byte bf16 pieces)", R);
    SUBGC_REQUIRE(n_dst >= 1 && n_dst <= SUBGC_DECODE_B16_MAX_DST, "decode_cell_b16: %d destinations (1..%d)", n_dst, SUBGC_DECODE_B16_MAX_DST);
    SUBGC_REQUIRE(g0 && c, "decode_cell_b16: null pointer");
    SUBGC_REQUIRE(c_prev != c, "decode_cell_b16: c_prev and c are the same buffer");
    CellDst d{{hd0, hd1, hd2}, {ldh0, ldh1, ldh2}, n_dst};
    for (int k = 0; k < n_dst; ++k) {
        SUBGC_REQUIRE(d.p[k], "decode_cell_b16: destination %d of %d is null", k, n_dst);
        SUBGC_REQUIRE(al16(d.p[k]), "decode_cell_b16: destination %d is not 16-byte aligned (address mod 16 = %d)", k,
                      (int)(reinterpret_cast<uintptr_t>(d.p[k]) & 15));
        SUBGC_REQUIRE(d.ld[k] >= R && d.ld[k] % 8 == 0, "decode_cell_b16: destination %d has pitch %lld (need a multiple of 8, >= R = %d)", k,
                      (long long)d.ld[k], R);
    }
    SUBGC_REQUIRE(ld0 >= 4 * (int64_t)R && ld0 % 4 == 0 && al16(g0), "decode_cell_b16: g0 pitch %lld / alignment (need a multiple of 4, >= 4R = %d, 16 bytes)",
                  (long long)ld0, 4 * R);
    SUBGC_REQUIRE(!g2 || (ld2 >= 4 * (int64_t)R && ld2 % 4 == 0 && al16(g2)), "decode_cell_b16: g2 pitch %lld / alignment (need a multiple of 4, >= 4R = %d, 16 bytes)",
                  (long long)ld2, 4 * R);
    SUBGC_REQUIRE(al16(b0) && al16(b1) && al16(c_prev) && al16(c), "decode_cell_b16: b0 / b1 / c_prev / c must be 16-byte aligned");
    if (table) {
        SUBGC_REQUIRE(tok && vocab_rows >= 1, "decode_cell_b16: a table needs tokens and vocab_rows >= 1 (got %d)", vocab_rows);
        SUBGC_REQUIRE(ldt >= 4 * (int64_t)R && ldt % 4 == 0 && al16(table), "decode_cell_b16: table pitch %lld / alignment (need a multiple of 4, >= 4R = %d, 16 bytes)",
                      (long long)ldt, 4 * R);
        SUBGC_DEBUG_RANGE(tok, 8, S, 1, tok_stride, 0, vocab_rows - 1, -1, "decode_cell_b16: tok (word ids)", stream);
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)S * R;
    subgc::ProfScope prof(SUBGC_FAM_LSTM, s, 4.0 * n * 12,
                          (double)n * (16.0 * (1 + (table ? 1 : 0) + (g2 ? 1 : 0)) + (c_prev ? 4.0 : 0.0) + 4.0 + 2.0 * n_dst));
    hipLaunchKernelGGL(decode_cell_b16_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, s, g0, ld0, table, ldt, tok, tok_stride,
                       vocab_rows, g2, ld2, b0, b1, c_prev, c, d, S, R);
    return subgc::check_launch("subgc_decode_cell_b16");
}

SUBGC_API int subgc_decode_fork_b16(const uint16_t* sb0, int64_t lds0, uint16_t* db0, int64_t ldd0, int cb0, const uint16_t* sb1, int64_t lds1,
                                    uint16_t* db1, int64_t ldd1, int cb1, const float* sf0, int64_t ldsf0, float* df0, int64_t lddf0, int cf0,
                                    const float* sf1, int64_t ldsf1, float* df1, int64_t lddf1, int cf1, const int32_t* src, int S, void* stream) {
    SUBGC_REQUIRE(S >= 1, "decode_fork_b16: S = %d rows (need >= 1)", S);
    SUBGC_REQUIRE(src, "decode_fork_b16: null src");
    const void* sp[4] = {sb0, sb1, sf0, sf1};
    void* dp[4] = {db0, db1, df0, df1};
    const int64_t ls[4] = {lds0, lds1, ldsf0, ldsf1}, ldn[4] = {ldd0, ldd1, lddf0, lddf1};
    const int cols[4] = {cb0, cb1, cf0, cf1};
    ForkSet g;
    for (int k = 0; k < 4; ++k) {
        const int per = k < 2 ? 8 : 4;      // elements of a 16-byte piece: bf16, fp32
        SUBGC_REQUIRE(sp[k] && dp[k], "decode_fork_b16: tensor %d is null", k);
        SUBGC_REQUIRE(cols[k] >= per && cols[k] % per == 0, "decode_fork_b16: tensor %d has %d columns (need a positive multiple of %d)", k, cols[k], per);
        SUBGC_REQUIRE(ls[k] >= cols[k] && ls[k] % per == 0 && ldn[k] >= cols[k] && ldn[k] % per == 0,
                      "decode_fork_b16: tensor %d has pitches %lld / %lld (need multiples of %d, >= %d)", k, (long long)ls[k], (long long)ldn[k], per, cols[k]);
        SUBGC_REQUIRE(al16(sp[k]) && al16(dp[k]), "decode_fork_b16: tensor %d is not 16-byte aligned", k);
        SUBGC_REQUIRE(sp[k] != dp[k], "decode_fork_b16: tensor %d forks onto itself", k);
        g.src[k] = static_cast<const uint4*>(sp[k]); g.dst[k] = static_cast<uint4*>(dp[k]);
        g.lds[k] = ls[k] / per; g.ldd[k] = ldn[k] / per; g.pieces[k] = cols[k] / per;
    }
    hipLaunchKernelGGL(decode_fork_b16_kernel, dim3(S, 4), dim3(256), 0, (hipStream_t)stream, g, src, S);
    return subgc::check_launch("subgc_decode_fork_b16");
}
