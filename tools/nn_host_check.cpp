// Host transliteration of subgc_nn_select_f64 (sub-gc_amd/csrc/neighbours.hip) over the SAME pure logic the kernel compiles
// (sub-gc_amd/csrc/nn_select_logic.h): the key transform, the digit walk of the radix select, the cut among equal keys and the order of
// the bitonic network.  A stand-alone program for the address and undefined-behaviour sanitizers on the CPU (tools/nn_host_check.py
// builds and runs it); the workgroup's lanes become loops, the LDS arrays std::vectors of the kernel's sizes.
//
//   nn_host_check in.bin out.bin
//   in.bin:  int64 Q, N, k; double dist[Q * N]          out.bin: int32 idx[Q * k]; double val[Q * k]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sub-gc_amd/csrc/nn_select_logic.h"

namespace {

constexpr int THREADS = 1024;

bool select_row(const double* dist, int64_t N, int k, int32_t* idx, double* val) {
    std::vector<uint64_t> row(N);
    std::memcpy(row.data(), dist, sizeof(double) * N);
    uint64_t prefix = 0;
    int need = k;
    for (int pass = 0; pass < nnsel::DIGITS; ++pass) {
        std::vector<int> hist(nnsel::BINS, 0);
        for (int64_t j = 0; j < N; ++j) {
            const uint64_t key = nnsel::key_of(row[j]);
            if (nnsel::follows(key, prefix, pass)) hist[nnsel::digit_of(key, pass)] += 1;
        }
        int owners = 0, below = 0;
        uint64_t next_prefix = 0;
        int next_need = 0;
        for (int d = 0; d < nnsel::BINS; ++d) {                          // lane d of the kernel
            if (nnsel::owns_rank(below, hist[d], need)) {
                next_prefix = prefix | ((uint64_t)d << nnsel::shift_of(pass));
                next_need = need - below;
                ++owners;
            }
            below += hist[d];
        }
        if (owners != 1) { std::fprintf(stderr, "pass %d: %d bins own the rank\n", pass, owners); return false; }
        prefix = next_prefix;
        need = next_need;
    }
    const uint64_t kth = prefix;
    const int n_below = k - need;
    std::vector<uint64_t> skey(nnsel::MAX_K);
    std::vector<int32_t> sidx(nnsel::MAX_K);
    std::vector<char> filled(nnsel::MAX_K, 0);
    int base_lt = 0, base_eq = 0;
    for (int64_t j0 = 0; j0 < N; j0 += THREADS) {
        int tot_lt = 0, tot_eq = 0;
        for (int tid = 0; tid < THREADS; ++tid) {                        // ascending lanes = ascending index: the kernel's ballot prefix
            const int64_t j = j0 + tid;
            if (j >= N) break;
            const uint64_t key = nnsel::key_of(row[j]);
            const bool lt = nnsel::is_below(key, kth), eq = key == kth;
            int slot = -1;
            if (lt) slot = base_lt + tot_lt;
            else if (eq && nnsel::keeps_tie(key, kth, base_eq + tot_eq, need)) slot = n_below + base_eq + tot_eq;
            if (slot >= 0 && slot < k) {
                if (filled[slot]) { std::fprintf(stderr, "slot %d written twice\n", slot); return false; }
                skey[slot] = key; sidx[slot] = (int32_t)j; filled[slot] = 1;
            }
            tot_lt += lt; tot_eq += eq;
        }
        base_lt += tot_lt; base_eq += tot_eq;
        if (base_lt >= n_below && base_eq >= need) break;
    }
    for (int c = 0; c < k; ++c)
        if (!filled[c]) { std::fprintf(stderr, "slot %d of %d never written\n", c, k); return false; }
    int P = 1;
    while (P < k) P <<= 1;
    for (int c = k; c < P; ++c) { skey[c] = ~0ull; sidx[c] = 0x7FFFFFFF; }
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1)
            for (int tid = 0; tid < P; ++tid) {
                const int o = tid ^ stride;
                if (o <= tid) continue;
                const bool up = (tid & size) == 0;
                if (up ? nnsel::pair_less(skey[o], sidx[o], skey[tid], sidx[tid]) : nnsel::pair_less(skey[tid], sidx[tid], skey[o], sidx[o])) {
                    const uint64_t tk = skey[tid]; skey[tid] = skey[o]; skey[o] = tk;
                    const int32_t ti = sidx[tid]; sidx[tid] = sidx[o]; sidx[o] = ti;
                }
            }
    for (int c = 0; c < k; ++c) { idx[c] = sidx[c]; val[c] = dist[sidx[c]]; }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: nn_host_check in.bin out.bin\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int64_t head[3];
    if (std::fread(head, sizeof(int64_t), 3, f) != 3) return 2;
    const int64_t Q = head[0], N = head[1], k = head[2];
    if (Q < 1 || N < 1 || k < 1 || k > N || k > nnsel::MAX_K) { std::fprintf(stderr, "bad sizes\n"); return 2; }
    std::vector<double> dist((size_t)(Q * N));
    if (std::fread(dist.data(), sizeof(double), dist.size(), f) != dist.size()) return 2;
    std::fclose(f);
    std::vector<int32_t> idx((size_t)(Q * k));
    std::vector<double> val((size_t)(Q * k));
    for (int64_t i = 0; i < Q; ++i)
        if (!select_row(dist.data() + i * N, N, (int)k, idx.data() + i * k, val.data() + i * k)) return 1;
    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    std::fwrite(idx.data(), sizeof(int32_t), idx.size(), f);
    std::fwrite(val.data(), sizeof(double), val.size(), f);
    std::fclose(f);
    return 0;
}
