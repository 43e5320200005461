// The pure logic of subgc_nn_select_f64 (neighbours.hip): the key of a distance, the digit walk of the MSB-first radix select and the
// cut among keys equal to the k-th.  Plain integer C++ without a HIP dependency: the kernel compiles it for the device and
// tools/nn_host_check.cpp compiles the SAME text for the host, where it runs under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NN_HD __host__ __device__ __forceinline__
#else
#define NN_HD inline
#endif

namespace nnsel {

constexpr int DIGITS = 8;          // 8-bit digits of a 64-bit key, most significant first
constexpr int BINS = 256;
constexpr int MAX_K = 1024;

// The distance's bit pattern with the sign bit cleared, as an unsigned integer: monotone for distances >= 0 (-0 = +0), +inf
// (0x7FF0...) above every finite value, every NaN (0x7FF0... + a non-zero mantissa, either sign) above +inf -- where np.argsort puts it.
NN_HD uint64_t key_of(uint64_t bits) { return bits & 0x7FFFFFFFFFFFFFFFull; }

NN_HD int shift_of(int pass) { return 8 * (DIGITS - 1 - pass); }
NN_HD int digit_of(uint64_t key, int pass) { return (int)((key >> shift_of(pass)) & 255u); }
// does `key` carry the digits chosen in passes 0 .. pass-1 (the high 8 * pass bits of `prefix`)?  pass 0: every key does
NN_HD bool follows(uint64_t key, uint64_t prefix, int pass) { return pass == 0 || ((key ^ prefix) >> (shift_of(pass) + 8)) == 0ull; }

// One step of the walk over a pass's histogram for the lane that owns bin `d`: `below` = keys in bins < d, `here` = keys in bin d,
// `need` = the rank (1-based) of the wanted key among the keys of the histogram.  True for exactly one bin: the one holding that rank.
NN_HD bool owns_rank(int below, int here, int need) { return below < need && need <= below + here; }

// After the last pass `prefix` IS the k-th smallest key and `need` says how many keys equal to it belong to the list.  A key is kept
// when it is smaller, or equal with fewer than `need` equal keys at lower indices (eq_rank: 0-based, in ascending index order).
NN_HD bool is_below(uint64_t key, uint64_t kth) { return key < kth; }
NN_HD bool keeps_tie(uint64_t key, uint64_t kth, int eq_rank, int need) { return key == kth && eq_rank < need; }

// The order of the kept pairs: ascending (key, index).
NN_HD bool pair_less(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

}  // namespace nnsel
