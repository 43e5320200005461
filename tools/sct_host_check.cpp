// Stand-alone host transliteration of sub-gc_amd/csrc/control_input.hip for sanitizer runs on the CPU (tools/sct_host_check.py builds it
// with -fsanitize=address,undefined -ffp-contract=off and feeds it the loader fixture).  A wave is a loop over 64 lanes; every global
// index expression is the kernel's own, on heap buffers of exactly the sizes the host module allocates, so an index that leaves a row is
// a sanitizer report here instead of a fault on the device.  The IoU and the box scaling are the kernel's (control_input_math.h).
//
//   sct_host_check <in.bin> <out.bin>
// in : int32 B, n_obj, C, n_sets, R, obj_num, rel_num, n_rel, n_seed, gt;  boxes, img_wh, regions (fp32); set_off (int64); object_dist
//      (fp32); rel_ind, rel_off, gt_seed, gt_seed_off (int64; the gt arrays only when gt != 0)
// out: seed_mask u64, match_idx i32, match_iou f32, status i32, object_cls i32, gpn_obj_ind i64, att_masks f32, gpn_pool_mtx f32,
//      gpn_pred_ind i64, gpn_nrel_ind i64, choice i32, status after the look-up i32
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../sub-gc_amd/csrc/control_input_math.h"

namespace {

constexpr int W = 64, GT_LISTS = 5, MAX_CHUNKS = 16;
enum { ST_OK = 0, ST_NO_OVERLAP = 1, ST_NO_GT = 2 };

template <class T>
std::vector<T> get(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T>
void put(FILE* f, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
}

int image_of(const int64_t* set_off, int B, int s) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (set_off[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}
uint64_t below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }
int ffs64(uint64_t m) { return __builtin_ctzll(m); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: sct_host_check in.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> h = get<int32_t>(f, 10);
    const int B = h[0], n_obj = h[1], C = h[2], n_sets = h[3], R = h[4], obj_num = h[5], rel_num = h[6], n_rel = h[7], n_seed = h[8], gt = h[9];
    if (n_obj < 1 || n_obj > W || R < 1 || R > W || obj_num < n_obj + 1 || rel_num < 2 || rel_num > W * MAX_CHUNKS || B < 1) { fprintf(stderr, "refused\n"); return 3; }
    const auto boxes = get<float>(f, (size_t)B * n_obj * 4);
    const auto img_wh = get<float>(f, (size_t)B * 2);
    const auto regions = get<float>(f, (size_t)n_sets * R * 5);
    const auto set_off = get<int64_t>(f, (size_t)B + 1);
    const auto dist = get<float>(f, (size_t)B * n_obj * C);
    const auto rel_ind = get<int64_t>(f, (size_t)n_rel * 2);
    const auto rel_off = get<int64_t>(f, (size_t)B + 1);
    const auto gt_seed = get<int64_t>(f, gt ? (size_t)n_seed : 0);
    const auto gt_seed_off = get<int64_t>(f, gt ? (size_t)B * GT_LISTS + 1 : 0);
    fclose(f);

    std::vector<uint64_t> seed_mask(n_sets);
    std::vector<int32_t> match_idx((size_t)n_sets * R), status(n_sets), cls((size_t)B * n_obj), choice(n_sets, -1);
    std::vector<float> match_iou((size_t)n_sets * R), att((size_t)n_sets * obj_num), pool((size_t)n_sets * obj_num * obj_num);
    std::vector<int64_t> obj((size_t)n_sets * obj_num), pred((size_t)n_sets * rel_num), nrel((size_t)n_sets * rel_num * 2);

    // sct_match_kernel
    for (int s = 0; s < n_sets; ++s) {
        const int b = image_of(set_off.data(), B, s);
        SubgcSctBox det[W], mine[W];
        bool flag[W];
        for (int lane = 0; lane < W; ++lane) {
            det[lane] = mine[lane] = SubgcSctBox{0.f, 0.f, 0.f, 0.f};
            flag[lane] = false;
            if (lane < n_obj) {
                const float* d = &boxes[((int64_t)b * n_obj + lane) * 4];
                det[lane] = subgc_sct_scale(SubgcSctBox{d[0], d[1], d[2], d[3]}, img_wh[2 * b], img_wh[2 * b + 1]);
            }
            if (lane < R) {
                const float* reg = &regions[(int64_t)s * R * 5];
                mine[lane] = SubgcSctBox{reg[lane * 5], reg[lane * 5 + 1], reg[lane * 5 + 2], reg[lane * 5 + 3]};
                flag[lane] = reg[lane * 5 + 4] != 0.f;
            }
        }
        int valid = 0;
        for (int lane = 0; lane < W; ++lane) valid += flag[lane];
        int my_idx[W];
        float my_iou[W];
        for (int lane = 0; lane < W; ++lane) { my_idx[lane] = -1; my_iou[lane] = 0.f; }
        for (int j = 0; j < valid; ++j) {
            float v[W], mx = 0.f;
            for (int lane = 0; lane < W; ++lane) {
                v[lane] = lane < n_obj ? subgc_sct_iou(mine[j], det[lane]) : 0.f;
                v[lane] = v[lane] > 0.f ? v[lane] : 0.f;
                mx = std::fmax(mx, v[lane]);
            }
            uint64_t at = 0;
            for (int lane = 0; lane < W; ++lane) at |= (uint64_t)(mx > 0.f && v[lane] == mx) << lane;
            if (at) { my_idx[j] = ffs64(at); my_iou[j] = mx; }
        }
        uint64_t keep = 0, any = 0;
        float best = 0.f;
        for (int lane = 0; lane < W; ++lane) {
            const bool m = my_idx[lane] >= 0;
            keep |= (uint64_t)(m && my_iou[lane] >= 0.5f) << lane;
            any |= (uint64_t)m << lane;
            best = std::fmax(best, m ? my_iou[lane] : 0.f);
        }
        if (keep == 0)
            for (int lane = 0; lane < W; ++lane) keep |= (uint64_t)(my_idx[lane] >= 0 && my_iou[lane] >= best) << lane;
        uint64_t seeds = 0;
        for (uint64_t m = keep; m; m &= m - 1) seeds |= 1ull << (my_idx[ffs64(m)] & 63);
        for (int lane = 0; lane < W; ++lane)
            if (lane < R) {
                match_idx[(int64_t)s * R + lane] = my_idx[lane];
                match_iou[(int64_t)s * R + lane] = my_iou[lane];
            }
        seed_mask[s] = seeds;
        status[s] = any ? ST_OK : ST_NO_OVERLAP;
    }

    // sct_class_kernel
    for (int64_t row = 0; row < (int64_t)B * n_obj; ++row) {
        const float* x = &dist[row * C];
        float best[W], mx = -INFINITY;
        int at[W];
        for (int lane = 0; lane < W; ++lane) {
            best[lane] = -INFINITY;
            at[lane] = 0x7fffffff;
            for (int c = lane; c < C; c += 64) {
                const float v = x[c];
                if (v > best[lane] || at[lane] == 0x7fffffff) { best[lane] = v; at[lane] = c; }
            }
            mx = std::fmax(mx, best[lane]);
        }
        int cand = 0x7fffffff;
        for (int lane = 0; lane < W; ++lane)
            if (at[lane] != 0x7fffffff && best[lane] == mx && at[lane] < cand) cand = at[lane];
        cls[row] = cand == 0x7fffffff ? 0 : cand;
    }

    // sct_extract_greedy_kernel
    for (int s = 0; s < n_sets; ++s) {
        unsigned int s_nodes[2] = {0u, 0u};
        int s_sel[64];
        const int b = image_of(set_off.data(), B, s);
        const bool ok = status[s] == ST_OK;
        const uint64_t seeds = ok ? (seed_mask[s] & below(n_obj)) : 0ull;
        int my_cls[W];
        for (int lane = 0; lane < W; ++lane) my_cls[lane] = lane < n_obj ? cls[(int64_t)b * n_obj + lane] : -1;
        uint64_t nodes0 = 0;
        for (int lane = 0; lane < W; ++lane) {
            bool in = false;
            for (uint64_t m = seeds; m; m &= m - 1) in = in || (lane < n_obj && my_cls[lane] == my_cls[ffs64(m)]);
            nodes0 |= (uint64_t)in << lane;
        }
        const int64_t k0 = rel_off[b];
        const int nk = ok ? (int)std::min<int64_t>(rel_num - 1, std::max<int64_t>(0, rel_off[b + 1] - k0)) : 0;
        const int chunks = (nk + 63) >> 6;
        uint64_t kept[MAX_CHUNKS];
        for (int ch = 0; ch < MAX_CHUNKS; ++ch) {
            kept[ch] = 0;
            if (ch < chunks)
                for (int lane = 0; lane < W; ++lane) {
                    const int r = ch * 64 + lane;
                    bool k = false;
                    if (r < nk) {
                        const int64_t e0 = rel_ind[(k0 + r) * 2], e1 = rel_ind[(k0 + r) * 2 + 1];
                        const bool v0 = e0 >= 0 && e0 < n_obj, v1 = e1 >= 0 && e1 < n_obj;
                        k = (v0 && ((nodes0 >> e0) & 1)) || (v1 && ((nodes0 >> e1) & 1));
                        if (k) {
                            if (v0) s_nodes[e0 >> 5] |= 1u << (e0 & 31);
                            if (v1) s_nodes[e1 >> 5] |= 1u << (e1 & 31);
                        }
                    }
                    kept[ch] |= (uint64_t)k << lane;
                }
        }
        const uint64_t nodes = nodes0 | ((uint64_t)s_nodes[0] | ((uint64_t)s_nodes[1] << 32));
        const int n_nodes = __builtin_popcountll(nodes);
        for (int lane = 0; lane < W; ++lane)
            if ((nodes >> lane) & 1) s_sel[__builtin_popcountll(nodes & below(lane))] = lane;
        for (int lane = 0; lane < W; ++lane)
            for (int i = lane; i < obj_num; i += 64) {
                obj[(int64_t)s * obj_num + i] = i < n_nodes ? s_sel[i] : obj_num - 1;
                att[(int64_t)s * obj_num + i] = i < n_nodes ? 1.f : 0.f;
            }
        float* pm = &pool[(int64_t)s * obj_num * obj_num];
        for (int lane = 0; lane < W; ++lane)
            for (int q = lane; q < obj_num * obj_num; q += 64) {
                const int r = q / obj_num, c = q - r * obj_num;
                pm[q] = (r == c && r < n_nodes) ? 1.f : 0.f;
            }
        int64_t* pr = &pred[(int64_t)s * rel_num];
        int64_t* nr = &nrel[(int64_t)s * rel_num * 2];
        int before = 0;
        for (int ch = 0; ch < MAX_CHUNKS; ++ch)
            if (ch < chunks) {
                for (int lane = 0; lane < W; ++lane) {
                    const int r = ch * 64 + lane;
                    if ((kept[ch] >> lane) & 1) {
                        const int at = before + __builtin_popcountll(kept[ch] & below(lane));
                        const int64_t e0 = rel_ind[(k0 + r) * 2], e1 = rel_ind[(k0 + r) * 2 + 1];
                        pr[at] = r;
                        nr[2 * at] = (e0 >= 0 && e0 < n_obj) ? __builtin_popcountll(nodes & below((int)e0)) : obj_num - 1;
                        nr[2 * at + 1] = (e1 >= 0 && e1 < n_obj) ? __builtin_popcountll(nodes & below((int)e1)) : obj_num - 1;
                    }
                }
                before += __builtin_popcountll(kept[ch]);
            }
        for (int lane = 0; lane < W; ++lane)
            for (int i = before + lane; i < rel_num; i += 64) {
                pr[i] = rel_num - 1;
                nr[2 * i] = obj_num - 1;
                nr[2 * i + 1] = obj_num - 1;
            }
    }

    // sct_gt_lookup_kernel
    std::vector<int32_t> status2 = status;
    if (gt)
        for (int s = 0; s < n_sets; ++s) {
            const int b = image_of(set_off.data(), B, s);
            const int st = status2[s];
            const uint64_t want = seed_mask[s];
            int found = -1;
            for (int j = 0; j < GT_LISTS; ++j) {
                int64_t a = gt_seed_off[b * GT_LISTS + j], e = gt_seed_off[b * GT_LISTS + j + 1];
                a = std::max<int64_t>(0, a);
                e = std::min<int64_t>(n_seed, e);
                uint64_t m = 0;
                bool bad = false;
                for (int lane = 0; lane < W; ++lane)
                    for (int64_t i = a + lane; i < e; i += 64) {
                        const int64_t v = gt_seed[i];
                        if (v >= 0 && v < n_obj) m |= 1ull << v; else bad = true;
                    }
                if (found < 0 && !bad && m == want) found = j;
            }
            choice[s] = st == ST_OK ? found : -1;
            if (st == ST_OK && found < 0) status2[s] = ST_NO_GT;
        }

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    put(o, seed_mask); put(o, match_idx); put(o, match_iou); put(o, status); put(o, cls); put(o, obj); put(o, att); put(o, pool); put(o, pred);
    put(o, nrel); put(o, choice); put(o, status2);
    fclose(o);
    return 0;
}
