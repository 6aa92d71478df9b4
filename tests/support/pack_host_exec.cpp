// Test-only, host-only: the packers of defensegan_amd/csrc/dg_pack.h run on VALUES and on an INDEX ARRAY (the gather map), for
// tests/test_gen_train_cpu.py.  Compiled with g++ (no HIP); also a stand-alone program (-DPACK_MAIN) for a sanitizer run.
//   which: 0 lin_transpose, 1 lin_fwd, 2 lin_bwd, 3 deconv_transpose, 4 deconv_frag, 5 tail32, 6 tail16
// a, b = (K, F) for the Linear layouts (c = nsplit), (cout, cin) for the deconv layouts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dg_pack.h"

namespace {
template <class T>
long long run(int which, const T* src, T* dst, int a, int b, int c) {
    switch (which) {
        case 0: dg::pack_lin_transpose(src, dst, a, b); return (long long)a * b;
        case 1: dg::pack_lin_fwd(src, dst, a, b); return (long long)a * b;
        case 2: dg::pack_lin_bwd(src, dst, a, b, c); return (long long)a * b;
        case 3: dg::pack_deconv_transpose(src, dst, a, b); return 25LL * a * b;
        case 4: dg::pack_deconv_frag(src, dst, a, b); return 25LL * a * b;
        case 5: dg::pack_tail32(src, dst, a, b); return (long long)dg::tail_pack32_elems(a, b);
        case 6: dg::pack_tail16(src, dst, b); return (long long)dg::tail_pack16_elems(b);
    }
    return -1;
}
}  // namespace

extern "C" {
// destination elements of layout `which`
long long dgk_size(int which, int a, int b) {
    if (which <= 2) return (long long)a * b;
    if (which <= 4) return 25LL * a * b;
    return which == 5 ? (long long)dg::tail_pack32_elems(a, b) : (long long)dg::tail_pack16_elems(b);
}
// dst (pre-filled with zeros by the caller) <- the values of src in layout `which`
long long dgk_pack_values(int which, const float* src, float* dst, int a, int b, int c) { return run(which, src, dst, a, b, c); }
// map (dgk_size entries) <- the gather map of layout `which`: the packer on 0, 1, 2, ..., -1 where the layout pads
long long dgk_pack_map(int which, int32_t* map, long long n_src, int a, int b, int c) {
    const std::vector<int32_t> idx = dg::pack_iota((size_t)n_src);
    const long long n = dgk_size(which, a, b);
    for (long long i = 0; i < n; ++i) map[i] = dg::kPackPad;
    return run(which, idx.data(), map, a, b, c);
}
}

#ifdef PACK_MAIN
int main() {
    int bad = 0;
    for (int nd : {64, 128}) {
        const int K = 128, F = 64 * nd;
        struct Case { int which, a, b, c; long long n_src; };
        const Case cases[] = {{0, K, F, 0, (long long)K * F}, {1, K, F, 0, (long long)K * F}, {2, K, F, 16, (long long)K * F},
                              {3, 2 * nd, 4 * nd, 0, 25LL * 8 * nd * nd}, {4, 2 * nd, 4 * nd, 0, 25LL * 8 * nd * nd},
                              {5, 1, nd, 0, 25LL * nd}, {6, 3, nd, 0, 75LL * nd}};
        for (const Case& q : cases) {
            const long long n = dgk_size(q.which, q.a, q.b);
            std::vector<float> src((size_t)q.n_src), dst((size_t)n, 0.f);
            for (size_t i = 0; i < src.size(); ++i) src[i] = (float)(i % 977) + 1.f;
            std::vector<int32_t> map((size_t)n);
            dgk_pack_values(q.which, src.data(), dst.data(), q.a, q.b, q.c);
            dgk_pack_map(q.which, map.data(), q.n_src, q.a, q.b, q.c);
            for (long long i = 0; i < n; ++i) {
                if (map[i] >= q.n_src) { ++bad; continue; }
                if ((map[i] < 0 ? 0.f : src[(size_t)map[i]]) != dst[(size_t)i]) ++bad;
            }
        }
    }
    printf("pack_host_exec: %d mismatches\n", bad);
    return bad != 0;
}
#endif
