// The generator's training step on the device (the generator half of the reference's train(), models/gan.py:167-199, 273-293, for
// the MNIST / F-MNIST generator without Batchnorm): forward on N latent rows, a backward seeded from OUTSIDE (dy = the gradient with
// respect to the generator's output after the sigmoid -- for WGAN-GP the critic's input gradient), the weight and bias gradients of
// the Linear layer and of the three transposed convolutions in the reference's layouts, TF's Adam on them, and the refresh of every
// derived weight layout of the engine.  fp32 throughout; gfx950.
//
// One call is a sequence of launches on the caller's stream:
//   forward          the engine's run_forward (NHWC path): h1 [N,4,4,4nd], h2 [N,7,7,2nd], h3 [N,14,14,nd] and y [N,28,28,1] stay in
//                    the engine's buffers
//   seed             dpre5 = dy * y * (1 - y)                                                   gen_seed_kernel
//   Generator.5      dF5 [5,5,1,nd], db5 from (dpre5, h3); then da2 = ReluGrad(h3) o (dpre5 * F5) IN PLACE over h3 -- a seeded form
//                    beside the projection's tails, which derive their seed from y - x and stay as they are
//   Generator.3      dF3, db3 from (dpre3 = the masked da2 in h3's buffer, h2); then the engine's Bd[1] in place over h2
//   Generator.2      dF2, db2 from (dpre2, h1); then the engine's Bd[0] in place over h1
//   Linear           dW = z^T dpre1, db = sum_n dpre1; then the engine's B1 and the slice sum -> dz
//   (step only)      Adam on the parameters, then one gather launch per derived layout
//
// ORDER.  The engine's backward runs in place: da overwrites the activation it masks.  A layer's weight gradient needs that layer's
// INPUT activation and the pre-activation gradient of its OUTPUT, so per layer, from the top down: weight gradient first, then
// backward-to-input (run_backward's before_layer hook, dg_engine.cpp).
//
// Weight gradient of a transposed convolution (stride 2, 5x5, output index i = 2 o + k - 1, output cropped to `used`):
//   dF[kh,kw,co,ci] = sum_n sum_(oh,ow) dpre[n, 2 oh + kh - 1, 2 ow + kw - 1, co] * a_in[n, oh, ow, ci]
// over the (oh, ow) whose output position lies inside the USED extent.  Generator.2 materialises 8x8 and keeps 7x7: row and column 7
// receive no gradient, so its taps are those of an 8x8 output with these positions removed (archs.valid_taps_1d), not those of a
// SAME convolution on 7x7.  dF2, dF3 and the Linear dW run on v_mfma_f32_32x32x2_f32 (gen_wgrad_mfma_kernel: one 32 x 64 tile of a
// tap's [co][ci] matrix per wave, the K axis = (row, oh, ow) gathered straight from the NHWC buffers, both operands read in 128-byte
// runs); dF5 (25 nd outputs) and the bias sums are plain reductions.  No float atomics: every reduction axis is cut into chunks
// whose number and length depend on the shapes (N and the layer) alone, each chunk is summed in index order and the chunk sums are
// added in chunk order -- two identical calls return identical bits.
//
// The parameters in the reference layouts (dg_handle::lin_w, lin_b, F[d], bias[d]) are the master copy Adam updates; m and v are
// flat arrays in the order of archs.weight_shapes(arch, use_bn=False) (W, b, then Filters and Biases per deconv), the step count
// is the handle's and enters the launch as lr_t (computed in float64 on the host, as dg_critic_step does).  The derived layouts
// (lin_wt, the Linear packs, Ft, Fp, the tail packs) are refreshed by gather maps made once per handle by running the packers of
// dg_pack.h on an index array: dst[i] = map[i] < 0 ? 0 : src[map[i]].  Neither a host round trip nor a synchronisation.
#include "dg_engine.h"
#include "dg_gen_internal.h"
#include "dg_pack.h"

struct GenTrain {
    float* dpre5 = nullptr;        // [cap_N, 784]
    int64_t cap_N = 0;
    float* part = nullptr;         // chunk sums of the reduction in flight (one at a time on the stream)
    size_t part_floats = 0;
    float* grads = nullptr;        // [n_params] flat gradient of a step (dg_gen_step only: dg_gen_param_gradient writes the caller's)
    float* m = nullptr;            // Adam moments, flat
    float* v = nullptr;
    long long t = 0;               // Adam steps taken since the last reset
    struct Map { float* dst; const float* src; int32_t* map; size_t n; };
    std::vector<Map> maps;
    uint64_t maps_epoch = ~0ull;
};

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxChunks = 256;      // chunk sums of a plain reduction
constexpr int kMaxSplits = 16;       // K splits of an MFMA weight gradient
constexpr int kSplitK = 256;         // their length while that gives at most kMaxSplits

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void gen_seed_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dpre,
                                                        long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float yy = y[e];
    dpre[e] = dy[e] * yy * (1.0f - yy);
}

// valid input positions of tap k along one axis: 0 <= 2 o + k - 1 < used, 0 <= o < h_in
__host__ __device__ inline void tap_range(int k, int h_in, int used, int* lo, int* hi) {
    *lo = k == 0 ? 1 : 0;
    const int top = (used - k) / 2;
    *hi = top < h_in - 1 ? top : h_in - 1;
}

// dF5 partial sums: block (chunk of rows, tap), thread = input channel; part [chunks][25][C]
__global__ void gen_tail_wgrad_kernel(const float* __restrict__ dpre5, const float* __restrict__ h3, float* __restrict__ part, int N, int C,
                                      int rows_per_chunk) {
    const int chunk = blockIdx.x, t = blockIdx.y, ci = threadIdx.x;
    const int kh = t / 5, kw = t % 5;
    int lo_h, hi_h, lo_w, hi_w;
    tap_range(kh, 14, 28, &lo_h, &hi_h);
    tap_range(kw, 14, 28, &lo_w, &hi_w);
    const int n1 = min(N, (chunk + 1) * rows_per_chunk);
    float acc = 0.f;
    for (int n = chunk * rows_per_chunk; n < n1; ++n)
        for (int ih = lo_h; ih <= hi_h; ++ih)
            for (int iw = lo_w; iw <= hi_w; ++iw)
                acc = fmaf(dpre5[(long long)n * 784 + (2 * ih + kh - 1) * 28 + (2 * iw + kw - 1)], h3[((long long)n * 196 + ih * 14 + iw) * C + ci], acc);
    part[((long long)chunk * 25 + t) * C + ci] = acc;
}

// da2 = ReluGrad(h3) o (dpre5 * F5), in place over h3 [N,14,14,C]; F5 [5,5,1,C]
__global__ __launch_bounds__(256) void gen_tail_bwd_kernel(float* __restrict__ h3, const float* __restrict__ dpre5, const float* __restrict__ F5,
                                                            long long total, int C) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int ci = (int)(e % C);
    const long long q = e / C;
    const int pos = (int)(q % 196);
    const long long n = q / 196;
    const int ih = pos / 14, iw = pos % 14;
    float acc = 0.f;
    if (h3[e] > 0.f) {
        for (int kh = 0; kh < 5; ++kh) {
            const int oh = 2 * ih + kh - 1;
            if (oh < 0 || oh >= 28) continue;
            for (int kw = 0; kw < 5; ++kw) {
                const int ow = 2 * iw + kw - 1;
                if (ow < 0 || ow >= 28) continue;
                acc = fmaf(dpre5[n * 784 + oh * 28 + ow], F5[(kh * 5 + kw) * C + ci], acc);
            }
        }
    }
    h3[e] = acc;
}

// column sums of src [rows][C] over chunks of rows: part [chunks][C]
__global__ __launch_bounds__(256) void gen_colsum_kernel(const float* __restrict__ src, long long rows, int C, long long rows_per_chunk,
                                                          float* __restrict__ part) {
    const long long r0 = (long long)blockIdx.x * rows_per_chunk;
    const long long r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (long long r = r0; r < r1; ++r) acc += src[r * C + c];
        part[(long long)blockIdx.x * C + c] = acc;
    }
}

// out[e] = sum of the chunk sums in chunk order
__global__ __launch_bounds__(256) void gen_reduce_kernel(const float* __restrict__ part, int slots, long long per, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    float g = 0.f;
    for (int z = 0; z < slots; ++z) g += part[(long long)z * per + e];
    out[e] = g;
}

// Weight gradient of a transposed convolution (or, with taps == 1, h_in == used == 1, of the Linear layer) on fp32 MFMA.
//   A = dpre [N][Po][Po][M], B = a_in [N][Pi][Pi][Nn], part [splits][taps][M][Nn]
// One wave per 32 (M) x 64 (Nn) tile of one tap, four waves per workgroup; blockIdx.y = the K split.  The K axis of tap (kh, kw) is
// (n, oh, ow) over the tap's valid positions; lanes 0-31 take the even, lanes 32-63 the odd term of a k-pair (the A / B operand
// layout of v_mfma_f32_32x32x2_f32: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]), so a wave's loads are
// 128-byte runs of 32 channels.
struct WgradArgs {
    const float* A;
    const float* B;
    float* part;
    int N, taps, M, Nn, h_in, Pi, Po, used, kchunk;
};

__global__ __launch_bounds__(256) void gen_wgrad_mfma_kernel(WgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tn = a.Nn / 64, tm = a.M / 32;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= a.taps * tm * tn) return;                    // (no barrier in this kernel)
    const int t = tile / (tm * tn), rem = tile % (tm * tn);
    const int m0 = (rem / tn) * 32, n0 = (rem % tn) * 64;
    const int kh = a.taps == 1 ? 1 : t / 5, kw = a.taps == 1 ? 1 : t % 5;
    int lo_h, hi_h, lo_w, hi_w;
    tap_range(kh, a.h_in, a.used, &lo_h, &hi_h);
    tap_range(kw, a.h_in, a.used, &lo_w, &hi_w);
    const int cnt_h = hi_h - lo_h + 1, cnt_w = hi_w - lo_w + 1;
    const long long per_row = (cnt_h > 0 && cnt_w > 0) ? (long long)cnt_h * cnt_w : 0;
    const long long K = (long long)a.N * per_row;
    const long long k0 = (long long)blockIdx.y * a.kchunk;
    const long long k1 = k0 + a.kchunk < K ? k0 + a.kchunk : K;
    const int col = lane & 31;
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    if (k0 < k1) {
        long long kk = k0 + (lane >> 5);
        long long n = kk / per_row;
        const int r = (int)(kk % per_row);
        int ih = lo_h + r / cnt_w, iw = lo_w + r % cnt_w;
        const long long a_row = (long long)a.Po * a.Po * a.M, b_row = (long long)a.Pi * a.Pi * a.Nn;
        for (long long k = k0; k < k1; k += 2) {
            float av = 0.f, b0 = 0.f, b1 = 0.f;
            if (kk < k1) {
                const float* ap = a.A + n * a_row + (long long)((2 * ih + kh - 1) * a.Po + (2 * iw + kw - 1)) * a.M + m0 + col;
                const float* bp = a.B + n * b_row + (long long)(ih * a.Pi + iw) * a.Nn + n0 + col;
                av = *ap;
                b0 = bp[0];
                b1 = bp[32];
            }
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
            kk += 2;
            iw += 2;
            while (iw > hi_w) { iw -= cnt_w; ++ih; }
            while (ih > hi_h) { ih -= cnt_h; ++n; }
        }
    }
    // C / D layout: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    float* out = a.part + ((long long)blockIdx.y * a.taps + t) * a.M * a.Nn;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        out[(long long)row * a.Nn + n0 + col] = acc0[i];
        out[(long long)row * a.Nn + n0 + col + 32] = acc1[i];
    }
}

// TF's Adam on the eight parameter tensors at once: element e of the flat order belongs to the first segment whose end exceeds it
struct AdamSegs {
    float* p[8];
    long long end[8];
};
__global__ __launch_bounds__(256) void gen_adam_kernel(AdamSegs sg, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        long long total, float lr_t, float b1, float b2) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int s = 0;
    while (s < 7 && e >= sg.end[s]) ++s;
    float* p = sg.p[s] + (e - (s ? sg.end[s - 1] : 0));
    const float gg = g[e];
    const float mm = b1 * m[e] + (1.0f - b1) * gg;
    const float vv = b2 * v[e] + (1.0f - b2) * (gg * gg);
    m[e] = mm;
    v[e] = vv;
    *p = *p - lr_t * mm / (sqrtf(vv) + 1e-8f);
}

__global__ __launch_bounds__(256) void gen_gather_kernel(float* __restrict__ dst, const float* __restrict__ src, const int32_t* __restrict__ map,
                                                          long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t j = map[i];
    dst[i] = j < 0 ? 0.f : src[j];
}

unsigned grid_of(long long total) { return (unsigned)((total + 255) / 256); }

// ------------------------------------------------------------------------------------------------ host
// the eight tensors in the order of archs.weight_shapes(arch, use_bn=False)
struct ParamSeg {
    std::string name;
    float* ptr;
    long long n, off;
};
std::vector<ParamSeg> param_segs(const dg_handle* h) {
    std::vector<ParamSeg> v;
    long long off = 0;
    auto add = [&](const std::string& nm, float* p, long long n) { v.push_back({nm, p, n, off}); off += n; };
    add("Generator.Input.W", h->lin_w, (long long)h->latent * h->lin_out);
    add("Generator.Input.b", h->lin_b, h->lin_out);
    for (size_t d = 0; d < h->dec.size(); ++d) {
        add(std::string(h->dec[d].name) + ".Filters", h->F[d], 25LL * h->dec[d].cout * h->dec[d].cin);
        add(std::string(h->dec[d].name) + ".Biases", h->bias[d], h->dec[d].cout);
    }
    return v;
}
long long param_total(const dg_handle* h) {
    const auto v = param_segs(h);
    return v.back().off + v.back().n;
}

struct SplitPlan { int chunks; long long len; };
// a reduction axis of `total` terms in at most `max_chunks` chunks of at least `min_len`: a function of the shapes alone
SplitPlan split_axis(long long total, int max_chunks, long long min_len, long long multiple) {
    long long len = min_len;
    if ((total + len - 1) / len > max_chunks) len = (total + max_chunks - 1) / max_chunks;
    len = (len + multiple - 1) / multiple * multiple;
    SplitPlan p;
    p.len = len;
    p.chunks = (int)std::max<long long>(1, (total + len - 1) / len);
    return p;
}

int grow(float*& p, size_t& have, size_t need) {
    if (need <= have) return DG_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (p) { (void)hipFree(p); p = nullptr; have = 0; }
    HIP_TRY(hipMalloc(&p, need * sizeof(float)));
    have = need;
    return DG_OK;
}

struct WgradShape { int taps, M, Nn, h_in, Pi, Po, used; };
std::vector<WgradShape> wgrad_shapes(const dg_handle* h) {
    // [0] the Linear layer, [1 + d] deconv d < 2 (Generator.2, Generator.3)
    std::vector<WgradShape> v;
    v.push_back({1, h->latent, h->lin_out, 1, 1, 1, 1});
    for (int d = 0; d < 2; ++d) v.push_back({25, h->dec[d].cout, h->dec[d].cin, h->dec[d].h_in, h->ai[d].pitch, h->ai[d + 1].pitch, h->dec[d].e_used});
    return v;
}
SplitPlan wgrad_split(const WgradShape& w, int N) { return split_axis((long long)N * w.h_in * w.h_in, kMaxSplits, kSplitK, 2); }

// workspace for calls of up to N rows, and (adam) the moments
int ensure(dg_handle* h, int N, bool adam) {
    if (!h->gen_train) h->gen_train = new GenTrain();
    GenTrain* g = h->gen_train;
    const long long total = param_total(h);
    if (adam && !g->grads) HIP_TRY(hipMalloc(&g->grads, (size_t)total * sizeof(float)));
    if (adam && !g->m) {
        HIP_TRY(hipMalloc(&g->m, (size_t)total * sizeof(float)));
        HIP_TRY(hipMalloc(&g->v, (size_t)total * sizeof(float)));
        HIP_TRY(hipMemset(g->m, 0, (size_t)total * sizeof(float)));
        HIP_TRY(hipMemset(g->v, 0, (size_t)total * sizeof(float)));
        g->t = 0;
    }
    if (N > g->cap_N) {
        HIP_TRY(hipDeviceSynchronize());
        if (g->dpre5) (void)hipFree(g->dpre5);
        g->dpre5 = nullptr;
        g->cap_N = 0;
        HIP_TRY(hipMalloc(&g->dpre5, (size_t)N * 784 * sizeof(float)));
        g->cap_N = N;
    }
    // the largest set of chunk sums any reduction of this row count leaves
    size_t need = 0;
    for (const WgradShape& w : wgrad_shapes(h)) need = std::max(need, (size_t)wgrad_split(w, N).chunks * w.taps * w.M * w.Nn);
    const int C5 = h->dec[2].cin;
    need = std::max(need, (size_t)split_axis(N, kMaxChunks, 1, 1).chunks * 25 * C5);
    need = std::max(need, (size_t)kMaxChunks * (size_t)h->lin_out);
    return grow(g->part, g->part_floats, need);
}

void drop_maps(GenTrain* g) {
    for (auto& m : g->maps) if (m.map) (void)hipFree(m.map);
    g->maps.clear();
}

// One gather map per derived weight buffer the handle holds, from the packers of dg_pack.h run on an index array.
int build_maps(dg_handle* h, GenTrain* g) {
    if (g->maps_epoch == h->pack_epoch && !g->maps.empty()) return DG_OK;
    HIP_TRY(hipDeviceSynchronize());
    drop_maps(g);
    int rc = DG_OK;
    auto add = [&](float* dst, const float* src, const std::vector<int32_t>& map) {
        if (rc) return;
        GenTrain::Map m{dst, src, nullptr, map.size()};
        if (hipMalloc(&m.map, map.size() * sizeof(int32_t)) != hipSuccess ||
            hipMemcpy(m.map, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            if (m.map) (void)hipFree(m.map);
            rc = fail(DG_E_NOMEM, "cannot place a gather map of %zu entries", map.size());
            return;
        }
        g->maps.push_back(m);
    };
    const int K = h->latent, F = h->lin_out;
    {
        const std::vector<int32_t> idx = dg::pack_iota((size_t)K * F);
        std::vector<int32_t> map((size_t)K * F, dg::kPackPad);
        dg::pack_lin_transpose(idx.data(), map.data(), K, F);
        add(h->lin_wt, h->lin_w, map);
        if (h->lin_pack_fwd) {
            map.assign((size_t)K * F, dg::kPackPad);
            dg::pack_lin_fwd(idx.data(), map.data(), K, F);
            add(h->lin_pack_fwd, h->lin_w, map);
        }
        if (h->lin_pack_bwd) {
            map.assign((size_t)K * F, dg::kPackPad);
            dg::pack_lin_bwd(idx.data(), map.data(), K, F, h->nsplit);
            add(h->lin_pack_bwd, h->lin_w, map);
        }
    }
    for (size_t d = 0; d < h->dec.size(); ++d) {
        const int cout = h->dec[d].cout, cin = h->dec[d].cin;
        const size_t n = (size_t)25 * cout * cin;
        const std::vector<int32_t> idx = dg::pack_iota(n);
        std::vector<int32_t> map(n, dg::kPackPad);
        dg::pack_deconv_transpose(idx.data(), map.data(), cout, cin);
        add(h->Ft[d], h->F[d], map);
        if (h->Fp[d]) {
            map.assign(n, dg::kPackPad);
            dg::pack_deconv_frag(idx.data(), map.data(), cout, cin);
            add(h->Fp[d], h->F[d], map);
        }
        if (d + 1 == h->dec.size()) {
            if (h->tail_pack) {
                map.assign(dg::tail_pack32_elems(cout, cin), dg::kPackPad);
                dg::pack_tail32(idx.data(), map.data(), cout, cin);
                add(h->tail_pack, h->F[d], map);
            }
            if (h->tail_pack16 && cout == 3) {
                map.assign(dg::tail_pack16_elems(cin), dg::kPackPad);
                dg::pack_tail16(idx.data(), map.data(), cin);
                add(h->tail_pack16, h->F[d], map);
            }
        }
    }
    if (rc) { drop_maps(g); return rc; }
    g->maps_epoch = h->pack_epoch;
    return DG_OK;
}

int launch_wgrad(dg_handle* h, GenTrain* g, const WgradShape& w, const float* A, const float* B, int N, float* out, hipStream_t s, bool prof,
                 const char* name) {
    const SplitPlan sp = wgrad_split(w, N);
    WgradArgs a;
    a.A = A; a.B = B; a.part = g->part;
    a.N = N; a.taps = w.taps; a.M = w.M; a.Nn = w.Nn; a.h_in = w.h_in; a.Pi = w.Pi; a.Po = w.Po; a.used = w.used;
    a.kchunk = (int)sp.len;
    const long long per = (long long)w.taps * w.M * w.Nn;
    if ((size_t)sp.chunks * per > g->part_floats) return fail(DG_E_STATE, "%s: the chunk-sum buffer is too small", name);
    const int tiles = w.taps * (w.M / 32) * (w.Nn / 64);
    {
        ProfScope ps(h, s, prof, std::string(name) + "@gen_wgrad_mfma_kernel", 2.0 * (double)per * N * w.h_in * w.h_in);
        hipLaunchKernelGGL(gen_wgrad_mfma_kernel, dim3((unsigned)((tiles + 3) / 4), (unsigned)sp.chunks), dim3(256), 0, s, a);
    }
    {
        ProfScope ps(h, s, prof, std::string(name) + "@gen_reduce_kernel", 0.0);
        hipLaunchKernelGGL(gen_reduce_kernel, dim3(grid_of(per)), dim3(256), 0, s, g->part, sp.chunks, per, out);
    }
    return launch_check(name);
}

int launch_colsum(dg_handle* h, GenTrain* g, const float* src, long long rows, int C, float* out, hipStream_t s, bool prof, const char* name) {
    const SplitPlan sp = split_axis(rows, kMaxChunks, 1, 1);
    if ((size_t)sp.chunks * C > g->part_floats) return fail(DG_E_STATE, "%s: the chunk-sum buffer is too small", name);
    ProfScope ps(h, s, prof, std::string(name) + "@gen_colsum_kernel", 0.0);
    hipLaunchKernelGGL(gen_colsum_kernel, dim3((unsigned)sp.chunks), dim3(256), 0, s, src, rows, C, sp.len, g->part);
    hipLaunchKernelGGL(gen_reduce_kernel, dim3(grid_of(C)), dim3(256), 0, s, g->part, sp.chunks, (long long)C, out);
    return launch_check(name);
}

// forward + seeded backward; the flat gradient lands in `grads` (device)
int gen_gradient(dg_handle* h, const float* z, const float* dy, int N, float* grads, float* out_y, float* out_dz, hipStream_t s) {
    GenTrain* g = h->gen_train;
    const bool prof = h->prof_stride > 0;
    h->prof_chain_last = -1;
    const auto segs = param_segs(h);
    const auto shapes = wgrad_shapes(h);
    const int nd = (int)h->dec.size();                    // 3
    const int C5 = h->dec[2].cin;
    HIP_TRY(hipMemcpyAsync(h->z, z, (size_t)N * h->latent * sizeof(float), hipMemcpyDeviceToDevice, s));
    int rc = clear_pair_counters(h, N, s);
    if (rc) return rc;
    RowGroup grp; grp.n_rows = N; grp.s = s;
    // (every row is compared with one all-zero image, as in dg_generate: the loss is not read)
    rc = run_forward(h, h->xzero, grp, /*R=*/N, /*want_y=*/true, /*want_loss=*/false, /*tail_backward=*/false, prof);
    if (rc) return rc;
    if (out_y) HIP_TRY(hipMemcpyAsync(out_y, h->y, (size_t)N * h->P * sizeof(float), hipMemcpyDeviceToDevice, s));
    {
        ProfScope ps(h, s, prof, "G5seed@gen_seed_kernel", 0.0);
        hipLaunchKernelGGL(gen_seed_kernel, dim3(grid_of((long long)N * 784)), dim3(256), 0, s, dy, h->y, g->dpre5, (long long)N * 784);
    }
    // Generator.5: weight gradient, bias gradient, then the backward over h3
    float* h3 = h->act[nd - 1];
    {
        const SplitPlan sp = split_axis(N, kMaxChunks, 1, 1);
        ProfScope ps(h, s, prof, "W5@gen_tail_wgrad_kernel", 2.0 * 67.0 * 67.0 * C5 * N);
        hipLaunchKernelGGL(gen_tail_wgrad_kernel, dim3((unsigned)sp.chunks, 25), dim3((unsigned)C5), 0, s, g->dpre5, h3, g->part, N, C5, (int)sp.len);
        hipLaunchKernelGGL(gen_reduce_kernel, dim3(grid_of(25LL * C5)), dim3(256), 0, s, g->part, sp.chunks, 25LL * C5, grads + segs[6].off);
    }
    if ((rc = launch_colsum(h, g, g->dpre5, (long long)N * 784, 1, grads + segs[7].off, s, prof, "W5b"))) return rc;
    {
        ProfScope ps(h, s, prof, "B5@gen_tail_bwd_kernel", 2.0 * 67.0 * 67.0 * C5 * N);
        const long long total = (long long)N * 196 * C5;
        hipLaunchKernelGGL(gen_tail_bwd_kernel, dim3(grid_of(total)), dim3(256), 0, s, h3, g->dpre5, h->F[nd - 1], total, C5);
    }
    if ((rc = launch_check("the seeded backward of Generator.5"))) return rc;
    // the layers below: weight gradient BEFORE the in-place backward-to-input of the same layer (see ORDER above)
    const std::function<int(int)> before = [&](int d) -> int {
        if (d >= 0) {
            // act[d + 1] holds dpre of deconv d, act[d] its input activation
            const ActInfo& o = h->ai[d + 1];
            int r = launch_wgrad(h, g, shapes[1 + d], h->act[d + 1], h->act[d], N, grads + segs[2 + 2 * d].off, s, prof, d == 0 ? "W2" : "W3");
            if (r) return r;
            return launch_colsum(h, g, h->act[d + 1], (long long)N * o.pitch * o.pitch, o.C, grads + segs[3 + 2 * d].off, s, prof, d == 0 ? "W2b" : "W3b");
        }
        int r = launch_wgrad(h, g, shapes[0], h->z, h->act[0], N, grads + segs[0].off, s, prof, "W1");
        if (r) return r;
        return launch_colsum(h, g, h->act[0], N, h->lin_out, grads + segs[1].off, s, prof, "W1b");
    };
    rc = run_backward(h, grp, prof, nullptr, /*without_b1=*/out_dz == nullptr, &before);
    if (rc) return rc;
    if (out_dz) dg::launch_momentum_update(nullptr, nullptr, h->part, h->nsplit, N, h->latent, 0.f, 0.f, out_dz, s);
    HIP_TRY(hipGetLastError());
    return DG_OK;
}

int gen_call(dg_handle* h, const float* z, const float* dy, int N, float* grads, float* out_y, float* out_dz, bool adam, float lr, float b1,
             float b2, void* stream, const char* who) {
    if (!h) return fail(DG_E_INVALID, "%s: null handle", who);
    if (!z || !dy || (!adam && !grads)) return fail(DG_E_INVALID, "%s: null argument", who);
    int rc = gen_check_trainable(h, who);
    if (rc) return rc;
    if ((rc = check_ready(h))) return rc;
    int n_checked = 0;
    if ((rc = check_rows(N, 1, &n_checked))) return rc;
    // (the forward's tail compares every row with image 0 by R = N, exact below 2^20 rows: dg_generate's limit)
    if (N > (1 << 20)) return fail(DG_E_INVALID, "%s: at most %d rows per call (got %d): split the batch", who, 1 << 20, N);
    if (h->latent % 32 || h->lin_out % 64) return fail(DG_E_INVALID, "%s: unsupported layer widths", who);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    // workspace and job lists: blocking on the first call of a row count, nothing afterwards
    if ((rc = prepare_rows(h, N, &N, 1, s))) return rc;
    NhwcScope nhwc(h);
    if ((rc = prepare_rows(h, N, &N, 1, s))) return rc;
    if ((rc = ensure(h, N, adam))) return rc;
    GenTrain* g = h->gen_train;
    if (adam && (rc = build_maps(h, g))) return rc;
    float* gr = grads ? grads : g->grads;
    if ((rc = gen_gradient(h, z, dy, N, gr, out_y, out_dz, s))) return rc;
    if (!adam) return DG_OK;
    const bool prof = h->prof_stride > 0;
    g->t += 1;
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)b2, (double)g->t)) / (1.0 - std::pow((double)b1, (double)g->t)));
    const auto segs = param_segs(h);
    AdamSegs sg;
    for (int i = 0; i < 8; ++i) { sg.p[i] = segs[i].ptr; sg.end[i] = segs[i].off + segs[i].n; }
    const long long total = sg.end[7];
    {
        ProfScope ps(h, s, prof, "ADAM@gen_adam_kernel", 0.0);
        hipLaunchKernelGGL(gen_adam_kernel, dim3(grid_of(total)), dim3(256), 0, s, sg, gr, g->m, g->v, total, lr_t, b1, b2);
    }
    h->lin_w_trained = true;
    for (const GenTrain::Map& m : g->maps) {
        ProfScope ps(h, s, prof, "REFRESH@gen_gather_kernel", 0.0);
        hipLaunchKernelGGL(gen_gather_kernel, dim3(grid_of((long long)m.n)), dim3(256), 0, s, m.dst, m.src, m.map, (long long)m.n);
    }
    return launch_check(who);
}

const ParamSeg* find_seg(const std::vector<ParamSeg>& segs, const char* name) {
    for (const ParamSeg& p : segs)
        if (p.name == name) return &p;
    return nullptr;
}

}  // namespace

#pragma GCC visibility push(hidden)
namespace dge {
int gen_check_trainable(const dg_handle* h, const char* who) {
    if (h->arch != DG_ARCH_MNIST28) return fail(DG_E_INVALID, "%s: not implemented for the CelebA generator (only the MNIST / F-MNIST one)", who);
    if (h->use_bn) return fail(DG_E_INVALID, "%s: not implemented for use_bn (a Batchnorm generator)", who);
    return DG_OK;
}

void gen_launch_seed(const float* dy, const float* y, float* dpre5, long long n, hipStream_t s) {
    hipLaunchKernelGGL(gen_seed_kernel, dim3(grid_of(n)), dim3(256), 0, s, dy, y, dpre5, n);
}

void gen_launch_tail_bwd(float* h3, const float* dpre5, const float* F5, long long total, int C, hipStream_t s) {
    hipLaunchKernelGGL(gen_tail_bwd_kernel, dim3(grid_of(total)), dim3(256), 0, s, h3, dpre5, F5, total, C);
}

void gen_train_release(dg_handle* h) {
    GenTrain* g = h->gen_train;
    if (!g) return;
    drop_maps(g);
    for (float* p : {g->dpre5, g->part, g->grads, g->m, g->v})
        if (p) (void)hipFree(p);
    delete g;
    h->gen_train = nullptr;
}
}  // namespace dge
#pragma GCC visibility pop

extern "C" {

int dg_gen_param_gradient(dg_handle* h, const float* z, const float* dy, int N, float* grads, float* out_y, float* out_dz, void* stream) {
    return gen_call(h, z, dy, N, grads, out_y, out_dz, false, 0.f, 0.f, 0.f, stream, "dg_gen_param_gradient");
}

int dg_gen_step(dg_handle* h, const float* z, const float* dy, int N, float lr, float beta1, float beta2, void* stream) {
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f))
        return fail(DG_E_INVALID, "dg_gen_step: betas (%g, %g) outside [0, 1)", (double)beta1, (double)beta2);
    return gen_call(h, z, dy, N, nullptr, nullptr, nullptr, true, lr, beta1, beta2, stream, "dg_gen_step");
}

int dg_get_weights(dg_handle* h, const char* name, float* out, int is_device) {
    if (!h || !name || !out) return fail(DG_E_INVALID, "dg_get_weights: null argument");
    const auto segs = param_segs(h);
    const ParamSeg* p = find_seg(segs, name);
    if (!p) return fail(DG_E_INVALID, "dg_get_weights: unknown weight name '%s'", name);
    if (!h->have.count(p->name)) return fail(DG_E_STATE, "dg_get_weights: '%s' has not been set", name);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, p->ptr, (size_t)p->n * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return DG_OK;
}

int dg_gen_adam_reset(dg_handle* h) {
    if (!h) return fail(DG_E_INVALID, "dg_gen_adam_reset: null handle");
    int rc = gen_check_trainable(h, "dg_gen_adam_reset");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    GenTrain* g = h->gen_train;
    if (!g || !g->m) return DG_OK;          // the moments are created zero on first use
    const size_t bytes = (size_t)param_total(h) * sizeof(float);
    HIP_TRY(hipMemset(g->m, 0, bytes));
    HIP_TRY(hipMemset(g->v, 0, bytes));
    g->t = 0;
    return DG_OK;
}

int dg_gen_get_adam(dg_handle* h, const char* name, float* m, float* v, int64_t* t, int is_device) {
    if (!h || !name) return fail(DG_E_INVALID, "dg_gen_get_adam: null argument");
    int rc = gen_check_trainable(h, "dg_gen_get_adam");
    if (rc) return rc;
    const auto segs = param_segs(h);
    const ParamSeg* p = find_seg(segs, name);
    if (!p) return fail(DG_E_INVALID, "dg_gen_get_adam: unknown weight name '%s'", name);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const GenTrain* g = h->gen_train;
    const bool have = g && g->m;
    const size_t bytes = (size_t)p->n * sizeof(float);
    for (int which = 0; which < 2; ++which) {
        float* out = which ? v : m;
        if (!out) continue;
        if (!have) { if (is_device) HIP_TRY(hipMemset(out, 0, bytes)); else memset(out, 0, bytes); continue; }
        HIP_TRY(hipMemcpy(out, (which ? g->v : g->m) + p->off, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    }
    if (t) *t = have ? g->t : 0;
    return DG_OK;
}

int dg_gen_set_adam(dg_handle* h, const char* name, const float* m, const float* v, int64_t t, int is_device) {
    if (!h || !name || !m || !v || t < 0) return fail(DG_E_INVALID, "dg_gen_set_adam: bad argument");
    int rc = gen_check_trainable(h, "dg_gen_set_adam");
    if (rc) return rc;
    const auto segs = param_segs(h);
    const ParamSeg* p = find_seg(segs, name);
    if (!p) return fail(DG_E_INVALID, "dg_gen_set_adam: unknown weight name '%s'", name);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    if (!h->gen_train) h->gen_train = new GenTrain();
    GenTrain* g = h->gen_train;
    const size_t all = (size_t)param_total(h) * sizeof(float);
    if (!g->m) {
        HIP_TRY(hipMalloc(&g->m, all));
        HIP_TRY(hipMalloc(&g->v, all));
        HIP_TRY(hipMemset(g->m, 0, all));
        HIP_TRY(hipMemset(g->v, 0, all));
    }
    const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpy(g->m + p->off, m, (size_t)p->n * sizeof(float), kind));
    HIP_TRY(hipMemcpy(g->v + p->off, v, (size_t)p->n * sizeof(float), kind));
    g->t = t;
    return DG_OK;
}

}  // extern "C"
