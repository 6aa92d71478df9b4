// The score-based black-box attack: SPSA (Uesato et al. 2018; Spall 1992) with Rademacher directions and the projected sign step of
// PGD and BPDA, L-infinity.  It needs only the attacked model's logits, so it works where the projection's gradient is identically
// zero.  Not in the reference; defined here and in DESIGN.md section 7 ("SPSA"), pinned by
// tests/support/spsa_reference.py; network_builder.SPSA drives the two entries.
//
// x [B,H,W,C] the originals, y the labels, P = H W C, n = spsa_samples direction pairs, delta the probe size, g = first_image + b
// an image's GLOBAL index, k the iteration, G = ceil(n / 32).
//
//   Directions   u_i[e] = +1 where bit (i & 31) of word (e & 3) of Philox4x32-10(key = (seed lo, seed hi),
//                counter = (e >> 2, g, k G + (i >> 5), 0x53505341 "SPSA")) is set, else -1: one Philox block serves 4 consecutive
//                elements x 32 directions, and a thread that owns a float4 of elements spends one block per 32 directions.
//                first_image + B > 2^32 and k G + G > 2^32 are refused (the counter words would wrap).
//   Queries      q[b,0] = x_k[b], the iterate itself (the defended prediction on it judges iterate k);
//                q[b,1+2i] = clip(x_k[b] + delta u_i),  q[b,2+2i] = clip(x_k[b] - delta u_i),  clipped to [clip_min, clip_max]: a
//                black-box oracle takes only valid images.  x +- delta is one float32 rounding, so a query is an exact function of
//                the Philox bits.
//   Loss         the margin of a query's logits Z: L = max_{j != y} Z_j - Z_y.  A label outside [0, classes) gives L = 0 for every
//                query of the image, hence a zero estimate and a zero step (dg_pgd's policy for its gradient).
//   Estimate     dL_i = L(q+_i) - L(q-_i), formed in float64 from the float32 logits and rounded once to float32;
//                ghat[b,e] = (1 / (2 delta n)) sum_{i<n} dL_i u_i[e]: a float32 sum in ascending i from 0 (one thread's fixed order),
//                times float32(1 / (2 delta n)).  u is regenerated from Philox, never stored, and the estimate uses u even where the
//                query was clipped.
//   Non-finite   a NaN logit makes its query's L NaN (the maximum propagates NaN).  A pair whose dL is not finite as a float32 --
//                NaN, +-inf, inf - inf -- contributes 0 to the sum; the divisor stays n.
//   Step         x_{k+1} = clip(x + clamp(x_k + eps_iter sign(ghat) - x, -eps, eps), clip_min, clip_max), sign(0) = 0: dg_bpda_step's
//                formula (clf_sign_step).
//
// dg_spsa_queries: one thread per 4 consecutive elements of one image; per group of 32 directions one Philox block and up to 64
// stores, each row-contiguous across the threads of an image.  dg_spsa_step: the workgroups of an image each stage dL for up to 1024
// directions at a time in LDS (two rows of `classes` logits per direction, read by whichever thread owns the direction), then every
// thread adds them in ascending i onto its 4 elements.  float4 where P is a multiple of 4 and every pointer is 16-byte aligned,
// otherwise the same threads move the same values as scalars.  Traffic per iteration: the queries are written once, (2n + 1) P
// floats per image (4 MB for 20 MNIST images at n = 32) -- microseconds beside their projection.  The step reads an image's
// 2 n classes logits once per workgroup of the image, ceil(P / 1024) times: once for MNIST's 784 elements, 12 times for CelebA's
// 12 288 (at n = 32, 10 classes: 30 KB per image out of L2, against the 3.2 MB of queries written for it).  A first launch that
// leaves dL in a buffer would read them once, at the price of a workspace, which these handle-free entries do not have.
//
// Every output element is one thread's fixed-order arithmetic on its own image, keyed by the image's global index: nothing depends
// on how the images are batched.  No atomics, no host read, no graph capture, no workspace.  The entries take no handle, so their
// launches carry no profile scope (those live in a handle).  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dg_clf_internal.h"
#include "dg_shared_math.h"

namespace {

constexpr uint32_t SPSA_TAG = 0x53505341u;
constexpr int SPSA_STAGE = 1024;          // directions whose dL a workgroup stages at once: a multiple of 32, 4 KB of LDS

// the four words that hold the bits of elements 4 quad .. 4 quad + 3 for the directions 32 group .. 32 group + 31
__device__ __forceinline__ void spsa_bits(uint32_t (&w)[4], uint32_t quad, uint32_t image, uint32_t block, uint32_t k0, uint32_t k1) {
    w[0] = quad; w[1] = image; w[2] = block; w[3] = SPSA_TAG;
    dg_philox4x32_10(w, k0, k1);
}

// The quad's elements that exist: 4, or fewer at the end of a row on the scalar path.
template <int V>
__device__ __forceinline__ int spsa_live(long long quad, long long row_elems) {
    if constexpr (V == 4) return 4;
    const long long left = row_elems - 4 * quad;
    return left < 4 ? (int)left : 4;
}
template <int V>
__device__ __forceinline__ void spsa_load(float (&v)[4], const float* row, long long quad, int live) {
    if constexpr (V == 4) {
        const float4 t = reinterpret_cast<const float4*>(row)[quad];
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < live ? row[4 * quad + j] : 0.f;
    }
}
template <int V>
__device__ __forceinline__ void spsa_store(const float (&v)[4], float* row, long long quad, int live) {
    if constexpr (V == 4) {
        reinterpret_cast<float4*>(row)[quad] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < live) row[4 * quad + j] = v[j];
    }
}

template <int V>
__global__ __launch_bounds__(256) void spsa_queries_kernel(const float* __restrict__ x_cur, long long total, long long nquads, long long row_elems,
                                                            int n, float delta, uint32_t k0, uint32_t k1, uint32_t first_image,
                                                            uint32_t block0, float lo, float hi, float* __restrict__ q) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long b = t / nquads, quad = t - b * nquads;
    const int live = spsa_live<V>(quad, row_elems);
    float x[4];
    spsa_load<V>(x, x_cur + b * row_elems, quad, live);
    float* qb = q + b * (2LL * n + 1) * row_elems;              // the image's 2n + 1 rows
    spsa_store<V>(x, qb, quad, live);
    for (int i0 = 0; i0 < n; i0 += 32) {
        uint32_t w[4];
        spsa_bits(w, (uint32_t)quad, first_image + (uint32_t)b, block0 + (uint32_t)(i0 >> 5), k0, k1);
        const int m = n - i0 < 32 ? n - i0 : 32;
        for (int j = 0; j < m; ++j) {
            float plus[4], minus[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = (w[e] >> j) & 1u ? delta : -delta;
                plus[e] = clf_clip(x[e] + d, lo, hi);
                minus[e] = clf_clip(x[e] - d, lo, hi);
            }
            float* row = qb + (1LL + 2LL * (i0 + j)) * row_elems;
            spsa_store<V>(plus, row, quad, live);
            spsa_store<V>(minus, row + row_elems, quad, live);
        }
    }
}

// L = max_{j != y} Z_j - Z_y in float64; the maximum propagates NaN.  0 <= y < classes.
__device__ __forceinline__ double spsa_margin(const float* __restrict__ z, int classes, int y) {
    float m = -INFINITY;
    for (int j = 0; j < classes; ++j) {
        if (j == y) continue;
        const float v = z[j];
        m = (v > m || v != v) ? v : m;
    }
    return (double)m - (double)z[y];
}

template <int V>
__global__ __launch_bounds__(256) void spsa_step_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, long long nquads,
                                                         int wgs_per_image, int classes, long long row_elems, int n, float scale, uint32_t k0,
                                                         uint32_t k1, uint32_t first_image, uint32_t block0, const float* __restrict__ x_cur,
                                                         const float* __restrict__ x_orig, float eps, float eps_iter, float lo, float hi,
                                                         float* __restrict__ x_next, float* __restrict__ out_grad) {
    __shared__ float dl[SPSA_STAGE];
    const long long b = blockIdx.x / wgs_per_image;
    const long long quad = (long long)(blockIdx.x - b * wgs_per_image) * 256 + threadIdx.x;
    const bool owner = quad < nquads;
    const int y = labels[b];
    const bool labelled = y >= 0 && y < classes;
    const float* zb = logits + b * (2LL * n + 1) * classes;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < n; s0 += SPSA_STAGE) {
        const int sm = n - s0 < SPSA_STAGE ? n - s0 : SPSA_STAGE;
        __syncthreads();                                          // the stage before has been read by every thread
        for (int j = threadIdx.x; j < sm; j += 256) {
            float d = 0.f;
            if (labelled) {
                const float* zp = zb + (1LL + 2LL * (s0 + j)) * classes;
                d = (float)(spsa_margin(zp, classes, y) - spsa_margin(zp + classes, classes, y));
                if (!isfinite(d)) d = 0.f;
            }
            dl[j] = d;
        }
        __syncthreads();
        if (!owner) continue;
        for (int i0 = 0; i0 < sm; i0 += 32) {
            uint32_t w[4];
            spsa_bits(w, (uint32_t)quad, first_image + (uint32_t)b, block0 + (uint32_t)((s0 + i0) >> 5), k0, k1);
            const int m = sm - i0 < 32 ? sm - i0 : 32;
            for (int j = 0; j < m; ++j) {
                const float d = dl[i0 + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = acc[e] + ((w[e] >> j) & 1u ? d : -d);
            }
        }
    }
    if (!owner) return;
    const int live = spsa_live<V>(quad, row_elems);
    const long long off = b * row_elems;
    float g[4], xc[4], xo[4], o[4];
    spsa_load<V>(xc, x_cur + off, quad, live);
    spsa_load<V>(xo, x_orig + off, quad, live);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        g[e] = acc[e] * scale;
        o[e] = clf_sign_step(g[e], xc[e], xo[e], eps, eps_iter, lo, hi);
    }
    spsa_store<V>(o, x_next + off, quad, live);
    if (out_grad) spsa_store<V>(g, out_grad + off, quad, live);
}

// What both entries check about the draw's keying; *block0 = k G.
int spsa_keying(const char* who, int B, int64_t row_elems, int n, float delta, int64_t first_image, int iter, uint32_t* block0) {
    if (B < 1 || n < 1 || row_elems < 1 || row_elems > INT32_MAX) return clf_fail(DG_E_INVALID, "%s: B, n and row_elems must be >= 1 (row_elems at most 2^31 - 1)", who);
    if (!(delta > 0.f)) return clf_fail(DG_E_INVALID, "%s: delta must be > 0", who);
    if (iter < 0 || first_image < 0) return clf_fail(DG_E_INVALID, "%s: iter and first_image must be >= 0", who);
    const uint64_t wrap = 1ull << 32, groups = ((uint64_t)n + 31) / 32;
    if ((uint64_t)first_image + (uint64_t)B > wrap) return clf_fail(DG_E_INVALID, "%s: first_image + B exceeds 2^32", who);
    if ((uint64_t)iter * groups + groups > wrap) return clf_fail(DG_E_INVALID, "%s: iter * ceil(n / 32) + ceil(n / 32) exceeds 2^32", who);
    *block0 = (uint32_t)((uint64_t)iter * groups);
    return DG_OK;
}

}  // namespace

extern "C" {

int dg_spsa_queries(const float* x_cur, int B, int64_t row_elems, int n, float delta, uint64_t seed, int64_t first_image, int iter,
                    float clip_min, float clip_max, float* q, void* stream) {
    if (!x_cur || !q) return clf_fail(DG_E_INVALID, "dg_spsa_queries: x_cur and q are required");
    uint32_t block0 = 0;
    int rc = spsa_keying("dg_spsa_queries", B, row_elems, n, delta, first_image, iter, &block0);
    if (rc) return rc;
    if (!(clip_min <= clip_max)) return clf_fail(DG_E_INVALID, "dg_spsa_queries: clip_min must not exceed clip_max");
    const long long nquads = ((long long)row_elems + 3) / 4, total = (long long)B * nquads, wgs = (total + 255) / 256;
    if (wgs > INT32_MAX) return clf_fail(DG_E_INVALID, "dg_spsa_queries: B * row_elems is too large for one launch");
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (row_elems % 4 == 0 && clf_aligned16(x_cur) && clf_aligned16(q))
        hipLaunchKernelGGL(spsa_queries_kernel<4>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, x_cur, total, nquads,
                           (long long)row_elems, n, delta, k0, k1, (uint32_t)first_image, block0, clip_min, clip_max, q);
    else
        hipLaunchKernelGGL(spsa_queries_kernel<1>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, x_cur, total, nquads,
                           (long long)row_elems, n, delta, k0, k1, (uint32_t)first_image, block0, clip_min, clip_max, q);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

int dg_spsa_step(const float* logits, const int32_t* labels, int B, int classes, int64_t row_elems, int n, float delta, uint64_t seed,
                 int64_t first_image, int iter, const float* x_cur, const float* x_orig, float eps, float eps_iter, float clip_min,
                 float clip_max, float* x_next, float* out_grad, void* stream) {
    if (!logits || !labels || !x_cur || !x_orig || !x_next) return clf_fail(DG_E_INVALID, "dg_spsa_step: logits, labels, x_cur, x_orig and x_next are required");
    uint32_t block0 = 0;
    int rc = spsa_keying("dg_spsa_step", B, row_elems, n, delta, first_image, iter, &block0);
    if (rc) return rc;
    if (classes < 2) return clf_fail(DG_E_INVALID, "dg_spsa_step: the margin needs at least 2 classes, got %d", classes);
    if (!(eps >= 0.f) || !(eps_iter >= 0.f) || !(clip_min <= clip_max))
        return clf_fail(DG_E_INVALID, "dg_spsa_step: eps and eps_iter must be >= 0 and clip_min <= clip_max");
    if (x_next == x_cur) return clf_fail(DG_E_INVALID, "dg_spsa_step: x_next must not be x_cur");
    if (out_grad && (out_grad == x_next || out_grad == x_cur || out_grad == x_orig))
        return clf_fail(DG_E_INVALID, "dg_spsa_step: out_grad must be a buffer of its own");
    const long long nquads = ((long long)row_elems + 3) / 4, per_image = (nquads + 255) / 256, wgs = (long long)B * per_image;
    if (wgs > INT32_MAX) return clf_fail(DG_E_INVALID, "dg_spsa_step: B * row_elems is too large for one launch");
    const float scale = (float)(1.0 / (2.0 * (double)delta * (double)n));
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const bool vec = row_elems % 4 == 0 && clf_aligned16(x_cur) && clf_aligned16(x_orig) && clf_aligned16(x_next) && clf_aligned16(out_grad);
    if (vec)
        hipLaunchKernelGGL(spsa_step_kernel<4>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, logits, labels, nquads, (int)per_image,
                           classes, (long long)row_elems, n, scale, k0, k1, (uint32_t)first_image, block0, x_cur, x_orig, eps, eps_iter,
                           clip_min, clip_max, x_next, out_grad);
    else
        hipLaunchKernelGGL(spsa_step_kernel<1>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, logits, labels, nquads, (int)per_image,
                           classes, (long long)row_elems, n, scale, k0, k1, (uint32_t)first_image, block0, x_cur, x_orig, eps, eps_iter,
                           clip_min, clip_max, x_next, out_grad);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

}  // extern "C"
