// The per-image reductions an Lp ball needs and the L-infinity attacks do not ("L2 balls"; pinned by
// tests/support/ball_reference.py).  All norms are over one image's P = H W C elements; tiny = 1e-12 guards every division, so a
// zero gradient gives a zero step, never a NaN.
//
//     row_norm_kernel        n_b = sum_i |v_bi - w_bi|  (ord 1)   or   sqrt(sum_i (v_bi - w_bi)^2)  (ord 2);  w == NULL: of v
//     fgm_norm_step_kernel   adv = clip(x + (eps / max(tiny, n(g))) g, lo, hi),  n = the ord-1 or ord-2 norm       (cleverhans fgm)
//     ball_step_kernel       t = gsum + g (t = g when gsum == NULL);  a = eps_iter / max(tiny, ||t||_2)
//                            d = (x_k + a t) - x;   f = min(1, eps / max(tiny, ||d||_2));   x_{k+1} = clip(x + f d, lo, hi)
//
// One workgroup of 256 threads per image, the workgroups strided over the images, one launch per step.  Thread t owns the
// vectors t, t + 256, ... of the row (V = 4: float4; V = 1 where P is no multiple of 4 or a pointer is not 16-byte aligned) and sums
// its terms in index order; a 64-lane __shfl_xor butterfly leaves the wave's sum in every lane, the four wave sums go through
// LDS and are added in wave order by every thread (clf_block_sum and the row vector ClfVec: dg_attack_device.h).  No atomics: an image's norm is one fixed-order float32 sum of its own row and
// does not depend on how many images share the launch.  Every product-sum that is evaluated twice (the re-read path forms d in
// the reduction and again in the write) is an explicit fma, so both evaluations have the same bits whatever the compiler contracts.
//
// A row of at most BALL_KEEP * 256 = 1024 elements (MNIST's 784) stays in the thread's registers between the passes: the step reads
// g, gsum, x_k and x once each.  A longer row (CelebA's 12 288) is read again by each pass -- g (and gsum) three times, x_k and x
// twice -- which is at most two reads of a row more than the L-infinity step and stays HBM-bound: 3 x 12 288 x 4 bytes x 4 streams
// per image, microseconds beside the convolutions.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dg_attack_device.h"
#include "dg_clf_internal.h"

namespace {

constexpr int BALL_KEEP = 4;          // floats a thread keeps per stream on the register path (one float4, or four scalars)
constexpr float BALL_TINY = 1e-12f;

__device__ __forceinline__ float ball_term(float d, int ord, float acc) { return ord == 1 ? acc + fabsf(d) : __fmaf_rn(d, d, acc); }

template <int V>
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ v, const float* __restrict__ w, int B, long long row_elems,
                                                        int ord, float* __restrict__ out) {
    __shared__ float part[4];
    const long long nvec = row_elems / V;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const float* rv = v + b * row_elems;
        const float* rw = w ? w + b * row_elems : nullptr;
        float acc = 0.f;
        for (long long i = threadIdx.x; i < nvec; i += 256) {
            ClfVec<V> a = ClfVec<V>::load(rv, i);
            if (rw) {
                const ClfVec<V> c = ClfVec<V>::load(rw, i);
#pragma unroll
                for (int j = 0; j < V; ++j) a.e[j] -= c.e[j];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) acc = ball_term(a.e[j], ord, acc);
        }
        const float s = clf_block_sum(acc, part);
        if (threadIdx.x == 0) out[b] = ord == 1 ? s : sqrtf(s);
    }
}

// KEEP: the row fits the registers (P <= BALL_KEEP * 256); otherwise the write pass reads g again.
template <int V, bool KEEP>
__global__ __launch_bounds__(256) void fgm_norm_step_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ out,
                                                             int B, int row_elems, int ord, float eps, float lo, float hi) {
    __shared__ float part[4];
    constexpr int NK = BALL_KEEP / V;                     // vectors a thread keeps
    const int nvec = row_elems / V;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const float* rg = g + b * row_elems;
        const float* rx = x + b * row_elems;
        float* ro = out + b * row_elems;
        ClfVec<V> kept[NK];
        float acc = 0.f;
        if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = threadIdx.x + k * 256;
                if (i < nvec) {
                    kept[k] = ClfVec<V>::load(rg, i);
#pragma unroll
                    for (int j = 0; j < V; ++j) acc = ball_term(kept[k].e[j], ord, acc);
                }
            }
        } else {
            for (int i = threadIdx.x; i < nvec; i += 256) {
                const ClfVec<V> a = ClfVec<V>::load(rg, i);
#pragma unroll
                for (int j = 0; j < V; ++j) acc = ball_term(a.e[j], ord, acc);
            }
        }
        const float s = clf_block_sum(acc, part);
        const float scale = eps / fmaxf(BALL_TINY, ord == 1 ? s : sqrtf(s));
        if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = threadIdx.x + k * 256;
                if (i < nvec) {
                    ClfVec<V> o = ClfVec<V>::load(rx, i);
#pragma unroll
                    for (int j = 0; j < V; ++j) o.e[j] = clf_clip(__fmaf_rn(scale, kept[k].e[j], o.e[j]), lo, hi);
                    o.store(ro, i);
                }
            }
        } else {
            for (int i = threadIdx.x; i < nvec; i += 256) {
                const ClfVec<V> a = ClfVec<V>::load(rg, i);
                ClfVec<V> o = ClfVec<V>::load(rx, i);
#pragma unroll
                for (int j = 0; j < V; ++j) o.e[j] = clf_clip(__fmaf_rn(scale, a.e[j], o.e[j]), lo, hi);
                o.store(ro, i);
            }
        }
    }
}

// t of vector i: gsum + g in dg_bpda_step's order, or g
template <int V>
__device__ __forceinline__ ClfVec<V> ball_t(const float* rg, const float* rs, long long i) {
    ClfVec<V> t = ClfVec<V>::load(rg, i);
    if (rs) {
        const ClfVec<V> a = ClfVec<V>::load(rs, i);
#pragma unroll
        for (int j = 0; j < V; ++j) t.e[j] = a.e[j] + t.e[j];
    }
    return t;
}

template <int V, bool KEEP>
__global__ __launch_bounds__(256) void ball_step_kernel(const float* __restrict__ g, const float* __restrict__ gsum, const float* __restrict__ x_cur,
                                                         const float* __restrict__ x_orig, float* __restrict__ x_next, int B, int row_elems,
                                                         float eps, float eps_iter, float lo, float hi) {
    __shared__ float part[4];
    constexpr int NK = BALL_KEEP / V;
    const int nvec = row_elems / V;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const long long off = b * row_elems;
        const float* rg = g + off;
        const float* rs = gsum ? gsum + off : nullptr;
        const float* rc = x_cur + off;
        const float* ro = x_orig + off;
        float* rn = x_next + off;
        ClfVec<V> kt[NK], ko[NK];                        // t, then d; x_orig
        // ---- ||t||
        float acc = 0.f;
        if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = threadIdx.x + k * 256;
                if (i < nvec) {
                    kt[k] = ball_t<V>(rg, rs, i);
#pragma unroll
                    for (int j = 0; j < V; ++j) acc = __fmaf_rn(kt[k].e[j], kt[k].e[j], acc);
                }
            }
        } else {
            for (int i = threadIdx.x; i < nvec; i += 256) {
                const ClfVec<V> t = ball_t<V>(rg, rs, i);
#pragma unroll
                for (int j = 0; j < V; ++j) acc = __fmaf_rn(t.e[j], t.e[j], acc);
            }
        }
        const float a = eps_iter / fmaxf(BALL_TINY, sqrtf(clf_block_sum(acc, part)));
        // ---- d = (x_k + a t) - x and ||d||
        acc = 0.f;
        if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = threadIdx.x + k * 256;
                if (i < nvec) {
                    const ClfVec<V> xc = ClfVec<V>::load(rc, i);
                    ko[k] = ClfVec<V>::load(ro, i);
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const float d = __fmaf_rn(a, kt[k].e[j], xc.e[j]) - ko[k].e[j];
                        kt[k].e[j] = d;
                        acc = __fmaf_rn(d, d, acc);
                    }
                }
            }
        } else {
            for (int i = threadIdx.x; i < nvec; i += 256) {
                const ClfVec<V> t = ball_t<V>(rg, rs, i), xc = ClfVec<V>::load(rc, i), xo = ClfVec<V>::load(ro, i);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float d = __fmaf_rn(a, t.e[j], xc.e[j]) - xo.e[j];
                    acc = __fmaf_rn(d, d, acc);
                }
            }
        }
        const float f = fminf(1.f, eps / fmaxf(BALL_TINY, sqrtf(clf_block_sum(acc, part))));
        // ---- x_{k+1} = clip(x + f d)
        if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i = threadIdx.x + k * 256;
                if (i < nvec) {
                    ClfVec<V> o;
#pragma unroll
                    for (int j = 0; j < V; ++j) o.e[j] = clf_clip(__fmaf_rn(f, kt[k].e[j], ko[k].e[j]), lo, hi);
                    o.store(rn, i);
                }
            }
        } else {
            for (int i = threadIdx.x; i < nvec; i += 256) {
                const ClfVec<V> t = ball_t<V>(rg, rs, i), xc = ClfVec<V>::load(rc, i), xo = ClfVec<V>::load(ro, i);
                ClfVec<V> o;
#pragma unroll
                for (int j = 0; j < V; ++j) o.e[j] = clf_clip(__fmaf_rn(f, __fmaf_rn(a, t.e[j], xc.e[j]) - xo.e[j], xo.e[j]), lo, hi);
                o.store(rn, i);
            }
        }
    }
}

unsigned ball_grid(int B) { return (unsigned)(B < 65536 ? B : 65536); }

}  // namespace

int clf_launch_row_norms(const float* v, const float* w, int B, long long row_elems, int ord, float* out, hipStream_t s) {
    if (row_elems % 4 == 0 && clf_aligned16(v) && clf_aligned16(w))
        hipLaunchKernelGGL(row_norm_kernel<4>, dim3(ball_grid(B)), dim3(256), 0, s, v, w, B, row_elems, ord, out);
    else
        hipLaunchKernelGGL(row_norm_kernel<1>, dim3(ball_grid(B)), dim3(256), 0, s, v, w, B, row_elems, ord, out);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

int clf_launch_fgm_norm_step(const float* x, const float* g, float* out, int B, int row_elems, int ord, float eps, float lo, float hi,
                             hipStream_t s) {
    const bool vec = row_elems % 4 == 0 && clf_aligned16(x) && clf_aligned16(g) && clf_aligned16(out);
    const bool keep = row_elems <= BALL_KEEP * 256;
    const dim3 grid(ball_grid(B)), block(256);
    if (vec && keep) hipLaunchKernelGGL((fgm_norm_step_kernel<4, true>), grid, block, 0, s, x, g, out, B, row_elems, ord, eps, lo, hi);
    else if (vec) hipLaunchKernelGGL((fgm_norm_step_kernel<4, false>), grid, block, 0, s, x, g, out, B, row_elems, ord, eps, lo, hi);
    else if (keep) hipLaunchKernelGGL((fgm_norm_step_kernel<1, true>), grid, block, 0, s, x, g, out, B, row_elems, ord, eps, lo, hi);
    else hipLaunchKernelGGL((fgm_norm_step_kernel<1, false>), grid, block, 0, s, x, g, out, B, row_elems, ord, eps, lo, hi);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

int clf_launch_ball_step(const float* g, const float* gsum, const float* x_cur, const float* x_orig, float* x_next, int B, int row_elems,
                         float eps, float eps_iter, float lo, float hi, hipStream_t s) {
    const bool vec = row_elems % 4 == 0 && clf_aligned16(g) && clf_aligned16(gsum) && clf_aligned16(x_cur) && clf_aligned16(x_orig) && clf_aligned16(x_next);
    const bool keep = row_elems <= BALL_KEEP * 256;
    const dim3 grid(ball_grid(B)), block(256);
    if (vec && keep) hipLaunchKernelGGL((ball_step_kernel<4, true>), grid, block, 0, s, g, gsum, x_cur, x_orig, x_next, B, row_elems, eps, eps_iter, lo, hi);
    else if (vec) hipLaunchKernelGGL((ball_step_kernel<4, false>), grid, block, 0, s, g, gsum, x_cur, x_orig, x_next, B, row_elems, eps, eps_iter, lo, hi);
    else if (keep) hipLaunchKernelGGL((ball_step_kernel<1, true>), grid, block, 0, s, g, gsum, x_cur, x_orig, x_next, B, row_elems, eps, eps_iter, lo, hi);
    else hipLaunchKernelGGL((ball_step_kernel<1, false>), grid, block, 0, s, g, gsum, x_cur, x_orig, x_next, B, row_elems, eps, eps_iter, lo, hi);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

extern "C" {

int dg_row_norms(const float* v, const float* w, int B, int64_t row_elems, int ord, float* out, void* stream) {
    if (!v || !out || B <= 0 || row_elems <= 0) return clf_fail(DG_E_INVALID, "dg_row_norms: bad argument");
    if (ord != 1 && ord != 2) return clf_fail(DG_E_INVALID, "dg_row_norms: ord must be 1 or 2, got %d", ord);
    return clf_launch_row_norms(v, w, B, (long long)row_elems, ord, out, (hipStream_t)stream);
}

}  // extern "C"
