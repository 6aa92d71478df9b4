// The white-box attack that sees the defense: BPDA with EOT (Athalye, Carlini, Wagner 2018, "Obfuscated gradients give a false
// sense of security"), L-infinity, as a projected sign-gradient iteration.  Not in the reference (whose attacks differentiate
// through ReconstructionLayer and get an identically zero gradient); defined in DESIGN.md section 7 and
// pinned by tests/support/bpda_reference.py.  Per iteration k and EOT sample s the host driver (network_builder.BPDA) enqueues
//
//     rec_{k,s} = reconstruct(x_k)                      dg_reconstruct, the real projection, latents of seed + k m + s
//     g_{k,s}   = d CE(logits(r), y) / dr at rec_{k,s}    the classifier's own chain: dg_clf_input_gradient's bits
//     g_k       = g_{k,0} + g_{k,1} + ... + g_{k,m-1}     summed in that order (a sum, not a mean)
//     x_{k+1}   = clip(x + clamp(x_k + eps_iter sign(g_k) - x, -eps, eps), lo, hi),  sign(0) = 0
//
// i.e. the projection's backward is taken as the identity: the gradient at rec is applied at x_k.  dg_bpda_step is one (k, s):
// clf_kept_forward, clf_launch_ce_grad and clf_seeded_backward (dg_clf_internal.h, the launchers dg_clf_input_gradient uses, in
// its order), then ONE new elementwise kernel that either adds the gradient into gsum (accumulate_only: the samples s < m - 1) or
// forms gsum + g and writes x_next (the last sample; gsum == NULL when m = 1).  dg_bpda_track is the best tracking: the defended
// prediction on iterate k comes from the next iteration's first projection (dg_eval_batch, unchanged), and an image keeps the
// first iterate that was misclassified, or the last one.
//
// Every output element is one thread's fixed-order arithmetic on its own inputs: a result does not depend on how many images share
// a launch.  No atomics, no host synchronisation, no graph capture.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dg_clf_internal.h"

struct BpdaWork {
    float* seed = nullptr;          // [B, n] dCE/dlogits
    size_t seed_floats = 0;
};

void bpda_release(BpdaWork* w) {
    if (!w) return;
    if (w->seed) (void)hipFree(w->seed);
    delete w;
}

namespace {

// The step, elementwise over V-wide vectors (V = 4: float4 loads and stores; V = 1 where H W C is no multiple of 4 or a
// pointer is not 16-byte aligned).  accumulate_only: gsum += g.  Otherwise t = gsum + g (t = g when gsum == NULL) and
// x_next = the projected sign step of t.  HBM-bound: three reads (g, x_cur, x_orig; with gsum a fourth) and one write of 4 bytes
// per element and a dozen VALU operations -- 12.5 MB for 1000 MNIST images, microseconds beside the projection's milliseconds.
template <int V>
__global__ __launch_bounds__(256) void bpda_step_kernel(const float* __restrict__ g, float* __restrict__ gsum, const float* __restrict__ x_cur,
                                                         const float* __restrict__ x_orig, float* __restrict__ x_next, long long nvec,
                                                         int accumulate_only, float eps, float eps_iter, float lo, float hi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    if constexpr (V == 4) {
        float4 t = reinterpret_cast<const float4*>(g)[i];
        if (gsum) {
            const float4 a = reinterpret_cast<const float4*>(gsum)[i];
            t.x = a.x + t.x; t.y = a.y + t.y; t.z = a.z + t.z; t.w = a.w + t.w;
        }
        if (accumulate_only) {
            reinterpret_cast<float4*>(gsum)[i] = t;
            return;
        }
        const float4 xc = reinterpret_cast<const float4*>(x_cur)[i];
        const float4 xo = reinterpret_cast<const float4*>(x_orig)[i];
        float4 o;
        o.x = clf_sign_step(t.x, xc.x, xo.x, eps, eps_iter, lo, hi);
        o.y = clf_sign_step(t.y, xc.y, xo.y, eps, eps_iter, lo, hi);
        o.z = clf_sign_step(t.z, xc.z, xo.z, eps, eps_iter, lo, hi);
        o.w = clf_sign_step(t.w, xc.w, xo.w, eps, eps_iter, lo, hi);
        reinterpret_cast<float4*>(x_next)[i] = o;
    } else {
        float t = g[i];
        if (gsum) t = gsum[i] + t;
        if (accumulate_only) {
            gsum[i] = t;
            return;
        }
        x_next[i] = clf_sign_step(t, x_cur[i], x_orig[i], eps, eps_iter, lo, hi);
    }
}

// Best tracking, the workgroups strided over the images: an image that has not succeeded yet (first_success < 0) takes iterate k
// as its best so far, and where the defended prediction on that iterate is not the label, k becomes its first success -- after
// which the image is left alone.  So x_best ends as the first misclassified iterate, or the last iterate judged.
__global__ __launch_bounds__(256) void bpda_track_kernel(const int32_t* __restrict__ preds, const int32_t* __restrict__ labels, int B, int k,
                                                          const float* __restrict__ x_iter, float* __restrict__ x_best,
                                                          int32_t* __restrict__ first_success, long long row_elems) {
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const bool open = first_success[b] < 0;                 // uniform over the workgroup
        const bool hit = preds[b] != labels[b];
        __syncthreads();                                        // every thread has read first_success[b] before it is written
        if (!open) continue;
        const float* src = x_iter + (long long)b * row_elems;
        float* dst = x_best + (long long)b * row_elems;
        for (long long i = threadIdx.x; i < row_elems; i += 256) dst[i] = src[i];
        if (hit && threadIdx.x == 0) first_success[b] = k;
    }
}

}  // namespace

int clf_launch_bpda_step(const float* g, float* gsum, const float* x_cur, const float* x_orig, float* x_next, long long total,
                         int row_elems, int accumulate_only, float eps, float eps_iter, float lo, float hi, hipStream_t s) {
    const bool vec = row_elems % 4 == 0 && clf_aligned16(g) && clf_aligned16(gsum) && clf_aligned16(x_cur) && clf_aligned16(x_orig) && clf_aligned16(x_next);
    const long long nvec = vec ? total / 4 : total;
    const unsigned grid = (unsigned)((nvec + 255) / 256);
    if (vec)
        hipLaunchKernelGGL(bpda_step_kernel<4>, dim3(grid), dim3(256), 0, s, g, gsum, x_cur, x_orig, x_next, nvec, accumulate_only ? 1 : 0,
                           eps, eps_iter, lo, hi);
    else
        hipLaunchKernelGGL(bpda_step_kernel<1>, dim3(grid), dim3(256), 0, s, g, gsum, x_cur, x_orig, x_next, nvec, accumulate_only ? 1 : 0,
                           eps, eps_iter, lo, hi);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

// dg_bpda_step and dg_bpda_step_ball: the gradient chain, then gsum += g, or the projected sign step, or (ball) dg_ball.hip's L2 step.
static int bpda_step_run(const char* who, bool ball, dg_clf* h, const float* rec, const int32_t* labels, int B, const float* x_cur,
                         const float* x_orig, float* gsum, int accumulate_only, float eps, float eps_iter, float clip_min, float clip_max,
                         float* x_next, void* stream) {
    if (!h || !rec || !labels || B <= 0) return clf_fail(DG_E_INVALID, "%s: bad argument", who);
    if (accumulate_only ? !gsum : (!x_cur || !x_orig || !x_next))
        return clf_fail(DG_E_INVALID, "%s: %s", who, accumulate_only ? "accumulate_only needs gsum" : "the step needs x_cur, x_orig and x_next");
    if (!accumulate_only && (!(eps >= 0.f) || !(eps_iter >= 0.f) || !(clip_min <= clip_max)))
        return clf_fail(DG_E_INVALID, "%s: eps and eps_iter must be >= 0 and clip_min <= clip_max", who);
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = clf_kept_forward(h, rec, B, s);
    if (rc) return rc;
    if (!h->bpda) h->bpda = new BpdaWork();
    if ((rc = clf_grow(&h->bpda->seed, 1, h->bpda->seed_floats, (size_t)B * h->n_logits))) return rc;
    clf_launch_ce_grad(h->acts[h->logit_layer], labels, h->bpda->seed, B, h->n_logits, s);
    float* g = nullptr;
    if ((rc = clf_seeded_backward(h, h->bpda->seed, B, s, &g))) return rc;
    if (ball && !accumulate_only) return clf_launch_ball_step(g, gsum, x_cur, x_orig, x_next, B, h->pixels(), eps, eps_iter, clip_min, clip_max, s);
    return clf_launch_bpda_step(g, gsum, x_cur, x_orig, x_next, (long long)B * h->pixels(), h->pixels(), accumulate_only, eps, eps_iter,
                                clip_min, clip_max, s);
}

extern "C" {

int dg_bpda_step(dg_clf* h, const float* rec, const int32_t* labels, int B, const float* x_cur, const float* x_orig, float* gsum,
                 int accumulate_only, float eps, float eps_iter, float clip_min, float clip_max, float* x_next, void* stream) {
    return bpda_step_run("dg_bpda_step", false, h, rec, labels, B, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, clip_min, clip_max,
                         x_next, stream);
}

int dg_bpda_step_ball(dg_clf* h, const float* rec, const int32_t* labels, int B, const float* x_cur, const float* x_orig, float* gsum,
                      int accumulate_only, float eps, float eps_iter, int ord, float clip_min, float clip_max, float* x_next, void* stream) {
    if (ord != 2) return clf_fail(DG_E_INVALID, "dg_bpda_step_ball: ord must be 2 (the L1 projection needs a sort), got %d", ord);
    return bpda_step_run("dg_bpda_step_ball", true, h, rec, labels, B, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, clip_min, clip_max,
                         x_next, stream);
}

int dg_bpda_track(const int32_t* preds, const int32_t* labels, int B, int k, const float* x_iter, float* x_best, int32_t* first_success,
                  int64_t row_elems, void* stream) {
    if (!preds || !labels || !x_iter || !x_best || !first_success || B <= 0 || k < 0 || row_elems <= 0)
        return clf_fail(DG_E_INVALID, "dg_bpda_track: bad argument");
    if (x_iter == x_best) return clf_fail(DG_E_INVALID, "dg_bpda_track: x_best must not be x_iter");
    const int grid = B < 1024 ? B : 1024;
    hipLaunchKernelGGL(bpda_track_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, preds, labels, B, k, x_iter, x_best, first_success,
                       (long long)row_elems);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

}  // extern "C"
