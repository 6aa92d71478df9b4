// Projected gradient descent (Madry et al. 2018, L-infinity) on the BARE classifier, the whole attack enqueued by one call.  Not in
// the reference; it is BPDA (dg_bpda.hip) with the projection replaced by the identity and one EOT sample:
//
//     x_0     = x_start                                     the caller's clip(x), clip(x + noise) or x_init
//     g_k     = d CE(logits(x_k), y) / dx                   dg_clf_input_gradient's bits (a label outside [0, n): zero)
//     x_{k+1} = clip(x + clamp(x_k + eps_iter sign(g_k) - x, -eps, eps), lo, hi),  sign(0) = 0          k = 0 .. nb_iter - 1
//
// and dg_bpda_track's best tracking: iterate j = 1 .. nb_iter succeeds for an image when the model's prediction on it is not the
// label; an image keeps its first successful iterate, or the last one.  The prediction on iterate j costs no forward of its own: it
// is the first arg-max of the logits that iteration j's forward keeps for its backward (pgd_track_kernel); only the last iterate
// needs one trailing forward.  A call is nb_iter + 1 forwards and nb_iter backwards through clf_kept_forward, clf_launch_ce_grad and
// clf_seeded_backward (dg_clf_internal.h: the launchers dg_clf_input_gradient and dg_bpda_step use, in their order) and
// clf_launch_bpda_step with gsum == NULL.  dg_pgd_ball is the same call with the L2 step of dg_ball.hip (clf_launch_ball_step) in
// the projected sign step's place (still one launch per step); the chain and the tracking are shared.
//
// Every output element is one thread's (or one wave's) fixed-order arithmetic on its own image: the result does not depend on how
// many images share a call.  No atomics, no host synchronisation, no graph capture.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dg_attack_device.h"
#include "dg_clf_internal.h"

struct PgdWork {
    float* seed = nullptr;               // [B, n] dCE/dlogits
    size_t seed_floats = 0;
    float* iter[2] = {nullptr, nullptr}; // [B, H W C] each: x_{k+1} goes to iter[k & 1]
    size_t iter_floats = 0;
};

void pgd_release(PgdWork* w) {
    if (!w) return;
    if (w->seed) (void)hipFree(w->seed);
    for (float* p : w->iter)
        if (p) (void)hipFree(p);
    delete w;
}

namespace {

// Training's policy for a label outside [0, n) (dg_clf_train.hip: it contributes nothing): its row of the seed becomes zero, so
// the chain returns a zero gradient and the step leaves the image where it is.  One thread per seed element.
__global__ __launch_bounds__(256) void pgd_mask_seed_kernel(float* __restrict__ seed, const int32_t* __restrict__ labels, long long total, int n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int y = labels[i / n];
    if (y < 0 || y >= n) seed[i] = 0.f;
}

// Best tracking for iterate k off the logits its forward kept.  One wave per image (four per workgroup, the waves strided over the
// images), the prediction by clf_wave_class (dg_attack_device.h) -- dg_eval_batch's first arg-max, NaN rules included: a NaN is
// never a candidate; a NaN at class 0 wins every comparison of clf_eval_kernel's scan, as does a row of NaNs, and the answer is
// class 0.  Then dg_bpda_track's rule: an image without a
// success so far (first_success < 0) takes iterate k as its best, and k as its first success where the arg-max is not the label.
// first_success[b] is read and written by image b's wave alone, the read (one load instruction of the whole wave) before the write.
__global__ __launch_bounds__(256) void pgd_track_kernel(const float* __restrict__ logits, int n, const int32_t* __restrict__ labels, int B, int k,
                                                         const float* __restrict__ x_iter, float* __restrict__ x_best,
                                                         int32_t* __restrict__ first_success, long long row_elems) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) {
        if (first_success[b] >= 0) continue;                    // uniform over the wave
        const int arg = clf_wave_class(logits + b * n, n, lane);          // uniform over the wave
        const float* src = x_iter + b * row_elems;
        float* dst = x_best + b * row_elems;
        for (long long i = lane; i < row_elems; i += 64) dst[i] = src[i];
        if (lane == 0 && arg != labels[b]) first_success[b] = k;
    }
}

int pgd_track(const dg_clf* h, const int32_t* labels, int B, int k, const float* x_iter, float* x_best, int32_t* first_success, hipStream_t s) {
    const int grid = (B + 3) / 4 < 4096 ? (B + 3) / 4 : 4096;
    hipLaunchKernelGGL(pgd_track_kernel, dim3(grid), dim3(256), 0, s, h->acts[h->logit_layer], h->n_logits, labels, B, k, x_iter, x_best,
                       first_success, (long long)h->pixels());
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

// dg_pgd and dg_pgd_ball: the same chain, the step either the projected sign step or (ball) the L2 step of dg_ball.hip.
int pgd_run(const char* who, bool ball, dg_clf* h, const float* x, const float* x_start, const int32_t* labels, int B, float eps, float eps_iter,
            int nb_iter, float clip_min, float clip_max, float* x_adv, int32_t* first_success, void* stream) {
    if (nb_iter < 1) return clf_fail(DG_E_INVALID, "%s: nb_iter must be >= 1, got %d", who, nb_iter);
    if (!(eps >= 0.f) || !(eps_iter >= 0.f)) return clf_fail(DG_E_INVALID, "%s: eps and eps_iter must be >= 0", who);
    if (!(clip_min <= clip_max)) return clf_fail(DG_E_INVALID, "%s: clip_min must not exceed clip_max", who);
    if (!h || !x || !x_start || !labels || !x_adv || !first_success || B <= 0) return clf_fail(DG_E_INVALID, "%s: bad argument", who);
    if (x_adv == x || x_adv == x_start) return clf_fail(DG_E_INVALID, "%s: x_adv must not be x or x_start", who);
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (!h->pgd) h->pgd = new PgdWork();
    PgdWork* w = h->pgd;
    const int n = h->n_logits, P = h->pixels();
    int rc = clf_grow(&w->seed, 1, w->seed_floats, (size_t)B * n);
    if (rc || (rc = clf_grow(w->iter, 2, w->iter_floats, (size_t)B * P))) return rc;
    CLF_TRY(hipMemsetAsync(first_success, 0xFF, (size_t)B * sizeof(int32_t), s));          // -1: no success yet
    const long long nseed = (long long)B * n;
    const float* cur = x_start;
    for (int k = 0; k < nb_iter; ++k) {
        if ((rc = clf_kept_forward(h, cur, B, s))) return rc;
        if (k > 0 && (rc = pgd_track(h, labels, B, k, cur, x_adv, first_success, s))) return rc;          // iterate k, off its own forward
        clf_launch_ce_grad(h->acts[h->logit_layer], labels, w->seed, B, n, s);
        hipLaunchKernelGGL(pgd_mask_seed_kernel, dim3((unsigned)((nseed + 255) / 256)), dim3(256), 0, s, w->seed, labels, nseed, n);
        float* g = nullptr;
        if ((rc = clf_seeded_backward(h, w->seed, B, s, &g))) return rc;
        float* next = w->iter[k & 1];
        rc = ball ? clf_launch_ball_step(g, nullptr, cur, x, next, B, P, eps, eps_iter, clip_min, clip_max, s)
                  : clf_launch_bpda_step(g, nullptr, cur, x, next, (long long)B * P, P, 0, eps, eps_iter, clip_min, clip_max, s);
        if (rc) return rc;
        cur = next;
    }
    if ((rc = clf_kept_forward(h, cur, B, s))) return rc;                                   // the last iterate's trailing forward
    return pgd_track(h, labels, B, nb_iter, cur, x_adv, first_success, s);
}

}  // namespace

extern "C" {

int dg_pgd(dg_clf* h, const float* x, const float* x_start, const int32_t* labels, int B, float eps, float eps_iter, int nb_iter,
           float clip_min, float clip_max, float* x_adv, int32_t* first_success, void* stream) {
    return pgd_run("dg_pgd", false, h, x, x_start, labels, B, eps, eps_iter, nb_iter, clip_min, clip_max, x_adv, first_success, stream);
}

int dg_pgd_ball(dg_clf* h, const float* x, const float* x_start, const int32_t* labels, int B, float eps, float eps_iter, int nb_iter,
                int ord, float clip_min, float clip_max, float* x_adv, int32_t* first_success, void* stream) {
    if (ord != 2) return clf_fail(DG_E_INVALID, "dg_pgd_ball: ord must be 2 (the L1 projection needs a sort), got %d", ord);
    return pgd_run("dg_pgd_ball", true, h, x, x_start, labels, B, eps, eps_iter, nb_iter, clip_min, clip_max, x_adv, first_success, stream);
}

}  // extern "C"
