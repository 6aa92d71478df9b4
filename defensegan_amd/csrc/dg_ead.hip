// The elastic-net attack (Chen, Sharma, Zhang, Yi, Hsieh 2018, "EAD"; cleverhans' ElasticNetMethod), the L1 attack of the suite, run
// as ONE asynchronous device call (dg_ead in include/defensegan_hip.h).  The reference has no counterpart (cleverhans is an empty,
// un-pinned submodule there); the published attack is restated and this text is the specification.  It is Carlini-Wagner's loss
// plus beta * ||delta||_1, minimised by iterative shrinkage-thresholding (ISTA, with `fista` FISTA).  Per image, lo / hi =
// clip_min / clip_max, P pixels, Z = logits (the layer before Softmax), t = label (y, y_target or the model's own first argmax on
// x), x0 = clip(x, lo, hi):
//
//   setup        x_adv = x0, o_best = 1e10, o_bestscore = -1, const = initial_const, lower = 0, upper = 1e10
//   outer step   (binary_search_steps) X = Y = x0 (X the iterate "newimg", Y the slack), best = 1e10, bestscore = -1, chunk
//                prev = 1e6; the iteration counter, and with it the rate schedule, restarts at 0;
//                const = upper on the last step when binary_search_steps >= 10 ("repeat")
//   iteration i  1 gradient on the slack: real = Z_t(Y), oth = max_k((1 - [k=t]) Z_k(Y) - [k=t] 10000),
//                  loss1_Y = max(0, real - oth + kappa)   (targeted: max(0, oth - real + kappa))
//                  dloss1/dZ by dg_cw's rules: only where the max argument is > 0, the max's share split evenly over its
//                  maximisers, the label's own entry takes none of oth's share;  g = const * dloss1_Y/dY + 2 (Y - x0)
//                2 rate: lr_i = learning_rate * (1 - i / max_iterations)^0.5 (polynomial decay to 0), float64 on the host, passed
//                  as float32
//                3 step and shrinkage: S = Y - lr_i g, d = S - x0;  d > beta: X' = min(S - beta, hi);  |d| <= beta: X' = x0 (the
//                  exact bits of x0);  d < -beta: X' = max(S + beta, lo)
//                4 extrapolation: zt = (i + 1) / (i + 4) with fista (float64 on the host, a float32 argument), 0 without;
//                  Y' = X' + zt (X' - X), NOT clipped: it may leave [lo, hi];  then X = X', Y = Y'
//                5 values of the new iterate: l2 = sum (X - x0)^2, l1 = sum |X - x0|, crit = l2 + beta l1 (decision rule EN) or l1
//                  (L1);  loss1_X as in 1 on Z(X);  the CHUNK's L = sum (const loss1_X + l2 + beta l1)
//                6 abort early on i % max(max_iterations / 10, 1) == 0: L > prev * 0.9999 stops the chunk (the iteration's update
//                  happened, its best tracking does not); otherwise prev = L
//                7 success = first argmax(Z'(X)) != t (targeted: == t), Z'_t = Z_t + kappa (targeted: Z_t - kappa);
//                  crit < best and success: best = crit, bestscore = argmax Z(X); crit < o_best and success: the same for
//                  o_best / o_bestscore, and x_adv = X
//   after step   dg_cw's lower / upper / const update, rule for rule
//
// Chunks of batch_size images share L and the abort decision; nothing else couples images.  A trailing partial chunk is a chunk
// of its own.  Documented differences from cleverhans: L is summed in float64 in a fixed order (TF: float32 reduce_sum); the
// constants are float64 and enter the loss as float32; the model's own prediction sends ties to the first class.
//
// The launches.  Iteration i's new iterate X and iteration i + 1's slack Y are independent, so they go through the classifier as
// ONE forward over 2 B rows [Y; X] (dg_clf.hip's kernels, unchanged; every row's bits are those of a B-row call).  The handle's
// activation buffers only grow, so the 2 B rows cost one reallocation on the handle's first call, none per call; both halves'
// activations are kept (the forward walk keeps all rows or none), the backward reads the first B rows, the slack's.  Hence the
// values of iteration i's X (steps 5-7) are formed at the head of iteration i + 1, before its update overwrites X, and those of
// the last iteration after one closing forward of X alone (B rows).  Iteration 0's forward has B rows: X = Y = x0 there.  Per
// iteration: the forward; (a) ead_iterate_head_kernel on the X half: loss1_X, success, argmax; (b) ead_chunk_kernel, one workgroup
// per chunk: L, the abort decision, best tracking, the "improved" flag; (c) ead_slack_head_kernel on the Y half: the logit seed; the
// seeded backward (dg_clf.hip's chain, unchanged); (d) ead_update_kernel, one workgroup per image: x_adv = X where improved, then
// S, X', Y' and l1 / l2 of X' in one pass over the image (thread t sums its elements t, t + 256, ... in order, then the block in
// clf_block_sum's order).  (e) ead_reset_kernel once per outer step.  No host synchronisation, copy or decision inside the
// call, no graph capture, no float atomics.  As in dg_cw the classifier kernels know no chunks and keep running over stopped
// chunks; (a) to (d) return at once for them.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dg_attack_device.h"
#include "dg_bsearch.h"

namespace {

// the workspace, carved from one allocation: the search state (seed = const * dloss1_Y/dlogits, loss1 = const * loss1_X, best /
// obest by the decision rule's criterion) and the rows
struct EadBufs : SearchBufs {
    float* xy;                                     // [2 N, P]: rows 0 .. N the slack Y, rows N .. 2 N the iterate X
    float* x0;                                     // [N, P] clip(x)
    float *l1, *l2;                                // [N]
};

size_t carve(EadBufs* b, char* base, long long N, long long P, long long n, long long chunks) {
    SearchCarver c{base};
    b->xy = c.take<float>((size_t)(2 * N * P));
    b->x0 = c.take<float>((size_t)(N * P));
    b->l1 = c.take<float>(N);
    b->l2 = c.take<float>(N);
    search_carve(b, c, N, n, chunks);
    return c.off;
}

// once per call, one workgroup per image: the label, x0 = x_adv = clip(x), the per-image constants and outer bests
__global__ __launch_bounds__(256) void ead_setup_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                         const float* __restrict__ logits, int n, long long P, float lo, float hi,
                                                         double initial_const, EadBufs bf, float* __restrict__ xadv) {
    const long long b = blockIdx.x;
    if (threadIdx.x == 0) search_setup(bf, b, labels, logits, n, initial_const);
    const float* xb = x + b * P;
    for (long long i = threadIdx.x; i < P; i += 256) {
        const float c = clf_clip(xb[i], lo, hi);
        bf.x0[b * P + i] = c;
        xadv[b * P + i] = c;
    }
}

// (e) once per outer step, one workgroup per image: the constant update of the step before (update != 0), the repeat rule and the
// resets X = Y = x0, the step's bests, the chunk's abort state (reset != 0; reset == 0 after the last step: the update alone)
__global__ __launch_bounds__(256) void ead_reset_kernel(EadBufs bf, long long N, long long P, int batch_size, int update, int reset,
                                                         int repeat_last, int targeted) {
    const long long b = blockIdx.x;
    if (threadIdx.x == 0) {
        if (update) search_update_const(bf, b, targeted);
        if (reset) {
            search_reset_scalars(bf, b, batch_size, repeat_last);
            bf.improved[b] = 0;
        }
    }
    if (!reset) return;
    for (long long i = threadIdx.x; i < P; i += 256) {
        const float v = bf.x0[b * P + i];
        bf.xy[b * P + i] = v;
        bf.xy[(N + b) * P + i] = v;
    }
}

// (c) one thread per image, on the slack's logits: seed = const * dloss1_Y/dZ (zero for a stopped chunk or a label outside the classes)
__global__ __launch_bounds__(64) void ead_slack_head_kernel(const float* __restrict__ logits, int N, int n, int batch_size, int targeted,
                                                             float confidence, EadBufs bf) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= N) return;
    float* sd = bf.seed + (long long)b * n;
    const int t = bf.lab[b];
    if (bf.abort_iter[b / batch_size] >= 0 || t < 0 || t >= n) {
        for (int k = 0; k < n; ++k) sd[k] = 0.f;
        return;
    }
    const float* z = logits + (long long)b * n;
    float oth;
    const float arg = cw_hinge_arg(z, n, t, targeted, confidence, &oth);
    cw_hinge_seed(sd, z, n, t, targeted, (float)bf.cst[b], arg, oth);
}

// (a) one thread per image, on the iterate's logits: const * loss1_X, success on Z', the first argmax of Z
__global__ __launch_bounds__(64) void ead_iterate_head_kernel(const float* __restrict__ logits, int N, int n, int batch_size, int targeted,
                                                               float confidence, EadBufs bf) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= N || bf.abort_iter[b / batch_size] >= 0) return;
    const float* z = logits + (long long)b * n;
    const int t = bf.lab[b];
    bf.score[b] = clf_first_argmax(z, n);
    if (t < 0 || t >= n) {                             // a label outside the classes: never a success, no loss
        bf.loss1[b] = 0.f;
        bf.succ[b] = 0;
        return;
    }
    float oth;
    const float arg = cw_hinge_arg(z, n, t, targeted, confidence, &oth);
    bf.loss1[b] = (float)bf.cst[b] * (arg > 0.f ? arg : 0.f);
    bf.succ[b] = cw_success(z, n, t, targeted, confidence);
}

// (b) one workgroup per chunk: the chunk's loss in a fixed order, the abort decision on check iterations, best tracking by the
// decision rule's criterion (rule 0: l2 + beta l1, rule 1: l1)
__global__ __launch_bounds__(256) void ead_chunk_kernel(EadBufs bf, int N, int batch_size, int iter, int check, float beta, int rule) {
    search_chunk(
        bf, N, batch_size, iter, check, [&](int b) { return ((double)bf.loss1[b] + (double)bf.l2[b]) + (double)beta * (double)bf.l1[b]; },
        [&](int b) { return rule ? bf.l1[b] : __builtin_fmaf(beta, bf.l1[b], bf.l2[b]); });
}

// (d) one workgroup per image: x_adv = X where the image improved (the iterate the chunk kernel just judged), then -- unless
// take_only -- the step on the slack, the shrinkage, the extrapolation, and l1 / l2 of the new iterate
__global__ __launch_bounds__(256) void ead_update_kernel(EadBufs bf, const float* __restrict__ grad, float* __restrict__ xadv, long long N,
                                                          long long P, int batch_size, float lr, float zt, float beta, float lo, float hi,
                                                          int take_only) {
    __shared__ float red[4];
    const long long b = blockIdx.x;
    if (bf.abort_iter[b / batch_size] >= 0) return;
    float* Y = bf.xy + b * P;
    float* X = bf.xy + (N + b) * P;
    const float* x0 = bf.x0 + b * P;
    float* xa = xadv + b * P;
    const int imp = bf.improved[b];
    if (take_only) {
        if (imp)
            for (long long i = threadIdx.x; i < P; i += 256) xa[i] = X[i];
        return;
    }
    const float* gb = grad + b * P;
    float s1 = 0.f, s2 = 0.f;
    for (long long i = threadIdx.x; i < P; i += 256) {
        const float xo = X[i], y = Y[i], o = x0[i];
        if (imp) xa[i] = xo;
        const float g = __builtin_fmaf(2.0f, y - o, gb[i]);
        const float S = __builtin_fmaf(-lr, g, y);
        const float d = S - o;
        float xn = o;
        if (d > beta) xn = fminf(S - beta, hi);
        else if (d < -beta) xn = fmaxf(S + beta, lo);
        X[i] = xn;
        Y[i] = __builtin_fmaf(zt, xn - xo, xn);
        const float e = xn - o;
        s1 += fabsf(e);
        s2 = __builtin_fmaf(e, e, s2);
    }
    const float t1 = clf_block_sum(s1, red);
    const float t2 = clf_block_sum(s2, red);
    if (threadIdx.x == 0) {
        bf.l1[b] = t1;
        bf.l2[b] = t2;
    }
}

}  // namespace

extern "C" {

int dg_ead(dg_clf* h, const float* x, const int32_t* labels, int B, int targeted, int batch_size, float confidence, float beta,
           int decision_rule, int fista, float learning_rate, int binary_search_steps, int max_iterations, int abort_early,
           double initial_const, float clip_min, float clip_max, float* x_adv, float* best_dist, int32_t* best_class, double* final_const,
           int32_t* chunk_stop, void* stream) {
    if (!h || !x || !x_adv || !best_dist || !best_class) return clf_fail(DG_E_INVALID, "dg_ead: null handle, x, x_adv, best_dist or best_class");
    if (B < 1) return clf_fail(DG_E_INVALID, "dg_ead: B must be >= 1, got %d", B);
    if (!(beta >= 0.f)) return clf_fail(DG_E_INVALID, "dg_ead: beta must be >= 0, got %g", (double)beta);
    if (!(clip_max > clip_min)) return clf_fail(DG_E_INVALID, "dg_ead: clip_min must be below clip_max, got [%g, %g]", (double)clip_min, (double)clip_max);
    if (max_iterations < 1) return clf_fail(DG_E_INVALID, "dg_ead: max_iterations must be >= 1, got %d", max_iterations);
    if (decision_rule != 0 && decision_rule != 1) return clf_fail(DG_E_INVALID, "dg_ead: decision_rule must be 0 (EN) or 1 (L1), got %d", decision_rule);
    if (batch_size <= 0 || binary_search_steps < 0)
        return clf_fail(DG_E_INVALID, "dg_ead: bad parameters (batch_size %d, binary_search_steps %d)", batch_size, binary_search_steps);
    const int n = h->n_logits;
    if (n <= 0) return clf_fail(DG_E_STATE, "dg_ead: classifier has no layers");
    const long long N = B, P = h->pixels(), chunks = (N + batch_size - 1) / batch_size;
    if (2 * N > 2147483647LL) return clf_fail(DG_E_INVALID, "dg_ead: B too large");
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    EadBufs bf;
    const size_t need = carve(&bf, nullptr, N, P, n, chunks);
    int rc = search_workspace(&h->ead, need);
    if (rc) return rc;
    carve(&bf, h->ead->mem, N, P, n, chunks);

    const float lo = clip_min, hi = clip_max;
    const int tg = targeted ? 1 : 0;
    if (!labels && (rc = clf_kept_forward(h, x, B, s))) return rc;      // the model's own prediction on x
    hipLaunchKernelGGL(ead_setup_kernel, dim3((unsigned)N), dim3(256), 0, s, x, labels, labels ? nullptr : h->acts[h->logit_layer], n, P,
                       lo, hi, initial_const, bf, x_adv);
    CLF_TRY(hipGetLastError());
    const unsigned hgrid = (unsigned)((N + 63) / 64);
    const int every = search_every(max_iterations);
    float* const Yrows = bf.xy;
    float* const Xrows = bf.xy + N * P;
    // steps 5-7 of iteration `it` from the logits of its X, which lie `row0` rows into the kept logits
    auto judge = [&](int it, long long row0) {
        hipLaunchKernelGGL(ead_iterate_head_kernel, dim3(hgrid), dim3(64), 0, s, h->acts[h->logit_layer] + row0 * n, B, n, batch_size, tg,
                           confidence, bf);
        hipLaunchKernelGGL(ead_chunk_kernel, dim3((unsigned)chunks), dim3(256), 0, s, bf, B, batch_size, it,
                           (abort_early && it % every == 0) ? 1 : 0, beta, decision_rule);
    };
    for (int step = 0; step < binary_search_steps; ++step) {
        hipLaunchKernelGGL(ead_reset_kernel, dim3((unsigned)N), dim3(256), 0, s, bf, N, P, batch_size, step > 0 ? 1 : 0, 1,
                           search_repeat_last(binary_search_steps, step), tg);
        for (int it = 0; it < max_iterations; ++it) {
            if (it == 0) {
                if ((rc = clf_kept_forward(h, Yrows, B, s))) return rc;
            } else {
                if ((rc = clf_kept_forward(h, Yrows, 2 * B, s))) return rc;
                judge(it - 1, N);
            }
            hipLaunchKernelGGL(ead_slack_head_kernel, dim3(hgrid), dim3(64), 0, s, h->acts[h->logit_layer], B, n, batch_size, tg, confidence, bf);
            float* grad = nullptr;
            if ((rc = clf_seeded_backward(h, bf.seed, B, s, &grad))) return rc;
            const float lr = (float)((double)learning_rate * std::sqrt(1.0 - (double)it / (double)max_iterations));
            const float zt = fista ? (float)((double)(it + 1) / (double)(it + 4)) : 0.f;
            hipLaunchKernelGGL(ead_update_kernel, dim3((unsigned)N), dim3(256), 0, s, bf, grad, x_adv, N, P, batch_size, lr, zt, beta, lo, hi, 0);
            CLF_TRY(hipGetLastError());
        }
        if ((rc = clf_kept_forward(h, Xrows, B, s))) return rc;          // the closing forward: the last iteration's X alone
        judge(max_iterations - 1, 0);
        hipLaunchKernelGGL(ead_update_kernel, dim3((unsigned)N), dim3(256), 0, s, bf, nullptr, x_adv, N, P, batch_size, 0.f, 0.f, beta, lo, hi, 1);
        CLF_TRY(hipGetLastError());
        if ((rc = search_copy_chunk_stop(bf, chunk_stop, step, chunks, s))) return rc;
    }
    if (final_const && binary_search_steps > 0)          // the last step's constant update alone
        hipLaunchKernelGGL(ead_reset_kernel, dim3((unsigned)N), dim3(256), 0, s, bf, N, P, batch_size, 1, 0, 0, tg);
    return search_copy_out(bf, N, final_const, best_dist, best_class, s);
}

}  // extern "C"
