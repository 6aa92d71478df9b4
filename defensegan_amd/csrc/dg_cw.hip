// The third white-box attack of the reference (whitebox.py:192-210, --attack_type cw): cleverhans' CarliniWagnerL2, run as
// ONE asynchronous device call (dg_cw in include/defensegan_hip.h).  cleverhans is an empty, un-pinned submodule of the
// reference; its published attack (cleverhans 2.x attacks_tf.py, after Carlini's nn_robust_attacks) is restated.  Per image,
// lo / hi = clip_min / clip_max, P pixels, Z = logits (the layer before Softmax), t = label (y, y_target or the model's own
// first argmax on x):
//
//   setup        oimg = clip(x, lo, hi);  timg = atanh((clip((x - lo) / (hi - lo), 0, 1) * 2 - 1) * 0.999999)
//                other = (tanh(timg) + 1) / 2 * (hi - lo) + lo;  x_adv = oimg, o_bestl2 = 1e10, o_bestscore = -1, const = c0
//   outer step   (binary_search_steps) w = m = v = 0, bestl2 = 1e10, bestscore = -1, chunk prev = 1e6;
//                const = upper_bound on the last step when binary_search_steps >= 10 ("repeat")
//   iteration i  values from the PRE-update w (what sess.run([train, loss, l2dist, output, newimg]) returns):
//                newimg = (tanh(w + timg) + 1) / 2 * (hi - lo) + lo,  l2 = sum (newimg - other)^2
//                real = Z_t,  oth = max_k((1 - [k=t]) Z_k - [k=t] 10000)
//                loss1 = const * max(0, real - oth + kappa)   (targeted: max(0, oth - real + kappa))
//                dloss1/dZ only where the max argument is > 0 (TF Maximum sends ties to the constant 0), the max's share split
//                evenly over its maximisers (TF _MaxGrad), the label's own entry takes none of it
//                g = (dloss1/dnewimg + 2 (newimg - other)) * (hi - lo) / 2 * (1 - tanh^2(w + timg))
//                TF Adam (beta1 0.9, beta2 0.999, eps 1e-8, step = i + 1): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
//                w -= lr sqrt(1 - b2^step) / (1 - b1^step) * m / (sqrt(v) + eps)
//                abort early on i % max(max_iterations / 10, 1) == 0: the CHUNK's L = sum (loss1 + l2) > prev * 0.9999 stops
//                the chunk (that iteration's Adam step happened, its best tracking does not); otherwise prev = L
//                success = first argmax(Z') != t (targeted: == t), Z'_t = Z_t + kappa (targeted: Z_t - kappa);
//                l2 < bestl2 and success: bestl2 = l2, bestscore = argmax Z; l2 < o_bestl2 and success: the same for
//                o_bestl2 / o_bestscore, and x_adv = newimg
//   after step   bestscore != -1 and it counts as success: upper = min(upper, const), else lower = max(lower, const);
//                const = (lower + upper) / 2 if upper < 1e9, else (failure branch only) const *= 10
//
// Chunks of batch_size images share L and the abort decision; nothing else couples images.  A trailing partial chunk is a chunk
// of its own (cleverhans cannot run one).  Documented differences: L is summed in float64 in a fixed order (TF: float32
// reduce_sum), the constants are float64 and enter the loss as float32 (as the fed placeholder does), ties in the model's own
// prediction go to the first class (cleverhans splits them evenly).
//
// Per iteration the call enqueues: the classifier forward over all N images, keeping activations (dg_clf.hip, unchanged); (a)
// cw_head_kernel, one workgroup per image: l2, real / oth / loss1, the logit seed, success and argmax; the seeded backward to the
// input (dg_clf.hip's chain, unchanged); (b) cw_chunk_kernel, one workgroup per chunk: L in a fixed order (no float atomics:
// deterministic, and a chunk's images give the same bits alone or inside a larger call), the abort decision, best tracking,
// an "improved" flag per image; (c) cw_update_kernel, elementwise: x_adv = newimg where improved, the tanh / L2 gradient, Adam,
// the next w and newimg.  (d) cw_reset_kernel runs once per outer step: the constant update of the step before, the resets.
// No host synchronisation, copy or decision inside the call, and no graph capture (include/defensegan_hip.h, graph_max_rows).
//
// Deviation from "aborted chunks cost nothing": (a), (b) and (c) return at once for a chunk that has stopped, but the classifier
// kernels are FGSM's, untouched by this attack (bit-identity of dg_clf_input_gradient / dg_fgsm), and know no chunks; they
// keep running over all N images.  tools/cw_time.py measures abort_early on and off.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dg_attack_device.h"
#include "dg_bsearch.h"
#include "dg_shared_math.h"

namespace {

// the workspace, carved from one allocation: the search state (best = bestl2, obest = o_bestl2) and the N x P planes
struct CwBufs : SearchBufs {
    float *w, *m, *v, *timg, *other, *newimg;      // [N, P]
    float* l2;                                     // [N]
};

size_t carve(CwBufs* b, char* base, long long N, long long P, long long n, long long chunks) {
    SearchCarver c{base};
    for (float** p : {&b->w, &b->m, &b->v, &b->timg, &b->other, &b->newimg}) *p = c.take<float>((size_t)(N * P));
    b->l2 = c.take<float>(N);
    search_carve(b, c, N, n, chunks);
    return c.off;
}

__device__ __forceinline__ float cw_to_img(float t, float lo, float hi) { return (t + 1.0f) * 0.5f * (hi - lo) + lo; }

// once per call, one workgroup per image: the label, timg, other, x_adv = clip(x), the per-image constants and outer bests
__global__ __launch_bounds__(256) void cw_setup_kernel(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                        const float* __restrict__ logits, int n, long long P, float lo, float hi,
                                                        double initial_const, CwBufs bf, float* __restrict__ xadv) {
    const long long b = blockIdx.x;
    if (threadIdx.x == 0) search_setup(bf, b, labels, logits, n, initial_const);
    const float* xb = x + b * P;
    for (long long i = threadIdx.x; i < P; i += 256) {
        const float xv = xb[i];
        float u = (xv - lo) / (hi - lo);
        u = u < 0.f ? 0.f : (u > 1.f ? 1.f : u);
        const float ti = atanhf((u * 2.0f - 1.0f) * 0.999999f);
        bf.timg[b * P + i] = ti;
        bf.other[b * P + i] = cw_to_img(tanhf(ti), lo, hi);
        xadv[b * P + i] = xv < lo ? lo : (xv > hi ? hi : xv);
    }
}

// (d) once per outer step, one workgroup per image: the constant update of the previous step (update != 0), the repeat rule,
// and the resets of w, m, v, newimg, the step's bests and the chunk's abort state (reset != 0; reset == 0 after the last step:
// the constant update alone, so that the constants returned are cleverhans' final ones)
__global__ __launch_bounds__(256) void cw_reset_kernel(CwBufs bf, long long P, int batch_size, int update, int reset, int repeat_last,
                                                        int targeted, float lo, float hi) {
    const long long b = blockIdx.x;
    if (threadIdx.x == 0) {
        if (update) search_update_const(bf, b, targeted);
        if (reset) search_reset_scalars(bf, b, batch_size, repeat_last);
    }
    if (!reset) return;
    for (long long i = threadIdx.x; i < P; i += 256) {
        const long long j = b * P + i;
        bf.w[j] = 0.f;
        bf.m[j] = 0.f;
        bf.v[j] = 0.f;
        bf.newimg[j] = cw_to_img(tanhf(0.f + bf.timg[j]), lo, hi);
    }
}

// (a) one workgroup per image: l2 (fixed-order block reduction), loss1, the seed dloss1/dZ, success and argmax.  l2 adds the four
// wave sums as (p0 + p1) + (p2 + p3), NOT in clf_block_sum's order: deliberate, tests/support/cw_reference.py pins this association
// and another one changes bits.
__global__ __launch_bounds__(256) void cw_head_kernel(const float* __restrict__ logits, int n, long long P, int batch_size, int targeted,
                                                       float confidence, CwBufs bf) {
    __shared__ float red[4];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* sd = bf.seed + b * n;
    if (bf.abort_iter[b / batch_size] >= 0) {          // stopped chunk: a zero seed, nothing else
        for (int k = tid; k < n; k += 256) sd[k] = 0.f;
        return;
    }
    const float* ni = bf.newimg + b * P;
    const float* ot = bf.other + b * P;
    float sq = 0.f;
    for (long long i = tid; i < P; i += 256) {
        const float d = ni[i] - ot[i];
        sq = __builtin_fmaf(d, d, sq);
    }
    sq = clf_wave_sum(sq);
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    if (tid != 0) return;
    const float l2 = (red[0] + red[1]) + (red[2] + red[3]);
    const float* z = logits + b * n;
    const int t = bf.lab[b];
    if (t < 0 || t >= n) {                             // a label outside the classes: never a success, no gradient
        for (int k = 0; k < n; ++k) sd[k] = 0.f;
        bf.l2[b] = l2;
        bf.loss1[b] = 0.f;
        bf.succ[b] = 0;
        bf.score[b] = clf_first_argmax(z, n);
        return;
    }
    const float c = (float)bf.cst[b];
    float oth;
    const float arg = cw_hinge_arg(z, n, t, targeted, confidence, &oth);
    cw_hinge_seed(sd, z, n, t, targeted, c, arg, oth);
    bf.l2[b] = l2;
    bf.loss1[b] = c * (arg > 0.f ? arg : 0.f);
    bf.succ[b] = cw_success(z, n, t, targeted, confidence);          // on Z' (the label's entry moved by the confidence)
    bf.score[b] = clf_first_argmax(z, n);                            // on Z itself
}

// (b) one workgroup per chunk: the chunk's loss in a fixed order, the abort decision on check iterations, best tracking
__global__ __launch_bounds__(256) void cw_chunk_kernel(CwBufs bf, int N, int batch_size, int iter, int check) {
    search_chunk(
        bf, N, batch_size, iter, check, [&](int b) { return (double)bf.loss1[b] + (double)bf.l2[b]; }, [&](int b) { return bf.l2[b]; });
}

// (c) elementwise: x_adv = newimg where the image improved, then the gradient through tanh, TF Adam, the next w and newimg
__global__ __launch_bounds__(256) void cw_update_kernel(CwBufs bf, const float* __restrict__ grad, float* __restrict__ xadv, long long total,
                                                         long long P, int batch_size, int iter, float lr_t, float lo, float hi) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / P;
    const int ai = bf.abort_iter[b / batch_size];
    if (ai >= 0 && ai != iter) return;
    const float ni = bf.newimg[i];
    if (bf.improved[b]) xadv[i] = ni;
    const float ti = bf.timg[i];
    const float w = bf.w[i];
    const float th = tanhf(w + ti);
    const float g = (grad[i] + 2.0f * (ni - bf.other[i])) * ((hi - lo) * 0.5f * (1.0f - th * th));
    float m = bf.m[i], v = bf.v[i];
    const float wn = w - dg_tf_adam_step(m, v, g, lr_t);
    bf.m[i] = m;
    bf.v[i] = v;
    bf.w[i] = wn;
    bf.newimg[i] = cw_to_img(tanhf(wn + ti), lo, hi);
}

}  // namespace

void search_release(SearchWork* w) {
    if (!w) return;
    if (w->mem) (void)hipFree(w->mem);
    delete w;
}

extern "C" {

int dg_cw(dg_clf* h, const float* x, const int32_t* labels, int B, int targeted, int batch_size, float confidence, float learning_rate,
          int binary_search_steps, int max_iterations, int abort_early, double initial_const, float clip_min, float clip_max,
          float* x_adv, float* best_l2, int32_t* best_class, double* final_const, int32_t* chunk_stop, void* stream) {
    if (!h || !x || !x_adv || B <= 0) return clf_fail(DG_E_INVALID, "dg_cw: bad argument");
    if (batch_size <= 0 || binary_search_steps < 0 || max_iterations < 0 || !(clip_max > clip_min))
        return clf_fail(DG_E_INVALID, "dg_cw: bad parameters (batch_size %d, binary_search_steps %d, max_iterations %d, clip [%g, %g])",
                        batch_size, binary_search_steps, max_iterations, (double)clip_min, (double)clip_max);
    const int n = h->n_logits;
    if (n <= 0) return clf_fail(DG_E_STATE, "dg_cw: classifier has no layers");
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const long long N = B, P = h->pixels(), chunks = (N + batch_size - 1) / batch_size;
    CwBufs bf;
    const size_t need = carve(&bf, nullptr, N, P, n, chunks);
    int rc = search_workspace(&h->cw, need);
    if (rc) return rc;
    carve(&bf, h->cw->mem, N, P, n, chunks);

    const float lo = clip_min, hi = clip_max;
    if (!labels && (rc = clf_kept_forward(h, x, B, s))) return rc;      // the model's own prediction on x
    hipLaunchKernelGGL(cw_setup_kernel, dim3((unsigned)N), dim3(256), 0, s, x, labels, labels ? nullptr : h->acts[h->logit_layer], n, P,
                       lo, hi, initial_const, bf, x_adv);
    CLF_TRY(hipGetLastError());
    const long long total = N * P;
    const unsigned egrid = (unsigned)((total + 255) / 256);
    const int every = search_every(max_iterations);
    for (int step = 0; step < binary_search_steps; ++step) {
        hipLaunchKernelGGL(cw_reset_kernel, dim3((unsigned)N), dim3(256), 0, s, bf, P, batch_size, step > 0 ? 1 : 0, 1,
                           search_repeat_last(binary_search_steps, step), targeted ? 1 : 0, lo, hi);
        for (int it = 0; it < max_iterations; ++it) {
            if ((rc = clf_kept_forward(h, bf.newimg, B, s))) return rc;
            hipLaunchKernelGGL(cw_head_kernel, dim3((unsigned)N), dim3(256), 0, s, h->acts[h->logit_layer], n, P, batch_size, targeted ? 1 : 0,
                               confidence, bf);
            float* grad = nullptr;
            if ((rc = clf_seeded_backward(h, bf.seed, B, s, &grad))) return rc;
            hipLaunchKernelGGL(cw_chunk_kernel, dim3((unsigned)chunks), dim3(256), 0, s, bf, B, batch_size, it,
                               (abort_early && it % every == 0) ? 1 : 0);
            hipLaunchKernelGGL(cw_update_kernel, dim3(egrid), dim3(256), 0, s, bf, grad, x_adv, total, P, batch_size, it,
                               dg_tf_adam_lr(learning_rate, it + 1), lo, hi);
            CLF_TRY(hipGetLastError());
        }
        if ((rc = search_copy_chunk_stop(bf, chunk_stop, step, chunks, s))) return rc;
    }
    if (final_const && binary_search_steps > 0)          // the last step's constant update alone: cleverhans' final constants
        hipLaunchKernelGGL(cw_reset_kernel, dim3((unsigned)N), dim3(256), 0, s, bf, P, batch_size, 1, 0, 0, targeted ? 1 : 0, lo, hi);
    return search_copy_out(bf, N, final_const, best_l2, best_class, s);
}

}  // extern "C"
