// DeepFool (Moosavi-Dezfooli, Fawzi, Frossard 2016; cleverhans' DeepFool, an empty, un-pinned submodule in the reference, restated
// in DESIGN.md section 7, "DeepFool"): the minimal L2 perturbation that carries an image over the nearest linearised decision
// boundary, the whole loop enqueued by one call.  No labels, no budget; the LOGITS are read, before any Softmax.
//
//     orig_b   = the first arg-max of logits(x_b);   cand_b[0 .. nc) = the nc classes of the largest logits at x_b, descending,
//                ties to the lower class (cand_b[0] = orig_b), fixed for the run;   r_b = 0, adv_b = x_b (not clipped)
//     an image is ACTIVE while the first arg-max over ALL classes at adv_b is orig_b
//     iteration, per active image:   f_j = Z[cand_j] - Z[cand_0],  w_j = dZ[cand_j]/dx - dZ[cand_0]/dx  at adv_b        0 < j < nc
//                                    pert_j = (|f_j| + 1e-5) / ||w_j||_2;   j* = the first index of the smallest pert_j
//                                    r_b += pert_j* w_j* / ||w_j*||_2;      adv_b = clip(x_b + r_b, lo, hi)
//     after max_iter iterations, or when no image is active:   x_adv_b = clip(x_b + (1 + overshoot) r_b, lo, hi)
//
// Where the textbook form divides by zero or compares a NaN: a candidate with ||w_j|| == 0 has pert_j = +inf; +inf and NaN are never the
// minimum; an image without a minimum becomes inactive and keeps its r_b (the iteration still counts in iters).  An image whose
// logits hold a NaN -- at x_b, or at the adv_b a step has just produced -- becomes inactive, and a step that produced one is taken
// back: the image returns clip(x_b + (1 + overshoot) r_b) from the last finite state.  A NaN is never a candidate for final_class
// (clf_wave_class: class 0 where class 0 is a NaN or nothing else is left).
//
// One iteration is: the class gradients of all nc candidates, the step (deepfool_step_kernel, one workgroup per image), one kept
// forward at the new adv, the activity kernel.  The class gradients come from the classifier's own chain (dg_clf_internal.h) and
// there are two ways to get them, equal bit for bit because every output element of that chain is one thread's fixed-order sum of
// its own row:
//     replicated rows   adv_b is kept nc times, rows b nc + j; ONE forward and ONE backward of B nc rows, the seed of row b nc + j
//                       the one-hot vector of cand_b[j].  2 L launches per iteration for L layers.
//     nc backwards      one forward of B rows, then nc backwards of B rows, each copied out of the gradient ping-pong: (nc + 1) L
//                       launches and nc copies.
// The product library runs the replicated rows (DESIGN.md has the measurement at B = 100, nc = 10); the measurement build
// (-DDG_MEASURE) runs the nc backwards, as a cross-check of the same bits and for tools/deepfool_time.py.
//
// Activity is a per-image flag on the device; r_b is double-buffered per image (rsel_b says which buffer is current), so that the
// NaN rule can take a step back without arithmetic.  Every DEEPFOOL_CHECK iterations the count of active images (an int32 atomic
// add per active image -- the only atomic, and an integer) is read back and the loop ends early when it is zero: iterations on
// no active image change nothing, so the result does not depend on that read, bit for bit.  Apart from it nothing waits for
// the device; no graph capture.  Every reduction is per image and in a fixed order: an image's result does not depend on which other
// images share the call.  gfx950 only, fp32, no float atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "dg_attack_device.h"
#include "dg_clf_internal.h"

#ifdef DG_MEASURE
#define DEEPFOOL_REPLICATED 0
#else
#define DEEPFOOL_REPLICATED 1
#endif

struct DeepfoolWork {
    float* seed = nullptr;               // [B nc, n] one-hot seeds: row b nc + j (replicated rows) or j B + b (nc backwards)
    size_t seed_floats = 0;
    float* rows = nullptr;               // [B copies, P] adv, copies = nc (replicated rows) or 1
    size_t rows_floats = 0;
    float* grads = nullptr;              // [nc, B, P] the class gradients of the nc backwards (not used by the replicated rows)
    size_t grads_floats = 0;
    float* r[2] = {nullptr, nullptr};    // [B, P] each: r_b lives in r[rsel_b]
    size_t r_floats = 0;
    int32_t* cand = nullptr;             // [B, nc]
    size_t cand_ints = 0;
    int32_t* flags = nullptr;            // [4, B]: orig, active, iters, rsel
    size_t flags_ints = 0;
    int32_t* choice = nullptr;           // [max_iter, B] the j* of every step, -1 where the image took none
    size_t choice_ints = 0;
    int32_t* count = nullptr;            // [max_iter + 1] active images after the setup and after every iteration
    size_t count_ints = 0;
    int32_t* host_count = nullptr;       // pinned, one int: where the early exit reads a count
    int last_B = 0, last_iter = -1;      // what `choice` holds (dg_deepfool_choices)
};

void deepfool_release(DeepfoolWork* w) {
    if (!w) return;
    for (void* p : {(void*)w->seed, (void*)w->rows, (void*)w->grads, (void*)w->r[0], (void*)w->r[1], (void*)w->cand, (void*)w->flags,
                    (void*)w->choice, (void*)w->count})
        if (p) (void)hipFree(p);
    if (w->host_count) (void)hipHostFree(w->host_count);
    delete w;
}

namespace {

constexpr int DEEPFOOL_CHECK = 2;            // iterations between two reads of the active count
constexpr int DEEPFOOL_MAX_CAND = 2048;      // 5 floats of LDS per candidate in the step kernel

// rows[(b copies + c), :] = x[b, :], one thread per element written
__global__ __launch_bounds__(256) void df_replicate_kernel(const float* __restrict__ x, float* __restrict__ rows, long long total, int P, int copies) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / P;
    rows[i] = x[(row / copies) * P + (i - row * P)];
}

// The setup of image b off the logits at x_b (row b * row_step of `logits`): cand_b = the nc largest logits in descending order, ties
// to the lower class; orig_b = cand_b[0]; active unless the row holds a NaN; iters = rsel = 0.  One wave per image (four per
// workgroup, the waves strided over the images), the classes strided over the 64 lanes.  Round t picks the first maximum among
// the classes that come after round t - 1's pick in the order (value descending, class ascending): nothing is stored per class, and
// -inf and +inf compare as numbers.  With a NaN in the row a round may find nothing; the slot then names class 0 (the image is
// inactive, its candidates are never read).
__global__ __launch_bounds__(256) void df_select_kernel(const float* __restrict__ logits, int n, long long row_step, int B, int nc,
                                                         int32_t* __restrict__ cand, int32_t* __restrict__ orig, int32_t* __restrict__ active,
                                                         int32_t* __restrict__ iters, int32_t* __restrict__ rsel, int32_t* __restrict__ count0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) {
        const float* r = logits + b * row_step * n;
        int bad = 0;
        for (int c = lane; c < n; c += 64) bad |= (r[c] != r[c]) ? 1 : 0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) bad |= __shfl_xor(bad, m, 64);
        float pv = 0.f;
        int pa = -1;                                            // round t - 1's pick; none before round 0
        for (int t = 0; t < nc; ++t) {
            float best = 0.f;
            int arg = clf_wave_argmax_if(r, n, lane, best, [&](float v, int c) { return pa < 0 ? (v == v) : (v < pv || (v == pv && c > pa)); });
            if (arg == INT_MAX) { arg = 0; best = -__builtin_inff(); }          // uniform over the wave; only with a NaN in the row
            if (lane == 0) cand[b * nc + t] = arg;
            pv = best;
            pa = arg;
            if (t == 0 && lane == 0) orig[b] = arg;
        }
        if (lane == 0) {
            active[b] = bad ? 0 : 1;
            iters[b] = 0;
            rsel[b] = 0;
            if (!bad) atomicAdd(count0, 1);
        }
    }
}

// seed[row, k] = (k == cand[b, j]): row = b nc + j (by_image) or j B + b.  One thread per element.
__global__ __launch_bounds__(256) void df_seed_kernel(const int32_t* __restrict__ cand, float* __restrict__ seed, long long total, int n, int B,
                                                       int nc, int by_image) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / n;
    const int k = (int)(i - row * n);
    const long long b = by_image ? row / nc : row % B;
    const int j = (int)(by_image ? row % nc : row / B);
    seed[i] = cand[b * nc + j] == k ? 1.0f : 0.0f;
}

// The DeepFool step of iteration k.  One workgroup of 256 threads per image, the workgroups strided over the images; an inactive
// image costs one load.  Class gradient j of image b is row b gb + j gj of `grads`, its logits row b row_step of `logits`.
//   pass 1   for j = 1 .. nc - 1: thread t sums (g_j - g_0)^2 over the vectors t, t + 256, ... of the row in index order (V = 4: float4);
//            a 64-lane butterfly leaves the wave's sum in every lane, lane 0 writes it to LDS: part[j][wave].  Every gradient
//            row is read once here; g_0's vector is read again per j, from the cache.
//   pass 2   thread j adds part[j][0 .. 4) in wave order, forms ||w_j|| and pert_j, and leaves both in LDS.
//   pass 3   every thread scans pert_1 .. pert_{nc-1} in order: the first index of the minimum, the same in every thread.
//   pass 4   rows j* and 0 are read a second time: r_new = r + (pert / ||w||) w, adv = clip(x + r_new), written `copies` times.
// LDS: 5 nc floats of the dynamic region (no static LDS, 32-bit accesses only).
template <int V>
__global__ __launch_bounds__(256) void deepfool_step_kernel(const float* __restrict__ grads, long long gb, long long gj, const float* __restrict__ logits,
                                                             int n, long long row_step, const int32_t* __restrict__ cand, int nc,
                                                             const float* __restrict__ x, float* __restrict__ r0, float* __restrict__ r1,
                                                             int32_t* __restrict__ rsel, float* __restrict__ rows, int copies,
                                                             int32_t* __restrict__ active, int32_t* __restrict__ iters, int32_t* __restrict__ choice,
                                                             int B, int P, float lo, float hi) {
    extern __shared__ __attribute__((aligned(16))) float df_lds[];
    float* part = df_lds;                      // [nc][4]; [j][0] becomes ||w_j|| in pass 2
    float* pert = df_lds + 4 * (size_t)nc;     // [nc]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long nvec = P / V;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        if (!active[b]) {                                       // uniform over the workgroup
            if (tid == 0) choice[b] = -1;
            continue;
        }
        const int sel = rsel[b];
        const float* g0 = grads + (b * gb) * P;
        // ---- pass 1
        for (int j = 1; j < nc; ++j) {
            const float* gjp = grads + (b * gb + j * gj) * P;
            float acc = 0.f;
            for (long long i = tid; i < nvec; i += 256) {
                const ClfVec<V> a = ClfVec<V>::load(gjp, i), c = ClfVec<V>::load(g0, i);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float d = a.e[e] - c.e[e];
                    acc = __fmaf_rn(d, d, acc);
                }
            }
            acc = clf_wave_sum(acc);
            if (lane == 0) part[4 * j + wave] = acc;
        }
        __syncthreads();
        // ---- pass 2
        const float* z = logits + b * row_step * n;
        const int32_t* cb = cand + b * nc;
        const float z0 = z[cb[0]];
        for (int j = 1 + tid; j < nc; j += 256) {
            const float wn = sqrtf(((part[4 * j] + part[4 * j + 1]) + part[4 * j + 2]) + part[4 * j + 3]);
            const float f = z[cb[j]] - z0;
            part[4 * j] = wn;
            pert[j] = wn > 0.f ? (fabsf(f) + 1e-5f) / wn : __builtin_inff();          // wn a NaN: +inf as well
        }
        __syncthreads();
        // ---- pass 3
        float best = __builtin_inff();
        int js = -1;
        for (int j = 1; j < nc; ++j) {
            const float p = pert[j];
            if (p < best) { best = p; js = j; }
        }
        if (js < 0) {                                           // uniform: no finite pert_j, the image stops where it is
            if (tid == 0) { active[b] = 0; iters[b] += 1; choice[b] = -1; }
            __syncthreads();                                    // the next image reuses the LDS
            continue;
        }
        const float coef = best / part[4 * js];
        // ---- pass 4
        const float* gs = grads + (b * gb + js * gj) * P;
        const float* rx = x + b * P;
        const float* rold = (sel ? r1 : r0) + b * P;
        float* rnew = (sel ? r0 : r1) + b * P;
        for (long long i = tid; i < nvec; i += 256) {
            const ClfVec<V> a = ClfVec<V>::load(gs, i), c = ClfVec<V>::load(g0, i), ro = ClfVec<V>::load(rold, i), xo = ClfVec<V>::load(rx, i);
            ClfVec<V> rn, av;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                rn.e[e] = __fmaf_rn(coef, a.e[e] - c.e[e], ro.e[e]);
                av.e[e] = clf_clip(xo.e[e] + rn.e[e], lo, hi);
            }
            rn.store(rnew, i);
            for (int c2 = 0; c2 < copies; ++c2) av.store(rows + (b * copies + c2) * P, i);
        }
        if (tid == 0) { rsel[b] = sel ^ 1; iters[b] += 1; choice[b] = js; }
        __syncthreads();
    }
}

// After the forward at the new adv: an active image stays active while its row holds no NaN and its first arg-max over all classes
// is orig_b.  A NaN takes the step of this iteration back (choice_b >= 0: the image took one; rsel_b flips to the buffer that
// holds the r_b from before it).  Every image that stays active adds one to *count.  One wave per image, as df_select_kernel.
__global__ __launch_bounds__(256) void df_activity_kernel(const float* __restrict__ logits, int n, long long row_step, int B,
                                                           const int32_t* __restrict__ orig, int32_t* __restrict__ active, int32_t* __restrict__ rsel,
                                                           const int32_t* __restrict__ choice, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) {
        if (!active[b]) continue;                               // uniform over the wave
        bool nan;
        const int arg = clf_wave_argmax(logits + b * row_step * n, n, lane, &nan);
        if (lane == 0) {
            if (nan) {
                active[b] = 0;
                if (choice[b] >= 0) rsel[b] ^= 1;
            } else if (arg != orig[b]) {
                active[b] = 0;
            } else {
                atomicAdd(count, 1);
            }
        }
    }
}

// x_adv_b = clip(x_b + (1 + overshoot) r_b, lo, hi) and r_norm_b = ||x_adv_b - x_b||_2, the distance of what was written: thread t's
// terms in index order, then clf_block_sum (dg_attack_device.h).  x_adv may be x.
template <int V>
__global__ __launch_bounds__(256) void deepfool_final_kernel(const float* x, const float* __restrict__ r0, const float* __restrict__ r1,
                                                              const int32_t* __restrict__ rsel, float* x_adv, float* __restrict__ r_norm, int B, int P,
                                                              float scale, float lo, float hi) {
    extern __shared__ __attribute__((aligned(16))) float df_lds[];
    const int tid = threadIdx.x;
    const long long nvec = P / V;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const float* rx = x + b * P;
        const float* rr = (rsel[b] ? r1 : r0) + b * P;
        float* ro = x_adv + b * P;
        float acc = 0.f;
        for (long long i = tid; i < nvec; i += 256) {
            const ClfVec<V> xo = ClfVec<V>::load(rx, i), rv = ClfVec<V>::load(rr, i);
            ClfVec<V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                o.e[e] = clf_clip(__fmaf_rn(scale, rv.e[e], xo.e[e]), lo, hi);
                const float d = o.e[e] - xo.e[e];
                acc = __fmaf_rn(d, d, acc);
            }
            o.store(ro, i);
        }
        const float s = clf_block_sum(acc, df_lds);
        if (tid == 0 && r_norm) r_norm[b] = sqrtf(s);
    }
}

// final_class_b = the first arg-max of row b, a NaN never a candidate; class 0 where class 0 is a NaN or nothing is left
__global__ __launch_bounds__(256) void df_class_kernel(const float* __restrict__ logits, int n, int B, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) {
        const int arg = clf_wave_class(logits + b * n, n, lane);
        if (lane == 0) out[b] = arg;
    }
}

unsigned df_wave_grid(int B) { return (unsigned)((B + 3) / 4 < 4096 ? (B + 3) / 4 : 4096); }
unsigned df_image_grid(int B) { return (unsigned)(B < 65536 ? B : 65536); }
unsigned df_flat_grid(long long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

extern "C" {

int dg_deepfool(dg_clf* h, const float* x, int B, int nb_candidate, float overshoot, int max_iter, float clip_min, float clip_max,
                float* x_adv, float* r_norm, int32_t* iters, int32_t* final_class, void* stream) {
    if (!h || !x || !x_adv) return clf_fail(DG_E_INVALID, "dg_deepfool: null handle, x or x_adv");
    if (B < 1) return clf_fail(DG_E_INVALID, "dg_deepfool: B must be >= 1, got %d", B);
    if (nb_candidate < 2 || nb_candidate > h->n_logits)
        return clf_fail(DG_E_INVALID, "dg_deepfool: nb_candidate must be in [2, %d] (the number of logits), got %d", h->n_logits, nb_candidate);
    if (nb_candidate > DEEPFOOL_MAX_CAND)
        return clf_fail(DG_E_INVALID, "dg_deepfool: not implemented for more than %d candidates, got %d", DEEPFOOL_MAX_CAND, nb_candidate);
    if (max_iter < 0) return clf_fail(DG_E_INVALID, "dg_deepfool: max_iter must be >= 0, got %d", max_iter);
    if (!(clip_min <= clip_max)) return clf_fail(DG_E_INVALID, "dg_deepfool: clip_min must not exceed clip_max");
    const int nc = nb_candidate, n = h->n_logits, P = h->pixels();
    const int copies = DEEPFOOL_REPLICATED ? nc : 1;
    if ((long long)B * nc > INT_MAX || (long long)B * max_iter > INT_MAX)
        return clf_fail(DG_E_INVALID, "dg_deepfool: B * nb_candidate and B * max_iter must fit an int32");
    const int missing = clf_missing_weights(h);
    if (missing >= 0) return clf_fail(DG_E_STATE, "classifier layer %d has no weights", missing);
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (!h->deepfool) h->deepfool = new DeepfoolWork();
    DeepfoolWork* w = h->deepfool;
    const int RB = B * copies;                                  // rows the classifier sees per forward
    int rc = clf_grow(&w->seed, 1, w->seed_floats, (size_t)B * nc * n);
    if (rc || (rc = clf_grow(&w->rows, 1, w->rows_floats, (size_t)RB * P)) || (rc = clf_grow(w->r, 2, w->r_floats, (size_t)B * P)) ||
        (rc = clf_grow(&w->cand, 1, w->cand_ints, (size_t)B * nc)) || (rc = clf_grow(&w->flags, 1, w->flags_ints, (size_t)4 * B)) ||
        (rc = clf_grow(&w->choice, 1, w->choice_ints, (size_t)B * (max_iter > 0 ? max_iter : 1))) ||
        (rc = clf_grow(&w->count, 1, w->count_ints, (size_t)max_iter + 1)))
        return rc;
    if (!DEEPFOOL_REPLICATED && (rc = clf_grow(&w->grads, 1, w->grads_floats, (size_t)nc * B * P))) return rc;
    if (!w->host_count) CLF_TRY(hipHostMalloc((void**)&w->host_count, sizeof(int32_t), hipHostMallocDefault));
    int32_t *orig = w->flags, *active = w->flags + B, *it = w->flags + 2 * (size_t)B, *rsel = w->flags + 3 * (size_t)B;
    w->last_B = B;
    w->last_iter = max_iter;

    CLF_TRY(hipMemsetAsync(w->r[0], 0, (size_t)B * P * sizeof(float), s));
    CLF_TRY(hipMemsetAsync(w->choice, 0xFF, (size_t)B * (max_iter > 0 ? max_iter : 1) * sizeof(int32_t), s));          // -1: no step
    CLF_TRY(hipMemsetAsync(w->count, 0, ((size_t)max_iter + 1) * sizeof(int32_t), s));
    const long long nrow = (long long)RB * P, nseed = (long long)B * nc * n;
    hipLaunchKernelGGL(df_replicate_kernel, dim3(df_flat_grid(nrow)), dim3(256), 0, s, x, w->rows, nrow, P, copies);
    if ((rc = clf_kept_forward(h, w->rows, RB, s))) return rc;
    hipLaunchKernelGGL(df_select_kernel, dim3(df_wave_grid(B)), dim3(256), 0, s, h->acts[h->logit_layer], n, (long long)copies, B, nc, w->cand, orig,
                       active, it, rsel, w->count);
    hipLaunchKernelGGL(df_seed_kernel, dim3(df_flat_grid(nseed)), dim3(256), 0, s, w->cand, w->seed, nseed, n, B, nc, DEEPFOOL_REPLICATED);
    CLF_TRY(hipGetLastError());

    const bool vec = P % 4 == 0 && clf_aligned16(x) && clf_aligned16(x_adv);          // the workspace rows are aligned where P % 4 == 0
    const size_t lds = (size_t)5 * nc * sizeof(float);
    for (int k = 0; k < max_iter; ++k) {
        const float* g = nullptr;
        long long gb, gj;
        if (DEEPFOOL_REPLICATED) {
            float* gg = nullptr;
            if ((rc = clf_seeded_backward(h, w->seed, RB, s, &gg))) return rc;
            g = gg; gb = nc; gj = 1;
        } else {
            for (int j = 0; j < nc; ++j) {
                float* gg = nullptr;
                if ((rc = clf_seeded_backward(h, w->seed + (size_t)j * B * n, B, s, &gg))) return rc;
                CLF_TRY(hipMemcpyAsync(w->grads + (size_t)j * B * P, gg, (size_t)B * P * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
            g = w->grads; gb = 1; gj = B;
        }
        int32_t* ch = w->choice + (size_t)k * B;
        if (vec)
            hipLaunchKernelGGL(deepfool_step_kernel<4>, dim3(df_image_grid(B)), dim3(256), lds, s, g, gb, gj, h->acts[h->logit_layer], n, (long long)copies,
                               w->cand, nc, x, w->r[0], w->r[1], rsel, w->rows, copies, active, it, ch, B, P, clip_min, clip_max);
        else
            hipLaunchKernelGGL(deepfool_step_kernel<1>, dim3(df_image_grid(B)), dim3(256), lds, s, g, gb, gj, h->acts[h->logit_layer], n, (long long)copies,
                               w->cand, nc, x, w->r[0], w->r[1], rsel, w->rows, copies, active, it, ch, B, P, clip_min, clip_max);
        CLF_TRY(hipGetLastError());
        if ((rc = clf_kept_forward(h, w->rows, RB, s))) return rc;
        hipLaunchKernelGGL(df_activity_kernel, dim3(df_wave_grid(B)), dim3(256), 0, s, h->acts[h->logit_layer], n, (long long)copies, B, orig, active,
                           rsel, ch, w->count + k + 1);
        CLF_TRY(hipGetLastError());
        if ((k + 1) % DEEPFOOL_CHECK == 0 && k + 1 < max_iter) {          // the early exit: nothing is active, nothing would change
            CLF_TRY(hipMemcpyAsync(w->host_count, w->count + k + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            CLF_TRY(hipStreamSynchronize(s));
            if (*w->host_count == 0) break;
        }
    }

    const float scale = 1.0f + overshoot;
    if (vec)
        hipLaunchKernelGGL(deepfool_final_kernel<4>, dim3(df_image_grid(B)), dim3(256), 4 * sizeof(float), s, x, w->r[0], w->r[1], rsel, x_adv, r_norm,
                           B, P, scale, clip_min, clip_max);
    else
        hipLaunchKernelGGL(deepfool_final_kernel<1>, dim3(df_image_grid(B)), dim3(256), 4 * sizeof(float), s, x, w->r[0], w->r[1], rsel, x_adv, r_norm,
                           B, P, scale, clip_min, clip_max);
    CLF_TRY(hipGetLastError());
    if (iters) CLF_TRY(hipMemcpyAsync(iters, it, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (final_class) {
        if ((rc = clf_kept_forward(h, x_adv, B, s))) return rc;
        hipLaunchKernelGGL(df_class_kernel, dim3(df_wave_grid(B)), dim3(256), 0, s, h->acts[h->logit_layer], n, B, final_class);
        CLF_TRY(hipGetLastError());
    }
    return DG_OK;
}

int dg_deepfool_choices(dg_clf* h, int B, int max_iter, int32_t* choices, void* stream) {
    if (!h || !choices || B < 1 || max_iter < 1) return clf_fail(DG_E_INVALID, "dg_deepfool_choices: bad argument");
    const DeepfoolWork* w = h->deepfool;
    if (!w || w->last_B != B || w->last_iter != max_iter)
        return clf_fail(DG_E_STATE, "dg_deepfool_choices: the handle's last dg_deepfool call was not one of B = %d, max_iter = %d", B, max_iter);
    CLF_TRY(hipSetDevice(h->device));
    CLF_TRY(hipMemcpyAsync(choices, w->choice, (size_t)B * max_iter * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DG_OK;
}

}  // extern "C"
