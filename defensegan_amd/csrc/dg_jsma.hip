// The Jacobian saliency-map attack (Papernot, McDaniel, Jha, Fredrikson, Celik, Swami 2016; cleverhans' SaliencyMapMethod, an empty,
// un-pinned submodule in the reference, restated in DESIGN.md section 7, "Saliency map"): the L0 attack of the suite.  A targeted
// attack that moves two features per iteration by theta until the model says the target class, the whole loop enqueued by one call.
//
//     adv_b = x_b;   dom_b[p] = x_b[p] < clip_max (theta > 0) or x_b[p] > clip_min (theta < 0);   active_b = the target is a class
//     iteration, per active image:
//       1   O = the outputs at adv_b: the logits, or (of_probs) softmax(logits), the maximum subtracted before exp.  The image
//           becomes inactive when the first arg-max of O is t_b (a NaN is never a candidate: clf_wave_argmax), when O holds a NaN,
//           or when fewer than 2 features are left in dom_b.
//       2   a = grad_adv O[t_b],   b = grad_adv sum_{j != t_b} O[j]: two seeded backwards, the seeds e_t and 1 - e_t on O.  They
//           are no full Jacobian.  With of_probs the outputs sum to one, so b = -a in exact arithmetic (in float32: up to rounding)
//           and the score below is (a_p + a_q)^2: cleverhans' behaviour on its default get_probs, and the reason of_probs = 0 exists.
//       3   over the pairs p < q, both in dom_b:  A = a_p + a_q,  Bs = b_p + b_q;  admissible where A > 0 and Bs < 0 (theta > 0)
//           or A < 0 and Bs > 0 (theta < 0);  score = -(A Bs).  The admissible pair of the largest score is taken, ties to the
//           smallest p, then the smallest q (the first arg-max of the flat [F, F] index); a NaN score is never larger.
//       4   without an admissible pair of score > 0 the image becomes inactive and keeps adv_b.  (A departure: cleverhans' arg-max
//           of an all-zero tensor is pair (0, 0), and feature 0 is then moved twice.)
//       5   adv_b[p] = clip(adv_b[p] + theta), the same for q; both leave dom_b, saturated or not; iters_b += 1;
//           choices[k][b] = (p, q).
//     after max_iters iterations, or when no image is active:   x_adv_b = adv_b;   final_class_b = the first arg-max of the logits
//     at x_adv_b, from one more forward (clf_wave_class);   n_changed_b = the number of elements with x_adv != x (a NaN element of
//     x is a bit copy and is not counted).
//
// Restricting the pairs to dom_b equals cleverhans' `increase_coef * max|.|` trick: there an excluded feature has 2 max|a| subtracted
// from its entry of a and 2 max|b| added to its entry of b (theta > 0; the signs turned for theta < 0), so that its shifted sum with
// any other feature can never pass the sign test; here it is not in the list.  The result is the same pair, without a magnitude that
// depends on the whole row.
//
// The frameworks build a [B, F, F] score tensor per iteration for step 3 (2.4 GB at B = 1000 on MNIST).  Here jsma_pair_kernel, the
// hot path, runs one workgroup of 256 threads per image and needs no such tensor:
//     compact   thread t takes the features [t chunk, (t + 1) chunk), counts those in dom_b; a wave scan and the four wave totals give
//               its offset; it writes (a_p, b_p) and p of its in-domain features to LDS, in index order: D entries.
//     search    the triangle's row i (i < D - 1, the pairs (i, j), j > i: D - 1 - i of them) belongs to wave i mod 4 -- rows dealt
//               round-robin, so the four waves' shares differ by 3 pairs per row dealt, 6 / D of the whole -- and the wave's lanes
//               stride its columns: lane l takes j = i + 1 + l, + 64, ...  The (a, b) of 64 neighbouring columns are one conflict-free
//               8-byte LDS read, row i's is a broadcast.  Every lane meets its pairs in increasing (i, j) and keeps its first strict
//               maximum among the admissible scores > 0.
//     merge     a 64-lane xor butterfly, then the four waves in order, by (score descending, flat index i D + j ascending): the
//               compaction keeps the order of p, so that is (p, q) ascending.  No float atomics; comparisons only, no sums.
//     apply     thread 0 moves the two features in both rows of adv, clears dom, writes choices, iters and the domain count.
// Rows 2b and 2b + 1 of the workspace both hold adv_b: per iteration the classifier runs ONE kept forward and ONE seeded backward
// of 2B rows, the seeds of rows 2b and 2b + 1 the ones for a and b (jsma_activity_kernel, one wave per image, which also decides
// step 1).  LDS: 12 bytes per feature (dynamic, sized by F) + 48: JSMA_MAX_FEATURES = 5120 fits the 64 KiB a workgroup gets
// without asking for more; 32 x 32 x 3 = 3072 is inside, CelebA's 12288 is not.
//
// Every second iteration the count of active images (an int32 atomic add per active image -- the only atomic, and an integer) is
// read back and the loop ends early when it is zero: iterations on no active image change nothing, so no bit of the result
// depends on that read.  Apart from it nothing waits for the device; no graph capture.  An image's result does not depend on B, on the
// other images or on the stream.  float4 where F % 4 == 0 and x, x_adv are 16-byte aligned (the workspace rows then are), scalar
// otherwise, as dg_ball.hip decides; both give the same bits.  gfx950 only, fp32.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "dg_attack_device.h"
#include "dg_clf_internal.h"

struct JsmaWork {
    float* rows = nullptr;               // [2B, P]: rows 2b and 2b + 1 are adv_b
    size_t rows_floats = 0;
    float* seed = nullptr;               // [2B, n]: d O[t] / d logits and d sum_{j != t} O[j] / d logits
    size_t seed_floats = 0;
    float* out = nullptr;                // [B, n] O = softmax(logits) (of_probs only)
    size_t out_floats = 0;
    uint8_t* dom = nullptr;              // [B, P] 1: the feature is in the search domain
    size_t dom_bytes = 0;
    int32_t* flags = nullptr;            // [3, B]: active, iters, ndom (the features left in dom)
    size_t flags_ints = 0;
    int32_t* choice = nullptr;           // [max_iters, B, 2] the (p, q) of every step, -1 where the image took none
    size_t choice_ints = 0;
    int32_t* count = nullptr;            // [max_iters] active images after step 1 of every iteration
    size_t count_ints = 0;
    int32_t* host_count = nullptr;       // pinned, one int: where the early exit reads a count
    int last_B = 0, last_iters = -1;     // what `choice` holds (dg_jsma_choices)
};

void jsma_release(JsmaWork* w) {
    if (!w) return;
    for (void* p : {(void*)w->rows, (void*)w->seed, (void*)w->out, (void*)w->dom, (void*)w->flags, (void*)w->choice, (void*)w->count})
        if (p) (void)hipFree(p);
    if (w->host_count) (void)hipHostFree(w->host_count);
    delete w;
}

namespace {

constexpr int JSMA_CHECK = 2;                // iterations between two reads of the active count
constexpr int JSMA_MAX_FEATURES = 5120;      // 12 bytes of LDS per feature in the pair kernel, + 48: under 64 KiB

// V domain flags at vector index i of a row of bytes, as bits 0 .. V - 1 (V = 4: one 32-bit access, the row 4-byte aligned)
template <int V> struct JsmaDom;
template <> struct JsmaDom<1> {
    __device__ __forceinline__ static unsigned load(const uint8_t* p, long long i) { return p[i] ? 1u : 0u; }
    __device__ __forceinline__ static void store(uint8_t* p, long long i, unsigned bits) { p[i] = (uint8_t)(bits & 1u); }
};
template <> struct JsmaDom<4> {
    __device__ __forceinline__ static unsigned load(const uint8_t* p, long long i) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(p)[i];
        return ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
    }
    __device__ __forceinline__ static void store(uint8_t* p, long long i, unsigned bits) {
        reinterpret_cast<uint32_t*>(p)[i] = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
    }
};

// The sum of `v` over the 256 threads of a workgroup, the same in every thread (integers: any order gives it).  `red` is 4 ints of
// LDS; two barriers, as clf_block_sum.
__device__ __forceinline__ int jsma_block_count(int v, int* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

// The start of image b: rows 2b and 2b + 1 = x_b, dom_b and its count, iters = 0, active unless the target is no class.  One workgroup
// per image, the workgroups strided over the images.
template <int V>
__global__ __launch_bounds__(256) void jsma_init_kernel(const float* __restrict__ x, const int32_t* __restrict__ target, int n, float* __restrict__ rows,
                                                         uint8_t* __restrict__ dom, int32_t* __restrict__ active, int32_t* __restrict__ iters,
                                                         int32_t* __restrict__ ndom, int B, int P, float theta, float lo, float hi) {
    __shared__ int red[4];
    const int tid = threadIdx.x;
    const long long nvec = P / V;
    const bool up = theta > 0.f;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const float* rx = x + b * P;
        float* r0 = rows + 2 * b * P;
        float* r1 = r0 + P;
        int cnt = 0;
        for (long long i = tid; i < nvec; i += 256) {
            const ClfVec<V> xv = ClfVec<V>::load(rx, i);
            unsigned bits = 0;
#pragma unroll
            for (int e = 0; e < V; ++e) bits |= ((up ? xv.e[e] < hi : xv.e[e] > lo) ? 1u : 0u) << e;
            xv.store(r0, i);
            xv.store(r1, i);
            JsmaDom<V>::store(dom + b * P, i, bits);
            cnt += __popc(bits);
        }
        cnt = jsma_block_count(cnt, red);
        if (tid == 0) {
            const int t = target[b];
            active[b] = (t >= 0 && t < n) ? 1 : 0;
            iters[b] = 0;
            ndom[b] = cnt;
        }
    }
}

// Step 1 of an iteration and the seeds of step 2, off the logits at adv_b (row 2b of `logits`; row 2b + 1 is the same image).  One
// wave per image (four per workgroup, the waves strided over the images), the classes strided over the 64 lanes.  of_probs: O =
// softmax(logits) goes to out[b, :] -- each lane reads back only what it wrote --, the seeds are TF's softmax gradient for the
// upstream s on O, dz_k = p_k (s_k - sum_j s_j p_j):  s = e_t gives p_k ((k == t) - p_t),  s = 1 - e_t gives p_k ((k != t) - S),
// S = sum_{j != t} p_j, the lanes' terms in class order, then the butterfly.  Otherwise O = the logits and the seeds are e_t and
// 1 - e_t.  Every image that stays active adds one to *count.
__global__ __launch_bounds__(256) void jsma_activity_kernel(const float* __restrict__ logits, int n, int B, const int32_t* __restrict__ target,
                                                             int of_probs, float* __restrict__ out, float* __restrict__ seed,
                                                             int32_t* __restrict__ active, const int32_t* __restrict__ ndom, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) {
        if (!active[b]) continue;                               // uniform over the wave
        const float* z = logits + 2 * b * n;
        const int t = target[b];
        const float* o = z;
        float inv = 0.f, mx = 0.f;
        if (of_probs) {
            float m = -INFINITY;
            for (int k = lane; k < n; k += 64) m = fmaxf(m, z[k]);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
            float s = 0.f;
            for (int k = lane; k < n; k += 64) s += expf(z[k] - m);
            s = clf_wave_sum(s);
            inv = 1.0f / s;
            mx = m;
            float* ob = out + b * n;
            for (int k = lane; k < n; k += 64) ob[k] = expf(z[k] - m) * inv;
            o = ob;
        }
        bool nan;
        const int arg = clf_wave_argmax(o, n, lane, &nan);
        if (nan || arg == t || ndom[b] < 2) {                   // uniform over the wave
            if (lane == 0) active[b] = 0;
            continue;
        }
        float* sa = seed + 2 * b * n;
        float* sb = sa + n;
        if (of_probs) {
            const float pt = expf(z[t] - mx) * inv;
            float S = 0.f;
            for (int k = lane; k < n; k += 64) S += (k == t) ? 0.f : o[k];
            S = clf_wave_sum(S);
            for (int k = lane; k < n; k += 64) {
                const float pk = o[k];
                sa[k] = pk * ((k == t ? 1.0f : 0.0f) - pt);
                sb[k] = pk * ((k == t ? 0.0f : 1.0f) - S);
            }
        } else {
            for (int k = lane; k < n; k += 64) {
                sa[k] = k == t ? 1.0f : 0.0f;
                sb[k] = k == t ? 0.0f : 1.0f;
            }
        }
        if (lane == 0) atomicAdd(count, 1);
    }
}

// Steps 3 to 5 of an iteration (the header comment has the passes).  One workgroup of 256 threads per image, the workgroups strided
// over the images; an inactive image costs one load.  grads rows 2b and 2b + 1 are a and b of image b.  `choice` is this iteration's
// [B, 2], preset to -1.  Dynamic LDS: (a, b) [P] as float2, index [P], 4 wave totals, 4 scores, 4 flat indices.
template <int V>
__global__ __launch_bounds__(256) void jsma_pair_kernel(const float* __restrict__ grads, float* __restrict__ rows, uint8_t* __restrict__ dom,
                                                         int32_t* __restrict__ active, int32_t* __restrict__ iters, int32_t* __restrict__ ndom,
                                                         int32_t* __restrict__ choice, int B, int P, float theta, float lo, float hi) {
    extern __shared__ __attribute__((aligned(16))) float jsma_lds[];
    float2* ab = reinterpret_cast<float2*>(jsma_lds);          // [P]
    int* idx = reinterpret_cast<int*>(jsma_lds + 2 * (size_t)P);   // [P]
    int* wtot = idx + P;                                        // [4]
    float* wscore = reinterpret_cast<float*>(wtot + 4);         // [4]
    int* wflat = reinterpret_cast<int*>(wscore + 4);            // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = ((P + 255) / 256 + V - 1) / V * V;        // features per thread, a multiple of V
    const int p0 = tid * chunk < P ? tid * chunk : P, p1 = p0 + chunk < P ? p0 + chunk : P;
    const bool up = theta > 0.f;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        if (!active[b]) continue;                               // uniform over the workgroup
        const float* ga = grads + 2 * b * P;
        const float* gb = ga + P;
        uint8_t* db = dom + b * P;
        // ---- compact
        int cnt = 0;
        for (int p = p0; p < p1; p += V) cnt += __popc(JsmaDom<V>::load(db, p / V));
        int inc = cnt;                                          // the inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int off = inc - cnt;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        const int D = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        for (int p = p0; p < p1; p += V) {
            const unsigned bits = JsmaDom<V>::load(db, p / V);
            if (!bits) continue;
            const ClfVec<V> av = ClfVec<V>::load(ga, p / V), bv = ClfVec<V>::load(gb, p / V);
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (bits & (1u << e)) {
                    ab[off] = make_float2(av.e[e], bv.e[e]);
                    idx[off] = p + e;
                    ++off;
                }
        }
        __syncthreads();
        // ---- search
        float best = 0.f;
        int flat = INT_MAX;
        for (int i = wave; i < D - 1; i += 4) {
            const float2 pi = ab[i];
            for (int j = i + 1 + lane; j < D; j += 64) {
                const float2 pj = ab[j];
                const float A = pi.x + pj.x, Bs = pi.y + pj.y;
                const bool adm = up ? (A > 0.f && Bs < 0.f) : (A < 0.f && Bs > 0.f);
                const float s = -(A * Bs);
                if (adm && s > best) { best = s; flat = i * D + j; }
            }
        }
        // ---- merge
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ob = __shfl_xor(best, m, 64);
            const int of = __shfl_xor(flat, m, 64);
            if (ob > best || (ob == best && of < flat)) { best = ob; flat = of; }
        }
        if (lane == 0) { wscore[wave] = best; wflat[wave] = flat; }
        __syncthreads();
        // ---- apply
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (wscore[w] > best || (wscore[w] == best && wflat[w] < flat)) { best = wscore[w]; flat = wflat[w]; }
            if (flat == INT_MAX) {
                active[b] = 0;                                  // no admissible pair of score > 0
            } else {
                const int i = flat / D, j = flat - i * D;
                const int p = idx[i], q = idx[j];
                float* r0 = rows + 2 * b * P;
                float* r1 = r0 + P;
                const float vp = clf_clip(r0[p] + theta, lo, hi), vq = clf_clip(r0[q] + theta, lo, hi);
                r0[p] = vp; r1[p] = vp;
                r0[q] = vq; r1[q] = vq;
                db[p] = 0; db[q] = 0;
                ndom[b] = D - 2;
                iters[b] += 1;
                choice[2 * b] = p;
                choice[2 * b + 1] = q;
            }
        }
        __syncthreads();                                        // the next image reuses the LDS
    }
}

// x_adv_b = adv_b (row 2b) and n_changed_b = the number of elements with x_adv != x, a NaN element of x not counted.  x_adv may be x.
template <int V>
__global__ __launch_bounds__(256) void jsma_final_kernel(const float* x, const float* __restrict__ rows, float* x_adv, int32_t* __restrict__ n_changed,
                                                          int B, int P) {
    __shared__ int red[4];
    const int tid = threadIdx.x;
    const long long nvec = P / V;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const float* rx = x + b * P;
        const float* ra = rows + 2 * b * P;
        float* ro = x_adv + b * P;
        int cnt = 0;
        for (long long i = tid; i < nvec; i += 256) {
            const ClfVec<V> xo = ClfVec<V>::load(rx, i), av = ClfVec<V>::load(ra, i);
#pragma unroll
            for (int e = 0; e < V; ++e) cnt += (av.e[e] != xo.e[e] && xo.e[e] == xo.e[e]) ? 1 : 0;
            av.store(ro, i);
        }
        cnt = jsma_block_count(cnt, red);
        if (tid == 0 && n_changed) n_changed[b] = cnt;
    }
}

// final_class_b = the first arg-max of row b, a NaN never a candidate; class 0 where class 0 is a NaN or nothing is left
__global__ __launch_bounds__(256) void jsma_class_kernel(const float* __restrict__ logits, int n, int B, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) {
        const int arg = clf_wave_class(logits + b * n, n, lane);
        if (lane == 0) out[b] = arg;
    }
}

unsigned jsma_wave_grid(int B) { return (unsigned)((B + 3) / 4 < 4096 ? (B + 3) / 4 : 4096); }
unsigned jsma_image_grid(int B) { return (unsigned)(B < 65536 ? B : 65536); }

}  // namespace

extern "C" {

int dg_jsma(dg_clf* h, const float* x, const int32_t* target, int B, float theta, int max_iters, float clip_min, float clip_max, int of_probs,
            float* x_adv, int32_t* iters, int32_t* final_class, int32_t* n_changed, void* stream) {
    if (!h || !x || !target || !x_adv) return clf_fail(DG_E_INVALID, "dg_jsma: null handle, x, target or x_adv");
    if (B < 1) return clf_fail(DG_E_INVALID, "dg_jsma: B must be >= 1, got %d", B);
    if (!std::isfinite(theta) || theta == 0.f) return clf_fail(DG_E_INVALID, "dg_jsma: theta must be finite and not zero");
    if (max_iters < 0) return clf_fail(DG_E_INVALID, "dg_jsma: max_iters must be >= 0, got %d", max_iters);
    if (!(clip_min <= clip_max)) return clf_fail(DG_E_INVALID, "dg_jsma: clip_min must not exceed clip_max");
    if (of_probs != 0 && of_probs != 1) return clf_fail(DG_E_INVALID, "dg_jsma: of_probs must be 0 or 1, got %d", of_probs);
    const int n = h->n_logits, P = h->pixels();
    if (P < 2) return clf_fail(DG_E_INVALID, "dg_jsma: the image must have at least 2 features, got %d", P);
    if (P > JSMA_MAX_FEATURES)
        return clf_fail(DG_E_INVALID, "dg_jsma: not implemented for more than %d features, got %d", JSMA_MAX_FEATURES, P);
    if (2LL * B > INT_MAX || 2LL * B * (max_iters > 0 ? max_iters : 1) > INT_MAX)
        return clf_fail(DG_E_INVALID, "dg_jsma: 2 * B and 2 * B * max_iters must fit an int32");
    const int missing = clf_missing_weights(h);
    if (missing >= 0) return clf_fail(DG_E_STATE, "classifier layer %d has no weights", missing);
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (!h->jsma) h->jsma = new JsmaWork();
    JsmaWork* w = h->jsma;
    const int RB = 2 * B;                                       // rows the classifier sees
    const size_t nchoice = (size_t)2 * B * (max_iters > 0 ? max_iters : 1);
    int rc = clf_grow(&w->rows, 1, w->rows_floats, (size_t)RB * P);
    if (rc || (rc = clf_grow(&w->seed, 1, w->seed_floats, (size_t)RB * n)) || (rc = clf_grow(&w->out, 1, w->out_floats, (size_t)B * n)) ||
        (rc = clf_grow(&w->dom, 1, w->dom_bytes, (size_t)B * P)) || (rc = clf_grow(&w->flags, 1, w->flags_ints, (size_t)3 * B)) ||
        (rc = clf_grow(&w->choice, 1, w->choice_ints, nchoice)) || (rc = clf_grow(&w->count, 1, w->count_ints, (size_t)max_iters + 1)))
        return rc;
    if (!w->host_count) CLF_TRY(hipHostMalloc((void**)&w->host_count, sizeof(int32_t), hipHostMallocDefault));
    int32_t *active = w->flags, *it = w->flags + B, *ndom = w->flags + 2 * (size_t)B;
    w->last_B = B;
    w->last_iters = max_iters;

    CLF_TRY(hipMemsetAsync(w->seed, 0, (size_t)RB * n * sizeof(float), s));           // an image inactive from the start has no seed
    CLF_TRY(hipMemsetAsync(w->choice, 0xFF, nchoice * sizeof(int32_t), s));           // -1: no step
    CLF_TRY(hipMemsetAsync(w->count, 0, ((size_t)max_iters + 1) * sizeof(int32_t), s));
    const bool vec = P % 4 == 0 && clf_aligned16(x) && clf_aligned16(x_adv);          // the workspace rows are aligned where P % 4 == 0
    if (vec)
        hipLaunchKernelGGL(jsma_init_kernel<4>, dim3(jsma_image_grid(B)), dim3(256), 0, s, x, target, n, w->rows, w->dom, active, it, ndom, B, P, theta,
                           clip_min, clip_max);
    else
        hipLaunchKernelGGL(jsma_init_kernel<1>, dim3(jsma_image_grid(B)), dim3(256), 0, s, x, target, n, w->rows, w->dom, active, it, ndom, B, P, theta,
                           clip_min, clip_max);
    CLF_TRY(hipGetLastError());

    const size_t lds = (size_t)12 * P + 48;
    for (int k = 0; k < max_iters; ++k) {
        if ((rc = clf_kept_forward(h, w->rows, RB, s))) return rc;
        hipLaunchKernelGGL(jsma_activity_kernel, dim3(jsma_wave_grid(B)), dim3(256), 0, s, h->acts[h->logit_layer], n, B, target, of_probs, w->out,
                           w->seed, active, ndom, w->count + k);
        CLF_TRY(hipGetLastError());
        if ((k + 1) % JSMA_CHECK == 0) {                        // the early exit: nothing is active, nothing would change
            CLF_TRY(hipMemcpyAsync(w->host_count, w->count + k, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            CLF_TRY(hipStreamSynchronize(s));
            if (*w->host_count == 0) break;
        }
        float* g = nullptr;
        if ((rc = clf_seeded_backward(h, w->seed, RB, s, &g))) return rc;
        int32_t* ch = w->choice + (size_t)k * 2 * B;
        if (vec)
            hipLaunchKernelGGL(jsma_pair_kernel<4>, dim3(jsma_image_grid(B)), dim3(256), lds, s, g, w->rows, w->dom, active, it, ndom, ch, B, P, theta,
                               clip_min, clip_max);
        else
            hipLaunchKernelGGL(jsma_pair_kernel<1>, dim3(jsma_image_grid(B)), dim3(256), lds, s, g, w->rows, w->dom, active, it, ndom, ch, B, P, theta,
                               clip_min, clip_max);
        CLF_TRY(hipGetLastError());
    }

    if (vec)
        hipLaunchKernelGGL(jsma_final_kernel<4>, dim3(jsma_image_grid(B)), dim3(256), 0, s, x, w->rows, x_adv, n_changed, B, P);
    else
        hipLaunchKernelGGL(jsma_final_kernel<1>, dim3(jsma_image_grid(B)), dim3(256), 0, s, x, w->rows, x_adv, n_changed, B, P);
    CLF_TRY(hipGetLastError());
    if (iters) CLF_TRY(hipMemcpyAsync(iters, it, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (final_class) {
        if ((rc = clf_kept_forward(h, x_adv, B, s))) return rc;
        hipLaunchKernelGGL(jsma_class_kernel, dim3(jsma_wave_grid(B)), dim3(256), 0, s, h->acts[h->logit_layer], n, B, final_class);
        CLF_TRY(hipGetLastError());
    }
    return DG_OK;
}

int dg_jsma_choices(dg_clf* h, int B, int max_iters, int32_t* choices, void* stream) {
    if (!h || !choices || B < 1 || max_iters < 1) return clf_fail(DG_E_INVALID, "dg_jsma_choices: bad argument");
    const JsmaWork* w = h->jsma;
    if (!w || w->last_B != B || w->last_iters != max_iters)
        return clf_fail(DG_E_STATE, "dg_jsma_choices: the handle's last dg_jsma call was not one of B = %d, max_iters = %d", B, max_iters);
    CLF_TRY(hipSetDevice(h->device));
    CLF_TRY(hipMemcpyAsync(choices, w->choice, (size_t)2 * B * max_iters * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DG_OK;
}

}  // extern "C"
