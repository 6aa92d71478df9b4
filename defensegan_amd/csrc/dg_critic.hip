// The WGAN-GP critic: its cost, the gradient of that cost with respect to every parameter -- the gradient penalty's double
// backward included -- and one Adam step (the reference's models/gan.py:167-199, mode "wgan-gp", and the critic half of its
// train(), gan.py:285-291; DESIGN.md section 7, "The critic").  The critic D is a dg_clf model of Conv2D, LeakyReLU (ReLU), Flatten
// and Linear layers with one output (models/dataset_models.py:74-97).  With real, fake [B,H,W,C], alpha [B]:
//
//   xhat = real + alpha (fake - real)
//   w    = mean_b D(fake_b) - mean_b D(real_b)
//   g    = d(sum_b D(xhat_b)) / dxhat                                   [B,H,W,C]
//   s    = sqrt(sum over the reduced axes of g^2)       penalty_axes 0: over H alone, s [B,W,C] (the reference's reduction_indices=[1]
//                                                        on an NHWC tensor); 1: over H, W, C, s [B] (the published form)
//   P    = mean over what is left of (s - 1)^2,  cost = w + lambda P
//
// D is piecewise linear in its input, so the activation slopes (1 / 0.2 for LeakyReLU, 1 / 0 for ReLU) at xhat's pre-activations are
// constants of differentiation: g = C_1^T a_1 with a_L = seed, a_j = m_j . C_{j+1}^T a_{j+1} is LINEAR in every layer's weights, the
// penalty has no second-order term through the slopes and no bias gradient.  With v = dP/dg = (2 / N) ((s - 1) / s) g (0 where
// s == 0, where TF has NaN: a deliberate departure) and the tangent pass u_0 = v, u_j = m_j . C_j u_{j-1} (no biases),
//
//   dP/dC_j = wgrad(input u_{j-1}, output gradient a_j)
//
// which is the weight-gradient GEMM training already has (tr_wgrad_kernel), fed another (input, output gradient) pair and no bias
// row.  One call therefore runs: the three batches [fake; real; xhat] as ONE forward and ONE backward of 3 B images with the seed
// (+1/B, -1/B, 1) -- which leaves a_j of all three --, the Wasserstein weight gradients over the first 2 B images, the norms and v
// (lambda folded into v), the tangent pass over B images and its weight gradients, and the reduction of both sets of partial sums
// in a fixed order, optionally with Adam.  New kernels: the interpolation, the norms, the slope mask, the cost and the reduction
// with an Adam whose betas are arguments; the convolutions are dg_clf.hip's, the weight gradients dg_clf_train.hip's.  No atomics,
// every sum has a fixed order: a call repeated returns the same bits.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "dg_attack_device.h"
#include "dg_clf_internal.h"

struct CriticWork {
    int cap_B = 0;
    std::vector<float*> act, gout, tan;       // per layer: outputs [3 cap_B, f], gradients at the output [3 cap_B, f], tangents [cap_B, f]
    std::vector<float*> part;                 // per parameter layer: partial sums, Wasserstein slots then penalty slots
    std::vector<size_t> part_floats;
    float *X = nullptr, *gx = nullptr, *v = nullptr;      // [3 cap_B, P] the three batches, [cap_B, P] g, [cap_B, P] v
    float *pen = nullptr, *cost = nullptr, *zero = nullptr;   // [cap_B] per-image penalty sums, [3], [widest cout] zeros
};

namespace {

constexpr int kMaxB = 1 << 20;

// X = [fake; real; xhat], xhat = real + alpha_b (fake - real); seed = (+1/B, -1/B, 1) per image of the three batches
__global__ __launch_bounds__(256) void critic_interp_kernel(const float* __restrict__ real, const float* __restrict__ fake,
                                                             const float* __restrict__ alpha, int B, long long P, float* __restrict__ X,
                                                             float* __restrict__ seed) {
    const long long total = (long long)B * P;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / P;
    const float r = real[i], f = fake[i];
    X[i] = f;
    X[total + i] = r;
    X[2 * total + i] = __fmaf_rn(alpha[b], f - r, r);
    if (i - b * P == 0) {
        const float inv = 1.0f / (float)B;
        seed[b] = inv;
        seed[B + b] = -inv;
        seed[2 * B + b] = 1.0f;
    }
}

// v's factor of g: coef (s - 1) / s with coef = lambda 2 / N; 0 where s == 0 (and where lambda is 0)
__device__ __forceinline__ float critic_factor(float s, float coef) { return (s > 0.f && coef != 0.f) ? coef * ((s - 1.0f) / s) : 0.f; }

// One workgroup per image, strided over the images.  IMAGE: s_b over the image's H * WC elements (thread t sums elements t, t + 256,
// ... in order, then the block).  Otherwise: thread t owns the columns t, t + 256, ... of the WC columns and sums each over the H
// rows in order.  v = factor(s) g; slopes (may be NULL) = s; pen[b] = the image's sum of (s - 1)^2.
template <bool IMAGE>
__global__ __launch_bounds__(256) void critic_norm_kernel(const float* __restrict__ g, int B, int H, int WC, float coef,
                                                           float* __restrict__ v, float* __restrict__ slopes, float* __restrict__ pen) {
    __shared__ float red[4];
    const long long P = (long long)H * WC;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const float* gb = g + b * P;
        float* vb = v + b * P;
        if constexpr (IMAGE) {
            float acc = 0.f;
            for (long long i = threadIdx.x; i < P; i += 256) acc = __fmaf_rn(gb[i], gb[i], acc);
            const float s = sqrtf(clf_block_sum(acc, red));
            const float f = critic_factor(s, coef);
            for (long long i = threadIdx.x; i < P; i += 256) vb[i] = f * gb[i];
            if (threadIdx.x == 0) {
                if (slopes) slopes[b] = s;
                pen[b] = (s - 1.0f) * (s - 1.0f);
            }
        } else {
            float mine = 0.f;
            for (int col = threadIdx.x; col < WC; col += 256) {
                float acc = 0.f;
                for (int r = 0; r < H; ++r) {
                    const float e = gb[(long long)r * WC + col];
                    acc = __fmaf_rn(e, e, acc);
                }
                const float s = sqrtf(acc);
                const float f = critic_factor(s, coef);
                for (int r = 0; r < H; ++r) vb[(long long)r * WC + col] = f * gb[(long long)r * WC + col];
                if (slopes) slopes[b * WC + col] = s;
                mine = __fmaf_rn(s - 1.0f, s - 1.0f, mine);
            }
            const float tot = clf_block_sum(mine, red);
            if (threadIdx.x == 0) pen[b] = tot;
        }
    }
}

// t *= the activation's slope at the reference pass: ref > 0 ? 1 : low (0.2 LeakyReLU, 0 ReLU); ref is the activation's OUTPUT at
// xhat, which has its input's sign.  out may be t.
__global__ __launch_bounds__(256) void critic_mask_kernel(const float* t, const float* __restrict__ ref, float low, float* out,
                                                           long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out[i] = ref[i] > 0.f ? t[i] : low * t[i];
}

// one thread: cost[0..2] = cost, w, P from D [3 B] (fake, real, xhat) and the per-image penalty sums, each summed in image order
__global__ __launch_bounds__(64) void critic_cost_kernel(const float* __restrict__ D, const float* __restrict__ pen, int B, double n_slopes,
                                                          float lambda, float* __restrict__ cost) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sf = 0.0, sr = 0.0, sp = 0.0;
    for (int b = 0; b < B; ++b) sf += (double)D[b];
    for (int b = 0; b < B; ++b) sr += (double)D[B + b];
    for (int b = 0; b < B; ++b) sp += (double)pen[b];
    const double w = sf / B - sr / B, p = sp / n_slopes;
    cost[0] = (float)(w + (double)lambda * p);
    cost[1] = (float)w;
    cost[2] = (float)p;
}

// per element e of (W; b): g = the slots' partial sums in order; grads[e] = g (grads != NULL); TF Adam with the given betas on
// W / b (m != NULL): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr_t m / (sqrt(v) + 1e-8)
__global__ __launch_bounds__(256) void critic_reduce_adam_kernel(const float* __restrict__ part, int slots, long long per,
                                                                  float* __restrict__ W, float* __restrict__ bias, long long nW,
                                                                  float* __restrict__ m, float* __restrict__ v, float* __restrict__ grads,
                                                                  float lr_t, float b1, float b2) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    float g = 0.f;
    for (int z = 0; z < slots; ++z) g += part[(long long)z * per + e];
    if (grads) grads[e] = g;
    if (!m) return;
    const float mm = b1 * m[e] + (1.0f - b1) * g;
    const float vv = b2 * v[e] + (1.0f - b2) * (g * g);
    m[e] = mm;
    v[e] = vv;
    float* p = e < nW ? W + e : bias + (e - nW);
    *p = *p - lr_t * mm / (sqrtf(vv) + 1e-8f);
}

unsigned grid_of(long long total) { return (unsigned)((total + 255) / 256); }

// the layers that run a kernel, in order; the model must be a critic
int kernel_layers(const dg_clf* h, std::vector<int>* ker) {
    for (int j = 0; j < (int)h->layers.size(); ++j) {
        const ClfLayer& l = h->layers[j];
        if (l.kind == DG_LAYER_DROPOUT || l.kind == DG_LAYER_SOFTMAX)
            return clf_fail(DG_E_INVALID, "a critic holds no Dropout or Softmax layer (layer %d)", j);
        if (!l.skip) ker->push_back(j);
    }
    if (ker->empty() || h->logit_layer != ker->back()) return clf_fail(DG_E_STATE, "critic has no layers");
    if (h->n_logits != 1 || h->cur_h * h->cur_w * h->cur_c != 1)
        return clf_fail(DG_E_INVALID, "a critic has one output per image, this model has %d", h->cur_h * h->cur_w * h->cur_c);
    const int missing = clf_missing_weights(h);
    if (missing >= 0) return clf_fail(DG_E_STATE, "critic layer %d has no weights", missing);
    return DG_OK;
}

template <class T>
int regrow(T*& ptr, size_t count) {
    size_t none = 0;
    return clf_grow(&ptr, 1, none, count);
}

int ensure(dg_clf* h, const std::vector<int>& ker, int B) {
    if (!h->critic) h->critic = new CriticWork();
    CriticWork* w = h->critic;
    const size_t cnt = h->layers.size();
    if (w->act.size() != cnt) {          // layers were added since the last call: every per-layer buffer is sized anew
        critic_release(w);
        h->critic = w = new CriticWork();
    }
    if (B <= w->cap_B) return DG_OK;
    w->act.resize(cnt, nullptr);
    w->gout.resize(cnt, nullptr);
    w->tan.resize(cnt, nullptr);
    w->part.resize(cnt, nullptr);
    w->part_floats.resize(cnt, 0);
    w->cap_B = 0;
    int rc;
    size_t widest = 1;
    for (int j : ker) {
        const ClfLayer& l = h->layers[j];
        const size_t f = (size_t)l.features();
        if ((rc = regrow(w->act[j], 3 * (size_t)B * f)) || (rc = regrow(w->gout[j], 3 * (size_t)B * f)) || (rc = regrow(w->tan[j], (size_t)B * f)))
            return rc;
        if (l.has_params()) widest = std::max(widest, (size_t)l.cout);
    }
    const size_t P = (size_t)h->pixels();
    if ((rc = regrow(w->X, 3 * (size_t)B * P)) || (rc = regrow(w->gx, (size_t)B * P)) || (rc = regrow(w->v, (size_t)B * P)) ||
        (rc = regrow(w->pen, (size_t)B)) || (rc = regrow(w->cost, 3)) || (rc = regrow(w->zero, widest)))
        return rc;
    CLF_TRY(hipMemset(w->zero, 0, widest * sizeof(float)));
    w->cap_B = B;
    return DG_OK;
}

// Everything but the reduction: leaves the partial sums of every parameter layer (plan_w slots, then plan_t slots) and cost [3].
int critic_partials(dg_clf* h, const std::vector<int>& ker, const float* real, const float* fake, const float* alpha, int B, float lambda,
                    int axes, float* cost, float* slopes, std::vector<ClfWgradPlan>* plan_w, std::vector<ClfWgradPlan>* plan_t,
                    hipStream_t s) {
    CriticWork* w = h->critic;
    const long long P = h->pixels();
    const int last = ker.back();
    int rc;
    plan_w->assign(h->layers.size(), ClfWgradPlan());
    plan_t->assign(h->layers.size(), ClfWgradPlan());
    for (int j : ker) {
        const ClfLayer& l = h->layers[j];
        if (!l.has_params()) continue;
        (*plan_w)[j] = train_wgrad_plan(l, 2 * B);
        (*plan_t)[j] = train_wgrad_plan(l, B);
        const size_t need = ((size_t)(*plan_w)[j].slots + (size_t)(*plan_t)[j].slots) * (*plan_w)[j].per;
        if ((rc = clf_grow(&w->part[j], 1, w->part_floats[j], need))) return rc;
    }
    // the three batches, forward and backward as one
    hipLaunchKernelGGL(critic_interp_kernel, dim3(grid_of(B * P)), dim3(256), 0, s, real, fake, alpha, B, P, w->X, w->gout[last]);
    const float* cur = w->X;
    for (int j : ker) {
        clf_launch_forward(h, j, cur, w->act[j], 3 * B, s);
        cur = w->act[j];
    }
    for (int k = (int)ker.size() - 1; k >= 0; --k) {
        const int j = ker[k];
        const ClfLayer& l = h->layers[j];
        const long long f = l.features();
        if (l.has_params()) {
            const float* in = k > 0 ? w->act[ker[k - 1]] : w->X;
            train_launch_wgrad(l, in, w->gout[j], w->act[j], 2 * B, (*plan_w)[j], w->part[j], true, s);
        }
        if (k > 0)
            clf_launch_input_grad(h, j, w->gout[j], w->act[j], w->gout[ker[k - 1]], 3 * B, s);
        else            // only xhat's gradient reaches the input
            clf_launch_input_grad(h, j, w->gout[j] + 2 * B * f, w->act[j] + 2 * B * f, w->gx, B, s);
    }
    // the norms, v (lambda folded in) and the cost
    const int H = h->in_h, WC = h->in_w * h->in_c;
    const double n_slopes = axes == 0 ? (double)B * WC : (double)B;
    const float coef = (float)(2.0 * (double)lambda / n_slopes);
    const unsigned ngrid = (unsigned)std::min(B, 65536);
    if (axes == 0)
        hipLaunchKernelGGL(critic_norm_kernel<false>, dim3(ngrid), dim3(256), 0, s, w->gx, B, H, WC, coef, w->v, slopes, w->pen);
    else
        hipLaunchKernelGGL(critic_norm_kernel<true>, dim3(ngrid), dim3(256), 0, s, w->gx, B, H, WC, coef, w->v, slopes, w->pen);
    hipLaunchKernelGGL(critic_cost_kernel, dim3(1), dim3(64), 0, s, w->act[last], w->pen, B, n_slopes, lambda, cost);
    // the tangent pass over xhat's slopes and its weight gradients (no bias row)
    const float* t = w->v;
    for (int k = 0; k < (int)ker.size(); ++k) {
        const int j = ker[k];
        const ClfLayer& l = h->layers[j];
        const long long f = l.features(), total = B * f;
        const float* ref = w->act[j] + 2 * B * f;
        if (l.has_params()) {
            float* part_t = w->part[j] + (size_t)(*plan_w)[j].slots * (*plan_w)[j].per;
            train_launch_wgrad(l, t, w->gout[j] + 2 * B * f, ref, B, (*plan_t)[j], part_t, false, s);
            if (j == last) break;            // nothing reads the last layer's tangent
            clf_launch_linear_part(h, j, t, w->zero, w->tan[j], B, s);
            if (l.fused_relu) hipLaunchKernelGGL(critic_mask_kernel, dim3(grid_of(total)), dim3(256), 0, s, w->tan[j], ref, 0.f, w->tan[j], total);
        } else {
            hipLaunchKernelGGL(critic_mask_kernel, dim3(grid_of(total)), dim3(256), 0, s, t, ref, l.kind == DG_LAYER_LEAKY_RELU ? 0.2f : 0.f,
                               w->tan[j], total);
        }
        t = w->tan[j];
    }
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

int critic_call(dg_clf* h, const float* real, const float* fake, const float* alpha, int B, float lambda, int axes, float* grads,
                float* cost, float* slopes, bool adam, float lr, float b1, float b2, hipStream_t s, const char* who) {
    if (!h || !real || !fake || !alpha) return clf_fail(DG_E_INVALID, "%s: null argument", who);
    if (B < 1 || B > kMaxB) return clf_fail(DG_E_INVALID, "%s: B = %d outside [1, %d]", who, B, kMaxB);
    if (axes != 0 && axes != 1) return clf_fail(DG_E_INVALID, "%s: penalty_axes must be 0 (reference: height) or 1 (image), got %d", who, axes);
    std::vector<int> ker;
    int rc = kernel_layers(h, &ker);
    if (rc) return rc;
    CLF_TRY(hipSetDevice(h->device));
    float **m = nullptr, **v = nullptr;
    long long* t = nullptr;
    if (adam && (rc = train_adam_state(h, &m, &v, &t))) return rc;
    if ((rc = ensure(h, ker, B))) return rc;
    CriticWork* w = h->critic;
    std::vector<ClfWgradPlan> plan_w, plan_t;
    if ((rc = critic_partials(h, ker, real, fake, alpha, B, lambda, axes, cost ? cost : w->cost, slopes, &plan_w, &plan_t, s))) return rc;
    float lr_t = 0.f;
    if (adam) {
        *t += 1;
        lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)b2, (double)*t)) / (1.0 - std::pow((double)b1, (double)*t)));
    }
    size_t off = 0;
    for (int j : ker) {
        const ClfLayer& l = h->layers[j];
        if (!l.has_params()) continue;
        const long long per = (long long)plan_w[j].per;
        hipLaunchKernelGGL(critic_reduce_adam_kernel, dim3(grid_of(per)), dim3(256), 0, s, w->part[j], plan_w[j].slots + plan_t[j].slots, per,
                           l.W, l.b, per - l.cout, adam ? m[j] : nullptr, adam ? v[j] : nullptr, grads ? grads + off : nullptr, lr_t, b1, b2);
        off += (size_t)per;
    }
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

}  // namespace

void critic_release(CriticWork* w) {
    if (!w) return;
    auto drop = [](auto& vec) {
        for (float* q : vec)
            if (q) (void)hipFree(q);
    };
    drop(w->act); drop(w->gout); drop(w->tan); drop(w->part);
    for (float* q : {w->X, w->gx, w->v, w->pen, w->cost, w->zero})
        if (q) (void)hipFree(q);
    delete w;
}

extern "C" {

int dg_critic_gradient(dg_clf* h, const float* real, const float* fake, const float* alpha, int B, float gp_lambda, int penalty_axes,
                       float* grads, float* cost, float* slopes, void* stream) {
    if (!grads || !cost) return clf_fail(DG_E_INVALID, "dg_critic_gradient: null argument");
    return critic_call(h, real, fake, alpha, B, gp_lambda, penalty_axes, grads, cost, slopes, false, 0.f, 0.f, 0.f, (hipStream_t)stream,
                       "dg_critic_gradient");
}

int dg_critic_step(dg_clf* h, const float* real, const float* fake, const float* alpha, int B, float gp_lambda, int penalty_axes,
                   float learning_rate, float beta_a, float beta_b, float* cost, void* stream) {
    if (!(beta_a >= 0.f && beta_a < 1.f && beta_b >= 0.f && beta_b < 1.f))
        return clf_fail(DG_E_INVALID, "dg_critic_step: betas (%g, %g) outside [0, 1)", (double)beta_a, (double)beta_b);
    return critic_call(h, real, fake, alpha, B, gp_lambda, penalty_axes, nullptr, cost, nullptr, true, learning_rate, beta_a, beta_b,
                       (hipStream_t)stream, "dg_critic_step");
}

}  // extern "C"
