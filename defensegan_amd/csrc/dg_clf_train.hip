// Training of the classifier zoo (the reference's whitebox.py:120-170 and blackbox.py's prep_bbox: cleverhans model_train with
// TF Adam, optionally adversarial).  cleverhans is an empty, un-pinned submodule of the reference; its published utils_tf.model_train
// / model_loss is restated ("Classifier training").  One Adam step on a batch (x, y) of B images:
//
//   clean half     training-phase forward of x (Dropout active, mask pass 0), ce_b = logsumexp(z_b) - z_b[y_b], z = logits
//                  (the Softmax layer's input); seed = (softmax(z) - onehot(y)) * s, s = 1 / B (0.5 / B with the adversarial half)
//   adversarial    (adv_eps > 0; whitebox.py:147-163) a second training-phase forward of x (mask pass 1), dCE/dz on the model's own
//                  first argmax (dg_fgsm's seed), the backward to the input, x_adv = clip(x + adv_eps * sign(grad), lo, hi) (a stopped
//                  gradient), a third forward on x_adv (mask pass 2) with the clean half's loss and seed
//   loss           mean_b ce (clean), or (mean_b ce_clean + mean_b ce_adv) / 2
//   gradients      Conv2D dK[a,c,ci,co] = sum_{b,yo,xo} x[b, yo*sh+a-pt, xo*sw+c-pl, ci] * gm[b,yo,xo,co], db[co] = sum gm;
//                  Linear dW = X^T G, db = sum_b G; gm = the output gradient masked by the layer's fused ReLU (out > 0)
//   Dropout        tf.nn.dropout(x, prob) in TF 1.x takes KEEP_prob: Dropout(0.25) keeps 25 % and scales by 4.  mask = floor(keep + u),
//                  y = (x / keep) * mask, dx = (g * mask) / keep (TF's autodiff of Mul and RealDiv).  u in [0, 1) from Philox4x32-10,
//                  key = seed, counter = (element / 4, layer | pass << 16, step lo, step hi), u_r = (word_r >> 8) * 2^-24 for element
//                  4 q + r of the layer's [B, features] output
//   Adam           TF's, as in dg_cw.hip: m = 0.9 m + 0.1 g, v = 0.999 v + 0.001 g^2, p -= lr_t * m / (sqrt(v) + 1e-8),
//                  lr_t = lr sqrt(1 - 0.999^t) / (1 - 0.9^t), t counted from 1 and held in the handle with m and v
//
// The forward and input-gradient kernels are dg_clf.hip's own, launched through the launchers its own walkers use
// (dg_clf_internal.h), so that the inner FGSM of a model without Dropout is dg_fgsm bit for bit.  New here: the weight gradients (tr_wgrad_kernel, an implicit GEMM
// whose reduction axis B*OH*OW is split over fixed slots of workgroups), the slot reduction fused with Adam (tr_reduce_adam_kernel),
// Dropout, the cross-entropy seed and the loss.  No floating-point atomics: every sum has a fixed order, training is bit-reproducible.
// gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "dg_clf_internal.h"
#include "dg_shared_math.h"

struct TrainWork {
    int cap_B = 0;
    std::vector<float*> act, mask;            // per layer [cap_B, features]: kept outputs, Dropout masks (0 / 1)
    std::vector<const float*> in;             // per layer: its input in the current pass
    float* gbuf[2] = {nullptr, nullptr};      // gradient ping-pong [cap_B, widest layer]
    float *xb = nullptr, *xadv = nullptr;     // [cap_B, P]: the gathered batch, the adversarial inputs
    float *seed = nullptr, *ce = nullptr;     // [cap_B, n] dLoss/dlogits, [2, cap_B] per-image cross-entropy
    float* loss = nullptr;                    // [1] when the caller keeps no loss
    int32_t* lab = nullptr;                   // [cap_B]
    std::vector<float*> part;                 // per parameter layer [2, slots, M + 1, N]: partial sums of (dW; db)
    std::vector<size_t> part_floats;          // their capacities
    std::vector<int> slots, kc;               // per parameter layer, for the current B
    std::vector<float*> m, v;                 // per parameter layer [M + 1, N]: Adam moments of (W; b)
    long long t = 0;                          // Adam steps taken since the last reset
};

namespace {

// Training-phase Dropout over [total] elements, four per thread: mask = floor(keep + u), y = (x / keep) * mask (x == NULL: mask only)
__global__ __launch_bounds__(256) void tr_dropout_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ mask,
                                                          long long total, float keep, uint32_t k0, uint32_t k1, uint32_t c1,
                                                          uint32_t c2, uint32_t c3) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long first = q * 4;
    if (first >= total) return;
    uint32_t c[4] = {(uint32_t)q, c1, c2, c3};
    dg_philox4x32_10(c, k0, k1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = first + r;
        if (i >= total) break;
        const float u = (float)(c[r] >> 8) * 5.9604644775390625e-08f;      // 2^-24: exact, in [0, 1)
        const float mk = floorf(keep + u);
        mask[i] = mk;
        if (x) y[i] = (x[i] / keep) * mk;
    }
}

__global__ __launch_bounds__(256) void tr_dropout_bwd_kernel(const float* __restrict__ g, const float* __restrict__ mask,
                                                              float* __restrict__ dx, long long total, float keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) dx[i] = (g[i] * mask[i]) / keep;
}

// batch gather: xb[b] = X[idx[b]], lab[b] = labels[idx[b]]; an index outside [0, n) gives a zero image without a label
__global__ __launch_bounds__(256) void tr_gather_kernel(const float* __restrict__ X, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ idx, int n, long long P, int B,
                                                         float* __restrict__ xb, int32_t* __restrict__ lab) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * P) return;
    const long long b = i / P, p = i - b * P;
    const int src = idx[b];
    const bool ok = src >= 0 && src < n;
    xb[i] = ok ? X[(long long)src * P + p] : 0.f;
    if (p == 0) lab[b] = ok ? labels[src] : -1;
}

// one thread per image: seed = (softmax(z) - onehot(y)) * scale, ce = logsumexp(z) - z_y; a label outside [0, n) contributes nothing
__global__ __launch_bounds__(64) void tr_ce_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                    float* __restrict__ seed, float* __restrict__ ce, int B, int n, float scale) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float* z = logits + (long long)b * n;
    float* sd = seed + (long long)b * n;
    const int y = labels[b];
    if (y < 0 || y >= n) {
        for (int k = 0; k < n; ++k) sd[k] = 0.f;
        ce[b] = 0.f;
        return;
    }
    float mx = z[0];
    for (int k = 1; k < n; ++k) mx = z[k] > mx ? z[k] : mx;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += expf(z[k] - mx);
    const float inv = 1.0f / s;
    for (int k = 0; k < n; ++k) sd[k] = (expf(z[k] - mx) * inv - (k == y ? 1.0f : 0.0f)) * scale;
    ce[b] = (logf(s) + mx) - z[y];
}

// one thread: the step's loss, each half's sum in image order
__global__ __launch_bounds__(64) void tr_loss_kernel(const float* __restrict__ ce, int B, int halves, float* __restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float l[2] = {0.f, 0.f};
    for (int h = 0; h < halves; ++h) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += ce[h * B + b];
        l[h] = s / (float)B;
    }
    loss[0] = halves == 2 ? (l[0] + l[1]) * 0.5f : l[0];
}

// ---- weight gradients: an implicit GEMM per Conv2D / Linear layer -------------------------------------------------------------
// part[z, m, n] = sum_{k in slot z} A[k, m] * G[k, n], k = (b, yo, xo) of the layer output, m = (a, c, ci) of the kernel (row M: the
// bias, A = bias_one), n = co; A[k, (a,c,ci)] = x[b, yo*sh + a - pt, xo*sw + c - pl, ci] (0 in the padding), G = gm.  A Linear layer is a
// 1x1 convolution of a 1x1 image.  64 x 64 output tiles, 256 threads with a 4 x 4 register tile each, k in chunks of 16 through LDS;
// slot z owns k in [z Kc, (z + 1) Kc) and sums it in order.  The k index of a thread's loads depends on its wave only, so the
// (b, yo, xo) decode is wave-uniform.
struct WGeo {
    int ih, iw, ic, oh, ow, kh, kw, sh, sw, pt, pl;
    int M, N, K, Kc;
};

constexpr int WT = 64, WKC = 16;

__global__ __launch_bounds__(256) void tr_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ out, int relu, float bias_one,
                                                        float* __restrict__ part, WGeo q) {
    __shared__ __attribute__((aligned(16))) float As[WKC][WT];
    __shared__ __attribute__((aligned(16))) float Gs[WKC][WT];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * WT, n0 = blockIdx.y * WT, z = blockIdx.z;
    const int kbeg = z * q.Kc;
    const int kend = min(kbeg + q.Kc, q.K);
    const int lm = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mrow = m0 + lm, ncol = n0 + lm;
    const bool is_w = mrow < q.M, is_b = mrow == q.M, nok = ncol < q.N;
    int a = 0, c = 0, ci = 0;
    if (is_w) {
        ci = mrow % q.ic;
        const int ac = mrow / q.ic;
        c = ac % q.kw;
        a = ac / q.kw;
    }
    const long long img = (long long)q.ih * q.iw * q.ic;
    const int tm = tid >> 4, tn = tid & 15;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += WKC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = wv + 4 * r;
            const int k = k0 + kk;
            float av = 0.f, gv = 0.f;
            if (k < kend) {
                if (is_b) {
                    av = bias_one;                 // 1, or 0 for a term without a bias gradient (the critic's penalty)
                } else if (is_w) {
                    const int xo = k % q.ow, t1 = k / q.ow;
                    const int yo = t1 % q.oh, b = t1 / q.oh;
                    const int yi = yo * q.sh + a - q.pt, xi = xo * q.sw + c - q.pl;
                    if (yi >= 0 && yi < q.ih && xi >= 0 && xi < q.iw) av = x[b * img + ((long long)yi * q.iw + xi) * q.ic + ci];
                }
                if (nok) {
                    const long long gi = (long long)k * q.N + ncol;
                    gv = g[gi];
                    if (relu && !(out[gi] > 0.f)) gv = 0.f;
                }
            }
            As[kk][lm] = av;
            Gs[kk][lm] = gv;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < WKC; ++kk) {
            const float4 av = *reinterpret_cast<const float4*>(&As[kk][tm * 4]);
            const float4 gv = *reinterpret_cast<const float4*>(&Gs[kk][tn * 4]);
            const float ar[4] = {av.x, av.y, av.z, av.w}, gr[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(ar[i], gr[j], acc[i][j]);
        }
        __syncthreads();
    }
    const int M1 = q.M + 1;
    float* pz = part + (long long)z * M1 * q.N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + tm * 4 + i;
        if (m >= M1) break;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tn * 4 + j;
            if (n < q.N) pz[(long long)m * q.N + n] = acc[i][j];
        }
    }
}

// per element e of (W; b): g = sum of the slots in order; grads[e] = g (grads != NULL); Adam on W / b (m != NULL)
__global__ __launch_bounds__(256) void tr_reduce_adam_kernel(const float* __restrict__ part, int slots, long long per, float* __restrict__ W,
                                                              float* __restrict__ bias, long long nW, float* __restrict__ m,
                                                              float* __restrict__ v, float* __restrict__ grads, float lr_t) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    float g = 0.f;
    for (int z = 0; z < slots; ++z) g += part[(long long)z * per + e];
    if (grads) grads[e] = g;
    if (!m) return;
    float* p = e < nW ? W + e : bias + (e - nW);
    *p = *p - dg_tf_adam_step(m[e], v[e], g, lr_t);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// What training derives from the handle's layers (read in place, h->layers): the layer whose output is the logits, the first
// parameterised layer (nothing below it needs a gradient) and the Conv2D / Linear layers in order.
struct Plan {
    int last = -1, first_param = -1;
    std::vector<int> params;
};

// a layer that writes an output in the training phase (Dropout does, other than at evaluation)
bool has_output(const ClfLayer& v) { return v.has_params() || v.kind == DG_LAYER_DROPOUT || ((v.kind == DG_LAYER_RELU || v.kind == DG_LAYER_LEAKY_RELU) && !v.skip); }

WGeo geometry(const ClfLayer& v, int B) {
    WGeo q;
    if (v.kind == DG_LAYER_CONV2D)
        q = WGeo{v.ih, v.iw, v.ic, v.oh, v.ow, v.kh, v.kw, v.sh, v.sw, v.pad_t, v.pad_l, v.kh * v.kw * v.ic, v.oc, B * v.oh * v.ow, 0};
    else
        q = WGeo{1, 1, v.ic * v.ih * v.iw, 1, 1, 1, 1, 1, 1, 0, 0, v.ic * v.ih * v.iw, v.oc, B, 0};
    return q;
}

size_t param_floats(const ClfLayer& v) {      // (W; b) of a Conv2D / Linear layer
    const WGeo q = geometry(v, 1);
    return (size_t)(q.M + 1) * q.N;
}

// slots of the reduction axis: about 1024 workgroups per layer (four per CU), at least 64 terms per slot, at most 256 slots
void slot_plan(const WGeo& q, int* slots, int* kc) {
    const long long tiles = (long long)((q.M + 1 + WT - 1) / WT) * ((q.N + WT - 1) / WT);
    long long S = std::max(1LL, 1024 / tiles);
    S = std::min(S, std::max(1LL, (long long)q.K / 64));
    S = std::min(S, 256LL);
    const long long Kc = (q.K + S - 1) / S;
    *kc = (int)Kc;
    *slots = (int)((q.K + Kc - 1) / Kc);
}

int plan_of(const dg_clf* h, Plan* p) {
    const int cnt = (int)h->layers.size();
    p->last = h->logit_layer;
    for (int j = 0; j < cnt; ++j)
        if (h->layers[j].has_params()) p->params.push_back(j);
    if (p->last < 0 || p->params.empty()) return clf_fail(DG_E_STATE, "classifier has no parameterised layers");
    p->first_param = p->params.front();
    if (clf_missing_weights(h) >= 0) return clf_fail(DG_E_STATE, "classifier weights not set");
    for (int j = 0; j < cnt; ++j) {
        const ClfLayer& v = h->layers[j];
        if (v.kind != DG_LAYER_DROPOUT) continue;
        if (!(v.keep_prob > 0.f)) return clf_fail(DG_E_STATE, "Dropout layer %d has no keep_prob (dg_clf_set_dropout)", j);
        if (j > p->last) return clf_fail(DG_E_INVALID, "Dropout layer %d after the logits is not supported in training", j);
    }
    return DG_OK;
}

// a buffer that follows cap_B (or is allocated once): it has no capacity of its own and is always allocated anew
template <class T>
int regrow(T*& ptr, size_t count) {
    size_t none = 0;
    return clf_grow(&ptr, 1, none, count);
}

// the workspace for batches of up to B images, and the Adam state (zero, t = 0) on first use
int ensure(const dg_clf* h, TrainWork* w, const Plan& p, int B) {
    const int cnt = (int)h->layers.size();
    int rc;
    if ((int)w->m.size() != cnt) {
        w->m.assign(cnt, nullptr);
        w->v.assign(cnt, nullptr);
        for (int j : p.params) {
            const size_t per = param_floats(h->layers[j]);
            if ((rc = regrow(w->m[j], per)) || (rc = regrow(w->v[j], per))) return rc;
            CLF_TRY(hipMemset(w->m[j], 0, per * sizeof(float)));
            CLF_TRY(hipMemset(w->v[j], 0, per * sizeof(float)));
        }
        w->t = 0;
    }
    if (B <= w->cap_B) return DG_OK;
    w->act.resize(cnt, nullptr);
    w->mask.resize(cnt, nullptr);
    w->in.assign(cnt, nullptr);
    w->part.resize(cnt, nullptr);
    w->part_floats.resize(cnt, 0);
    w->slots.resize(cnt, 0);
    w->kc.resize(cnt, 0);
    const size_t P = (size_t)h->pixels();
    size_t widest = P;
    for (int j = 0; j < cnt; ++j) {
        const ClfLayer& v = h->layers[j];
        widest = std::max(widest, (size_t)v.features());
        if (has_output(v) && (rc = regrow(w->act[j], (size_t)B * v.features()))) return rc;
        if (v.kind == DG_LAYER_DROPOUT && (rc = regrow(w->mask[j], (size_t)B * v.features()))) return rc;
    }
    for (float*& g : w->gbuf)
        if ((rc = regrow(g, (size_t)B * widest))) return rc;
    if ((rc = regrow(w->xb, (size_t)B * P)) || (rc = regrow(w->xadv, (size_t)B * P)) || (rc = regrow(w->seed, (size_t)B * h->n_logits)) ||
        (rc = regrow(w->ce, 2 * (size_t)B)) || (rc = regrow(w->loss, 1)) || (rc = regrow(w->lab, (size_t)B)))
        return rc;
    w->cap_B = B;
    return DG_OK;
}

// slots for this B (the same B always gives the same slots: the sums' order depends on B alone) and room for both halves
int plan_slots(const dg_clf* h, TrainWork* w, const Plan& p, int B) {
    for (int j : p.params) {
        const WGeo q = geometry(h->layers[j], B);
        int S = 0, Kc = 0;
        slot_plan(q, &S, &Kc);
        int rc = clf_grow(&w->part[j], 1, w->part_floats[j], 2 * (size_t)S * (q.M + 1) * q.N);
        if (rc) return rc;
        w->slots[j] = S;
        w->kc[j] = Kc;
    }
    return DG_OK;
}

void launch_dropout(const float* x, float* y, float* mask, long long total, float keep, uint64_t seed, int layer, int pass, int64_t step,
                    hipStream_t s) {
    const long long quads = (total + 3) / 4;
    hipLaunchKernelGGL(tr_dropout_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, x, y, mask, total, keep, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)layer | ((uint32_t)pass << 16), (uint32_t)(uint64_t)step,
                       (uint32_t)((uint64_t)step >> 32));
}

void forward_pass(dg_clf* h, TrainWork* w, const Plan& p, const float* x, int B, int pass, uint64_t seed, int64_t step, hipStream_t s) {
    const float* cur = x;
    for (int j = 0; j <= p.last; ++j) {
        const ClfLayer& v = h->layers[j];
        if (!has_output(v)) continue;
        w->in[j] = cur;
        if (v.kind == DG_LAYER_DROPOUT)
            launch_dropout(cur, w->act[j], w->mask[j], (long long)B * v.features(), v.keep_prob, seed, j, pass, step, s);
        else
            clf_launch_forward(h, j, cur, w->act[j], B, s);
        cur = w->act[j];
    }
}

// from the seed dLoss/dlogits down; half >= 0: the weight gradients go to slot set `half`; to_input: carry the gradient to x
const float* backward_pass(dg_clf* h, TrainWork* w, const Plan& p, const float* seed, int B, int half, bool to_input, hipStream_t s) {
    const float* g = seed;
    int which = 0;
    for (int j = p.last; j >= 0; --j) {
        const ClfLayer& v = h->layers[j];
        if (!has_output(v)) continue;
        if (half >= 0 && v.has_params()) {
            ClfWgradPlan wp;
            wp.slots = w->slots[j];
            wp.kc = w->kc[j];
            wp.per = param_floats(v);
            train_launch_wgrad(v, w->in[j], g, w->act[j], B, wp, w->part[j] + (size_t)half * wp.slots * wp.per, true, s);
        }
        if (!to_input && j <= p.first_param) break;              // nothing below needs a gradient
        float* dx = w->gbuf[which ^ 1];
        if (v.kind == DG_LAYER_DROPOUT) {
            const long long total = (long long)B * v.features();
            hipLaunchKernelGGL(tr_dropout_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, w->mask[j], dx, total,
                               v.keep_prob);
        } else {
            clf_launch_input_grad(h, j, g, w->act[j], dx, B, s);
        }
        which ^= 1;
        g = dx;
    }
    return g;
}

// one step's gradient partials (both halves) and its loss; x_adv_out receives the adversarial inputs when not NULL
int gradient_step(dg_clf* h, TrainWork* w, const Plan& p, const float* x, const int32_t* lab, int B, float adv_eps, float lo, float hi,
                  uint64_t seed, int64_t step, float* loss, float* x_adv_out, hipStream_t s) {
    const bool adv = adv_eps > 0.f;
    const float scale = (adv ? 0.5f : 1.0f) / (float)B;
    const unsigned rgrid = (unsigned)((B + 63) / 64);
    forward_pass(h, w, p, x, B, 0, seed, step, s);
    hipLaunchKernelGGL(tr_ce_kernel, dim3(rgrid), dim3(64), 0, s, w->act[p.last], lab, w->seed, w->ce, B, h->n_logits, scale);
    backward_pass(h, w, p, w->seed, B, 0, false, s);
    if (adv) {
        forward_pass(h, w, p, x, B, 1, seed, step, s);
        clf_launch_ce_grad(w->act[p.last], nullptr, w->seed, B, h->n_logits, s);
        const float* gin = backward_pass(h, w, p, w->seed, B, -1, true, s);
        clf_launch_fgsm(x, gin, w->xadv, (long long)B * h->pixels(), adv_eps, lo, hi, s);
        forward_pass(h, w, p, w->xadv, B, 2, seed, step, s);
        hipLaunchKernelGGL(tr_ce_kernel, dim3(rgrid), dim3(64), 0, s, w->act[p.last], lab, w->seed, w->ce + B, B, h->n_logits, scale);
        backward_pass(h, w, p, w->seed, B, 1, false, s);
        if (x_adv_out) CLF_TRY(hipMemcpyAsync(x_adv_out, w->xadv, (size_t)B * h->pixels() * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(tr_loss_kernel, dim3(1), dim3(64), 0, s, w->ce, B, adv ? 2 : 1, loss);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

// the slot reduction of every parameter layer: gradients to grads (concatenated (W; b) per layer) and / or Adam with lr_t
int reduce(const dg_clf* h, TrainWork* w, const Plan& p, int B, bool adv, float* grads, bool adam, float lr_t, hipStream_t s) {
    size_t off = 0;
    for (int j : p.params) {
        const ClfLayer& v = h->layers[j];
        const WGeo q = geometry(v, B);
        const long long per = (long long)(q.M + 1) * q.N;
        hipLaunchKernelGGL(tr_reduce_adam_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, w->part[j], w->slots[j] * (adv ? 2 : 1),
                           per, v.W, v.b, (long long)q.M * q.N, adam ? w->m[j] : nullptr, adam ? w->v[j] : nullptr,
                           grads ? grads + off : nullptr, lr_t);
        off += (size_t)per;
    }
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

// the plan, and h->tr ready for batches of B images
int prepare(dg_clf* h, Plan* p, int B) {
    int rc = plan_of(h, p);
    if (rc) return rc;
    CLF_TRY(hipSetDevice(h->device));
    if (!h->tr) h->tr = new TrainWork();
    if ((rc = ensure(h, h->tr, *p, B))) return rc;
    return plan_slots(h, h->tr, *p, B);
}

}  // namespace

ClfWgradPlan train_wgrad_plan(const ClfLayer& v, int B) {
    ClfWgradPlan p;
    slot_plan(geometry(v, B), &p.slots, &p.kc);
    p.per = param_floats(v);
    return p;
}

void train_launch_wgrad(const ClfLayer& v, const float* x, const float* g, const float* out, int B, const ClfWgradPlan& p, float* part,
                        bool bias_row, hipStream_t s) {
    WGeo q = geometry(v, B);
    q.Kc = p.kc;
    hipLaunchKernelGGL(tr_wgrad_kernel, dim3((unsigned)((q.M + 1 + WT - 1) / WT), (unsigned)((q.N + WT - 1) / WT), (unsigned)p.slots),
                       dim3(256), 0, s, x, g, out, v.fused_relu ? 1 : 0, bias_row ? 1.f : 0.f, part, q);
}

int train_adam_state(dg_clf* h, float*** m, float*** v, long long** t) {
    Plan p;
    int rc = prepare(h, &p, 1);
    if (rc) return rc;
    *m = h->tr->m.data();
    *v = h->tr->v.data();
    *t = &h->tr->t;
    return DG_OK;
}

void train_release(TrainWork* w) {
    if (!w) return;
    auto drop = [](auto& vec) {
        for (auto* q : vec)
            if (q) (void)hipFree((void*)q);
    };
    drop(w->act); drop(w->mask); drop(w->part); drop(w->m); drop(w->v);
    for (float* q : {w->gbuf[0], w->gbuf[1], w->xb, w->xadv, w->seed, w->ce, w->loss})
        if (q) (void)hipFree(q);
    if (w->lab) (void)hipFree(w->lab);
    delete w;
}

extern "C" {

int dg_clf_adam_reset(dg_clf* h) {
    if (!h) return clf_fail(DG_E_INVALID, "null handle");
    Plan p;
    int rc = prepare(h, &p, 1);
    if (rc) return rc;
    TrainWork* w = h->tr;
    for (int j : p.params) {
        const size_t per = param_floats(h->layers[j]);
        CLF_TRY(hipMemset(w->m[j], 0, per * sizeof(float)));
        CLF_TRY(hipMemset(w->v[j], 0, per * sizeof(float)));
    }
    w->t = 0;
    return DG_OK;
}

int dg_clf_get_adam(dg_clf* h, int layer, float* m, float* v, int64_t* t, int is_device) {
    if (!h) return clf_fail(DG_E_INVALID, "null handle");
    Plan p;
    int rc = prepare(h, &p, 1);
    if (rc) return rc;
    TrainWork* w = h->tr;
    if (layer < 0 || layer >= (int)h->layers.size() || !h->layers[layer].has_params())
        return clf_fail(DG_E_INVALID, "layer %d has no parameters", layer);
    const size_t per = param_floats(h->layers[layer]);
    const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (m) CLF_TRY(hipMemcpy(m, w->m[layer], per * sizeof(float), kind));
    if (v) CLF_TRY(hipMemcpy(v, w->v[layer], per * sizeof(float), kind));
    if (t) *t = w->t;
    return DG_OK;
}

int dg_clf_set_adam(dg_clf* h, int layer, const float* m, const float* v, int64_t t, int is_device) {
    if (!h || !m || !v || t < 0) return clf_fail(DG_E_INVALID, "dg_clf_set_adam: bad argument");
    Plan p;
    int rc = prepare(h, &p, 1);
    if (rc) return rc;
    TrainWork* w = h->tr;
    if (layer < 0 || layer >= (int)h->layers.size() || !h->layers[layer].has_params())
        return clf_fail(DG_E_INVALID, "layer %d has no parameters", layer);
    const size_t per = param_floats(h->layers[layer]);
    const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    CLF_TRY(hipMemcpy(w->m[layer], m, per * sizeof(float), kind));
    CLF_TRY(hipMemcpy(w->v[layer], v, per * sizeof(float), kind));
    w->t = t;
    return DG_OK;
}

int dg_clf_dropout_mask(dg_clf* h, int layer, int B, uint64_t seed, int64_t step, int pass, float* mask, void* stream) {
    if (!h || !mask || B <= 0) return clf_fail(DG_E_INVALID, "dg_clf_dropout_mask: bad argument");
    if (layer < 0 || layer >= (int)h->layers.size()) return clf_fail(DG_E_INVALID, "layer %d out of range", layer);
    const ClfLayer& v = h->layers[layer];
    if (v.kind != DG_LAYER_DROPOUT || !(v.keep_prob > 0.f)) return clf_fail(DG_E_INVALID, "layer %d is not a Dropout layer with a keep_prob", layer);
    CLF_TRY(hipSetDevice(h->device));
    launch_dropout(nullptr, nullptr, mask, (long long)B * v.features(), v.keep_prob, seed, layer, pass, step, (hipStream_t)stream);
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

int dg_clf_param_gradient(dg_clf* h, const float* x, const int32_t* labels, int B, float adv_eps, float clip_min, float clip_max,
                          uint64_t seed, int64_t step, float* grads, float* loss, float* x_adv, void* stream) {
    if (!h || !x || !labels || !grads || B <= 0) return clf_fail(DG_E_INVALID, "dg_clf_param_gradient: bad argument");
    if (adv_eps > 0.f && !(clip_max > clip_min)) return clf_fail(DG_E_INVALID, "dg_clf_param_gradient: clip [%g, %g] is empty", (double)clip_min, (double)clip_max);
    Plan p;
    int rc = prepare(h, &p, B);
    if (rc) return rc;
    TrainWork* w = h->tr;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = gradient_step(h, w, p, x, labels, B, adv_eps, clip_min, clip_max, seed, step, loss ? loss : w->loss, x_adv, s))) return rc;
    return reduce(h, w, p, B, adv_eps > 0.f, grads, false, 0.f, s);
}

int dg_clf_train(dg_clf* h, const float* X, const int32_t* labels, int n, const int32_t* idx, int n_steps, int batch_size,
                 float learning_rate, float adv_eps, float clip_min, float clip_max, uint64_t seed, float* losses, void* stream) {
    if (!h || !X || !labels || !idx || n <= 0 || n_steps < 0 || batch_size <= 0) return clf_fail(DG_E_INVALID, "dg_clf_train: bad argument");
    if (adv_eps > 0.f && !(clip_max > clip_min)) return clf_fail(DG_E_INVALID, "dg_clf_train: clip [%g, %g] is empty", (double)clip_min, (double)clip_max);
    Plan p;
    int rc = prepare(h, &p, batch_size);
    if (rc) return rc;
    TrainWork* w = h->tr;
    hipStream_t s = (hipStream_t)stream;
    const long long P = h->pixels(), total = batch_size * P;
    const bool adv = adv_eps > 0.f;
    for (int st = 0; st < n_steps; ++st) {
        hipLaunchKernelGGL(tr_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, X, labels, idx + (long long)st * batch_size, n,
                           P, batch_size, w->xb, w->lab);
        if ((rc = gradient_step(h, w, p, w->xb, w->lab, batch_size, adv_eps, clip_min, clip_max, seed, w->t, losses ? losses + st : w->loss,
                                nullptr, s)))
            return rc;
        w->t += 1;
        if ((rc = reduce(h, w, p, batch_size, adv, nullptr, true, dg_tf_adam_lr(learning_rate, (double)w->t), s))) return rc;
    }
    return DG_OK;
}

}  // extern "C"
