// The classifier handle as its source files see it.  Included by: dg_clf.hip (the layers, the evaluation and input-gradient kernels),
// dg_clf_train.hip (training), dg_jacobian.hip (class gradients, Jacobian augmentation), dg_bpda.hip (the BPDA/EOT step), dg_pgd.hip
// (PGD on the bare classifier), dg_ball.hip (the per-image norms and steps of the L1 / L2 attacks), dg_spsa.hip (SPSA), dg_latent.hip
// (the latent-space attack), dg_critic.hip (the WGAN-GP critic's cost, gradient and step), dg_deepfool.hip (the DeepFool loop), dg_jsma.hip (the saliency-map
// attack) and,
// through dg_bsearch.h, dg_cw.hip (the Carlini-Wagner attack) and dg_ead.hip (the elastic-net attack).  Everything here is internal
// to the library: plain C++ under hidden visibility, nothing of it is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/defensegan_hip.h"

extern "C" __attribute__((visibility("hidden"))) void dg_set_error_message(const char* msg);   // dg_engine.cpp (dg_last_error storage)

#pragma GCC visibility push(hidden)

// One layer; its kind is a DG_LAYER_* of the public header.
struct ClfLayer {
    int kind = 0;
    // conv
    int kh = 0, kw = 0, sh = 1, sw = 1, same = 0, cin = 0, cout = 0, pad_t = 0, pad_l = 0;
    // shapes (per image; flat layers: h = w = 1)
    int ih = 0, iw = 0, ic = 0, oh = 0, ow = 0, oc = 0;
    bool fused_relu = false;     // the ReLU that follows is applied in this layer's kernel
    bool skip = false;           // no kernel at evaluation: a ReLU folded into its predecessor / identity layers
    float* W = nullptr;          // Conv2D kernels [kh,kw,cin,cout] / Linear W [cin,cout], device
    float* b = nullptr;          // bias [cout], device
    bool have_w = false;
    float keep_prob = 0.f;       // Dropout: the reference's Dropout(prob), used by the training phase only (0 = never set)

    bool has_params() const { return kind == DG_LAYER_CONV2D || kind == DG_LAYER_LINEAR; }
    long long features() const { return (long long)oh * ow * oc; }
};

struct SearchWork;   // dg_bsearch.h: the workspace of dg_cw.hip and of dg_ead.hip
struct TrainWork;    // dg_clf_train.hip
struct JacWork;      // dg_jacobian.hip
struct BpdaWork;     // dg_bpda.hip
struct PgdWork;      // dg_pgd.hip
struct CriticWork;   // dg_critic.hip
struct DeepfoolWork; // dg_deepfool.hip
struct JsmaWork;     // dg_jsma.hip

struct dg_clf {
    int device = 0;
    int in_h = 0, in_w = 0, in_c = 0;
    std::vector<ClfLayer> layers;
    int cur_h = 0, cur_w = 0, cur_c = 0;      // running shape while layers are added (flat: h = w = 1, c = width)
    bool flat = false;
    // the logits are the output of the last layer that runs a kernel other than Softmax ("logits" = layers[-2] when the model
    // ends in Softmax, network_builder.py:148-153); kept up to date as layers are added
    int logit_layer = -1;
    int n_logits = 0;
    bool has_softmax = false;
    float* buf[2] = {nullptr, nullptr};
    size_t buf_floats = 0;
    float* scores = nullptr;                  // [B, n_out] scratch of dg_eval_batch
    size_t scores_floats = 0;
    std::vector<float*> acts;                 // per-layer outputs kept by the gradient path
    std::vector<size_t> acts_floats;
    float* gbuf[2] = {nullptr, nullptr};      // gradient ping-pong
    size_t gbuf_floats = 0;
    SearchWork* cw = nullptr;                 // Carlini-Wagner workspace, grown on demand
    TrainWork* tr = nullptr;                  // training workspace and Adam state
    JacWork* jac = nullptr;                   // class-gradient seed, grown on demand
    BpdaWork* bpda = nullptr;                 // BPDA's cross-entropy seed, grown on demand
    PgdWork* pgd = nullptr;                   // PGD's seed and its two iterate buffers, grown on demand
    CriticWork* critic = nullptr;             // the WGAN-GP critic's three-batch workspace, grown on demand
    DeepfoolWork* deepfool = nullptr;         // DeepFool's candidates, seeds, iterate rows and per-image state, grown on demand
    SearchWork* ead = nullptr;               // the elastic-net attack's slack / iterate rows and per-image state, grown on demand
    JsmaWork* jsma = nullptr;                 // the saliency-map attack's doubled iterate rows, seeds, domain and per-image state, grown on demand

    int pixels() const { return in_h * in_w * in_c; }
};

// ---- errors ---------------------------------------------------------------------------------------------------------------------
int clf_fail(int code, const char* fmt, ...);      // sets dg_last_error's message, returns code

#define CLF_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return clf_fail(DG_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));        \
    } while (0)

// Device buffers that only grow: when `need` elements exceed the capacity `cap` that the n buffers p[0..n) share, each is freed
// and allocated anew with exactly `need` elements.
template <class T>
int clf_grow(T** p, int n, size_t& cap, size_t need) {
    if (need <= cap) return DG_OK;
    cap = 0;
    for (int i = 0; i < n; ++i) {
        if (p[i]) (void)hipFree(p[i]);
        p[i] = nullptr;
        CLF_TRY(hipMalloc(&p[i], need * sizeof(T)));
    }
    cap = need;
    return DG_OK;
}

// ---- dg_clf.hip -----------------------------------------------------------------------------------------------------------------
int clf_missing_weights(const dg_clf* h);          // the first Conv2D / Linear layer without weights, or -1
// layer j's evaluation kernel (Conv2D / Linear with its fused ReLU, or an unfused ReLU): in [B, ih, iw, ic] -> out [B, oh, ow, oc]
void clf_launch_forward(const dg_clf* h, int j, const float* in, float* out, int B, hipStream_t s);
// layer j's Conv2D / Linear map alone: its bias replaced by zero_bias [cout] and no fused ReLU (the critic's tangent pass)
void clf_launch_linear_part(const dg_clf* h, int j, const float* in, const float* zero_bias, float* out, int B, hipStream_t s);
// layer j's input gradient: dx = d/din of sum(g * out), out = the layer's kept output
void clf_launch_input_grad(const dg_clf* h, int j, const float* g, const float* out, float* dx, int B, hipStream_t s);
// dCE/dlogits with the label or (labels == NULL) the model's own first argmax
void clf_launch_ce_grad(const float* logits, const int32_t* labels, float* g, int B, int n, hipStream_t s);
// x_adv = clip(x + eps * sign(grad), lo, hi)
void clf_launch_fgsm(const float* x, const float* grad, float* xadv, long long total, float eps, float lo, float hi, hipStream_t s);
// Forward of x [B, ...] keeping every layer's output in h->acts; the logits are h->acts[h->logit_layer] until the next forward.
int clf_kept_forward(dg_clf* h, const float* x, int B, hipStream_t s);
// dLoss/dx from the seed dLoss/dlogits [B, n] after clf_kept_forward of the same B images; *grad lies in h->gbuf, never in seed.
int clf_seeded_backward(dg_clf* h, const float* seed, int B, hipStream_t s, float** grad);

void search_release(SearchWork* w); // dg_cw.hip, for h->cw and h->ead
void train_release(TrainWork* w);    // dg_clf_train.hip
void jac_release(JacWork* w);        // dg_jacobian.hip
void bpda_release(BpdaWork* w);      // dg_bpda.hip
void pgd_release(PgdWork* w);        // dg_pgd.hip
void critic_release(CriticWork* w);  // dg_critic.hip
void deepfool_release(DeepfoolWork* w);   // dg_deepfool.hip
void jsma_release(JsmaWork* w);      // dg_jsma.hip

// ---- dg_clf_train.hip -------------------------------------------------------------------------------------------------------------
// How a Conv2D / Linear layer's weight gradient over B images is cut: `slots` runs of kc terms of its reduction axis, each slot
// leaving `per` = (M + 1) * N partial sums of (dW; db).  The same B always gives the same plan.
struct ClfWgradPlan {
    int slots = 0, kc = 0;
    size_t per = 0;
};
ClfWgradPlan train_wgrad_plan(const ClfLayer& v, int B);
// part [slots, per] = the partial sums of layer v's (dW; db) for its inputs x [B, ...] and output gradients g [B, features], g masked
// by out > 0 where the layer's ReLU is fused.  bias_row false: the db row is left zero (a term that carries no bias gradient).
void train_launch_wgrad(const ClfLayer& v, const float* x, const float* g, const float* out, int B, const ClfWgradPlan& p, float* part,
                        bool bias_row, hipStream_t s);
// The handle's Adam state, created (zero, t = 0) on first use: per layer index the moments [(W; b)] of a Conv2D / Linear layer,
// and the step count.  Fetch them per call: adding a layer moves them.
int train_adam_state(dg_clf* h, float*** m, float*** v, long long** t);

// ---- shared by the attack steps (dg_bpda.hip, dg_ball.hip, dg_spsa.hip, dg_deepfool.hip, dg_ead.hip, dg_jsma.hip; dg_attack_device.h has the reductions) ----
// the final clip of every attack step: clip(v, lo, hi) with lo <= hi
__device__ __forceinline__ float clf_clip(float v, float lo, float hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}
// the projected sign step of one element: clip(xo + clamp(xc + eps_iter sign(g) - xo, -eps, eps), lo, hi), sign(0) = sign(NaN) = 0
__device__ __forceinline__ float clf_sign_step(float g, float xc, float xo, float eps, float eps_iter, float lo, float hi) {
    const float sgn = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);
    float d = (xc + eps_iter * sgn) - xo;
    d = d < -eps ? -eps : (d > eps ? eps : d);
    return clf_clip(xo + d, lo, hi);
}
// whether float4 may be used on p (NULL counts as aligned: an absent operand)
inline bool clf_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- dg_bpda.hip ----------------------------------------------------------------------------------------------------------------
// The projected sign step over `total` elements (rows of row_elems): accumulate_only: gsum += g; otherwise t = gsum + g (t = g when
// gsum == NULL) and x_next = clip(x_orig + clamp(x_cur + eps_iter sign(t) - x_orig, -eps, eps), lo, hi).  float4 where row_elems is
// a multiple of 4 and every pointer given is 16-byte aligned.
int clf_launch_bpda_step(const float* g, float* gsum, const float* x_cur, const float* x_orig, float* x_next, long long total,
                         int row_elems, int accumulate_only, float eps, float eps_iter, float lo, float hi, hipStream_t s);

// ---- dg_ball.hip ----------------------------------------------------------------------------------------------------------------
// One workgroup per image; float4 where row_elems is a multiple of 4 and every pointer given is 16-byte aligned.  ord is 1 or 2.
// out[b] = the ord-norm of row b of v - w (of v when w == NULL)
int clf_launch_row_norms(const float* v, const float* w, int B, long long row_elems, int ord, float* out, hipStream_t s);
// out = clip(x + eps * g / max(1e-12, ||g||_ord), lo, hi), the norm per image
int clf_launch_fgm_norm_step(const float* x, const float* g, float* out, int B, int row_elems, int ord, float eps, float lo, float hi,
                             hipStream_t s);
// The L2 step: t = gsum + g (t = g when gsum == NULL), d = (x_cur + eps_iter * t / max(1e-12, ||t||)) - x_orig,
// x_next = clip(x_orig + d * min(1, eps / max(1e-12, ||d||)), lo, hi); the norms per image.
int clf_launch_ball_step(const float* g, const float* gsum, const float* x_cur, const float* x_orig, float* x_next, int B, int row_elems,
                         float eps, float eps_iter, float lo, float hi, hipStream_t s);

#pragma GCC visibility pop
