// Library-internal view of a classifier handle (dg_clf.hip) for the training path (dg_clf_train.hip): the layer geometry and
// parameter pointers, and launchers of dg_clf.hip's own forward / input-gradient kernels, so that training reuses them unchanged.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/defensegan_hip.h"

struct TrainWork;

struct DgClfLayerView {
    int kind;                      // DG_LAYER_*
    int ih, iw, ic, oh, ow, oc;    // per-image input / output shapes (flat layers: h = w = 1)
    int kh, kw, sh, sw, pad_t, pad_l;
    int fused_relu;                // the following ReLU is applied in this layer's kernel
    int skip;                      // no kernel at evaluation (Flatten, Dropout, a folded ReLU)
    float keep_prob;               // Dropout: the reference's Dropout(prob) (0 = never set)
    float* W;                      // Conv2D kernels [kh,kw,ic,oc] / Linear W [ic,oc], device
    float* b;                      // bias [oc], device
};

extern "C" {
__attribute__((visibility("hidden"))) int dg_clf_layer_count(const dg_clf* h);
__attribute__((visibility("hidden"))) void dg_clf_layer_view(const dg_clf* h, int j, DgClfLayerView* v);
// device, pixels per image, whether every Conv2D / Linear layer has weights, and the training workspace slot
__attribute__((visibility("hidden"))) TrainWork** dg_clf_train_slot(dg_clf* h, int* device, int* P, int* have_weights);
// layer j's evaluation kernel (Conv2D / Linear with its fused ReLU, or an unfused ReLU): in [B, ih, iw, ic] -> out [B, oh, ow, oc]
__attribute__((visibility("hidden"))) void dg_clf_launch_forward(const dg_clf* h, int j, const float* in, float* out, int B, hipStream_t s);
// layer j's input gradient as dg_clf_input_gradient computes it: dx = d/din of sum(g * out), out = the layer's kept output
__attribute__((visibility("hidden"))) void dg_clf_launch_input_grad(const dg_clf* h, int j, const float* g, const float* out, float* dx, int B,
                                                                    hipStream_t s);
// dCE/dlogits with the label or (labels == NULL) the model's own first argmax, as dg_fgsm seeds its backward
__attribute__((visibility("hidden"))) void dg_clf_launch_ce_grad(const float* logits, const int32_t* labels, float* g, int B, int n, hipStream_t s);
// x_adv = clip(x + eps * sign(grad), lo, hi), dg_fgsm's last kernel
__attribute__((visibility("hidden"))) void dg_clf_launch_fgsm(const float* x, const float* grad, float* xadv, long long total, float eps, float lo,
                                                              float hi, hipStream_t s);
__attribute__((visibility("hidden"))) void dg_train_release(TrainWork* w);    // dg_clf_train.hip
}
