// The Jacobian side of Papernot's substitute attack (the reference's blackbox.py:143-213; cleverhans' jacobian_graph and
// jacobian_augmentation, an empty, un-pinned submodule there, restated):
//
//     jacobian_graph(preds_sub, x, nb_classes)    grads[k] = d model_sub(x)[:, k] / dx, k < nb_classes
//     jacobian_augmentation(X, Y, grads, lmbda)   X_new[i] = X[i] + lmbda * sign(grads[Y[i]](X[i])),  returns vstack([X, X_new])
//
// model_sub(x) is MLP.__call__, the PROBABILITIES, so for a model that ends in Softmax the class gradient is that of
// softmax(logits)[c], neither the logit's nor the cross-entropy's.  TF's softmax gradient for the one-hot upstream on class c is
//
//     dz_k = (delta_kc - p_c) * p_k
//
// and that form is computed here, in float32: once p_c rounds to 1, dz_c is exactly 0 and dz_k = -p_k, exactly 0 as well as soon
// as exp(z_k - z_c) underflows; the new image then equals the old one, as in the reference.  For a model without Softmax the
// output is the logits and the seed is the one-hot vector.  The new point is not clipped.
//
// Everything after the seed is the classifier's own chain (dg_clf_internal.h): clf_kept_forward, clf_seeded_backward and, for the
// step, clf_launch_fgsm with infinite bounds.  Each output element of those kernels is one thread's fixed-order sum, so a result
// does not depend on how many images share the launch: the Jacobian's slice k is the class gradient of classes == k, and the
// augmentation does not depend on its chunk size, bit for bit.  No float atomics, no host synchronisation.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dg_clf_internal.h"

struct JacWork {
    float* seed = nullptr;          // [B, n] d out[b, class] / d logits
    size_t seed_floats = 0;
};

void jac_release(JacWork* w) {
    if (!w) return;
    if (w->seed) (void)hipFree(w->seed);
    delete w;
}

namespace {

// seed[b, :] = d out[b, c] / d logits[b, :], c = classes[b] (or `fixed` for every image when classes == nullptr).  One wave per
// image, the classes strided over its lanes.  of_probs: out = softmax(logits), seed_k = (delta_kc - p_c) * p_k with the maximum
// subtracted before exp; otherwise out = logits, seed = onehot(c).  c outside [0, n): a zero seed, nothing is read at c.
__global__ __launch_bounds__(64) void jac_seed_kernel(const float* __restrict__ logits, const int32_t* __restrict__ classes, int fixed,
                                                       float* __restrict__ seed, int n, int of_probs) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int c = classes ? classes[b] : fixed;
    const bool valid = c >= 0 && c < n;
    const float* r = logits + (long long)b * n;
    float* g = seed + (long long)b * n;
    if (!of_probs || !valid) {                                   // uniform over the wave
        for (int k = lane; k < n; k += 64) g[k] = (valid && k == c) ? 1.0f : 0.0f;
        return;
    }
    float m = -INFINITY;
    for (int k = lane; k < n; k += 64) m = fmaxf(m, r[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    float s = 0.f;
    for (int k = lane; k < n; k += 64) s += expf(r[k] - m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);   // a + b == b + a: every lane ends with the same bits
    const float inv = 1.0f / s;
    const float pc = expf(r[c] - m) * inv;
    for (int k = lane; k < n; k += 64) g[k] = ((k == c ? 1.0f : 0.0f) - pc) * (expf(r[k] - m) * inv);
}

// jac[b, k, :] = g[b, :]: image b's gradient [P] to its slice of [B, n, P]
__global__ __launch_bounds__(256) void jac_store_kernel(const float* __restrict__ g, float* __restrict__ jac, long long total, int P,
                                                         int n, int k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / P;
    jac[(b * n + k) * P + (i - b * P)] = g[i];
}

int jac_work(dg_clf* h, int B) {
    if (!h->jac) h->jac = new JacWork();
    return clf_grow(&h->jac->seed, 1, h->jac->seed_floats, (size_t)B * h->n_logits);
}

// After clf_kept_forward of the same B images: *grad = d out[b, class_b] / dx in h->gbuf.
int jac_class_backward(dg_clf* h, const int32_t* classes, int fixed, int B, int of_probs, hipStream_t s, float** grad) {
    hipLaunchKernelGGL(jac_seed_kernel, dim3(B), dim3(64), 0, s, h->acts[h->logit_layer], classes, fixed, h->jac->seed, h->n_logits,
                       (of_probs && h->has_softmax) ? 1 : 0);
    CLF_TRY(hipGetLastError());                                            // the seed's launch, for all three entries
    return clf_seeded_backward(h, h->jac->seed, B, s, grad);
}

}  // namespace

extern "C" {

int dg_clf_class_gradient(dg_clf* h, const float* x, const int32_t* classes, int B, int of_probs, float* grad, void* stream) {
    if (!h || !x || !classes || !grad || B <= 0) return clf_fail(DG_E_INVALID, "dg_clf_class_gradient: bad argument");
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    float* g = nullptr;
    int rc = clf_kept_forward(h, x, B, s);
    if (rc || (rc = jac_work(h, B)) || (rc = jac_class_backward(h, classes, 0, B, of_probs, s, &g))) return rc;
    CLF_TRY(hipMemcpyAsync(grad, g, (size_t)B * h->pixels() * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DG_OK;
}

int dg_clf_jacobian(dg_clf* h, const float* x, int B, int of_probs, float* jac, void* stream) {
    if (!h || !x || !jac || B <= 0) return clf_fail(DG_E_INVALID, "dg_clf_jacobian: bad argument");
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = clf_kept_forward(h, x, B, s);
    if (rc || (rc = jac_work(h, B))) return rc;
    const long long total = (long long)B * h->pixels();
    for (int k = 0; k < h->n_logits; ++k) {
        float* g = nullptr;
        if ((rc = jac_class_backward(h, nullptr, k, B, of_probs, s, &g))) return rc;
        hipLaunchKernelGGL(jac_store_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, jac, total, h->pixels(),
                           h->n_logits, k);
    }
    CLF_TRY(hipGetLastError());
    return DG_OK;
}

int dg_jacobian_augment(dg_clf* h, const float* X, const int32_t* labels, int n, float lmbda, int batch_size, float* X_out,
                        void* stream) {
    if (!h || !X || !labels || !X_out || n <= 0 || batch_size <= 0) return clf_fail(DG_E_INVALID, "dg_jacobian_augment: bad argument");
    const size_t P = (size_t)h->pixels();
    if (X_out != X && X_out < X + (size_t)n * P && X < X_out + 2 * (size_t)n * P)
        return clf_fail(DG_E_INVALID, "dg_jacobian_augment: X_out overlaps X (pass X_out == X for the in-place form)");
    CLF_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (X_out != X) CLF_TRY(hipMemcpyAsync(X_out, X, (size_t)n * P * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int c0 = 0; c0 < n; c0 += batch_size) {
        const int Bc = n - c0 < batch_size ? n - c0 : batch_size;          // the last chunk is partial, not shifted back
        const float* xc = X + (size_t)c0 * P;
        float* g = nullptr;
        int rc = clf_kept_forward(h, xc, Bc, s);
        if (rc || (rc = jac_work(h, Bc)) || (rc = jac_class_backward(h, labels + c0, 0, Bc, 1, s, &g))) return rc;
        clf_launch_fgsm(xc, g, X_out + ((size_t)n + c0) * P, (long long)Bc * (long long)P, lmbda, -INFINITY, INFINITY, s);
        CLF_TRY(hipGetLastError());
    }
    return DG_OK;
}

}  // extern "C"
