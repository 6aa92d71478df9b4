// Device arithmetic that more than one source file uses, written once so that the users cannot drift apart: the Philox4x32-10
// block (latent init in dg_small.hip, Dropout in dg_clf_train.hip) and TF's Adam (dg_cw.hip, dg_clf_train.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

// one Philox4x32 round on the counter c with the round key (k0, k1)
__device__ __forceinline__ void dg_philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// Philox4x32-10: ten rounds on the counter c with the key (k0, k1), the key bumped by the Weyl constants after each; c holds
// the four output words afterwards
__device__ __forceinline__ void dg_philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        dg_philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// One element of tf.train.AdamOptimizer (beta1 0.9, beta2 0.999, epsilon 1e-8): updates the moments m and v with the gradient g
// and returns what the parameter decreases by, lr_t * m / (sqrt(v) + epsilon), lr_t from dg_tf_adam_lr
__device__ __forceinline__ float dg_tf_adam_step(float& m, float& v, float g, float lr_t) {
    const float mm = 0.9f * m + 0.1f * g;
    const float vv = 0.999f * v + 0.001f * (g * g);
    m = mm;
    v = vv;
    return lr_t * mm / (sqrtf(vv) + 1e-8f);
}

// lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) of Adam step t (counted from 1), in float64 as TF computes it
inline float dg_tf_adam_lr(float lr, double t) {
    return (float)((double)lr * std::sqrt(1.0 - std::pow(0.999, t)) / (1.0 - std::pow(0.9, t)));
}
