// The device arithmetic the attack kernels share, each rule written once so that its users cannot drift apart: the fixed-order
// sums, the row vector, the first arg-max (by one wave and by one thread) and Carlini-Wagner's hinge.  Included by dg_ball.hip,
// dg_critic.hip, dg_cw.hip, dg_deepfool.hip, dg_ead.hip, dg_jsma.hip, dg_pgd.hip and dg_clf.hip.  Nothing but __device__ __forceinline__
// functions: no state, no kernels, no launch geometry.  The bits of every function here are pinned by the CPU references under
// tests/support/; changing an order of operations changes results.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

// ---- fixed-order sums -------------------------------------------------------------------------------------------------------------
// The sum of `v` over the 64 lanes of a wave by an xor butterfly, the same bits in every lane.
__device__ __forceinline__ float clf_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The sum of `v` over the 256 threads of a workgroup, the same bits in every thread: the wave sums, then the four waves left to
// right.  `red` is 4 floats of LDS; the trailing barrier frees it for the next reduction.  Holds two barriers: all 256 threads call
// it, on a path that is uniform over the workgroup.
__device__ __forceinline__ float clf_block_sum(float v, float* red) {
    v = clf_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

// ---- V floats at vector index i of a row (V = 4: one float4, the row 16-byte aligned and a multiple of 4 long) ----------------------
template <int V> struct ClfVec;
template <> struct ClfVec<1> {
    float e[1];
    __device__ __forceinline__ static ClfVec load(const float* p, long long i) { return {{p[i]}}; }
    __device__ __forceinline__ void store(float* p, long long i) const { p[i] = e[0]; }
};
template <> struct ClfVec<4> {
    float e[4];
    __device__ __forceinline__ static ClfVec load(const float* p, long long i) {
        const float4 q = reinterpret_cast<const float4*>(p)[i];
        return {{q.x, q.y, q.z, q.w}};
    }
    __device__ __forceinline__ void store(float* p, long long i) const { reinterpret_cast<float4*>(p)[i] = make_float4(e[0], e[1], e[2], e[3]); }
};

// ---- the first arg-max by one wave ------------------------------------------------------------------------------------------------
// (best, arg) takes over the other lane's (ob, oa) where that is the larger value or, of equal values, the smaller class.
// arg == INT_MAX: the lane holds no candidate.
__device__ __forceinline__ void clf_argmax_merge(float& best, int& arg, float ob, int oa) {
    if (oa != INT_MAX && (arg == INT_MAX || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
}

// The first arg-max among the classes c of r[0 .. n) for which cand(r[c], c) holds, the classes strided over the 64 lanes, the same
// answer in every lane: each lane keeps the first maximum of its candidates, a butterfly merges them.  INT_MAX when there is no
// candidate.  `best` comes in as the value a lane without a candidate carries (it is never compared) and goes out as the maximum.
template <class Cand>
__device__ __forceinline__ int clf_wave_argmax_if(const float* r, int n, int lane, float& best, Cand cand) {
    int arg = INT_MAX;
    for (int c = lane; c < n; c += 64) {
        const float v = r[c];
        if (cand(v, c) && (arg == INT_MAX || v > best)) { best = v; arg = c; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oa = __shfl_xor(arg, m, 64);
        clf_argmax_merge(best, arg, ob, oa);
    }
    return arg;
}

// The first arg-max of r[0 .. n), a NaN never a candidate; INT_MAX when nothing is left.  *nan: whether the row holds a NaN.
__device__ __forceinline__ int clf_wave_argmax(const float* r, int n, int lane, bool* nan) {
    float best = -__builtin_inff();
    int bad = 0;
    const int arg = clf_wave_argmax_if(r, n, lane, best, [&](float v, int) {
        if (v != v) bad = 1;
        return v == v;
    });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad |= __shfl_xor(bad, m, 64);
    *nan = bad != 0;
    return arg;
}

// The class a row is given, dg_eval_batch's first arg-max: a NaN is never a candidate, and class 0 where class 0 is a NaN or nothing
// is left (clf_eval_kernel's scan, best = 0 and s[k] > s[best] moves it, ends there too).  Uniform over the wave.
__device__ __forceinline__ int clf_wave_class(const float* r, int n, int lane) {
    float best = -__builtin_inff();
    const int arg = clf_wave_argmax_if(r, n, lane, best, [](float v, int) { return v == v; });
    return (r[0] != r[0] || arg == INT_MAX) ? 0 : arg;
}

// ---- the first arg-max by one thread ----------------------------------------------------------------------------------------------
__device__ __forceinline__ int clf_first_argmax(const float* z, int n) {
    int best = 0;
    for (int k = 1; k < n; ++k)
        if (z[k] > z[best]) best = k;
    return best;
}

// ---- Carlini-Wagner's hinge on the logits z[0 .. n) for a label t in [0, n) (dg_cw.hip's header has the rules; dg_ead.hip shares them) ----
// The hinge's argument real - oth + kappa (targeted: oth - real + kappa), real = z[t], oth = max_k of z with the label's entry
// masked to -10000; *oth_out = oth.
__device__ __forceinline__ float cw_hinge_arg(const float* z, int n, int t, int targeted, float kappa, float* oth_out) {
    float oth = -3.402823466e38f;
    for (int k = 0; k < n; ++k) {
        const float o = k == t ? -10000.0f : z[k];
        oth = o > oth ? o : oth;
    }
    *oth_out = oth;
    return targeted ? (oth - z[t] + kappa) : (z[t] - oth + kappa);
}

// sd[0 .. n) = c * d max(0, arg)/dz: zero unless arg > 0 (a tie with the constant 0 and a NaN give no gradient); otherwise the
// label's entry +-c and the max's share split evenly over its maximisers, the label's own entry taking none of it.
__device__ __forceinline__ void cw_hinge_seed(float* sd, const float* z, int n, int t, int targeted, float c, float arg, float oth) {
    for (int k = 0; k < n; ++k) sd[k] = 0.f;
    if (!(arg > 0.f)) return;
    int cnt = 0;
    for (int k = 0; k < n; ++k) cnt += ((k == t ? -10000.0f : z[k]) == oth) ? 1 : 0;
    const float sgn = targeted ? -1.0f : 1.0f;
    const float share = (1.0f / (float)cnt) * (-sgn * c);
    for (int k = 0; k < n; ++k)
        if (k != t && z[k] == oth) sd[k] = share;
    sd[t] = sgn * c;
}

// Success on Z' = z with the label's entry moved by kappa (+ kappa, targeted: - kappa): the first arg-max of Z' is not the label
// (targeted: is the label).
__device__ __forceinline__ int cw_success(const float* z, int n, int t, int targeted, float kappa) {
    int am = 0;
    float best = t == 0 ? (targeted ? z[0] - kappa : z[0] + kappa) : z[0];
    for (int k = 1; k < n; ++k) {
        const float zk = k == t ? (targeted ? z[k] - kappa : z[k] + kappa) : z[k];
        if (zk > best) { best = zk; am = k; }
    }
    return targeted ? (am == t) : (am != t);
}
