// The derived weight layouts of the engine, written once as templates over the element type.  Every layout is a pure permutation
// (with zero padding in the tail packs) of a parameter in the reference's layout, so the same routine serves two callers:
//   float   dg_set_weights packs the VALUES on the host (dg_engine.cpp);
//   int32   run on the index array 0, 1, 2, ... it yields the GATHER MAP of the layout, destination element -> source element
//           (kPackPad = -1 where the layout pads), with which the generator's training step refreshes the layout on the device
//           after Adam has moved the weights (dg_gen_train.hip: dst[i] = map[i] < 0 ? 0 : src[map[i]]).
// A routine writes every destination element it owns exactly once or leaves it at `pad` (the caller pre-fills).  Plain C++: the
// host-only test program tests/support/pack_host_exec.cpp includes this header without the HIP runtime.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define DG_PACK_HD __host__ __device__
#else
#define DG_PACK_HD
#endif

namespace dg {

// float index inside a Linear pack (dg_linear.hip) of element e of the fragment (unit, wave, chunk c, k-step kk, lane): the weight of
// output column wave*32 + (lane & 31) of the unit at k = c*32 + (kk*2 + (lane >> 5))*4 + e
DG_PACK_HD inline long long lin_pack_index(int unit, int wave, int kch, int c, int kk, int lane, int e) {
    return ((((long long)(unit * 4 + wave) * kch + c) * 4 + kk) * 64 + lane) * 4 + e;
}

constexpr int kPackPad = -1;

// W [K][F] (reference Linear layout) -> W^T [F][K]
template <class T>
void pack_lin_transpose(const T* W, T* dst, int K, int F) {
    for (int d = 0; d < K; ++d)
        for (int f = 0; f < F; ++f) dst[(size_t)f * K + d] = W[(size_t)d * F + f];
}

// forward pack of dg_linear.hip: 128-feature column tiles of W^T, K / 32 chunks (needs F % 128 == 0, K % 32 == 0); K * F elements
template <class T>
void pack_lin_fwd(const T* W, T* dst, int K, int F) {
    const int kch = K / 32;
    for (int u = 0; u < F / 128; ++u)
        for (int w = 0; w < 4; ++w)
            for (int c = 0; c < kch; ++c)
                for (int kk = 0; kk < 4; ++kk)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int f = u * 128 + w * 32 + (lane & 31), k = c * 32 + (kk * 2 + (lane >> 5)) * 4 + e;
                            dst[(size_t)lin_pack_index(u, w, kch, c, kk, lane, e)] = W[(size_t)k * F + f];      // W^T[f][k]
                        }
}

// backward pack of dg_linear.hip: the nsplit K slices of W, all 128 latent columns each (needs K == 128, F % (nsplit * 32) == 0)
template <class T>
void pack_lin_bwd(const T* W, T* dst, int K, int F, int nsplit) {
    (void)K;
    const int ks = F / nsplit, kch = ks / 32;
    for (int s = 0; s < nsplit; ++s)
        for (int w = 0; w < 4; ++w)
            for (int c = 0; c < kch; ++c)
                for (int kk = 0; kk < 4; ++kk)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int d = w * 32 + (lane & 31), f = s * ks + c * 32 + (kk * 2 + (lane >> 5)) * 4 + e;
                            dst[(size_t)lin_pack_index(s, w, kch, c, kk, lane, e)] = W[(size_t)d * F + f];
                        }
}

// Deconv2D filters [25][cout][cin] (reference layout) -> [25][cin][cout], the operand of the backward-to-input GEMM
template <class T>
void pack_deconv_transpose(const T* F, T* dst, int cout, int cin) {
    for (int k = 0; k < 25; ++k)
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) dst[((size_t)k * cin + ci) * cout + co] = F[((size_t)k * cout + co) * cin + ci];
}

// forward filters in fragment order (dg_fgemm.hip): the slab of tap k keeps its float offset k * cout * cin; inside it
// [cout / 32][cin / 8][64 lanes][4]: lane = ((ci % 8) / 4) * 32 + co % 32, element ci % 4   (needs cout % 32 == 0, cin % 8 == 0)
template <class T>
void pack_deconv_frag(const T* F, T* dst, int cout, int cin) {
    const int kc8 = cin / 8;
    for (int k = 0; k < 25; ++k)
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                dst[(size_t)k * cout * cin + (((size_t)(co / 32) * kc8 + ci / 8) * 64 + ((ci % 8) / 4) * 32 + co % 32) * 4 + ci % 4] =
                    F[((size_t)k * cout + co) * cin + ci];
}

// tail forward GEMM: B fragments of v_mfma_f32_32x32x2_f32 in load order.  kappa = (kh*5+kw)*cout + co is the row of F (layout
// [25][cout][cin] == [kappa][c]); lane = (kappa & 31) + 32*half holds c = 8*kk + 4*half + e of kappa tile t.  Padded.
inline size_t tail_pack32_elems(int cout, int cin) { return (size_t)((25 * cout + 31) / 32) * (cin / 8) * 64 * 4; }
template <class T>
void pack_tail32(const T* F, T* dst, int cout, int cin) {
    const int nk = 25 * cout, nt = (nk + 31) / 32, kkn = cin / 8;
    for (int tt = 0; tt < nt; ++tt)
        for (int kk = 0; kk < kkn; ++kk)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int kappa = tt * 32 + (lane & 31), c = kk * 8 + (lane >> 5) * 4 + e;
                    if (kappa < nk) dst[(((size_t)tt * kkn + kk) * 64 + lane) * 4 + e] = F[(size_t)kappa * cin + c];
                }
}

// B fragments of v_mfma_f32_16x16x4_f32, one 16-column tile per filter row kh (cout == 3): column j = kw*3 + co (< 15) is
// kappa = 15*kh + j; lane = j + 16*g holds c = 16*kk + 4*g + e.  Padded.
inline size_t tail_pack16_elems(int cin) { return (size_t)5 * (cin / 16) * 64 * 4; }
template <class T>
void pack_tail16(const T* F, T* dst, int cin) {
    const int kk16 = cin / 16;
    for (int kh = 0; kh < 5; ++kh)
        for (int kk = 0; kk < kk16; ++kk)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int j = lane & 15, c = kk * 16 + (lane >> 4) * 4 + e;
                    if (j < 15) dst[(((size_t)kh * kk16 + kk) * 64 + lane) * 4 + e] = F[(size_t)(15 * kh + j) * cin + c];
                }
}

// the index array a packer is run on to obtain its gather map
inline std::vector<int32_t> pack_iota(size_t n) {
    std::vector<int32_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (int32_t)i;
    return v;
}

}  // namespace dg
