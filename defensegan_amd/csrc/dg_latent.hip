// The latent-space attack on the device (Athalye, Carlini, Wagner 2018, section 5: the attack that breaks Defense-GAN): search the
// generator's range for z such that G(z) is misclassified and close to x, by TF's Adam on z.  G(z) lies on the manifold, so the
// projection returns it almost unchanged.  Not in the reference; defined in DESIGN.md section 7 ("The latent-space attack") and
// pinned by tests/support/latent_reference.py.  R restarts per image, row j = i R + r belongs to image i.  For k = 0 .. nb_iter - 1,
// every row on its own:
//
//     y_j  = G(z_j)                                          the engine's forward (NHWC path), y stays in the engine's buffer
//     Z_j  = logits(y_j)                                     clf_kept_forward
//     m_j  = Z_j[label_i] - max_{c != label_i} Z_j[c]        the first maximum on ties, its index o_j        latent_margin_kernel
//     d_j  = mean over the pixels of (y_j - x_i)^2           one workgroup per row, a fixed tree             latent_dist_seed_kernel
//     f_j  = d_j + cweight max(m_j + kappa, 0)
//     dlogits_j = (+cweight at label_i, -cweight at o_j) if m_j + kappa > 0, else zero
//     dy_j = (the classifier's input gradient for dlogits_j: clf_seeded_backward, dg_clf_backward's bits) + 2 (y_j - x_i) / P,
//            written in place over that gradient
//     dz_j = the generator's backward seeded with dy_j       gen_seed_kernel, gen_tail_bwd_kernel (dg_gen_train.hip), the engine's
//            run_backward with no hook, the slice sum: what dg_gen_param_gradient returns as out_dz, without the weight gradients
//     z_j <- Adam(z_j, dz_j)                                 latent_adam_kernel; lr_t in float64 on the host, t = t_start + k + 1
//
// and, unless keep_state, one closing forward (k = nb_iter) so that the last iterate is judged too.  Every evaluated iterate goes
// through latent_track_kernel (one workgroup per image): a row succeeds when m_j < -kappa; the image keeps the successful (k, r) of
// the smallest d_j (ties: the earliest k, then the smallest r) and, while it has none, the smallest-margin row of the iterate just
// judged (smallest r on ties) with best_iter = -1 -- which the closing forward leaves as the final iterate's.  The winning row of y
// is copied into x_adv as the forward wrote it.  Non-finite values: a row whose margin is NaN is never a success and never the
// smallest margin; a successful row whose distance is NaN is never taken; if every margin of the iterate is NaN the no-success
// result is row 0; +inf compares as a number.  Refused: a call that would evaluate nothing (nb_iter = 0 with keep_state and
// t_start = 0: x_adv and best_* would stay unwritten), and t_start + nb_iter above INT32_MAX (best_iter is int32).
//
// No float atomics, every sum has a fixed order, nothing reads the device between the first and the last launch: two identical
// calls return identical bits, and an image's result does not depend on which other images share the call.  fp32; gfx950.
#include "dg_gen_internal.h"
#include "dg_clf_internal.h"

struct LatentWork {
    int64_t cap_rows = 0;          // rows the per-row buffers hold
    float* dpre5 = nullptr;        // [rows, P]
    float* dz = nullptr;           // [rows, latent]
    float* m = nullptr;            // [rows, latent]   the moments of a call that brings none
    float* v = nullptr;
    float* margin = nullptr;       // [rows]           the iterate in flight, when no trace is asked for
    float* dist = nullptr;         // [rows]
    float* seed = nullptr;         // [rows * classes] dlogits
    size_t seed_floats = 0;
    int64_t cap_images = 0;        // images the tracker state holds (outputs the caller left NULL)
    float* best_dist = nullptr;
    float* best_margin = nullptr;
    int32_t* best_iter = nullptr;
    int32_t* best_row = nullptr;
};

namespace {

// m_j, o_j and the hinge's seed; one thread per row.  A label outside [0, n) reads nothing: zero seed, margin +inf (never a success).
__global__ __launch_bounds__(256) void latent_margin_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, int N, int R,
                                                             int n, float cweight, float kappa, float* __restrict__ dlogits,
                                                             float* __restrict__ margin) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const float* Z = logits + (long long)j * n;
    float* g = dlogits + (long long)j * n;
    const int lab = labels[j / R];
    for (int c = 0; c < n; ++c) g[c] = 0.f;
    if (lab < 0 || lab >= n) { margin[j] = __builtin_inff(); return; }
    float best = -__builtin_inff();
    int o = -1;
    for (int c = 0; c < n; ++c) {
        if (c == lab) continue;
        const float zc = Z[c];
        if (o < 0 || zc > best) { best = zc; o = c; }       // strict ">" keeps the first maximum
    }
    const float mj = Z[lab] - best;
    margin[j] = mj;
    if (mj + kappa > 0.f) { g[lab] = cweight; g[o] = -cweight; }
}

// d_j and, with g given, dy_j = g_j + 2 (y_j - x_i) / P in place over g.  One workgroup per row; V = 4: float4 loads and stores (P a
// multiple of 4, every pointer 16-byte aligned), V = 1 otherwise.  The squared differences are summed per thread in index order,
// the 256 thread sums by one fixed tree.  HBM-bound: three reads and one write of 4 bytes per pixel.
template <int V>
__global__ __launch_bounds__(256) void latent_dist_seed_kernel(const float* __restrict__ y, const float* __restrict__ x, float* __restrict__ g,
                                                                int R, int P, float inv_p, float two_over_p, float* __restrict__ dist) {
    __shared__ float red[256];
    const int j = blockIdx.x, tid = threadIdx.x;
    const float* yr = y + (long long)j * P;
    const float* xr = x + (long long)(j / R) * P;
    float* gr = g ? g + (long long)j * P : nullptr;
    float acc = 0.f;
    if constexpr (V == 4) {
        for (int q = tid; q < (P >> 2); q += 256) {
            const float4 a = reinterpret_cast<const float4*>(yr)[q];
            const float4 b = reinterpret_cast<const float4*>(xr)[q];
            const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
            acc = fmaf(dx, dx, acc); acc = fmaf(dy, dy, acc); acc = fmaf(dz, dz, acc); acc = fmaf(dw, dw, acc);
            if (gr) {
                float4 t = reinterpret_cast<const float4*>(gr)[q];
                t.x = fmaf(dx, two_over_p, t.x); t.y = fmaf(dy, two_over_p, t.y); t.z = fmaf(dz, two_over_p, t.z); t.w = fmaf(dw, two_over_p, t.w);
                reinterpret_cast<float4*>(gr)[q] = t;
            }
        }
    } else {
        for (int i = tid; i < P; i += 256) {
            const float d = yr[i] - xr[i];
            acc = fmaf(d, d, acc);
            if (gr) gr[i] = fmaf(d, two_over_p, gr[i]);
        }
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) dist[j] = red[0] * inv_p;
}

// TF's Adam (epsilon 1e-8) on z, dg_critic_step's form: 1 - beta formed in float32, lr_t from the host
__device__ __forceinline__ void latent_adam1(float& z, float& m, float& v, float g, float lr_t, float b1, float b2) {
    m = b1 * m + (1.0f - b1) * g;
    v = b2 * v + (1.0f - b2) * (g * g);
    z = z - lr_t * m / (sqrtf(v) + 1e-8f);
}

template <int V>
__global__ __launch_bounds__(256) void latent_adam_kernel(float* __restrict__ z, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long long nvec, float lr_t, float b1, float b2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    if constexpr (V == 4) {
        float4 zz = reinterpret_cast<float4*>(z)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        latent_adam1(zz.x, mm.x, vv.x, gg.x, lr_t, b1, b2);
        latent_adam1(zz.y, mm.y, vv.y, gg.y, lr_t, b1, b2);
        latent_adam1(zz.z, mm.z, vv.z, gg.z, lr_t, b1, b2);
        latent_adam1(zz.w, mm.w, vv.w, gg.w, lr_t, b1, b2);
        reinterpret_cast<float4*>(z)[i] = zz;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    } else {
        float zz = z[i], mm = m[i], vv = v[i];
        latent_adam1(zz, mm, vv, g[i], lr_t, b1, b2);
        z[i] = zz; m[i] = mm; v[i] = vv;
    }
}

// The tracker, one workgroup per image over its R rows of the iterate `iter`.  Wave 0 finds the successful row of the smallest
// distance and the row of the smallest margin (both: the smallest r on ties; a NaN never wins), lane 0 decides, everybody copies.
// init: the image has no state yet (the first iterate of a fresh attack).
__global__ __launch_bounds__(256) void latent_track_kernel(const float* __restrict__ margin, const float* __restrict__ dist,
                                                            const float* __restrict__ y, int R, int P, float kappa, int iter, int init,
                                                            float* __restrict__ best_dist, float* __restrict__ best_margin,
                                                            int32_t* __restrict__ best_iter, int32_t* __restrict__ best_row,
                                                            float* __restrict__ x_adv, int vec4) {
    __shared__ int s_take;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float* mr = margin + (long long)b * R;
    const float* dr = dist + (long long)b * R;
    if (tid < 64) {
        const int none = 0x7fffffff;
        float sd = __builtin_inff(), fm = __builtin_inff();
        int sr = none, fr = none;
        for (int r = lane; r < R; r += 64) {
            const float mj = mr[r], dj = dr[r];
            if (mj < -kappa && (dj < sd || (dj == sd && r < sr))) { sd = dj; sr = r; }
            if (mj < fm || (mj == fm && r < fr)) { fm = mj; fr = r; }
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {
            const float osd = __shfl_xor(sd, w, 64), ofm = __shfl_xor(fm, w, 64);
            const int osr = __shfl_xor(sr, w, 64), ofr = __shfl_xor(fr, w, 64);
            if (osr != none && (sr == none || osd < sd || (osd == sd && osr < sr))) { sd = osd; sr = osr; }
            if (ofr != none && (fr == none || ofm < fm || (ofm == fm && ofr < fr))) { fm = ofm; fr = ofr; }
        }
        if (lane == 0) {
            const int prev_iter = init ? -1 : best_iter[b];
            int take = -1;
            if (sr != none) {
                if (prev_iter < 0 || sd < best_dist[b]) {           // strict "<": ties stay with the earlier iterate
                    take = sr;
                    best_dist[b] = sd; best_margin[b] = mr[sr]; best_iter[b] = iter; best_row[b] = sr;
                }
            } else if (prev_iter < 0) {
                take = fr == none ? 0 : fr;                         // (all-NaN margins: row 0)
                best_dist[b] = dr[take]; best_margin[b] = mr[take]; best_iter[b] = -1; best_row[b] = take;
            }
            s_take = take;
        }
    }
    __syncthreads();
    const int take = s_take;
    if (take < 0) return;
    const float* src = y + ((long long)b * R + take) * P;
    float* dst = x_adv + (long long)b * P;
    if (vec4) {
        for (int i = tid; i < (P >> 2); i += 256) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        for (int i = tid; i < P; i += 256) dst[i] = src[i];
    }
}

template <class T>
int regrow(T*& p, size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    HIP_TRY(hipMalloc(&p, n * sizeof(T)));
    return DG_OK;
}

// Workspace for calls of up to N rows of B images with n classes: blocking when something grows, nothing otherwise.
int latent_ensure(dg_handle* h, int N, int B, int n) {
    if (!h->latent_work) h->latent_work = new LatentWork();
    LatentWork* w = h->latent_work;
    int rc;
    if (N > w->cap_rows) {
        HIP_TRY(hipDeviceSynchronize());
        w->cap_rows = 0;
        if ((rc = regrow(w->dpre5, (size_t)N * h->P)) || (rc = regrow(w->dz, (size_t)N * h->latent)) || (rc = regrow(w->m, (size_t)N * h->latent)) ||
            (rc = regrow(w->v, (size_t)N * h->latent)) || (rc = regrow(w->margin, (size_t)N)) || (rc = regrow(w->dist, (size_t)N)))
            return rc;
        w->cap_rows = N;
    }
    if ((size_t)N * n > w->seed_floats) {
        HIP_TRY(hipDeviceSynchronize());
        w->seed_floats = 0;
        if ((rc = regrow(w->seed, (size_t)N * n))) return rc;
        w->seed_floats = (size_t)N * n;
    }
    if (B > w->cap_images) {
        HIP_TRY(hipDeviceSynchronize());
        w->cap_images = 0;
        if ((rc = regrow(w->best_dist, (size_t)B)) || (rc = regrow(w->best_margin, (size_t)B)) || (rc = regrow(w->best_iter, (size_t)B)) ||
            (rc = regrow(w->best_row, (size_t)B)))
            return rc;
        w->cap_images = B;
    }
    return DG_OK;
}

}  // namespace

#pragma GCC visibility push(hidden)
namespace dge {
void latent_release(dg_handle* h) {
    LatentWork* w = h->latent_work;
    if (!w) return;
    for (void* p : {(void*)w->dpre5, (void*)w->dz, (void*)w->m, (void*)w->v, (void*)w->margin, (void*)w->dist, (void*)w->seed,
                    (void*)w->best_dist, (void*)w->best_margin, (void*)w->best_iter, (void*)w->best_row})
        if (p) (void)hipFree(p);
    delete w;
    h->latent_work = nullptr;
}
}  // namespace dge
#pragma GCC visibility pop

extern "C" int dg_latent_attack(dg_handle* h, dg_clf* c, const float* x, const int32_t* labels, int B, int R, const float* z0, uint64_t seed,
                                int64_t first_row, int nb_iter, float lr, float beta1, float beta2, float cweight, float kappa, float* m, float* v,
                                int64_t t_start, int keep_state, float* x_adv, float* best_dist, float* best_margin, int32_t* best_iter,
                                int32_t* best_row, float* out_z, float* out_margin, float* out_dist, float* out_dz, void* stream) {
    const char* who = "dg_latent_attack";
    if (!h || !c) return fail(DG_E_INVALID, "%s: null handle", who);
    if (!x || !labels || !x_adv) return fail(DG_E_INVALID, "%s: x, labels and x_adv must be non-null", who);
    int rc = gen_check_trainable(h, who);
    if (rc) return rc;
    if (c->in_h != h->img_h || c->in_w != h->img_h || c->in_c != h->img_c)
        return fail(DG_E_INVALID, "%s: the classifier's input [%d,%d,%d] is not the generator's image [%d,%d,%d]", who, c->in_h, c->in_w, c->in_c,
                    h->img_h, h->img_h, h->img_c);
    if (c->device != h->device) return fail(DG_E_INVALID, "%s: the classifier (device %d) and the generator (device %d) are on different devices", who, c->device, h->device);
    if (c->logit_layer < 0) return fail(DG_E_STATE, "%s: the classifier has no layers", who);
    for (int j = 0; j <= c->logit_layer; ++j)
        if (c->layers[j].kind == DG_LAYER_DROPOUT)
            return fail(DG_E_INVALID, "%s: not implemented for a classifier with Dropout before the logits (layer %d)", who, j);
    const int n = c->n_logits;
    if (n < 2) return fail(DG_E_INVALID, "%s: the margin needs at least two classes (the classifier has %d)", who, n);
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f))
        return fail(DG_E_INVALID, "%s: betas (%g, %g) outside [0, 1)", who, (double)beta1, (double)beta2);
    if (nb_iter < 0 || t_start < 0) return fail(DG_E_INVALID, "%s: need nb_iter >= 0 and t_start >= 0 (got %d, %lld)", who, nb_iter, (long long)t_start);
    if (nb_iter == 0 && keep_state && t_start == 0)
        return fail(DG_E_INVALID, "%s: nb_iter = 0 with keep_state and t_start = 0 evaluates nothing: no iterate would be judged and x_adv and best_* would stay unwritten", who);
    // (the tracker's iterate number and best_iter are int32)
    if (t_start > (int64_t)INT32_MAX - nb_iter)
        return fail(DG_E_INVALID, "%s: t_start + nb_iter (%lld + %d) does not fit best_iter (int32)", who, (long long)t_start, nb_iter);
    if (!(kappa >= 0.f) || !(cweight >= 0.f) || !std::isfinite(lr))
        return fail(DG_E_INVALID, "%s: need kappa >= 0, cweight >= 0 and a finite learning rate", who);
    if ((m == nullptr) != (v == nullptr)) return fail(DG_E_INVALID, "%s: give both moments or neither", who);
    if (!m && t_start > 0) return fail(DG_E_INVALID, "%s: t_start > 0 continues an attack and needs its moments m and v", who);
    if (t_start > 0 && (!best_dist || !best_margin || !best_iter || !best_row))
        return fail(DG_E_INVALID, "%s: t_start > 0 continues an attack and needs its best_dist, best_margin, best_iter and best_row", who);
    if ((rc = check_ready(h))) return rc;
    const int missing = clf_missing_weights(c);
    if (missing >= 0) return fail(DG_E_STATE, "%s: classifier layer %d has no weights", who, missing);
    int N = 0;
    if ((rc = check_rows(B, R, &N))) return rc;
    // (the forward's tail compares every row with image 0 by R = N, exact below 2^20 rows: dg_generate's limit)
    if (N > (1 << 20)) return fail(DG_E_INVALID, "%s: at most %d rows per call (got B*R = %d): split the batch", who, 1 << 20, N);
    if (h->latent % 32 || h->lin_out % 64) return fail(DG_E_INVALID, "%s: unsupported layer widths", who);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    // workspace and job lists: blocking on the first call of a row count, nothing afterwards (the order gen_call keeps, see NhwcScope)
    if ((rc = prepare_rows(h, N, &N, 1, s))) return rc;
    NhwcScope nhwc(h);
    if ((rc = prepare_rows(h, N, &N, 1, s))) return rc;
    if ((rc = latent_ensure(h, N, B, n))) return rc;
    LatentWork* w = h->latent_work;
    const bool prof = h->prof_stride > 0;
    h->prof_chain_last = -1;
    const int P = h->P, nd = (int)h->dec.size(), C5 = h->dec[nd - 1].cin;
    const size_t zbytes = (size_t)N * h->latent * sizeof(float);
    if (z0) HIP_TRY(hipMemcpyAsync(h->z, z0, zbytes, hipMemcpyDeviceToDevice, s));
    else dg::launch_init_latents(h->z, N, h->latent, seed, first_row, std::sqrt(1.0f / (float)h->latent), s);
    if (!m) {
        m = w->m; v = w->v;
        HIP_TRY(hipMemsetAsync(m, 0, zbytes, s));
        HIP_TRY(hipMemsetAsync(v, 0, zbytes, s));
    }
    if (!best_dist) best_dist = w->best_dist;
    if (!best_margin) best_margin = w->best_margin;
    if (!best_iter) best_iter = w->best_iter;
    if (!best_row) best_row = w->best_row;
    if ((rc = clear_pair_counters(h, N, s))) return rc;
    RowGroup grp; grp.n_rows = N; grp.s = s;
    const float inv_p = 1.0f / (float)P, two_over_p = 2.0f / (float)P;
    const bool adam4 = clf_aligned16(h->z) && clf_aligned16(w->dz) && clf_aligned16(m) && clf_aligned16(v) && h->latent % 4 == 0;
    const int evals = keep_state ? nb_iter : nb_iter + 1;
    for (int k = 0; k < evals; ++k) {
        // (every row is compared with one all-zero image, as in dg_generate: the engine's loss is not read)
        if ((rc = run_forward(h, h->xzero, grp, /*R=*/N, /*want_y=*/true, /*want_loss=*/false, /*tail_backward=*/false, prof))) return rc;
        if ((rc = clf_kept_forward(c, h->y, N, s))) return rc;
        float* mk = out_margin ? out_margin + (size_t)k * N : w->margin;
        float* dk = out_dist ? out_dist + (size_t)k * N : w->dist;
        {
            ProfScope ps(h, s, prof, "LAT@latent_margin_kernel", 0.0);
            hipLaunchKernelGGL(latent_margin_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, c->acts[c->logit_layer], labels, N, R,
                               n, cweight, kappa, w->seed, mk);
        }
        float* gy = nullptr;
        if (k < nb_iter && (rc = clf_seeded_backward(c, w->seed, N, s, &gy))) return rc;
        {
            ProfScope ps(h, s, prof, "LAT@latent_dist_seed_kernel", 0.0);
            if (P % 4 == 0 && clf_aligned16(h->y) && clf_aligned16(x) && clf_aligned16(gy))
                hipLaunchKernelGGL(latent_dist_seed_kernel<4>, dim3((unsigned)N), dim3(256), 0, s, h->y, x, gy, R, P, inv_p, two_over_p, dk);
            else
                hipLaunchKernelGGL(latent_dist_seed_kernel<1>, dim3((unsigned)N), dim3(256), 0, s, h->y, x, gy, R, P, inv_p, two_over_p, dk);
        }
        {
            ProfScope ps(h, s, prof, "LAT@latent_track_kernel", 0.0);
            const int vec4 = P % 4 == 0 && clf_aligned16(h->y) && clf_aligned16(x_adv);
            hipLaunchKernelGGL(latent_track_kernel, dim3((unsigned)B), dim3(256), 0, s, mk, dk, h->y, R, P, kappa, (int)(t_start + k),
                               (t_start == 0 && k == 0) ? 1 : 0, best_dist, best_margin, best_iter, best_row, x_adv, vec4);
        }
        if ((rc = launch_check("the latent attack's margin, distance and tracker"))) return rc;
        if (k == nb_iter) break;
        // the generator's backward seeded with dy (dg_gen_train.hip's chain without the weight gradients)
        float* h3 = h->act[nd - 1];
        {
            ProfScope ps(h, s, prof, "G5seed@gen_seed_kernel", 0.0);
            gen_launch_seed(gy, h->y, w->dpre5, (long long)N * P, s);
        }
        {
            ProfScope ps(h, s, prof, "B5@gen_tail_bwd_kernel", 2.0 * 67.0 * 67.0 * C5 * N);
            gen_launch_tail_bwd(h3, w->dpre5, h->F[nd - 1], (long long)N * 196 * C5, C5, s);
        }
        if ((rc = launch_check("the seeded backward of Generator.5"))) return rc;
        if ((rc = run_backward(h, grp, prof))) return rc;
        dg::launch_momentum_update(nullptr, nullptr, h->part, h->nsplit, N, h->latent, 0.f, 0.f, w->dz, s);
        const double t = (double)(t_start + k + 1);
        const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t)));
        const long long elems = (long long)N * h->latent;
        ProfScope ps(h, s, prof, "LAT@latent_adam_kernel", 0.0);
        if (adam4)
            hipLaunchKernelGGL(latent_adam_kernel<4>, dim3((unsigned)((elems / 4 + 255) / 256)), dim3(256), 0, s, h->z, w->dz, m, v, elems / 4, lr_t,
                               beta1, beta2);
        else
            hipLaunchKernelGGL(latent_adam_kernel<1>, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, h->z, w->dz, m, v, elems, lr_t, beta1,
                               beta2);
    }
    if (out_z) HIP_TRY(hipMemcpyAsync(out_z, h->z, zbytes, hipMemcpyDeviceToDevice, s));
    if (out_dz && nb_iter > 0) HIP_TRY(hipMemcpyAsync(out_dz, w->dz, zbytes, hipMemcpyDeviceToDevice, s));
    return launch_check(who);
}
