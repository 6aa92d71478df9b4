// What the generator's seeded backward (dg_gen_train.hip) shares with the latent-space attack (dg_latent.hip): the refusals, the
// scope that runs a call on the NHWC path, and the launchers of the two kernels that carry a dy given from OUTSIDE down to h3.
// Internal to the library: hidden visibility, nothing of it is exported.
#pragma once
#include "dg_engine.h"

#pragma GCC visibility push(hidden)
namespace dge {

// what the training entry points and the latent-space attack refuse, by name
int gen_check_trainable(const dg_handle* h, const char* who);
// dpre5 [n] = dy * y * (1 - y): the seed behind the sigmoid                                        (gen_seed_kernel)
void gen_launch_seed(const float* dy, const float* y, float* dpre5, long long n, hipStream_t s);
// da2 = ReluGrad(h3) o (dpre5 * F5), in place over h3 [N,14,14,C]; F5 [5,5,1,C]; total = N * 196 * C  (gen_tail_bwd_kernel)
void gen_launch_tail_bwd(float* h3, const float* dpre5, const float* F5, long long total, int C, hipStream_t s);

// The training forward and backward read and write the NHWC activation buffers: a handle on the fragment-order path (option
// frag_path) runs these calls on the NHWC path, with the job lists of that path, and returns to its own afterwards.
// This is NOT dg_set_option("frag_path"): the option frees the workspace and drops the job lists because the handle changes path
// for good; here both paths must stay usable side by side, so nothing is freed and the flag only selects, for the length of one call,
// which launches run_forward / run_backward make and which kind of list prepare_rows looks for.  Two consequences the caller of
// this scope (gen_call, dg_latent_attack) relies on and must keep:
//   * prepare_rows runs once BEFORE the scope, with the handle's own path.  Only that call may grow the workspace: grown inside
//     the scope it would come back without the fragment-order buffers (ensure_workspace sizes them by frag_path), and the
//     handle's next projection call would quietly leave its path.  Inside the scope the workspace is already large enough and
//     the second prepare_rows only adds the NHWC forward lists the fragment-order path never built.
//   * the backward layers' lists are shared by both paths.  On a frag_path handle they were TIMED with the gate-bit epilogue and
//     run here with the in-place mask: the choice among equally correct, bit-identical lists may then not be the fastest for
//     this epilogue.  Results do not depend on it (tests/test_gpu_gen_train.py, the frag_path case of the refresh test).
struct NhwcScope {
    dg_handle* h;
    int saved;
    explicit NhwcScope(dg_handle* h_) : h(h_), saved(h_->frag_path) { h->frag_path = 0; }
    ~NhwcScope() { h->frag_path = saved; }
};

}  // namespace dge
#pragma GCC visibility pop
