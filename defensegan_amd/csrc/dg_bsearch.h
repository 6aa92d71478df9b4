// The binary search over the loss constant that Carlini-Wagner (dg_cw.hip) and the elastic-net attack (dg_ead.hip) share, rule for
// rule (dg_cw.hip's header states them): the per-image and per-chunk state, its place in the workspace, the constant update after
// an outer step, the resets before one, the chunk's abort decision and best tracking, and what the two host loops have in common.
// Each attack adds its own planes, its iteration and the two expressions the chunk body takes.  Included by those two files only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dg_attack_device.h"
#include "dg_clf_internal.h"

#pragma GCC visibility push(hidden)

// An attack's workspace, one allocation that only grows; the handle keeps one per attack (h->cw, h->ead).
struct SearchWork {
    char* mem = nullptr;
    size_t bytes = 0;
};

// the handle's workspace `*w`, created on first use and grown to `need` bytes
inline int search_workspace(SearchWork** w, size_t need) {
    if (!*w) *w = new SearchWork();
    return clf_grow(&(*w)->mem, 1, (*w)->bytes, need);
}

// Hands out consecutive sub-buffers of an allocation, each 256-byte aligned; base == NULL only measures (off = the bytes needed).
struct SearchCarver {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t count) {
        char* p = base ? base + off : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return (T*)p;
    }
};

// what both attacks keep per image and per chunk
struct SearchBufs {
    float* seed;                                   // [N, n] dloss1/dlogits
    float *loss1, *best, *obest;                   // [N]: const * loss1; the step's and the call's best criterion
    double *cst, *lower, *upper;                   // [N]
    int32_t *lab, *score, *succ, *bestscore, *obestscore, *improved;   // [N]
    double* prev;                                  // [chunks]
    int32_t* abort_iter;                           // [chunks]: -1 running, else the iteration whose check stopped the chunk
};

inline void search_carve(SearchBufs* b, SearchCarver& c, long long N, long long n, long long chunks) {
    b->seed = c.take<float>((size_t)(N * n));
    for (float** p : {&b->loss1, &b->best, &b->obest}) *p = c.take<float>(N);
    for (double** p : {&b->cst, &b->lower, &b->upper}) *p = c.take<double>(N);
    for (int32_t** p : {&b->lab, &b->score, &b->succ, &b->bestscore, &b->obestscore, &b->improved}) *p = c.take<int32_t>(N);
    b->prev = c.take<double>(chunks);
    b->abort_iter = c.take<int32_t>(chunks);
}

// once per call and image: the label (the model's own first arg-max where none is given), the constants and the call's bests
__device__ __forceinline__ void search_setup(const SearchBufs& bf, long long b, const int32_t* labels, const float* logits, int n,
                                             double initial_const) {
    bf.lab[b] = labels ? labels[b] : clf_first_argmax(logits + b * n, n);
    bf.obest[b] = 1e10f;
    bf.obestscore[b] = -1;
    bf.cst[b] = initial_const;
    bf.lower[b] = 0.0;
    bf.upper[b] = 1e10;
}

// after an outer step: a step's best that counts as success lowers upper, anything else raises lower; const = their middle once
// upper has come down, else (failure only) const * 10
__device__ __forceinline__ void search_update_const(const SearchBufs& bf, long long b, int targeted) {
    const int bs = bf.bestscore[b], t = bf.lab[b];
    const double c = bf.cst[b];
    if (bs != -1 && (targeted ? bs == t : bs != t)) {
        bf.upper[b] = fmin(bf.upper[b], c);
        if (bf.upper[b] < 1e9) bf.cst[b] = (bf.lower[b] + bf.upper[b]) / 2;
    } else {
        bf.lower[b] = fmax(bf.lower[b], c);
        bf.cst[b] = bf.upper[b] < 1e9 ? (bf.lower[b] + bf.upper[b]) / 2 : c * 10;
    }
}

// before an outer step: the repeat rule, the step's bests and (the chunk's first image) the chunk's abort state
__device__ __forceinline__ void search_reset_scalars(const SearchBufs& bf, long long b, int batch_size, int repeat_last) {
    if (repeat_last) bf.cst[b] = bf.upper[b];
    bf.best[b] = 1e10f;
    bf.bestscore[b] = -1;
    if (b % batch_size == 0) {
        bf.prev[b / batch_size] = 1e6;
        bf.abort_iter[b / batch_size] = -1;
    }
}

// One workgroup of 256 threads per chunk: the chunk's loss L = the sum of term(b) over its images in index order (float64), the
// abort decision on check iterations, best tracking by crit(b), the "improved" flag per image.  Holds a barrier: all 256 threads
// call it.
template <class Term, class Crit>
__device__ __forceinline__ void search_chunk(const SearchBufs& bf, int N, int batch_size, int iter, int check, Term term, Crit crit) {
    __shared__ int abort_now, stopped;
    const int c = blockIdx.x;
    const int first = c * batch_size;
    const int cnt = N - first < batch_size ? N - first : batch_size;
    // thread 0 alone reads and writes the chunk's abort state; the others learn it after the barrier (a read of abort_iter by
    // another wave could otherwise see this iteration's write and skip the "improved" flags the update kernel still reads)
    if (threadIdx.x == 0) {
        stopped = bf.abort_iter[c] >= 0;
        abort_now = 0;
        if (!stopped && check) {
            double L = 0.0;
            for (int j = 0; j < cnt; ++j) L += term(first + j);
            if (L > bf.prev[c] * 0.9999) {
                bf.abort_iter[c] = iter;
                abort_now = 1;
            } else {
                bf.prev[c] = L;
            }
        }
    }
    __syncthreads();
    if (stopped) return;
    for (int j = threadIdx.x; j < cnt; j += 256) {
        const int b = first + j;
        int imp = 0;
        if (!abort_now && bf.succ[b]) {
            const float v = crit(b);
            if (v < bf.best[b]) {
                bf.best[b] = v;
                bf.bestscore[b] = bf.score[b];
            }
            if (v < bf.obest[b]) {
                bf.obest[b] = v;
                bf.obestscore[b] = bf.score[b];
                imp = 1;
            }
        }
        bf.improved[b] = imp;
    }
}

// ---- the host loops' common parts ---------------------------------------------------------------------------------------------------
// abort_early checks every `every` iterations
inline int search_every(int max_iterations) { return max_iterations / 10 > 0 ? max_iterations / 10 : 1; }
// the last of at least ten outer steps runs at const = upper ("repeat")
inline int search_repeat_last(int binary_search_steps, int step) { return (binary_search_steps >= 10 && step == binary_search_steps - 1) ? 1 : 0; }

// after outer step `step`: where each chunk stopped
inline int search_copy_chunk_stop(const SearchBufs& bf, int32_t* chunk_stop, int step, long long chunks, hipStream_t s) {
    if (chunk_stop)
        CLF_TRY(hipMemcpyAsync(chunk_stop + (long long)step * chunks, bf.abort_iter, chunks * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return DG_OK;
}

// the outputs after the last step (each may be NULL); the caller has enqueued the closing constant update where final_const is asked for
inline int search_copy_out(const SearchBufs& bf, long long N, double* final_const, float* best, int32_t* best_class, hipStream_t s) {
    CLF_TRY(hipGetLastError());
    if (final_const) CLF_TRY(hipMemcpyAsync(final_const, bf.cst, N * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (best) CLF_TRY(hipMemcpyAsync(best, bf.obest, N * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (best_class) CLF_TRY(hipMemcpyAsync(best_class, bf.obestscore, N * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return DG_OK;
}

#pragma GCC visibility pop
