/*
 * defensegan_hip.h -- C ABI of the MI355X-native Defense-GAN latent-projection engine.
 *
 * The reference has NO FFI for this path: the boundary is a Python method on a TF-graph-owning
 * object,
 *     DefenseGANBase.reconstruct(self, images, batch_size=None, back_prop=True,
 *                                reconstructor_id=0, z_init_val=None)
 *                                              /root/reference/models/gan.py:333-449
 * configured by attributes rec_iters / rec_rr / rec_lr / latent_dim / net_dim / use_bn / image_dim
 *                                              /root/reference/models/gan.py:41-68
 * with weights arriving through load_generator()   /root/reference/models/gan.py:80-87.
 * These entry points are what a ctypes binding of that method binds instead of building the
 * tf.while_loop graph (INTEGRATION.md shows the stub).  Plain pointers and sizes only; every tensor
 * argument of the compute calls is a DEVICE pointer (HIP), caller-owned, fp32 unless stated, in the
 * reference's layouts (NHWC images, Linear W[in,out], Deconv2D filters [5,5,Cout,Cin]).
 *
 * All functions return 0 on success, a negative DG_E_* code otherwise; dg_last_error() returns a
 * thread-local message.  A handle is bound to one device and is not thread-safe.
 */
#ifndef DEFENSEGAN_HIP_H
#define DEFENSEGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_ABI_VERSION 2

/* architectures: /root/reference/models/dataset_models.py:36-71 (mnist, f-mnist), :127-165 (celeba) */
#define DG_ARCH_MNIST28 0
#define DG_ARCH_CELEBA64 1

#define DG_OK 0
#define DG_E_INVALID (-1)      /* bad argument / unsupported configuration            */
#define DG_E_STATE (-2)        /* weights missing, handle destroyed ...               */
#define DG_E_HIP (-3)          /* a HIP runtime call failed (message has the detail)  */
#define DG_E_NOMEM (-4)

typedef struct dg_handle dg_handle;

int dg_version(void);
const char* dg_last_error(void);

/* number of HIP devices visible; <0 on error (no driver / no GPU). */
int dg_device_count(void);

/* Fills name (<= name_len bytes, NUL-terminated), CU count and HBM bytes of `device`. */
int dg_device_info(int device, char* name, int name_len, int* cu_count, int64_t* hbm_bytes);

/*
 * Replaces GAN(cfg).generator_fn construction (gan.py:657-665 mnist, :726-735 celeba).
 * latent_dim: LATENT_DIM (default.yml:4), net_dim: NET_DIM (default.yml:7), use_bn: USE_BN (default.yml:3).
 * Constraints of this build: latent_dim % 64 == 0, net_dim % 64 == 0.
 */
int dg_create(int arch, int latent_dim, int net_dim, int use_bn, int device, dg_handle** out);
int dg_destroy(dg_handle* h);

/*
 * Replaces load_generator() / tf.train.Saver restore of the `Generator*` variables
 * (gan.py:80-87, base_model.py:294-335).  `name` is the tflib parameter name
 * (tflib/__init__.py:9-33): "Generator.Input.W" [latent, 4*4*4*net_dim], "Generator.Input.b",
 * "Generator.{2,3,5,6}.Filters" [5,5,Cout,Cin], "Generator.N.Biases",
 * "Generator.BN{1,2,3}.{scale,offset}".  `data` holds prod(shape) fp32 values; is_device != 0 means
 * a device pointer on the handle's device, else host memory.  The engine keeps its own copy.
 */
int dg_set_weights(dg_handle* h, const char* name, const float* data, const int64_t* shape,
                   int ndim, int is_device);

/* 1 when every weight the configuration needs has been set. */
int dg_weights_complete(dg_handle* h);

/*
 * The hot path: R restarts x L momentum-GD steps on sum_j mean_pix (G(z_j) - x_j)^2, then the
 * per-image first-argmin over restarts -- DefenseGANBase.reconstruct, gan.py:333-449.
 *
 *   x        [B, H, W, C]  images already in generator range ([0,1] mnist, [-1,1] celeba; gan.py:684-685, 764-765)
 *   z0       [B*R, latent] initial latents, row j = b*R + r (gan.py:348-359), or NULL: rows are then drawn
 *            N(0, 1/latent) (gan.py:370-375) from a counter-based generator keyed by (seed, first_row + j),
 *            i.e. independent of how the image list is batched or sharded over GPUs
 *   L        rec_iters: L forwards, L-1 applied updates; L = 0 and L = 1 both return G(z0) (gan.py:409-437)
 *   lr       rec_lr, constant over the loop (the reference's decay never fires, gan.py:362-386)
 *   momentum 0.7 in the reference (gan.py:390), non-Nesterov, slots zero-initialised
 *   out_rec  [B, H, W, C]  G(z_{L-1}) of the selected restart
 *   out_idx  [B] int32     selected restart r*(b) in [0,R)  (first minimum, gan.py:438-445)   (may be NULL)
 *   out_loss [B*R]         image_rec_loss of every restart at step L-1                        (may be NULL)
 *   out_z    [B*R, latent] z_{L-1}                                                            (may be NULL)
 *   stream   hipStream_t (NULL = default stream).  Once the call shape (B, R) has been prepared -- by dg_prepare or by an
 *            earlier call of the same shape -- the call only enqueues kernels and copies on `stream`: it neither allocates
 *            device memory nor waits for the device, and may be recorded by a stream capture.  The FIRST call of a new shape
 *            prepares itself and therefore BLOCKS (see dg_prepare); under a stream capture it fails with DG_E_STATE instead.
 *
 * Stateless per call (fresh z / momentum each batch = model_eval_gan's behaviour,
 * /root/reference/utils/gan_defense.py:119); any B >= 1 is accepted (ragged last batch).
 */
int dg_reconstruct(dg_handle* h, const float* x, const float* z0, uint64_t seed, int64_t first_row,
                   int B, int R, int L, float lr, float momentum,
                   float* out_rec, int32_t* out_idx, float* out_loss, float* out_z, void* stream);

/*
 * Prepares calls of B images x R restarts (no reference counterpart: the reference builds its static graph for exactly
 * batch_size * rec_rr rows at this point, gan.py:345-377): sizes the workspace for B*R latent rows and builds the job list of
 * every GEMM layer for this shape -- with "jobs.tune" (default) by timing the candidate lists on the device, ~0.1-0.3 s.
 * Blocking: allocates, launches timing runs on `stream` and waits for them.  Afterwards dg_reconstruct / dg_loss_grad with
 * this (B, R) and dg_generate with N = B*R are asynchronous in the strict sense documented at dg_reconstruct.  Shapes stay
 * prepared until an option that changes the lists is set (at most 16 row counts are kept per layer, oldest dropped first).
 * Results never depend on which list was chosen (tiles are only cut along M / N): preparing is about latency only.
 * A handle serves ONE stream at a time: dg_prepare (and the self-preparation of a call with a new shape) waits for the
 * device and then times launches on the handle's own activation buffers -- work of the same handle still queued on another
 * stream is waited for, not overlapped.
 */
int dg_prepare(dg_handle* h, int B, int R, void* stream);
/* Number of row groups a dg_reconstruct call of B images x R restarts runs as (1, or option "two_streams" when the call is large
 * enough -- with "auto" the timed choice of this shape, which exists once the shape has been prepared or called; 1 before that:
 * the groups are whole images, run concurrently on the engine's own streams forked from / joined to the caller's, and the
 * results do not depend on the split); -1 on an invalid shape (dg_last_error). */
int dg_call_row_groups(dg_handle* h, int B, int R);

/* G(z): z [N, latent] -> y [N, H, W, C], N <= 2^20 rows per call.  (generator_fn(z, is_training=False), gan.py:399) */
int dg_generate(dg_handle* h, const float* z, int N, float* out_y, void* stream);

/*
 * One forward + backward-to-z at fixed z (the body of the loop without the update, gan.py:409-417):
 * x [B,H,W,C], z [B*R, latent] -> out_y [B*R,H,W,C] (may be NULL), out_loss [B*R] (may be NULL),
 * out_dz [B*R, latent] = d(sum_j loss_j)/dz (may be NULL).
 */
int dg_loss_grad(dg_handle* h, const float* x, const float* z, int B, int R,
                 float* out_y, float* out_loss, float* out_dz, void* stream);

/*
 * The job list a GEMM layer runs with for a row count is chosen by timing candidates on first use (dg_prepare), so two
 * processes can settle on different -- equally correct, bit-identical in their results -- lists.  dg_export_tuning writes the
 * choices made so far as text (one line per layer and row count: starting level, cutting threshold, order variant) into
 * buf and returns the bytes needed including the terminating NUL (call with buf = NULL to size); dg_import_tuning rebuilds
 * exactly those lists in another handle of the same configuration without timing and returns the number of lists installed
 * (>= 0) or a negative DG_E_* code.  Use: the ranks of a multi-GPU run import rank 0's text; a profiler pass imports the
 * bench's (defensegan_amd/gan.py: export_tuning / import_tuning / the DG_TUNING_CACHE file).
 */
int64_t dg_export_tuning(dg_handle* h, char* buf, int64_t cap);
int dg_import_tuning(dg_handle* h, const char* text);

/* Fills z [n_rows, latent] with the same N(0, std^2) draw dg_reconstruct uses for z0 == NULL
 * (std <= 0 selects sqrt(1/latent)). */
int dg_init_latents(dg_handle* h, float* z, int64_t n_rows, uint64_t seed, int64_t first_row,
                    float std, void* stream);

/*
 * Measurement hooks (bench.py's roofline leg).  When enabled, every dg_reconstruct brackets each
 * kernel family with hipEvents on the launch stream; dg_profile_read returns, for family `i`
 * (0 <= i < count), its name, number of launches and total milliseconds since the last reset.
 */
int dg_profile_enable(dg_handle* h, int on);
int dg_profile_count(dg_handle* h);
int dg_profile_read(dg_handle* h, int i, char* name, int name_len, int64_t* launches, double* total_ms,
                    double* flops);
int dg_profile_reset(dg_handle* h);

/* Copies an internal activation buffer of the last forward ("h1","h2","h3","h5" ...) to `dst`
 * (device pointer, capacity n floats); returns the number of floats copied.  Test hook only.
 * Names: "z", "m", "loss", "y", "part", "act<d>" (activation buffer d; after a backward pass it holds that layer's gradient), and
 * "raw<d>" (the NHWC buffer of activation d as it stands: with the option frag_path "act<d>" always returns the forward activation,
 * converted from fragment order, and the gradient a backward pass left is read through "raw<d>"), "gate<d>" (frag_path only: the
 * ReluGrad gate words of activation d, [rows][floats per row / 32] unsigned words viewed as floats, bit f % 32 of word f / 32 =
 * activation f > 0), "frag_launches" (one float: launches of the fragment-order GEMM this handle has made), and
 * with use_bn, for the Batchnorm layer behind activation d:
 *   "bnpre<d>"  the pre-activations the producing GEMM left ([rows][floats per row of act<d>])
 *   "bnf<d>"    [2][bn_C] forward statistics: mean, rstd = 1 / sqrt(biased variance + 1e-5)
 *   "bnb<d>"    [2][bn_C] backward statistics of the last backward pass: mean(dy), mean(dy * xhat) */
int64_t dg_debug_read(dg_handle* h, const char* what, float* dst, int64_t n);

/*
 * Tuning / measurement overrides (no reference counterpart; defaults are the measured optimum on MI355X):
 *   "jobs.tune"        1 (default): on first use of a row count every GEMM layer times its candidate job lists on the real
 *                      operands and keeps the fastest; 0: the cost model's simulated makespan decides
 *   "jobs.slack"       > 0 fixes the cutting threshold of the job lists (dg_plan.h build_jobs; 1e30 = whole tiles only)
 *   "jobs.min_level"   >= 0 forces every list to start cut to halves (1) / quarters (2)
 *   "jobs.xcd_head"    fraction (default 0 = off; measured, no gain) of a list that is ALSO offered to the timing in XCD-locality order: every
 *                      XCD gets the jobs of one contiguous range of latent rows, all tap classes of a row range next to each other
 *                      in time, so that their shared input rows stay in that XCD's L2 (a permutation of the list)
 *   "jobs.balance"     1 (default): layers that fit ONE dispatch round are also offered to the timing as lists whose jobs are placed
 *                      -- and, where the round has room, cut -- so that every CU carries the same predicted work (dg_plan.h
 *                      balance_order, jobs_balanced; +2.2 % at the reference's 500 rows, profiles/r05_ab_list_orders.txt)
 *   "jobs.pair_kernel" the kernel has an instantiation with and one without the K-pair hand-off code; lists without pairs can run on
 *                      either (same arithmetic, another register allocation): 1 (default) the two fastest lists are timed on both
 *                      and the faster form is kept (+0.3 % on the MNIST loop, profiles/r05_ab_pair_kernel.txt), 0 never, 2 always
 *   "jobs.prio"        wave priorities by predicted job length (s_setprio per job): 0 (default) never, 1 the fastest lists are timed
 *                      again with them, 2 always.  Measured: the launches last the same (profiles/r05_ab_prio.txt)
 *   "jobs.spread"      1: the first dispatch round of a multi-round list mixes all job lengths (dg_plan.h spread_order).  Default 0:
 *                      slower on every layer (profiles/r05_ab_list_orders.txt)
 *   "bn_fused"         with use_bn, where the Batchnorm sums come from.  1: the forward statistics are per-32-row-block column sums taken
 *                      in the producing GEMM's epilogue; 2 (default): so are the backward sums (of dy and dy * xhat) of the layers
 *                      normalised over rows x positions, taken in the epilogue of the GEMM that writes dy (which re-forms the ReLU gate
 *                      and xhat from the layer's pre-activations), and inside the projection loop the MNIST tail takes its Batchnorm form
 *                      (it reads the last Batchnorm layer's pre-activations, applies relu(bn(.)) itself and leaves that layer's backward
 *                      sums: the layer's activation image is not written in those steps -- dg_debug_read("act2") then returns the image
 *                      of the last launch that did write it); 0: separate passes (float64 sums from the first add)
 *   "jobs.slots0/1", "jobs.rate0..2", "jobs.fixed_us"   cost-model parameters
 *   "lr_schedule"      "constant" (default): lr == rec_lr at every step, which is what the reference executes -- the step variable
 *                      of its decay is never advanced (gan.py:362-386, 416-417); "intended": the schedule its code asks for,
 *                      tf.train.exponential_decay(rec_lr, k, ceil(0.8 * rec_iters), 0.1, staircase=True) (base_model.py:186-192)
 *   "nsplit"           split-K factor of the Linear backward (default 16)
 *   "two_streams"      number of concurrent row groups (0 = off, 2..8) of calls with at least "two_stream_min_rows" (1024) latent
 *                      rows, or "auto": two groups for the call shapes where that is faster -- timed once per (B, R) when the shape
 *                      is prepared (nine loop steps of each form, three times; kept when >= 1 % faster).  Default "auto" for CelebA
 *                      (+2-3 % at 1280 rows: its gather-bound tails run beside the other group's GEMMs; -4.5 % at 5120), 0 for
 *                      MNIST (-0.9 %).  Results are bit-identical either way (rows are independent).  "two_stream_split": two
 *                      groups, percent of the images in the first (default halves; unequal halves measured slower).  While the
 *                      per-launch profile is on (dg_profile_enable) the groups run one after the other on the caller's stream
 *   "latent_turn"      1 (default): Linear backward / forward on the weight-stationary kernels (dg_linear.hip) where the shapes
 *                      allow; 0: on the position-batched kernel like every other layer.  "lin_groups_fwd" / "lin_groups_bwd":
 *                      their workgroups per column tile / K slice (0 = from the CU count)
 *   "update_fold"      1: the momentum update rides in the Linear backward launch -- the workgroup that delivers the last K slice
 *                      of a 32-row block sums the slices (write-through partials, one arrival counter per block) and applies the
 *                      update; needs latent_turn, latent 128, nsplit a multiple of 8.  Bit-identical to the separate kernel and
 *                      1.6 % SLOWER on the MNIST loop (the reducer of a row group becomes the last arriver of every later block of
 *                      the group: profiles/r04_ab_update_fold.txt).  Default 0
 *   "turn_fused"       1: the whole latent turn -- Linear backward, momentum update and the NEXT step's Linear forward -- is ONE launch
 *                      (dg_turn.hip): the nsplit workgroups of a row group meet at two barriers of their own (write-through partials
 *                      and latents, one monotonic arrival counter per barrier, cleared at the start of every call).  Needs
 *                      latent_turn, latent 128, K slices of 256 features, no Batchnorm, frag_path 0.  Bit-identical to the three
 *                      launches and AT PARITY with them (MNIST -0.5 ... +0.2 %, -1.5 % beside CelebA's second row group: the seam
 *                      inside the launch costs what the two kernel boundaries did, profiles/r06_ab_turn_fused.txt).  A barrier poll
 *                      that does not end within ~0.5 s gives up (the next dg_reconstruct on the handle fails with DG_E_HIP) instead
 *                      of hanging the device.  Residency is guaranteed for the row groups of ONE call (two workgroups fit a CU, the
 *                      engine sizes the launches of concurrent row groups for that); do not run more than two handles with this
 *                      option at once on one device.  Default 0
 *   "graph_max_rows"   > 0: call shapes of at most this many latent rows replay a captured hipGraph of the L-step loop instead of
 *                      enqueuing its launches one by one (built on the first call with a new (B, R, L, lr, momentum); never while
 *                      the caller's stream is itself capturing).  Default 0 = always enqueue: measured no gain at the reference's
 *                      default batch (500 rows: 780 vs 779 img/s), and on ROCm 7.2 a graph the CALLER captured of a call on the same
 *                      handle replays wrongly after an internal replay ran in between (tools/graph_interplay_repro.py) -- do not
 *                      combine the two on one handle
 *   "frag_path"        1: the FORWARD deconvs run on the LDS-free fragment-order kernel (dg_fgemm.hip: both operands in MFMA fragment
 *                      order, fetched straight into registers; the Linear forward writes fragment order, the backward GEMMs take
 *                      their ReluGrad gates from one bit per element).  Agrees with the default path to float32 rounding (another
 *                      fixed summation tree per tap class: a tile's K axis is split over 1 / 2 / 4 waves), rows stay independent of
 *                      their batch.  Default 0: its loop is faster in isolation (147-149 vs 137-142 TFLOP/s) but the path is 2-10 %
 *                      SLOWER at 1280 ... 12 500 rows (profiles/r06_frag_path_ab.txt).  Not with use_bn or two_streams
 *   "debug.poison_pair_counters"   test hook: leaves every K-pair arrival counter of every prepared job list at `value` -- the state a
 *                      launch that died between a pair's two arrivals would leave.  Every call clears the counters of the lists it
 *                      launches, so the next call must not care (tests/test_gpu_variants.py)
 *   "tail_pipe"        MNIST tail: workgroups of the pipelined kernel (0 = fused per-row kernel)
 *   "tail_fwd_split"   CelebA forward tail (NET_DIM 64): workgroups of the role-split persistent kernel (default 512 = two per CU);
 *                      0 = the per-band kernel (celeba_tail_fwd16_kernel; same y and da6 bit for bit, the per-row loss to rounding)
 *   "tail_bwd_persist" CelebA backward tail: workgroups of the persistent kernel
 * Only in the measurement build of the library (same sources with -DDG_MEASURE -> libdefensegan_hip_measure.so; the product
 * library refuses them): "tail_pipe_version" = 2 (second-generation MNIST tail), "tail_fwd16" = 0 (32x32x2 CelebA forward tail), "tail_bwd_persist" = 0 + "tail_bwd_bands" (per-band
 * backward tail), "tail_trace", "tail_dbg", "tail_prio", "job_trace" (in-kernel phase traces and phase-removal switches, tools/)
 * Every job-list / launch-shape option leaves the results bit-identical (tests/test_gpu_variants.py): GEMM tiles are only
 * ever cut along M and N; along K only the classes of >= 80 K chunks, and those ALWAYS, in two fixed halves whose sums are added
 * once (K-pair jobs, dg_plan.h kPairMinChunks: a + b = b + a, so the arrival order does not show); "nsplit", "tail_fwd16" and
 * "bn_fused" and "frag_path" change a summation order (agreement to rounding).
 */
int dg_set_option(dg_handle* h, const char* key, const char* value);

/* =====================================================================================================
 * The step after the projection: classifier forward + the per-batch reduction of
 * model_eval_gan.  Replaces, for evaluation, `model(reconstructed_tensors)` over the cleverhans-style MLP
 * of /root/reference/utils/network_builder.py:129-331 (models A-F, :333-521) and the `acc_value / cur_preds /
 * diff_op` fetches of /root/reference/utils/gan_defense.py:91-179, /root/reference/blackbox.py:569-572.
 * ===================================================================================================== */
typedef struct dg_clf dg_clf;

#define DG_LAYER_CONV2D 0     /* p0..p5 = output_channels, kernel h, kernel w, stride h, stride w, 1 = "SAME" / 0 = "VALID" */
#define DG_LAYER_RELU 1
#define DG_LAYER_LINEAR 2     /* p0 = num_hid                                                                    */
#define DG_LAYER_FLATTEN 3
#define DG_LAYER_SOFTMAX 4
#define DG_LAYER_DROPOUT 5    /* identity: K.learning_phase() is 0 at evaluation (network_builder.py:296-297);    *
                               * active in training (dg_clf_set_dropout)                                          */
#define DG_LAYER_LEAKY_RELU 6 /* max(0.2 x, x), the critic's activation (models/dataset_models.py:10-11); the slope is   *
                               * fixed; its gradient is 1 for x > 0 and 0.2 for x <= 0 (TF's MaximumGrad at the tie)      */

/* An empty MLP for NHWC inputs [*, in_h, in_w, in_c] (network_builder.py:129-162). */
int dg_clf_create(int device, int in_h, int in_w, int in_c, dg_clf** out);
int dg_clf_destroy(dg_clf* h);
/* Appends a layer; returns its index (>= 0) or a negative DG_E_* code.  Shapes follow tf.nn.conv2d's SAME / VALID
 * rules (SAME: out = ceil(in / stride), pad_before = pad_total / 2). */
int dg_clf_add_layer(dg_clf* h, int kind, int p0, int p1, int p2, int p3, int p4, int p5);
/* Width of the last layer's output per image (the class count once the model is complete). */
int dg_clf_output_width(dg_clf* h);
/* Parameters of a Conv2D (kernels [kh,kw,cin,cout], network_builder.py:213-221) or Linear (W [in,out], :196-203) layer
 * and its bias; host or device pointers. */
int dg_clf_set_weights(dg_clf* h, int layer, const float* W, const int64_t* wshape, int wndim, const float* b,
                       int64_t blen, int is_device);
/* x [B,in_h,in_w,in_c] -> logits [B,n] (the layer before Softmax, may be NULL) and probs [B,n] (may be NULL; equals the
 * logits when the model has no Softmax).  Device pointers; asynchronous on `stream`. */
int dg_clf_forward(dg_clf* h, const float* x, int B, float* logits, float* probs, void* stream);
/* One evaluation batch: preds[b] = argmax_k model(rec)[b,k] (first maximum), *n_correct += #(preds == labels) (device
 * int32, caller zeroes it), diffs[b] = mean((orig[b] - rec[b])^2).  labels/preds/diffs/n_correct/orig may be NULL. */
int dg_eval_batch(dg_clf* h, const float* rec, const float* orig, const int32_t* labels, int B, int32_t* preds,
                  float* diffs, int32_t* n_correct, void* stream);

/*
 * The step before the path: the FGSM inputs of /root/reference/whitebox.py:198-210 and
 * /root/reference/blackbox.py:521-534 (cleverhans FastGradientMethod, ord = inf; cleverhans itself is an un-pinned,
 * empty submodule of the reference, its published fgm is restated):
 *     x_adv = clip(x + eps * sign(d CE(softmax(logits(x)), y) / dx), clip_min, clip_max)
 * y = labels, or the model's own prediction when labels == NULL (cleverhans' default, avoids label leaking).
 */
int dg_clf_input_gradient(dg_clf* h, const float* x, const int32_t* labels, int B, float* grad, void* stream);
int dg_fgsm(dg_clf* h, const float* x, const int32_t* labels, int B, float eps, float clip_min, float clip_max,
            float* x_adv, void* stream);
/* grad [B,in_h,in_w,in_c] = d(sum_{b,k} dlogits[b,k] * logits(x)[b,k]) / dx for an arbitrary seed dlogits [B,n]: the backward
 * chain of dg_clf_input_gradient (whose seed is dCE/dlogits) from any loss on the logits.  Device pointers; asynchronous. */
int dg_clf_backward(dg_clf* h, const float* x, const float* dlogits, int B, float* grad, void* stream);

/*
 * The third white-box attack (/root/reference/whitebox.py:192-210, --attack_type cw; whitebox.py:201-209 sets
 * binary_search_steps = 1, max_iterations = 100, learning_rate = 10, initial_const = 100, batch_size = BATCH_SIZE and no clip
 * bounds, so [0, 1] also for CelebA): cleverhans' CarliniWagnerL2, restated (defensegan_amd/csrc/dg_cw.hip's header comment
 * and DESIGN.md section 7 give the algorithm).  x [B,in_h,in_w,in_c]; labels [B] int32 = y, or y_target when `targeted`, or NULL
 * for the model's own first argmax on x.  The B images run in chunks of batch_size (a trailing partial chunk is a chunk of its
 * own) that share the abort-early decision and nothing else.  Out: x_adv [B,...] = the best successful newimg over all steps,
 * clip(x) where none succeeded; best_l2 [B] (1e10 when none) and best_class [B] int32 (-1 when none); final_const [B] float64,
 * the constants after the last step's binary-search update (initial_const is float64, as are the constants: cleverhans
 * keeps them in NumPy float64); chunk_stop [binary_search_steps, ceil(B / batch_size)] int32, the
 * iteration at whose check each chunk stopped in each outer step (-1: ran to max_iterations).  Every output but x_adv may be NULL.
 * Device pointers; the whole attack is enqueued on `stream` with no host synchronisation and no graph capture.  A chunk that
 * stopped early skips the attack's own kernels, but the classifier's forward and backward still run over all B images every
 * iteration: abort_early changes the result, not the duration.  The workspace (about 6 x B x pixels floats) lives in the handle
 * and grows on demand.
 */
int dg_cw(dg_clf* h, const float* x, const int32_t* labels, int B, int targeted, int batch_size, float confidence,
          float learning_rate, int binary_search_steps, int max_iterations, int abort_early, double initial_const,
          float clip_min, float clip_max, float* x_adv, float* best_l2, int32_t* best_class, double* final_const,
          int32_t* chunk_stop, void* stream);

/*
 * Classifier training (the reference's whitebox.py:120-170 and blackbox.py's prep_bbox: cleverhans utils_tf.model_train with Adam,
 * `--defense_type adv_tr` adding FGSM inputs of the current model, whitebox.py:147-163; cleverhans is an empty, un-pinned submodule,
 * its published model_train / model_loss is restated in defensegan_amd/csrc/dg_clf_train.hip's header comment and DESIGN.md
 * section 7).  Replaces the TF graph of model_train: the training-phase forward (K.learning_phase() = 1, Dropout active), the
 * softmax cross-entropy on the logits, tf.gradients over every Conv2D / Linear parameter and AdamOptimizer.minimize.  The
 * evaluation forward stays dg_clf_forward.  All pointers are device pointers unless `is_device` says otherwise; every call is
 * asynchronous on `stream` and the workspace grows on demand in the handle.
 */
/* The training phase of a Dropout layer: the reference's Dropout(prob) hands `prob` to TF 1.x tf.nn.dropout as KEEP_prob
 * (network_builder.py:296-297), so Dropout(0.25) keeps 25 % of the units, scaled by 4.  Required before training a model that
 * has Dropout layers. */
int dg_clf_set_dropout(dg_clf* h, int layer, float keep_prob);
/* Reads a Conv2D / Linear layer's parameters back, in the layouts of dg_clf_set_weights (what a TF saver would hold). */
int dg_clf_get_weights(dg_clf* h, int layer, float* W, float* b, int is_device);
/* A fresh AdamOptimizer (what each model_train call builds): m = v = 0, t = 0.  Synchronous. */
int dg_clf_adam_reset(dg_clf* h);
/* A layer's Adam state: m and v [(W; b) flattened, W first] and the step count t (host).  Any of m, v, t may be NULL. */
int dg_clf_get_adam(dg_clf* h, int layer, float* m, float* v, int64_t* t, int is_device);
/* Installs a layer's moments (the layout dg_clf_get_adam returns) and sets the handle's step count to t: what restoring a saved
 * optimiser needs.  Synchronous. */
int dg_clf_set_adam(dg_clf* h, int layer, const float* m, const float* v, int64_t t, int is_device);
/* The mask [B, features] a Dropout layer draws in the forward `pass` (0 clean, 1 the adversarial half's inner FGSM forward,
 * 2 the forward on x_adv) of step `step` under `seed`: floor(keep + u), u from Philox4x32-10 (dg_clf_train.hip). */
int dg_clf_dropout_mask(dg_clf* h, int layer, int B, uint64_t seed, int64_t step, int pass, float* mask, void* stream);
/* The gradient of one training step on x [B,...], labels [B] int32, with no parameter change: grads = every Conv2D / Linear
 * layer's (dW, db) in layer order, each flattened in the reference layout, W before b; *loss = the step's mean cross-entropy (with
 * adv_eps > 0: (clean + adversarial) / 2); x_adv [B,...] (may be NULL) = the adversarial inputs, clip(x + adv_eps * sign(...),
 * clip_min, clip_max).  adv_eps <= 0: no adversarial half.  Dropout masks are drawn with (seed, step). */
int dg_clf_param_gradient(dg_clf* h, const float* x, const int32_t* labels, int B, float adv_eps, float clip_min, float clip_max,
                          uint64_t seed, int64_t step, float* grads, float* loss, float* x_adv, void* stream);
/* n_steps Adam steps of model_train: step s trains on the images X[idx[s*batch_size + i]], i < batch_size, of the n images
 * X [n,...] with labels [n] int32 (the batch schedule is the caller's; an index outside [0, n) reads a zero image that
 * contributes nothing); losses [n_steps] (may be NULL) = each step's loss.  The Adam step count t continues from the last
 * call (dg_clf_adam_reset restarts it); step s draws its Dropout masks with (seed, t before the step).  A whole epoch is
 * enqueued with no host synchronisation and no graph capture. */
int dg_clf_train(dg_clf* h, const float* X, const int32_t* labels, int n, const int32_t* idx, int n_steps, int batch_size,
                 float learning_rate, float adv_eps, float clip_min, float clip_max, uint64_t seed, float* losses, void* stream);

/*
 * The Jacobian side of the black-box substitute attack (/root/reference/blackbox.py:143-213: cleverhans' jacobian_graph and
 * jacobian_augmentation, restated in defensegan_amd/csrc/dg_jacobian.hip's header comment and DESIGN.md section 7).  The reference
 * differentiates model_sub(x), the PROBABILITIES: with of_probs != 0 on a model that ends in Softmax, out = softmax(logits) and the
 * seed on the logits is TF's (delta_kc - p_c) * p_k; otherwise out = the logits and the seed is onehot(c).  Device pointers;
 * asynchronous on `stream`, no host synchronisation, no float atomics: a call repeated returns the same bits.
 */
/* grad [B,in_h,in_w,in_c] = d out(x)[b, classes[b]] / dx; classes [B] int32.  A class outside [0, n) gives a zero gradient (the
 * policy of training's out-of-range label), never a read outside the row. */
int dg_clf_class_gradient(dg_clf* h, const float* x, const int32_t* classes, int B, int of_probs, float* grad, void* stream);
/* jac [B, n, in_h, in_w, in_c]: one forward, n backwards; jac[:, k] has the bits of dg_clf_class_gradient with classes == k. */
int dg_clf_jacobian(dg_clf* h, const float* x, int B, int of_probs, float* jac, void* stream);
/* jacobian_augmentation: X [n,...], labels [n] int32 -> X_out [2n,...]: X_out[:n] = X (not copied when X_out == X, a buffer with
 * room for 2n images), X_out[n + i] = X[i] + lmbda * sign(d softmax(logits(X[i]))[labels[i]] / dx), sign(0) = 0, NOT clipped.
 * The new half is produced in chunks of batch_size images (a trailing partial chunk is a chunk of its own) inside the one call;
 * the result does not depend on batch_size.  Any other overlap of X_out with X is DG_E_INVALID. */
int dg_jacobian_augment(dg_clf* h, const float* X, const int32_t* labels, int n, float lmbda, int batch_size, float* X_out,
                        void* stream);

/*
 * The white-box attack on the DEFENDED model (no reference counterpart: the reference's attacks differentiate through
 * ReconstructionLayer, whose gradient is identically zero): BPDA with EOT, L-infinity -- the real projection forward, the identity
 * as its backward, the gradient summed over the projection's random restarts, a projected sign step (defensegan_amd/csrc/dg_bpda.hip's
 * header comment and DESIGN.md section 7 give the definition; network_builder.BPDA drives the two entries).  Device pointers;
 * asynchronous on `stream`, no host synchronisation, no graph capture, no atomics.
 */
/* One (iteration, EOT sample): g = d CE(softmax(logits(rec)), labels) / d rec with the bits of dg_clf_input_gradient (labels [B]
 * int32, required), then over the B x in_h x in_w x in_c elements either
 *   accumulate_only != 0:  gsum += g                                   (gsum required; x_cur, x_orig, x_next unused, may be NULL)
 *   accumulate_only == 0:  t = gsum + g (t = g when gsum == NULL; gsum is read, not written) and
 *                          x_next = clip(x_orig + clamp(x_cur + eps_iter * sign(t) - x_orig, -eps, eps), clip_min, clip_max),
 *                          sign(0) = 0; x_next is a buffer of its own.
 * float4 loads and stores where in_h * in_w * in_c is a multiple of 4 and the pointers are 16-byte aligned. */
int dg_bpda_step(dg_clf* h, const float* rec, const int32_t* labels, int B, const float* x_cur, const float* x_orig, float* gsum,
                 int accumulate_only, float eps, float eps_iter, float clip_min, float clip_max, float* x_next, void* stream);
/* Best tracking for iterate k (>= 0): for every image with first_success[b] < 0, x_best[b] = x_iter[b] (row_elems floats each),
 * and first_success[b] = k where preds[b] != labels[b] as well.  An image that has succeeded is left alone, so x_best ends as the
 * first misclassified iterate or the last iterate judged.  preds, labels, first_success [B] int32; x_best must not be x_iter.
 * Runs on the current device. */
int dg_bpda_track(const int32_t* preds, const int32_t* labels, int B, int k, const float* x_iter, float* x_best,
                  int32_t* first_success, int64_t row_elems, void* stream);

/*
 * Projected gradient descent (L-infinity) on the BARE classifier: BPDA above with the identity as the projection and one sample,
 * the whole attack enqueued by this one call (defensegan_amd/csrc/dg_pgd.hip's header comment and DESIGN.md section 7;
 * network_builder.ProjectedGradientDescent).  x [B,H,W,C] the original images, x_start [B,H,W,C] the iterate x_0 (the caller's
 * clip(x), or any start), labels [B] int32.  For k < nb_iter: g_k = d CE(softmax(logits(x_k)), labels) / dx with the bits of
 * dg_clf_input_gradient (a label outside [0, classes) gives a zero gradient instead) and
 *   x_{k+1} = clip(x + clamp(x_k + eps_iter * sign(g_k) - x, -eps, eps), clip_min, clip_max),  sign(0) = 0.
 * Iterate j = 1 .. nb_iter succeeds for an image when the model's first arg-max on it is not its label; x_adv [B,H,W,C] receives
 * per image the first successful iterate or else the last one, first_success [B] int32 that j or -1.  nb_iter + 1 forwards and
 * nb_iter backwards.  x_adv must not be x or x_start.  nb_iter < 1, eps < 0, eps_iter < 0 and clip_min > clip_max are
 * DG_E_INVALID.  Device pointers; asynchronous on `stream`, no host synchronisation, no graph capture, no atomics; the result
 * does not depend on how many images share a call.
 */
int dg_pgd(dg_clf* h, const float* x, const float* x_start, const int32_t* labels, int B, float eps, float eps_iter, int nb_iter,
           float clip_min, float clip_max, float* x_adv, int32_t* first_success, void* stream);

/*
 * The L1 / L2 forms of the attacks above (defensegan_amd/csrc/dg_ball.hip's header comment and DESIGN.md section 7, "L2 balls").
 * Every norm is per image, over its in_h * in_w * in_c elements, one fixed-order float32 sum computed by the image's own workgroup
 * inside the call: no atomics, no host synchronisation, and no dependence on how many images share a call.  tiny = 1e-12 guards
 * every division: a zero gradient gives a zero step, never a NaN.  Device pointers; asynchronous on `stream`.
 */
/* cleverhans' fgm for ord 1 and 2 (ord = inf is dg_fgsm): g = dg_clf_input_gradient's bits (labels [B] int32, or NULL for the model's
 * own first arg-max), x_adv = clip(x + eps * g / max(tiny, n(g)), clip_min, clip_max) with n = sum |g| (ord 1) or sqrt(sum g^2) (ord 2). */
int dg_fgm(dg_clf* h, const float* x, const int32_t* labels, int B, float eps, int ord, float clip_min, float clip_max, float* x_adv,
           void* stream);
/* dg_bpda_step with the L2 step (ord must be 2; the L1 projection needs a sort and is not implemented): accumulate_only != 0 is
 * dg_bpda_step's gsum += g; otherwise t = gsum + g (t = g when gsum == NULL), u = t / max(tiny, ||t||), d = (x_cur + eps_iter * u) - x_orig,
 * x_next = clip(x_orig + d * min(1, eps / max(tiny, ||d||)), clip_min, clip_max). */
int dg_bpda_step_ball(dg_clf* h, const float* rec, const int32_t* labels, int B, const float* x_cur, const float* x_orig, float* gsum,
                      int accumulate_only, float eps, float eps_iter, int ord, float clip_min, float clip_max, float* x_next, void* stream);
/* dg_pgd with that L2 step in the projected sign step's place (ord must be 2): the same gradients, tracking, outputs and checks. */
int dg_pgd_ball(dg_clf* h, const float* x, const float* x_start, const int32_t* labels, int B, float eps, float eps_iter, int nb_iter,
                int ord, float clip_min, float clip_max, float* x_adv, int32_t* first_success, void* stream);
/* out [B] = per row of row_elems floats the ord-norm (1: sum |.|, 2: sqrt(sum .^2)) of v - w, or of v when w == NULL.  Runs on the
 * current device. */
int dg_row_norms(const float* v, const float* w, int B, int64_t row_elems, int ord, float* out, void* stream);

/*
 * The WGAN-GP critic (models/gan.py:167-199, mode "wgan-gp"; defensegan_amd/csrc/dg_critic.hip's header comment and DESIGN.md
 * section 7, "The critic", give the restatement and the derivation of the penalty's gradient).  The handle is a dg_clf model of
 * Conv2D, LeakyReLU, ReLU, Flatten and Linear layers whose output width is 1 (defensegan_amd/critic.py builds the reference's
 * mnist_discriminator); a model holding Dropout or Softmax, an output width other than 1, B < 1 and an unknown penalty_axes are
 * DG_E_INVALID.  With real, fake [B,H,W,C], alpha [B] and xhat = real + alpha (fake - real):
 *     w = mean_b D(fake_b) - mean_b D(real_b);   g = d(sum_b D(xhat_b)) / dxhat;   s = sqrt(sum over the reduced axes of g^2)
 *     P = mean over what is left of (s - 1)^2;   cost = w + gp_lambda P
 * penalty_axes 0 ("reference"): the sum runs over the HEIGHT axis only, as the reference's reduction_indices=[1] on an NHWC tensor
 * has it: s is [B,W,C] and P the mean of B W C column norms.  penalty_axes 1 ("image"): the published form, s [B] over H, W, C.
 * Where s == 0 the penalty's gradient is defined as 0 (TF yields NaN there).  Device pointers; asynchronous on `stream`, no host
 * synchronisation, no graph capture, no float atomics: a call repeated returns the same bits.  The workspace grows on demand.
 */
/* grads = d cost / d(every Conv2D / Linear layer's (W; b)) in dg_clf_param_gradient's layout; cost [3] = cost, w, P; slopes
 * (may be NULL) = s, [B,W,C] or [B].  The parameters do not change. */
int dg_critic_gradient(dg_clf* h, const float* real, const float* fake, const float* alpha, int B, float gp_lambda,
                       int penalty_axes, float* grads, float* cost, float* slopes, void* stream);
/* One step of tf.train.AdamOptimizer(learning_rate, beta1 = beta_a, beta2 = beta_b, epsilon = 1e-8) on that gradient (the reference:
 * 1e-4, 0.5, 0.9): m = beta_a m + (1 - beta_a) g, v = beta_b v + (1 - beta_b) g^2 (1 - beta formed in float32),
 * p -= lr_t m / (sqrt(v) + 1e-8), lr_t = lr sqrt(1 - beta_b^t) / (1 - beta_a^t).  The moments and t are the handle's own
 * (dg_clf_adam_reset, dg_clf_get_adam).  cost [3] (may be NULL) = the step's cost, w, P before the update. */
int dg_critic_step(dg_clf* h, const float* real, const float* fake, const float* alpha, int B, float gp_lambda,
                   int penalty_axes, float learning_rate, float beta_a, float beta_b, float* cost, void* stream);

/*
 * The generator's training step (the generator half of models/gan.py:167-199, 273-293; defensegan_amd/csrc/dg_gen_train.hip's header
 * comment and DESIGN.md section 7, "The generator step").  Implemented for the MNIST / F-MNIST generator without Batchnorm; a CelebA
 * or use_bn handle is DG_E_INVALID with "not implemented for ..." in dg_last_error().  z [N, latent]; dy [N,28,28,1] = the gradient
 * of the loss with respect to the generator's OUTPUT (after the sigmoid) -- for WGAN-GP dg_clf_backward on the critic at x = G(z)
 * with dlogits = -1/N.  Null pointers, N < 1, N above 2^20 (dg_generate's limit), incomplete weights and unknown names are returned
 * as errors.  Device pointers; asynchronous on `stream`; the first call of a row count sizes workspaces and job lists (blocking, as
 * dg_prepare), later calls of it allocate nothing and wait for nothing.  No float atomics: a call repeated returns the same bits.
 */
/* Forward on z, then the seeded backward.  grads = the flat gradient in the order and layouts of the parameters -- Generator.Input.W
 * [latent, 4*4*4*nd], .b, then <layer>.Filters [5,5,Cout,Cin] and .Biases for Generator.2, .3, .5.  out_y [N,28,28,1] = G(z) and
 * out_dz [N, latent] may be NULL.  Stateless; the weights do not change. */
int dg_gen_param_gradient(dg_handle* h, const float* z, const float* dy, int N, float* grads, float* out_y, float* out_dz, void* stream);
/* The same gradient, then one step of tf.train.AdamOptimizer(lr, beta1, beta2, epsilon = 1e-8) in dg_critic_step's form on every
 * parameter, then the refresh of every derived weight layout of the handle (options frag_path and turn_fused included) on the device:
 * whatever runs next on the stream -- dg_generate, dg_reconstruct -- sees the new weights.  The moments and the step count are the
 * handle's own; a later dg_set_weights replaces the parameter and leaves them alone. */
int dg_gen_step(dg_handle* h, const float* z, const float* dy, int N, float lr, float beta1, float beta2, void* stream);
/* The current value of a parameter by its reference name (the layout dg_set_weights takes).  Synchronous. */
int dg_get_weights(dg_handle* h, const char* name, float* out, int is_device);
/* A fresh optimiser: m = v = 0, t = 0.  Synchronous. */
int dg_gen_adam_reset(dg_handle* h);
/* A parameter's Adam moments (its own shape) and the handle's step count t (host); any of m, v, t may be NULL.  Synchronous. */
int dg_gen_get_adam(dg_handle* h, const char* name, float* m, float* v, int64_t* t, int is_device);
/* Installs a parameter's moments and sets the handle's step count to t.  Synchronous. */
int dg_gen_set_adam(dg_handle* h, const char* name, const float* m, const float* v, int64_t t, int is_device);

/*
 * The latent-space attack (no reference counterpart; Athalye, Carlini, Wagner 2018, section 5; defensegan_amd/csrc/dg_latent.hip's
 * header comment and DESIGN.md section 7, "The latent-space attack"): TF's Adam on z so that G(z) is misclassified by the bare
 * classifier `c` and close to x.  `g` is a generator of the MNIST / F-MNIST architecture without Batchnorm (a CelebA or use_bn handle
 * is DG_E_INVALID with "not implemented for ..." in dg_last_error()); `c` a classifier of [28,28,1] inputs with at least two classes
 * and no Dropout layer before its logits, on the same device.  x [B,28,28,1] in generator range, labels [B] int32; R restarts per
 * image, row j = i R + r belongs to image i.  z0 [B*R, latent], or NULL: the rows are drawn as dg_init_latents(seed, first_row) draws
 * them (std sqrt(1/latent)), keyed by the global row first_row + j.  Per iteration k < nb_iter and row j:
 *     y = G(z_j);  Z = logits(y);  m_j = Z[label_i] - max_{c != label_i} Z[c] (the first maximum on ties, at o_j);
 *     d_j = mean over the pixels of (y - x_i)^2;   the loss is d_j + cweight max(m_j + kappa, 0);
 *     dy = dg_clf_backward's bits for dlogits = (+cweight at label_i, -cweight at o_j) if m_j + kappa > 0 else 0, plus 2 (y - x_i) / 784;
 *     dz_j = what dg_gen_param_gradient returns as out_dz for this dy;   z_j <- Adam(z_j, dz_j), epsilon 1e-8, dg_critic_step's form,
 *     lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) in float64 on the host with t = t_start + k + 1.
 * Unless keep_state != 0, one closing forward (k = nb_iter) judges the last iterate: nb_iter + 1 forwards, nb_iter backwards.
 * Tracking, per image, over every evaluated row (k, r): a success is m_j < -kappa; the result is the success of the smallest d_j
 * (ties: the earliest k, then the smallest r) and best_iter = t_start + k; while there is none, the row of the smallest m_j (smallest
 * r) of the iterate judged last, with best_iter = -1.
 *   m, v        [B*R, latent] Adam's moments, read and updated in place; both NULL: a fresh optimiser (zero moments, needs t_start 0)
 *   t_start     Adam steps already taken.  t_start > 0 CONTINUES an attack: the tracker then starts from what x_adv, best_dist,
 *               best_margin, best_iter, best_row hold (pass the buffers of the call before), so that nb_iter = 3 equals three calls of
 *               nb_iter = 1 with keep_state (z0 = the out_z before, t_start = 0, 1, 2) followed by one of nb_iter = 0, bit for bit
 *               (t_start > 0 with m, v or one of the best_* pointers NULL is DG_E_INVALID)
 *   x_adv       [B,28,28,1] the winning row's G(z), as the forward wrote it (required)
 *   best_dist, best_margin [B], best_iter, best_row [B] int32 (the r)                           (each may be NULL)
 *   out_z       [B*R, latent] the final z                                                       (may be NULL)
 *   out_margin, out_dist [nb_iter + 1, B*R] m_j and d_j of every evaluated iterate of THIS call, row k = its k-th forward; with
 *               keep_state row nb_iter is not written                                           (may be NULL)
 *   out_dz      [B*R, latent] dz of the call's last backward; not written when nb_iter = 0      (may be NULL: a test hook)
 * Labels are device memory and are trusted: one outside [0, classes) reads nothing, gives its rows a zero classification term and
 * the margin +inf (never a success).  Errors: null pointers, B*R < 1 or above 2^20 (dg_generate's limit), betas outside [0, 1),
 * kappa < 0, cweight < 0, nb_iter < 0, nb_iter = 0 with keep_state and t_start = 0 (nothing would be evaluated and the outputs would
 * stay unwritten; with t_start > 0 it is legal and leaves the passed state and x_adv as they are, out_z = z0), t_start + nb_iter
 * above INT32_MAX (best_iter is int32), incomplete weights of either handle (DG_E_STATE).  A row whose margin is NaN is never a
 * success and never the smallest margin, a successful row whose distance is NaN is never taken, all-NaN margins give row 0, +inf
 * compares as a number.  Device pointers; asynchronous on `stream`;
 * the first call of a row count sizes workspaces and job lists (blocking, as dg_prepare), later calls of it allocate nothing and
 * wait for nothing.  No float atomics, every sum in a fixed order: a call repeated returns the same bits, and an image's result does
 * not depend on which other images share the call.
 */
int dg_latent_attack(dg_handle* g, dg_clf* c, const float* x, const int32_t* labels, int B, int R, const float* z0, uint64_t seed,
                     int64_t first_row, int nb_iter, float lr, float beta1, float beta2, float cweight, float kappa, float* m, float* v,
                     int64_t t_start, int keep_state, float* x_adv, float* best_dist, float* best_margin, int32_t* best_iter,
                     int32_t* best_row, float* out_z, float* out_margin, float* out_dist, float* out_dz, void* stream);

/*
 * The score-based black-box attack (no reference counterpart): SPSA with Rademacher directions and dg_bpda_step's projected sign
 * step, L-infinity.  It reads only the attacked model's logits, so it works on the defended model, whose gradient is identically
 * zero (defensegan_amd/csrc/dg_spsa.hip's header comment and DESIGN.md section 7, "SPSA", give the definition;
 * network_builder.SPSA drives the two entries).  n direction pairs, probe size delta, iteration iter = k, image b of a call has
 * the GLOBAL index g = first_image + b.  u_i[e] = +1 where bit (i & 31) of word (e & 3) of Philox4x32-10(key = (seed lo, seed hi),
 * counter = (e >> 2, g, k ceil(n / 32) + (i >> 5), 0x53505341)) is set, else -1; never stored.  Device pointers; asynchronous on
 * `stream`, on the current device; no host synchronisation, no graph capture, no atomics, no workspace; an image's result does not
 * depend on which other images share the call.  DG_E_INVALID: a null required pointer, B < 1, n < 1, row_elems < 1 or above
 * 2^31 - 1, more than 2^31 - 1 workgroups of 256 threads in one launch (B ceil(row_elems / 4) threads for the queries,
 * B ceil(row_elems / 1024) workgroups for the step), classes < 2, delta <= 0, eps < 0, eps_iter < 0, clip_min > clip_max, iter < 0,
 * first_image < 0, first_image + B > 2^32, iter ceil(n / 32) + ceil(n / 32) > 2^32, x_next == x_cur, out_grad equal to x_next,
 * x_cur or x_orig.
 */
/* q [B, 2n + 1, row_elems]: q[b,0] = x_cur[b]; q[b,1+2i] = clip(x_cur[b] + delta u_i) and q[b,2+2i] = clip(x_cur[b] - delta u_i),
 * clipped to [clip_min, clip_max].  float4 where row_elems is a multiple of 4 and the pointers are 16-byte aligned. */
int dg_spsa_queries(const float* x_cur, int B, int64_t row_elems, int n, float delta, uint64_t seed, int64_t first_image, int iter,
                    float clip_min, float clip_max, float* q, void* stream);
/* logits [B (2n + 1), classes] of those queries as dg_clf_forward leaves them, labels [B] int32.  L = max_{j != y} Z_j - Z_y (0 for
 * every query of an image whose label lies outside [0, classes)); dL_i = L(q+_i) - L(q-_i), formed in float64 and rounded once to
 * float32, taken as 0 where that is not finite;  ghat[b,e] = float32(1 / (2 delta n)) * (the float32 sum over i, ascending, of
 * dL_i u_i[e]);  x_next = clip(x_orig + clamp(x_cur + eps_iter * sign(ghat) - x_orig, -eps, eps), clip_min, clip_max), sign(0) = 0.
 * out_grad [B, row_elems] (may be NULL; a buffer of its own) receives ghat. */
int dg_spsa_step(const float* logits, const int32_t* labels, int B, int classes, int64_t row_elems, int n, float delta, uint64_t seed,
                 int64_t first_image, int iter, const float* x_cur, const float* x_orig, float eps, float eps_iter, float clip_min,
                 float clip_max, float* x_next, float* out_grad, void* stream);

/*
 * DeepFool (Moosavi-Dezfooli et al. 2016; no reference counterpart: cleverhans is an empty submodule there): the minimal L2
 * perturbation over the nearest linearised decision boundary, the whole loop enqueued by this one call
 * (defensegan_amd/csrc/dg_deepfool.hip's header comment and DESIGN.md section 7, "DeepFool", give the definition; attacks.DeepFool).
 * x [B,H,W,C]; no labels; the LOGITS are read, before any Softmax.  orig = the first arg-max at x; the nb_candidate classes of the
 * largest logits at x, descending, ties to the lower class, are fixed for the run; r = 0, adv = x.  While the first arg-max over
 * all classes at adv is orig the image is active, and an iteration does, with f_j and w_j the differences of logit and class
 * gradient between candidate j and candidate 0 at adv:  pert_j = (|f_j| + 1e-5) / ||w_j||_2,  j* = the first index of the minimum,
 * r += pert_j* w_j* / ||w_j*||_2,  adv = clip(x + r, clip_min, clip_max).  After max_iter iterations, or when no image is active:
 *   x_adv       [B,H,W,C] clip(x + (1 + overshoot) r, clip_min, clip_max) (required; may be x)
 *   r_norm      [B] ||x_adv - x||_2 of what was written                                       (may be NULL)
 *   iters       [B] int32, the iterations the image entered active                            (may be NULL)
 *   final_class [B] int32, the first arg-max at x_adv (one more forward); a NaN is never a candidate, class 0 where class 0 is a NaN
 *               or nothing else is left                                                       (may be NULL)
 * ||w_j|| == 0 gives pert_j = +inf; +inf and NaN are never the minimum; an image without a minimum becomes inactive and keeps its r.
 * An image whose logits hold a NaN, at x or after a step, becomes inactive and that step is taken back: it returns
 * clip(x + (1 + overshoot) r) from the last finite state.  DG_E_INVALID: null h, x or x_adv, B < 1, nb_candidate < 2 or above the
 * number of logits (or above 2048), max_iter < 0, clip_min > clip_max, B * nb_candidate or B * max_iter above 2^31 - 1; DG_E_STATE:
 * incomplete weights.  Device pointers; asynchronous on `stream` except that every second iteration the count of active images is
 * read back and the loop ends when it is zero, which changes no bit of the result; no graph capture, no float atomics, every sum in
 * a fixed order: a call repeated returns the same bits and an image's result does not depend on which other images share the
 * call.  The workspace grows on demand (nb_candidate rows per image through the classifier).
 */
int dg_deepfool(dg_clf* h, const float* x, int B, int nb_candidate, float overshoot, int max_iter, float clip_min, float clip_max,
                float* x_adv, float* r_norm, int32_t* iters, int32_t* final_class, void* stream);
/* choices [max_iter, B] int32 (device): the j* of every step of the handle's LAST dg_deepfool call, -1 where the image took none
 * (inactive, no minimum, or an iteration the early exit skipped); DG_E_STATE unless that call had this B and max_iter (>= 1). */
int dg_deepfool_choices(dg_clf* h, int B, int max_iter, int32_t* choices, void* stream);

/*
 * The Jacobian saliency-map attack (Papernot et al. 2016; cleverhans' SaliencyMapMethod; no reference counterpart): the L0 attack of
 * the suite, targeted, the whole loop enqueued by this one call (defensegan_amd/csrc/dg_jsma.hip's header comment and DESIGN.md
 * section 7, "Saliency map", give the definition; attacks.SaliencyMapMethod).  x [B,H,W,C], F = H W C features; target [B] int32, the
 * class each image is to be given (outside [0, classes): the image is left alone).  adv = x; the search domain of an image is its
 * features with x < clip_max (theta > 0) or x > clip_min (theta < 0).  An iteration of an active image: O = the logits, or with
 * of_probs = 1 softmax(logits); the image becomes inactive when the first arg-max of O is its target, when O holds a NaN or when fewer
 * than 2 features are left in its domain; a = grad O[t], b = grad sum_{j != t} O[j] (two seeded backwards; with of_probs = 1, b = -a
 * up to rounding); over the pairs p < q of the domain, A = a_p + a_q, Bs = b_p + b_q, admissible where A > 0 and Bs < 0 (theta < 0:
 * A < 0 and Bs > 0), the admissible pair of the largest score -(A Bs) > 0 is taken, ties to the smallest p, then the smallest q, a
 * NaN score never; without such a pair the image becomes inactive and keeps adv; otherwise adv[p] = clip(adv[p] + theta, clip_min,
 * clip_max), the same for q, and both leave the domain.  After max_iters iterations, or when no image is active:
 *   x_adv       [B,H,W,C] adv (required; may be x)
 *   iters       [B] int32, the pairs the image moved                                              (may be NULL)
 *   final_class [B] int32, the first arg-max of the logits at x_adv (one more forward); a NaN is never a candidate, class 0 where
 *               class 0 is a NaN or nothing else is left                                          (may be NULL)
 *   n_changed   [B] int32, the elements with x_adv != x (a NaN element of x is not counted)       (may be NULL)
 * max_iters = 0 returns x_adv = x.  DG_E_INVALID: null h, x, target or x_adv, B < 1, theta zero or not finite, max_iters < 0,
 * clip_min > clip_max, of_probs not 0 or 1, F < 2, F above 5120 ("not implemented for more than"), 2 B max_iters above 2^31 - 1;
 * DG_E_STATE: incomplete weights.  Device pointers; asynchronous on `stream` except that every second iteration the count of active
 * images is read back and the loop ends when it is zero, which changes no bit of the result; no graph capture, no float atomics:
 * a call repeated returns the same bits and an image's result does not depend on which other images share the call.  The workspace
 * grows on demand (two rows per image through the classifier, one byte per feature).
 */
int dg_jsma(dg_clf* h, const float* x, const int32_t* target, int B, float theta, int max_iters, float clip_min, float clip_max,
            int of_probs, float* x_adv, int32_t* iters, int32_t* final_class, int32_t* n_changed, void* stream);
/* choices [max_iters, B, 2] int32 (device): the (p, q) of every step of the handle's LAST dg_jsma call, -1 where the image took none
 * (inactive, no admissible pair, or an iteration the early exit skipped); DG_E_STATE unless that call had this B and max_iters (>= 1). */
int dg_jsma_choices(dg_clf* h, int B, int max_iters, int32_t* choices, void* stream);

/*
 * The elastic-net attack (Chen et al. 2018, EAD; cleverhans' ElasticNetMethod; no reference counterpart): Carlini-Wagner's loss plus
 * beta * ||x_adv - x0||_1, minimised by iterative shrinkage-thresholding, with `fista` by FISTA; the L1 attack of the suite
 * (defensegan_amd/csrc/dg_ead.hip's header comment and DESIGN.md section 7, "Elastic net", give the algorithm;
 * attacks.ElasticNetMethod).  x [B,in_h,in_w,in_c]; labels [B] int32 = y, or y_target when `targeted`, or NULL for the model's own
 * first argmax on x.  decision_rule 0 ("EN") ranks successful iterates by ||d||_2^2 + beta ||d||_1, 1 ("L1") by ||d||_1, d = iterate -
 * clip(x).  The rate of iteration i is learning_rate * sqrt(1 - i / max_iterations).  Chunks of batch_size images (a trailing partial
 * chunk is a chunk of its own) share the abort-early decision and nothing else.  Out: x_adv [B,...] = the best successful iterate
 * over all steps, clip(x) bit for bit where none succeeded; best_dist [B] the rule's criterion there (1e10 when none); best_class [B]
 * int32 (-1 when none); final_const [B] float64 and chunk_stop [binary_search_steps, ceil(B / batch_size)] int32 as dg_cw's (both may
 * be NULL).  DG_E_INVALID: a null h, x, x_adv, best_dist or best_class, B < 1, beta < 0, clip_min >= clip_max, max_iterations < 1, a
 * rule outside {0, 1}, batch_size < 1, binary_search_steps < 0.  Device pointers; the whole attack is enqueued on `stream` with no host
 * synchronisation and no graph capture; no float atomics, every sum in a fixed order: a repeated call returns the same bits, and a
 * chunk's images give the same bits alone or inside a larger call.  Per iteration the classifier runs one forward over 2 B rows (the
 * slack and the iterate) and one backward over B; as for dg_cw they keep running over chunks that have stopped.  The workspace
 * (about 3 x B x pixels floats, and the handle's activations for 2 B rows) lives in the handle and grows on demand.
 */
int dg_ead(dg_clf* h, const float* x, const int32_t* labels, int B, int targeted, int batch_size, float confidence, float beta,
           int decision_rule, int fista, float learning_rate, int binary_search_steps, int max_iterations, int abort_early,
           double initial_const, float clip_min, float clip_max, float* x_adv, float* best_dist, int32_t* best_class,
           double* final_const, int32_t* chunk_stop, void* stream);

/*
 * The path's one collective: every rank projects and classifies its contiguous shard of the image list
 * (no collective on the data path) and ONE all_gather assembles the evaluation message -- per rank `count` int32 words, e.g.
 * [n | labels (cap) | preds (cap) | diffs (cap, float32 bits)] as defensegan_amd/gan_defense.py:model_eval_gan_sharded builds it
 * (the reduction of /root/reference/utils/gan_defense.py:166-179 over ranks; the reference itself is single-process).  RCCL
 * over xGMI, reachable WITHOUT torch.distributed: librccl.so is opened on first use.  Rank 0 draws a unique id, the caller
 * carries its 128 bytes to the other ranks (file, MPI, environment), every rank creates its communicator -- one process per GPU.
 * send [count], recv [nranks * count]: device pointers; asynchronous on `stream`.
 */
typedef struct { char internal[128]; } DgUniqueId;          /* = ncclUniqueId */
typedef struct dg_comm dg_comm;
int dg_comm_unique_id(DgUniqueId* id);
int dg_comm_create(int nranks, const DgUniqueId* id, int rank, int device, dg_comm** out);
int dg_comm_destroy(dg_comm* c);
int dg_gather_eval(dg_comm* c, const int32_t* send, int32_t* recv, int64_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEFENSEGAN_HIP_H */
