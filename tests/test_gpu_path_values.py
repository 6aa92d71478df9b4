"""-m gpu: the default projection path (USE_BN: False) value for value against tests/support/path_reference.py (float64),
layer by layer, per tap class, every row.  tests/test_path_reference_cpu.py shows without a GPU that these checks reject a
dropped border tap, a lost K-pair half, a partial last 32-row block left stale, a neighbour's gate and a stale dz-only gradient.

Per case: gan.generate(z), every act<d> read (the activations, hence the device's gates); gan.loss_grad(x, z), every act<d> read
again (now the gradient at that layer); a dz-only dg_loss_grad through the C ABI (out_y = out_loss = NULL, dz pre-filled with
NaN), every act<d> read once more.  Inputs: z = 0.3 * N(0, 1), uniform targets, synth.make_weights(seed 1234, gain 2, bias 0.1).

Routes (read off dg_engine.cpp run_forward / run_backward, dg_tail_mnist.hip launch_mnist_tail_mfma, dg_tail_celeba.hip
launch_celeba_tail_*), each at the smallest row counts that reach it:

  route                                                        how it is reached                        rows used here
  mnist_tail_mfma_kernel<64>, forward and forward + backward   defaults, rows < 2 * tail_pipe = 512      1, 33, 47
  mnist_tail_pipe_kernel<64>                                   tail_pipe = 8, all outputs               16 (= 2 * pipe), 33, 48
  mnist_tail_pipe3_kernel<64, false>                           tail_pipe = 8, dz-only                   16, 33, 48
  mnist_tail_pipe3_kernel<64, false> (and pipe_kernel)         default tail_pipe 256, dz-only (all)     600 (R = 10)
  GEMM: last 32-row block of a class partial; the K-pair       always                                   33, 47 (rows * positions % 32 != 0)
    classes of the 4x4 <-> 7x7 / 8x8 backward layers
  GEMM: whole tiles / quarters / everything cut                jobs.slack 1e30 + jobs.min_level 0;      33
                                                               jobs.min_level 2; jobs.slack 0.01
  Linear on the weight-stationary kernels / the generic GEMM   latent_turn 1 (default) / 0              1, 33 (CelebA 9)
  celeba_tail_fwd_split_kernel<64>, one item per workgroup     default 512 workgroups                   9 (144 items)
    ... iterating                                              default at 33 rows (528 items); = 8      9, 33
  celeba_tail_fwd16_kernel<64, false>                          tail_fwd_split = 0                       9
  CelebA forward tail with want_loss = 0 and y == nullptr,     dz-only                                  9, 33, 47
    then the backward
  celeba_tail_bwd_persist_kernel<64>, one item per workgroup   default 512 workgroups                   9, 33, 47
    ... iterating                                              tail_bwd_persist = 8                     9, 33
  C = 128 instantiations of both tails and of the GEMM layers  NET_DIM 128                              MNIST 33, CelebA 9

Not reached by any shape of at most 600 rows, and not run here: job lists of more than one dispatch round (a layer needs
thousands of rows to hold more jobs than 256 CUs x 2-5 slots); celeba_tail_bwd_persist_kernel iterating on its DEFAULT grid
(>= 65 rows; the loop is the one tail_bwd_persist = 8 runs); concurrent row groups (two_streams: >= 1024 rows, dg_reconstruct
only -- a row offset r0 != 0 into the activation buffers never occurs in dg_loss_grad / dg_generate).

The checks ((1) .. (5), tests/support/path_reference.py run_checks), all per tap class, relative to max|float64| over the class:
 (1) forward, teacher-forced: act<d> against the float64 layer fed the device's act<d - 1>; y (of both calls) against the float64
     tail fed the device's last activation.  2e-6.
 (2) gates: where (act<d> > 0) differs from the float64 layer's gate, the float64 |pre-activation| is < 1e-5.
 (3) backward, teacher-forced, every layer: grad<d> against the float64 layer fed the device's grad<d + 1> and the device's gate;
     the tail's gradient from the device's y; dz from the device's da0.  1e-5.
 (4) end to end, every row: dz against the float64 backward from z with the device's gates, 1e-5 of max|dz|, no row left out;
     the per-row loss at rtol 1e-5.
 (5) the dz-only call: (3) and (4) again, no NaN left.  Its gates are the all-outputs call's: the same GEMM layers run on the
     same z, and every tail forms its ReluGrad bits from the activation the last GEMM layer stored.
Yardstick: the same teacher-forced layer in numpy float32 on the same inputs.  Where its error in a class exceeds a quarter of
the figure (2e-6 / 1e-5) the class's bound is 4 x the yardstick's worst error in the class + 2 ulp; never a figure of the
device's.

Measured on MI355X, worst case of each group over all 26 cases (device error | float32 yardstick error | bound | bound / error;
all relative to max|float64| of the class):
  (1) forward GEMM layers   1.57e-06 | 1.18e-07 | 2e-06    | x1.3   CelebA 47 rows, act1 class 1 (per case: x1.3 .. x2.0, always a
                                                                    class of act1 -- MNIST-128: act2 --: K = 256 x up to 9 taps in one float32 chain)
  (1) y, MNIST              1.76e-07 | 1.81e-07 | 2e-06    | x11.4  600 rows, class 0 (every tail kernel: 1.3e-07 .. 1.8e-07)
  (1) y, CelebA             1.54e-06 | 5.38e-07 | 2.27e-06 | x1.5   NET_DIM 128, class 0; bound from the yardstick (below)
  (2) gates                 at most 2 of 3.8e6 differ from float64 (MNIST 600 rows, act1), largest |pre| there 1.74e-07 (< 1e-05)
  (3) backward GEMM layers  1.74e-06 | 1.89e-07 | 1e-05    | x5.8   CelebA 47 rows, grad2 class 2 (MNIST: grad0, x6.8 .. x9.3)
  (3) tail backward         3.85e-07 | 2.55e-07 | 1e-05    | x26.0  CelebA 47 rows, grad3 class 0 (MNIST: 2.4e-07, x41)
  (3) dz from da0           3.15e-07 | 2.98e-07 | 1e-05    | x31.7  MNIST 16 rows
  (4) dz end to end         8.83e-07 of 1e-05 (CelebA 9 rows); loss 1.93e-07 of 1e-05 (CelebA 33 rows)
  (5) dz-only call          no NaN; every figure equals the all-outputs call's (the gradients of the two calls agree to the digits printed
                            on every route, pipe3 against the per-row and first-generation MNIST tails included)
Classes whose bound comes from the yardstick (float32 error above a quarter of the figure): only y of CelebA, where tanh saturates
(|y| -> 1, numpy float32 tanh is off by up to 6.5e-07 there): classes 0, 3, 5, 11 at NET_DIM 64 (bounds 2.1e-06 .. 2.8e-06, device
0.9e-06 .. 1.45e-06) and class 0 at NET_DIM 128.  No class of a GEMM layer, of MNIST's y or of any gradient needed it."""

import numpy as np
import pytest

from defensegan_amd import archs, synth
from tests.support import path_reference as PR

pytestmark = pytest.mark.gpu

_W, _MEMO = {}, {}


def _weights(arch, net_dim):
    """One weight dict per (arch, width): the memo of reference evaluations keys on its identity."""
    if (arch, net_dim) not in _W:
        _W[(arch, net_dim)] = synth.make_weights(arch, seed=1234, gain=2.0, bias_range=0.1, net_dim=net_dim)
    return _W[(arch, net_dim)]


def _gan(arch, net_dim, opts):
    from defensegan_amd.gan import dataset_gan_dict
    gan = dataset_gan_dict[arch](cfg={"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": net_dim}, test_mode=True)
    assert gan.set_weights(_weights(arch, net_dim)) == []
    for k, v in opts.items():
        gan.set_option(k, v)
    return gan


def _inputs(arch, rows):
    a = archs.make_arch(arch)
    R = 1 if rows % 10 else 10
    rs = np.random.RandomState(700 + rows)
    z = (rs.standard_normal((rows, a.latent_dim)) * 0.3).astype(np.float32)
    rs = np.random.RandomState(701 + rows)
    x = (rs.rand(rows // R, *a.image_dim) * (a.in_hi - a.in_lo) + a.in_lo).astype(np.float32)
    return z, x, R


def _read_all(gan, arch, p, N):
    out = []
    for d in range(PR.n_act(arch)):
        if d == 0:
            shape = (N, 4, 4, p["Generator.Input.W"].shape[1] // 16)
        else:
            name, _, e, _, _ = PR.O._arch_layers(arch)[d - 1]
            shape = (N, e, e, p[name + ".Filters"].shape[2])
        n = int(np.prod(shape))
        t = gan.debug_read("act%d" % d, n)
        assert t.numel() == n, (d, t.numel(), n)
        out.append(t.cpu().numpy().reshape(shape))
    return out


def _record(gan, arch, p, z, x, R):
    import torch
    N = len(z)
    rec = {"z": z, "x": x, "R": R}
    rec["y_generate"] = np.asarray(gan.generate(z))
    rec["acts"] = _read_all(gan, arch, p, N)
    rec["y"], rec["loss"], rec["dz"] = (np.asarray(v) for v in gan.loss_grad(x, z))
    rec["grads"] = _read_all(gan, arch, p, N)
    xd, zd = torch.as_tensor(x).cuda(), torch.as_tensor(z).cuda()
    dz = torch.full_like(zd, float("nan"))
    gan._check(gan._lib().dg_loss_grad(gan._handle, xd.data_ptr(), zd.data_ptr(), N // R, R, None, None, dz.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    rec["only"] = {"dz": dz.cpu().numpy(), "grads": _read_all(gan, arch, p, N)}
    return rec


J_WHOLE = {"jobs.slack": 1e30, "jobs.min_level": 0}
J_QUART = {"jobs.min_level": 2}
J_CUT = {"jobs.slack": 0.01}

CASES = (
    [("mnist", 64, r, {}) for r in (1, 33, 47)] +
    [("mnist", 64, r, {"tail_pipe": 8}) for r in (16, 33, 48)] +
    [("mnist", 64, 600, {})] +
    [("mnist", 64, 33, o) for o in (J_WHOLE, J_QUART, J_CUT)] +
    [("mnist", 64, r, {"latent_turn": 0}) for r in (1, 33)] +
    [("mnist", 128, 33, {})] +
    [("celeba", 64, r, {}) for r in (9, 33, 47)] +
    [("celeba", 64, r, {"tail_fwd_split": 8}) for r in (9, 33)] +
    [("celeba", 64, 9, {"tail_fwd_split": 0})] +
    [("celeba", 64, r, {"tail_bwd_persist": 8}) for r in (9, 33)] +
    [("celeba", 64, 33, o) for o in (J_WHOLE, J_QUART, J_CUT)] +
    [("celeba", 64, 9, {"latent_turn": 0})] +
    [("celeba", 128, 9, {})]
)
CASES.sort(key=lambda c: c[:3])                  # cases on the same inputs next to each other: they share the memo below


def _memo(key):
    """The reference evaluations of ONE input set (float64 / float32 layers by the bytes of their inputs: settings that leave a
    layer's input bit for bit the same share them); dropped when the next input set begins."""
    if key not in _MEMO:
        _MEMO.clear()
        _MEMO[key] = PR.Memo()
    return _MEMO[key]


def _id(c):
    arch, net_dim, rows, opts = c
    return "%s-%d-rows%d-%s" % (arch, net_dim, rows, ",".join("%s=%g" % kv for kv in sorted(opts.items())) or "defaults")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_default_path_layer_by_layer(case):
    """(1) - (5) of the module docstring on one route of its table."""
    arch, net_dim, rows, opts = case
    lines = []
    try:
        p = _weights(arch, net_dim)
        z, x, R = _inputs(arch, rows)
        rec = _record(_gan(arch, net_dim, opts), arch, p, z, x, R)
        res = PR.run_checks(rec, p, arch, _memo(case[:3]))
        lines = res.lines + ["--"] + res.summary()
        assert res.fails == [], "\n".join(l for _, _, l in res.fails)
    finally:
        print("\n[%s]\n  " % _id(case) + "\n  ".join(lines))
