"""-m gpu: the Batchnorm path (USE_BN: True) value for value against tests/support/bn_reference.py (float64), plus the seeded
latent draw and the restart selection.

Batch statistics couple all rows, so no row-independence argument carries a large launch back to a small checked one: every
code route is run at the smallest row count that reaches it (routes read off dg_bn.hip / dg_engine.cpp):

  route                                                    condition                         rows used here
  bn_finalize_kernel<float> straight from the block sums   <= 256 blocks of 32 rows          MNIST 7, 40 (BN3: rows * 196 / 32 = 245)
  bn_fold_blocks_kernel -> bn_finalize_kernel<double>      > 256 blocks                      MNIST 47, 48 (BN3: 288 / 294), CelebA 33 (BN3: 264)
  bn_partial_kernel with more than 32 rows per block       bn_fused = 0, rows * pos > 32768  MNIST 176 (BN3: 34 496 rows)
  last 32-row block of a tap class partial                 rows * positions % 32 != 0        7, 9, 33, 47 (BN1: rows % 32)
  BN1's 4096 columns (16 column tiles, 256 finalize groups)  always                          every case
  BN1 in the fold (grid.y > 1 of bn_fold_blocks_kernel)    BN1 has rows / 32 blocks: > 8192 rows -- no shape <= 600 rows reaches
                                                           it; not run here

The checks ((a) .. (d) in the test names' docstrings):
 (a) statistics, teacher-forced: float64 statistics of the very floats the producing GEMM left (bnpre<d>) against bnf<d>.  The
     backward sums bnb<d> likewise: the masked dy is overwritten in place by da, but da = (scale * rstd) * (dy - m1 - xhat * m2)
     is affine in dy, so the device's dy is recovered exactly from the device's da and compared with the device's (m1, m2)
     (channels with scale = 0 carry no information and are left to (d)).  Bound: 4 x the worst error over the layer's channels
     of the float32 two-pass form (tf.nn.moments in float32) on the same inputs + 2 ulp of the statistic; never a figure of the
     device's.
 (b) forward, layer by layer: act<d> against the float64 layer fed with the device's previous activation, 2e-6 relative, no
     exclusions (ReLU is continuous).
 (c) gates: where (act<d> > 0) differs from the float64 layer's gate, the float64 |bn output| there is < 1e-5.
 (d) backward, every row: dz against the float64 backward run with the DEVICE's gates: 1e-5 of max|dz|, no row left out.

The yardstick of rule (a) is the WORST float32-two-pass error over the layer's channels (for the close-rows output: over its
elements), not the error on the same channel: the device adds in another order, so its error on a channel is not tied to the
two-pass error on that channel.  That is looser than a per-channel reading of the rule; the margins below are against it.
bn_fused 0, 1 and 2 run at every row count (176 rows reach the long-row-block route only with 0; 1 and 2 are then one more
fold-route case).

Measured on MI355X, worst case of each group (device error | float32 two-pass error | bound = 4 x that + 2 ulp | bound / error):
  test_bn_layers            bnf mean   2.8e-08 | 2.7e-08 | 1.7e-07 | x6.0     bnf rstd       1.1e-06 | 1.9e-06 | 9.6e-06 | x9.1
                            bnb m(dy)  1.8e-11 | 2.3e-11 | 9.4e-11 | x5.3     bnb m(dy xhat) 3.6e-11 | 2.9e-11 | 1.5e-10 | x4.1
                            (b) act 1.82e-06, pre-activations 1.48e-06 of 2e-06; (c) no gate differs; (d) dz 6.0e-06 of 1e-05
  test_mnist_tail_...       bnf mean   1.9e-08 | 2.8e-08 | 1.4e-07 | x7.3     bnf rstd       1.5e-06 | 2.6e-06 | 1.4e-05 | x9.4
                            bnb m(dy)  1.7e-11 | 1.8e-11 | 1.0e-10 | x6.0     bnb m(dy xhat) 2.0e-11 | 1.9e-11 | 8.5e-11 | x4.2
                            (b) act 1.43e-06, pre 1.34e-06; (c) 1 gate differs, |bn| 3.4e-08; (d) dz 2.0e-06 (both calls)
  test_close_rows           bnf mean   5.4e-08 | 6.0e-08 | 3.0e-07 | x5.6     bnf rstd       1.9e-05 | 3.1e-05 | 1.5e-04 | x8.3 (rstd ~ 230)
                            normalised output 1.7e-05 | 1.9e-05 | 7.7e-05 | x4.5
  test_degenerate_channels  bnf mean   2.2e-08 | 2.9e-08 | 1.5e-07 | x6.5     bnf rstd       1.5e-06 | 2.1e-06 | 1.1e-05 | x7.0
                            bnb m(dy)  3.2e-11 | 3.9e-11 | 1.6e-10 | x4.8     bnb m(dy xhat) 6.9e-11 | 4.4e-11 | 2.4e-10 | x3.4
                            (b) act 1.73e-06, pre 1.60e-06; (c) no gate differs; (d) dz 5.6e-06
  end-to-end y (plausibility bound, _full_case): 2.2e-05 of 4.8e-05 at worst.
Before the block sums were taken about the block mean, E[x^2] - mean^2 from float32 block sums gave bnf0 rstd errors of 1.1e-3
(spread 1e-2) to 2.4e-3 (1e-3, 1e-4) RELATIVE in a numpy model of the device's form (8e-8 .. 1e-10 after; float32 two-pass 1.2e-7);
with the sums taken of the accumulator instead of the stored value the device measured 3.4e-04 absolute against a bound of 1.4e-04
at spread 1e-2 (the rounding of accumulator + bias enters the variance of the stored floats through its cross term)."""

import numpy as np
import pytest

from defensegan_amd import archs, synth
from tests.helpers import make_gan
from tests.support import bn_reference as BR

pytestmark = pytest.mark.gpu


def _targets(arch, B, seed):
    a = archs.make_arch(arch)
    rs = np.random.RandomState(seed)
    return (rs.rand(B, *a.image_dim) * (a.in_hi - a.in_lo) + a.in_lo).astype(np.float32)


def _weights(arch, mutate=None):
    p = synth.make_weights(arch, seed=1234, gain=2.0, bias_range=0.1, use_bn=True, bn_jitter=0.2)
    if mutate:
        p = {k: np.array(v) for k, v in p.items()}
        mutate(p)
    return p


def _gan(arch, p, opts):
    gan, _ = make_gan(arch, gain=2.0, bias_range=0.1, use_bn=True)
    assert gan.set_weights(p) == []
    for k, v in opts.items():
        gan.set_option(k, v)
    return gan


_REF = {}


def _reference(key, p, arch, z, x, R):
    """Float64 forward from z (computed once per input set, shared by the bn_fused settings; never modified)."""
    if key not in _REF:
        fwd = BR.generator_forward(p, z.astype(np.float64), arch)
        loss, dy = BR.loss_and_dy(fwd["y"], x, R)
        _REF[key] = (fwd, loss, dy)
    return _REF[key]


def _read(gan, name, shape):
    n = int(np.prod(shape))
    t = gan.debug_read(name, n)
    assert t.numel() == n, (name, t.numel(), n)
    return t.cpu().numpy().reshape(shape)


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _stat_check(what, dev, ref, yard, report):
    """|dev - ref| <= 4 * max|yard - ref| + 2 ulp(ref), per channel."""
    dev, ref, yard = (np.asarray(v, np.float64).reshape(-1) for v in (dev, ref, yard))
    y = float(np.abs(yard - ref).max())
    bound = 4.0 * y + 2.0 * _ulp(ref)
    err = np.abs(dev - ref)
    k = int(np.argmax(err / bound))
    report.append("%s: device err %.3g (channel %d, value %.4g), float32 two-pass err %.3g, bound %.3g, margin x%.1f"
                  % (what, err[k], k, ref[k], y, bound[k], min(bound[k] / max(err[k], 1e-300), 9999.0)))
    assert np.isfinite(dev).all(), what
    assert (err <= bound).all(), report[-1]


def _forward_checks(gan, p, arch, z, report, rel_tol=2e-6, close_rows=False):
    """(a) forward statistics, (b) layer outputs, (c) gates.  Returns the device's activations (full stored maps).
    close_rows: rule (a) for the layer output too -- relu(bn(.)) of the device's pre-activations in float64, bound 4 x the error
    of the float32 two-pass form + 2 ulp (with rstd up to 1 / sqrt(eps) = 316 one ulp of ANY float32 mean shows in the output)."""
    names = BR.bn_names(arch)
    acts, prev = [], z
    y = gan.generate(z)
    N = len(z)
    for d, bn in enumerate(names):
        pre64 = BR.layer_pre(p, arch, d, prev)                                   # from the device's previous activation
        shape = pre64.shape
        pre = _read(gan, "bnpre%d" % d, shape)
        Cn = shape[-1]
        fst = _read(gan, "bnf%d" % d, (2, Cn))
        r = BR.layer_forward(pre, p[bn + ".scale"], p[bn + ".offset"])           # (a): from the device's own floats
        m32, _, r32 = BR.moments_f32(pre)
        _stat_check("bnf%d mean" % d, fst[0], r["mean"], m32, report)
        _stat_check("bnf%d rstd" % d, fst[1], r["rstd"], r32, report)
        act = _read(gan, "act%d" % d, shape)
        if close_rows:
            sc, of = p[bn + ".scale"].astype(np.float32), p[bn + ".offset"].astype(np.float32)
            out32 = np.maximum(((pre - m32) * r32) * sc + of, np.float32(0))
            _stat_check("act%d (normalised output)" % d, act, r["out"], out32, report)
            acts.append(act.reshape(N, 4, 4, -1) if d == 0 else act)
            prev = acts[-1]
            continue
        r64 = BR.layer_forward(pre64, p[bn + ".scale"], p[bn + ".offset"])       # (b): teacher-forced float64 layer
        rel = float(np.abs(act - r64["out"]).max() / (np.abs(r64["out"]).max() + 1e-30))
        relp = float(np.abs(pre - pre64).max() / (np.abs(pre64).max() + 1e-30))
        report.append("act%d: rel err %.3g (pre-activations %.3g), tolerance %.1g" % (d, rel, relp, rel_tol))
        assert rel < rel_tol and relp < rel_tol, report[-1]            # (the producing GEMM's output itself, and the layer's)
        flip = (act > 0) != (r64["bn"] > 0)                                      # (c)
        worst = float(np.abs(r64["bn"][flip]).max()) if flip.any() else 0.0
        report.append("act%d: %d of %d gates differ from float64, largest |bn| there %.3g (< 1e-5)" % (d, int(flip.sum()), flip.size, worst))
        assert worst < 1e-5, report[-1]
        act = act.reshape(N, 4, 4, -1) if d == 0 else act
        acts.append(act)
        prev = act
    return acts, np.asarray(y)


def _backward_stat_checks(gan, p, arch, acts, layers_to_check, report):
    """(a) for the backward sums, from the device's da (see the module docstring).  Call right after a backward pass."""
    names = BR.bn_names(arch)
    for d in layers_to_check:
        bn = names[d]
        shape = acts[d].shape if d else (acts[0].shape[0], acts[0].size // acts[0].shape[0])
        Cn = shape[-1]
        pre = _read(gan, "bnpre%d" % d, shape).astype(np.float64)
        fst = _read(gan, "bnf%d" % d, (2, Cn)).astype(np.float64)
        bst = _read(gan, "bnb%d" % d, (2, Cn)).astype(np.float64)
        da = _read(gan, "act%d" % d, shape).astype(np.float64)
        scale = p[bn + ".scale"].astype(np.float32).astype(np.float64)
        live = scale != 0
        xhat = (pre - fst[0]) * fst[1]
        k = np.where(live, scale * fst[1], 1.0)
        g = (da / k + bst[0] + xhat * bst[1]).astype(np.float32)                 # the device's masked dy
        g[..., ~live] = 0
        ax = tuple(range(g.ndim - 1))
        g64 = g.astype(np.float64)
        m1, m2 = g64.mean(axis=ax), (g64 * xhat).mean(axis=ax)
        y1, y2 = BR.backward_sums_f32(g, xhat)
        _stat_check("bnb%d mean(dy)" % d, bst[0][live], m1[live], y1[live], report)
        _stat_check("bnb%d mean(dy xhat)" % d, bst[1][live], m2[live], y2[live], report)


def _dz_check(what, dz, p, fwd, dy, arch, acts, report, tol=1e-5, ref=None):
    """(d): every row, against the float64 backward run with the device's gates."""
    if ref is None:
        ref = BR.generator_backward(p, fwd, dy, arch, [a > 0 for a in acts])
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(dz, np.float64) - ref).max(axis=1) / (scale + 1e-300)
    report.append("%s: worst row %.3g of max|dz| = %.3g (gate %.1g)" % (what, err.max(), scale, tol))
    assert np.isfinite(np.asarray(dz)).all()
    assert (err < tol).all(), report[-1]
    return ref


def _inputs(arch, rows, seed):
    a = archs.make_arch(arch)
    R = 1 if rows % 10 else 10
    rs = np.random.RandomState(seed)
    z = (rs.standard_normal((rows, a.latent_dim)) * 0.3).astype(np.float32)
    return z, _targets(arch, rows // R, seed + 1), R


def _full_case(arch, p, z, x, R, opts, key, report, bwd_layers=None):
    gan = _gan(arch, p, opts)
    fwd, loss64, dy = _reference(key, p, arch, z, x, R)
    acts, y = _forward_checks(gan, p, arch, z, report)
    # End to end (not teacher-forced; not asked for by (a) - (d), kept as a plausibility bound): every layer may add its (b)
    # tolerance, 2e-6 of the float64 reference's max|output| of that layer, and is taken to hand the errors of the layers in
    # front of it on with a gain of at most 1 (Batchnorm re-normalises; sigmoid and tanh have slope <= 1)
    y_atol = 2e-6 * sum(float(np.abs(a).max()) for a in fwd["act"] + fwd["tail"])
    report.append("y: max abs err %.3g (bound %.3g)" % (float(np.abs(y - fwd["y"]).max()), y_atol))
    np.testing.assert_allclose(y, fwd["y"], rtol=0, atol=y_atol)
    y2, loss, dz = gan.loss_grad(x, z)
    np.testing.assert_allclose(y2, fwd["y"], rtol=0, atol=y_atol)
    np.testing.assert_allclose(loss, loss64, rtol=5e-5)
    _backward_stat_checks(gan, p, arch, acts, range(len(acts)) if bwd_layers is None else bwd_layers, report)
    ref = _dz_check("dz", dz, p, fwd, dy, arch, acts, report)
    return gan, acts, fwd, dy, ref


CASES = [(a, r, (0, 1, 2)) for a, r in (("mnist", 7), ("mnist", 40), ("mnist", 48), ("mnist", 176), ("mnist", 33), ("mnist", 47),
                                        ("celeba", 9), ("celeba", 33))]


@pytest.mark.parametrize("arch,rows,fused", [(a, r, f) for a, r, fs in CASES for f in fs])
def test_bn_layers(arch, rows, fused):
    """(a) - (d) on ordinary inputs (z = 0.3 * N(0, 1)) at the row counts of the module docstring's route table."""
    report = []
    try:
        z, x, R = _inputs(arch, rows, 100 + rows)
        _full_case(arch, _weights(arch), z, x, R, {"bn_fused": fused}, (arch, rows), report)
    finally:
        print("\n[%s rows %d bn_fused %d]\n  " % (arch, rows, fused) + "\n  ".join(report))


@pytest.mark.parametrize("pipe,rows", [(8, 16), (8, 33), (8, 48), (256, 600)])
def test_mnist_tail_batchnorm_form(pipe, rows):
    """(e) mnist_tail_pipe3_kernel<64, true>: a dz-only dg_loss_grad with bn_fused = 2 and rows >= 2 * tail_pipe applies
    relu(bn(.)) of the last Batchnorm layer inside the tail and leaves that layer's backward sums, one record per workgroup.
    The all-outputs call before it (first-generation tail, activation image written) gives the gates; both dz meet (d), the
    last layer's bnb of the dz-only call meets (a)."""
    import torch
    report = []
    try:
        z, x, R = _inputs("mnist", rows, 300 + rows)
        p = _weights("mnist")
        gan, acts, fwd, dy, ref = _full_case("mnist", p, z, x, R, {"bn_fused": 2, "tail_pipe": pipe}, ("mnist-tail", rows), report)
        xd, zd = torch.as_tensor(x).cuda(), torch.as_tensor(z).cuda()
        dz = torch.full_like(zd, float("nan"))
        gan._check(gan._lib().dg_loss_grad(gan._handle, xd.data_ptr(), zd.data_ptr(), rows // R, R, None, None, dz.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        _backward_stat_checks(gan, p, "mnist", acts, [2, 1, 0], report)
        _dz_check("dz (dz-only call)", dz.cpu().numpy(), p, fwd, dy, "mnist", acts, report, ref=ref)
    finally:
        print("\n[tail_pipe %d rows %d]\n  " % (pipe, rows) + "\n  ".join(report))


@pytest.mark.parametrize("arch", ["mnist", "celeba"])
@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("spread", [1e-1, 1e-2, 1e-3, 1e-4, 0.0, None])
def test_close_rows(arch, fused, spread):
    """(f) the R restarts of ONE image late in a projection: B = 1, R = 10, z = z0 + spread * noise (spread 0: ten identical rows;
    None: a single row, variance exactly 0 in BN1: rstd = 1 / sqrt(eps), y finite, dz = 0 as the reference gives).  Statistics and
    the normalised output of every Batchnorm layer under rule (a); dz is not compared (ill-conditioned: rstd = 316 amplifies
    the last bit of mean(dy)).  BN1's variance
    is then small against mean^2: a float32 sum of x^2 cannot resolve it (E[x^2] - mean^2 from float32 block sums was wrong by up
    to 3e-3 in rstd here); the block sums are taken about each block's own mean and merged in float64 instead."""
    report = []
    try:
        a = archs.make_arch(arch)
        rs = np.random.RandomState(7)
        z0 = (rs.standard_normal((1, a.latent_dim)) * 0.3).astype(np.float32)
        R = 1 if spread is None else 10
        z = (z0 + (spread or 0.0) * rs.standard_normal((R, a.latent_dim))).astype(np.float32)
        x = _targets(arch, 1, 8)
        p = _weights(arch)
        gan = _gan(arch, p, {"bn_fused": fused})
        _forward_checks(gan, p, arch, z, report, close_rows=True)
        if spread is None:
            np.testing.assert_allclose(_read(gan, "bnf0", (2, 4096))[1], 1.0 / np.sqrt(1e-5), rtol=3e-7)
            y, loss, dz = gan.loss_grad(x, z)
            assert np.isfinite(np.asarray(y)).all() and np.isfinite(np.asarray(loss)).all()
            assert np.abs(np.asarray(dz)).max() == 0.0
    finally:
        print("\n[%s close rows spread %s bn_fused %d]\n  " % (arch, spread, fused) + "\n  ".join(report))


def _degenerate(kind, layer):
    def mutate(p):
        F = p[layer + ".Filters"]                                   # [5, 5, Cout, Cin]
        bn = {"Generator.2": "Generator.BN2", "Generator.3": "Generator.BN3"}[layer]
        if kind == "zero_filter":
            F[:, :, 3, :] = 0.0                                     # variance 0: the output is the offset
        elif kind == "one_signed":
            F[:, :, 3, :] = np.abs(F[:, :, 3, :])                   # inputs are >= 0 (ReLU): mean ~ 2.4 x spread of the channel
        else:
            p[bn + ".scale"][3] = 0.0
    return mutate


@pytest.mark.parametrize("arch,rows", [("mnist", 40), ("celeba", 9)])
@pytest.mark.parametrize("layer", ["Generator.2", "Generator.3"])
@pytest.mark.parametrize("kind", ["zero_filter", "one_signed", "scale_zero"])
def test_degenerate_channels(arch, rows, layer, kind):
    """(g) one output channel with an all-zero filter, with one-signed taps, or with scale = 0; default bn_fused.  (a), (b), (d)."""
    report = []
    try:
        z, x, R = _inputs(arch, rows, 500 + rows)
        p = _weights(arch, _degenerate(kind, layer))
        gan, acts, fwd, dy, _ = _full_case(arch, p, z, x, R, {}, (arch, rows, layer, kind), report)
        if kind == "zero_filter":
            d = 1 if layer == "Generator.2" else 2
            bn = BR.bn_names(arch)[d]
            np.testing.assert_array_equal(acts[d][..., 3], np.maximum(p[bn + ".offset"][3], 0).astype(np.float32))
    finally:
        print("\n[%s %s %s]\n  " % (arch, layer, kind) + "\n  ".join(report))


# ---- seeded latents -------------------------------------------------------------------------------------------------------------
def _host_latents(n_rows, latent, seed, first_row, std):
    """init_latents_kernel restated: Philox4x32-10, counter (row lo, row hi, column / 4, 0), key (seed lo, seed hi); uniforms
    (x + 1) * 2^-32 and the angle 2 pi u in float32 as the kernel forms them, Box-Muller itself in float64."""
    from tests.support.train_reference import philox4x32_10
    q = latent // 4
    ctr = np.zeros((n_rows * q, 4), np.uint64)
    grow = np.array([first_row + i for i in range(n_rows)], dtype=np.uint64)
    ctr[:, 0] = np.repeat(grow & np.uint64(0xFFFFFFFF), q)
    ctr[:, 1] = np.repeat(grow >> np.uint64(32), q)
    ctr[:, 2] = np.tile(np.arange(q, dtype=np.uint64), n_rows)
    w = np.asarray(philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)), np.uint64).reshape(-1, 4)
    u = np.minimum((w.astype(np.float32) + np.float32(1.0)) * np.float32(2.3283064365386963e-10), np.float32(1.0))
    t = (np.float32(6.283185307179586) * u[:, [1, 3]]).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u[:, [0, 2]].astype(np.float64))) * std
    out = np.stack([r[:, 0] * np.cos(t[:, 0]), r[:, 0] * np.sin(t[:, 0]), r[:, 1] * np.cos(t[:, 1]), r[:, 1] * np.sin(t[:, 1])], axis=1)
    return out.reshape(n_rows, latent)


@pytest.mark.parametrize("latent", [64, 128, 192])
def test_seeded_latents_value_for_value(latent):
    """dg_init_latents against the host restatement (abs 2e-6 * std: float32 logf / sqrtf / cosf / sinf on |values| up to ~6 std)
    for seeds and first rows that use the high words of the key and of the counter; seeds that differ only in the high word
    give different rows."""
    from defensegan_amd.gan import dataset_gan_dict
    gan = dataset_gan_dict["mnist"](cfg={"USE_BN": False, "LATENT_DIM": latent, "NET_DIM": 64}, test_mode=True)
    std, n = 0.5, 6
    seen = {}
    for seed in (5, 2 ** 32 + 5, 2 ** 63 + 5):
        for first_row in (0, 2 ** 32 - 3, 2 ** 40):
            z = gan.init_latents(n, seed=seed, first_row=first_row, std=std).cpu().numpy()
            ref = _host_latents(n, latent, seed, first_row, std)
            err = float(np.abs(z - ref).max())
            print("latent %d seed %d first_row %d: max abs err %.3g (bound %.3g)" % (latent, seed, first_row, err, 2e-6 * std))
            assert err <= 2e-6 * std, (seed, first_row, err)
            seen[(seed, first_row)] = z
    for first_row in (0, 2 ** 32 - 3, 2 ** 40):
        zs = [seen[(s, first_row)] for s in (5, 2 ** 32 + 5, 2 ** 63 + 5)]
        for i in range(3):
            for j in range(i + 1, 3):
                assert (zs[i] != zs[j]).mean() > 0.99
    # rows depend on the GLOBAL row only: the draw that crosses the 32-bit word continues the same sequence
    np.testing.assert_array_equal(seen[(5, 2 ** 32 - 3)][3:], gan.init_latents(3, seed=5, first_row=2 ** 32, std=std).cpu().numpy())
    assert not np.array_equal(seen[(5, 2 ** 32 - 3)][3:], seen[(5, 0)][:3])          # (a dropped high word would repeat rows 0..2)


# ---- selection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [65, 70, 130])
def test_selection_beyond_one_wave_of_restarts(R):
    """select_kernel's lane loop (R > 64): L = 0 with prescribed z0.  Image 0: the minimum twice, in different lanes of the same
    trip; image 1: in the same lane of different trips (r and r + 64); image 2: first in the last trip; image 3: a NaN and a +inf
    restart (rows of z0) in front of the minimum.  idx = first argmin of the returned losses (a NaN loss never wins), rec = that
    row of generate(z0), bit for bit.  (Measured: the NaN row comes back with a FINITE loss -- the ReLU epilogue's `t > 0 ? t : 0`
    sends NaN to 0 where tf.nn.relu would pass it on; noted, not in the scope of this test.)"""
    gan, p = make_gan("mnist", gain=2.0, bias_range=0.1, rec_rr=R, rec_iters=0)
    B = 4
    rs = np.random.RandomState(R)
    zt = (rs.standard_normal((B, 128)) * 0.1).astype(np.float32)
    x = np.asarray(gan.generate(zt))
    z0 = (rs.standard_normal((B, R, 128)) * 0.3 + 1.0).astype(np.float32)          # far from the targets
    near = (zt + 1e-3).astype(np.float32)                                          # the winning row of each image
    z0[0, 5] = near[0]; z0[0, 40] = near[0]
    a1 = 1 if R > 65 else 0
    z0[1, a1] = near[1]; z0[1, a1 + 64] = near[1]
    z0[2, R - 1] = near[2]
    z0[3, 0] = np.nan; z0[3, 2] = np.inf; z0[3, 64] = near[3]
    z0 = z0.reshape(B * R, 128)
    out = gan.reconstruct(x, z_init_val=z0, return_details=True)
    loss = np.asarray(out["loss"]).reshape(B, R)
    y = np.asarray(gan.generate(z0)).reshape(B, R, 28, 28, 1)
    want = np.array([int(np.flatnonzero(l == np.nanmin(l))[0]) for l in loss])
    assert want.tolist() == [5, a1, R - 1, 64], (want, loss[3, :4])
    assert not (loss[3, 0] < loss[3, 64]) and not (loss[3, 2] < loss[3, 64])
    assert np.asarray(out["idx"]).tolist() == want.tolist()
    for b in range(B):
        assert np.array_equal(np.asarray(out["rec"])[b], y[b, want[b]])
