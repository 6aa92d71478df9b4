"""The float64 Batchnorm reference of tests/support/bn_reference.py against the NumPy oracle and torch autograd (no GPU)."""
import numpy as np
import pytest

from defensegan_amd import archs, synth
from oracle import defensegan_oracle as O
from tests.support import bn_reference as BR


def _case(arch, N, seed, spread=0.3):
    p = synth.make_weights(arch, seed=1234, gain=2.0, bias_range=0.1, use_bn=True, bn_jitter=0.2)
    a = archs.make_arch(arch)
    rs = np.random.RandomState(seed)
    z = (rs.standard_normal((N, a.latent_dim)) * spread).astype(np.float32).astype(np.float64)
    x = rs.rand(N, *a.image_dim) * (a.in_hi - a.in_lo) + a.in_lo
    return p, z, x


def test_layer_form_equals_the_oracle():
    rs = np.random.RandomState(0)
    pre = rs.standard_normal((5, 6, 6, 8)) * 3 + 1
    scale, offset = rs.rand(8) + 0.5, rs.standard_normal(8)
    r = BR.layer_forward(pre, scale, offset)
    bo, (xh, rstd) = O.batchnorm_fwd(pre, scale, offset, (0, 1, 2))
    np.testing.assert_allclose(r["bn"], bo, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r["xhat"], xh, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r["rstd"], rstd.reshape(-1), rtol=1e-14)
    np.testing.assert_allclose(r["var"], pre.var(axis=(0, 1, 2)), rtol=1e-13)        # biased
    dy = rs.standard_normal(pre.shape)
    gate = r["out"] > 0
    m1, m2, da = BR.layer_backward(dy, gate, r["xhat"], r["rstd"], scale)
    np.testing.assert_allclose(da, O.batchnorm_bwd(dy * gate, scale, (xh, rstd), (0, 1, 2)), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(m1, (dy * gate).mean(axis=(0, 1, 2)), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(m2, (dy * gate * xh).mean(axis=(0, 1, 2)), rtol=1e-13, atol=1e-15)
    # the float32 two-pass form is a float32 rounding of the same numbers
    m32, v32, r32 = BR.moments_f32(pre.astype(np.float32))
    r = BR.layer_forward(pre.astype(np.float32), scale, offset)
    np.testing.assert_allclose(m32, r["mean"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r32, r["rstd"], rtol=2e-6)
    assert m32.dtype == np.float32 and v32.dtype == np.float32 and r32.dtype == np.float32


@pytest.mark.parametrize("arch,N", [("mnist", 5), ("celeba", 3)])
def test_prescribed_gate_backward_equals_the_oracle_and_autograd(arch, N):
    import torch
    from oracle import torch_ref as T
    p, z, x = _case(arch, N, 3)
    fwd = BR.generator_forward(p, z, arch)
    yo, cache = O.generator_forward(p, z, arch, True)
    np.testing.assert_allclose(fwd["y"], yo, rtol=1e-12, atol=1e-13)
    loss, dy = BR.loss_and_dy(fwd["y"], x, 1)
    gates = BR.own_gates(fwd)
    dz = BR.generator_backward(p, fwd, dy, arch, gates)
    go = O.generator_backward(p, cache, dy, arch, True)
    np.testing.assert_allclose(dz, go, rtol=1e-10, atol=1e-14 * np.abs(go).max())
    # torch autograd, float64
    g = T.TorchGenerator(p, arch, True, torch.float64)
    zt = torch.from_numpy(z).requires_grad_(True)
    yt = g.forward(zt)
    lt = ((yt - torch.from_numpy(x)) ** 2).reshape(N, -1).mean(dim=1)
    lt.sum().backward()
    np.testing.assert_allclose(loss, lt.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(dz, zt.grad.numpy(), rtol=1e-9, atol=1e-12 * np.abs(go).max())
    # a prescribed gate is really what is used: flipping one changes the result
    gates[1] = gates[1].copy()
    gates[1].flat[0] ^= True
    assert np.abs(BR.generator_backward(p, fwd, dy, arch, gates) - dz).max() > 0


def test_teacher_forced_layer_and_single_row():
    p, z, x = _case("mnist", 4, 5)
    fwd = BR.generator_forward(p, z, "mnist")
    for d in range(3):
        prev = z if d == 0 else fwd["act"][d - 1]
        np.testing.assert_array_equal(BR.layer_pre(p, "mnist", d, prev), fwd["pre"][d])
    # one row: BN1's variance is exactly 0 (rstd = 1/sqrt(eps)), y finite, dz = 0
    f1 = BR.generator_forward(p, z[:1], "mnist")
    assert (f1["bn"][0]["var"] == 0).all() and np.allclose(f1["bn"][0]["rstd"], 1 / np.sqrt(1e-5))
    assert np.isfinite(f1["y"]).all()
    _, dy = BR.loss_and_dy(f1["y"], x[:1], 1)
    assert np.abs(BR.generator_backward(p, f1, dy, "mnist", BR.own_gates(f1))).max() == 0.0
