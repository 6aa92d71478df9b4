"""-m "not gpu": the float64 critic reference checks itself (central differences, a hand-computed penalty, the two penalty axes, the
closed-form double backward against autograd), and the host side of the critic that needs no device (the model's layers, shapes,
names and initial values; the NotImplementedError and argument paths)."""
import numpy as np
import pytest

from defensegan_amd import _native, critic as K
from defensegan_amd import network_builder as nb
from tests.support import critic_reference as R


def _setup(net_dim=2, B=3, seed=0, shape=(28, 28, 1), critic=None):
    c = critic or K.mnist_discriminator(net_dim=net_dim, input_shape=(None,) + shape)
    w = c.tflib_init(seed)
    rs = np.random.RandomState(seed + 1)
    for _, bn in c.param_names:
        w[bn] = rs.uniform(-0.1, 0.1, w[bn].shape).astype(np.float32)
    params = [(w[a].astype(np.float64), w[b].astype(np.float64)) for a, b in c.param_names]
    real, fake = rs.uniform(0, 1, (B,) + shape), rs.uniform(0, 1, (B,) + shape)
    return c, R.describe(c), params, (real, fake, rs.uniform(0, 1, B))


@pytest.mark.parametrize("axes", [0, 1])
def test_reference_gradient_against_central_differences(axes):
    _, layers, params, batch = _setup(net_dim=2, seed=axes)
    assert R.margin(layers, params, *batch) > 1e-4                      # the steps below cross no kink
    _, grads, _ = R.param_gradient(layers, params, *batch, lam=10.0, axes=axes)
    rs, h = np.random.RandomState(5), 1e-6
    for i, (pair, gpair) in enumerate(zip(params, grads)):
        for k in range(2):
            for _ in range(4):
                idx = tuple(rs.randint(0, n) for n in pair[k].shape)
                vals = []
                for sgn in (1, -1):
                    q = [[W.copy(), b.copy()] for W, b in params]
                    q[i][k][idx] += sgn * h
                    vals.append(R.cost_of(layers, [tuple(t) for t in q], *batch, lam=10.0, axes=axes))
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - gpair[k][idx]) <= 1e-6 * max(1.0, np.abs(gpair[k]).max()), (i, k, idx, fd, gpair[k][idx])


def test_hand_computed_penalty_on_a_one_convolution_critic():
    """D(x) = sum over the 2 x 2 x 1 outputs of a 1x1 convolution with kernel k (no activation): g = k everywhere.  On a 4 x 3 x 1
    input of stride 1 the column norm is sqrt(4) |k| and the image norm sqrt(12) |k|, whatever the inputs are."""
    k = 0.3
    c = K.Critic([nb.Conv2D(1, (1, 1), (1, 1), "SAME"), nb.Flatten(), nb.Linear(1)], (None, 4, 3, 1), [("f", "fb"), ("w", "wb")])
    params = [(np.full((1, 1, 1, 1), k), np.zeros(1)), (np.ones((12, 1)), np.zeros(1))]
    rs = np.random.RandomState(0)
    real, fake, alpha = rs.uniform(0, 1, (2, 4, 3, 1)), rs.uniform(0, 1, (2, 4, 3, 1)), rs.uniform(0, 1, 2)
    for axes, s in ((0, 2 * k), (1, np.sqrt(12) * k)):
        (cost, w, P), grads, slopes = R.param_gradient(R.describe(c), params, real, fake, alpha, lam=10.0, axes=axes)
        assert slopes.shape == ((2, 3, 1) if axes == 0 else (2,))
        np.testing.assert_allclose(slopes, s, rtol=1e-12)
        assert abs(P - (s - 1) ** 2) <= 1e-12 and abs(w - k * (fake.sum() - real.sum()) / 2) <= 1e-12
        assert abs(cost - (w + 10 * P)) <= 1e-12
        # dP/dk = 2 (s - 1) ds/dk, ds/dk = s / k; the Wasserstein part adds (sum fake - sum real) / B
        want = 10 * 2 * (s - 1) * s / k + (fake.sum() - real.sum()) / 2
        assert abs(grads[0][0].item() - want) <= 1e-10


def test_the_two_penalty_axes_differ_and_match_their_formulas():
    import torch
    _, layers, params, (real, fake, alpha) = _setup(net_dim=2, seed=3)
    xhat = torch.tensor(real + alpha.reshape(-1, 1, 1, 1) * (fake - real), requires_grad=True)
    (g,) = torch.autograd.grad(R.forward(layers, R.as_params(params), xhat).sum(), xhat)
    g = g.numpy()
    t0, _, s0 = R.param_gradient(layers, params, real, fake, alpha, axes=0)
    t1, _, s1 = R.param_gradient(layers, params, real, fake, alpha, axes=1)
    np.testing.assert_allclose(s0, np.sqrt((g ** 2).sum(axis=1)), rtol=1e-12)           # over H alone: [B, W, C]
    np.testing.assert_allclose(s1, np.sqrt((g ** 2).sum(axis=(1, 2, 3))), rtol=1e-12)   # over the image: [B]
    assert abs(t0[2] - ((s0 - 1) ** 2).mean()) <= 1e-12 and abs(t1[2] - ((s1 - 1) ** 2).mean()) <= 1e-12
    assert t0[1] == t1[1] and abs(t0[2] - t1[2]) > 1e-3
    # a zero-gradient column takes s = 0 and a zero penalty gradient, not TF's NaN
    s = R.slopes_of(torch.zeros(1, 3, 2, 1, dtype=torch.float64, requires_grad=True), 0)
    assert float(s.detach().sum()) == 0.0
    (gz,) = torch.autograd.grad(((R.slopes_of(xz := torch.zeros(1, 3, 2, 1, dtype=torch.float64, requires_grad=True), 0) - 1) ** 2).sum(), xz)
    assert not gz.numpy().any()


@pytest.mark.parametrize("axes", [0, 1])
def test_the_derivation_equals_autograd(axes):
    """lambda dP/dC_j = wgrad(u_{j-1}, a_j) with v = dP/dg, frozen slopes, a bias-free tangent pass: equal to the double backward."""
    _, layers, params, batch = _setup(net_dim=3, B=4, seed=7)
    _, full, _ = R.param_gradient(layers, params, *batch, lam=10.0, axes=axes)
    _, wass, _ = R.param_gradient(layers, params, *batch, lam=0.0, axes=axes)
    derived = R.derived_gradient(layers, params, *batch, lam=10.0, axes=axes)
    for (fW, fb), (wW, wb), (dW, db) in zip(full, wass, derived):
        assert np.abs(fW - wW - dW).max() <= 1e-12 * max(1.0, np.abs(fW).max())
        assert np.abs(fb - wb).max() == 0.0 and not db.any()                # the penalty has no bias gradient


def test_mnist_discriminator_layers_shapes_and_names():
    c = K.mnist_discriminator()
    kinds = [l.__class__.__name__ for l in c.layers]
    assert kinds == ["Conv2D", "LeakyReLU", "Conv2D", "LeakyReLU", "Conv2D", "LeakyReLU", "Flatten", "Linear"]
    assert [l.output_channels for l in c.layers if isinstance(l, nb.Conv2D)] == [128, 256, 512]
    assert all(l.kernel_shape == (5, 5) and l.strides == (2, 2) and l.padding == "SAME" for l in c.layers if isinstance(l, nb.Conv2D))
    assert nb.KIND["LeakyReLU"] == 6 and nb.LeakyReLU().spec()[0] == 6
    shape = (28, 28, 1)
    sizes = []
    for l in c.layers:
        if isinstance(l, nb.Conv2D):
            shape = nb.conv_output_shape(shape, l)
            sizes.append(shape[0])
    assert sizes == [14, 7, 4]
    assert c.param_names == [("Discriminator.1.Filters", "Discriminator.1.Biases"), ("Discriminator.2.Filters", "Discriminator.2.Biases"),
                             ("Discriminator.3.Filters", "Discriminator.3.Biases"), ("Discriminator.Output.W", "Discriminator.Output.b")]
    assert c.named_shapes() == {"Discriminator.1.Filters": (5, 5, 1, 128), "Discriminator.1.Biases": (128,),
                                "Discriminator.2.Filters": (5, 5, 128, 256), "Discriminator.2.Biases": (256,),
                                "Discriminator.3.Filters": (5, 5, 256, 512), "Discriminator.3.Biases": (512,),
                                "Discriminator.Output.W": (4 * 4 * 4 * 128, 1), "Discriminator.Output.b": (1,)}
    assert c.layer_names[-1] == "logits"
    out = R.discriminate(R.describe(K.mnist_discriminator(net_dim=2)), [(v[0], v[1]) for v in _setup(net_dim=2)[2]], np.zeros((5, 28, 28, 1)))
    assert out.shape == (5,)


def test_initial_weights_follow_tflib():
    c = K.mnist_discriminator(net_dim=64)
    w = c.tflib_init(seed=3)
    # Conv2D: he_init, stdev = sqrt(4 / (fan_in + fan_out)), fan_in = cin k^2, fan_out = cout k^2 / stride^2
    for name, cin, cout in (("Discriminator.2.Filters", 64, 128), ("Discriminator.3.Filters", 128, 256)):
        sd = np.sqrt(4.0 / (cin * 25 + cout * 25 / 4.0))
        assert abs(K.tflib_conv_stdev(cin, cout, 5, 2) - sd) <= 1e-15
        v = w[name]
        assert v.dtype == np.float32 and abs(v.std(ddof=1) / sd - 1) < 0.01          # >= 2e5 uniform samples: 0.2 % expected
        assert np.abs(v).max() <= sd * np.sqrt(3) and np.abs(v).max() > 0.99 * sd * np.sqrt(3)
    sd = np.sqrt(2.0 / (4096 + 1))
    assert abs(w["Discriminator.Output.W"].std(ddof=1) / sd - 1) < 0.05
    assert all(not w[b].any() for _, b in c.param_names)
    again = c.tflib_init(seed=3)
    assert all(np.array_equal(w[k], again[k]) for k in w) and not np.array_equal(w["Discriminator.1.Filters"], c.tflib_init(4)["Discriminator.1.Filters"])


def test_adam_restatement_is_tf_adam():
    rs = np.random.RandomState(0)
    p, g, m, v = rs.randn(5), rs.randn(5), rs.randn(5) * 0.1, rs.rand(5) * 0.01
    q, m2, v2 = R.adam_update(p, g, m, v, 3, 1e-4, 0.5, 0.9)
    np.testing.assert_allclose(m2, 0.5 * m + 0.5 * g, rtol=1e-15)
    np.testing.assert_allclose(v2, 0.9 * v + 0.1 * g * g, rtol=1e-14)
    np.testing.assert_allclose(q, p - 1e-4 * np.sqrt(1 - 0.9 ** 3) / (1 - 0.5 ** 3) * m2 / (np.sqrt(v2) + 1e-8), rtol=1e-15)


def test_not_implemented_and_argument_paths():
    from defensegan_amd.gan import CelebADefenseGAN, MnistDefenseGAN
    with pytest.raises(NotImplementedError, match="Batchnorm critic"):
        K.mnist_discriminator(use_bn=True)
    with pytest.raises(NotImplementedError, match="CelebA critic"):
        K.celeba_discriminator()
    g = MnistDefenseGAN(cfg={"USE_BN": False}, test_mode=True)
    assert (g.mode, g.gradient_penalty_lambda, g.critic_iters) == ("wgan-gp", 10.0, 5)          # the reference's defaults
    g = MnistDefenseGAN(cfg={"USE_BN": False, "MODE": "wgan-gp", "GRADIENT_PENALTY_LAMBDA": 5.0, "CRITIC_ITERS": 2, "BATCH_SIZE": 4}, test_mode=True)
    assert (g.gradient_penalty_lambda, g.critic_iters) == (5.0, 2)
    x = np.zeros((8, 28, 28, 1), np.float32)
    with pytest.raises(NotImplementedError, match="generator step"):
        g.train(x, phase=None)
    sched = g.critic_schedule(10, 5, seed=1)
    assert sched.shape == (5, 4) and len(set(sched[:2].reshape(-1).tolist())) == 8 and np.array_equal(sched, g.critic_schedule(10, 5, seed=1))
    with pytest.raises(ValueError, match="do not fill one batch"):
        g.critic_schedule(3, 1, seed=1)
    for mode in ("wgan", "dcgan"):
        h = MnistDefenseGAN(cfg={"USE_BN": False, "MODE": mode}, test_mode=True)
        with pytest.raises(NotImplementedError, match="only 'wgan-gp'"):
            h.train(x, phase="disc")
        with pytest.raises(NotImplementedError, match="only 'wgan-gp'"):
            h.discriminator_cost(x)
    with pytest.raises(NotImplementedError, match="Batchnorm critic"):
        MnistDefenseGAN(cfg={"USE_BN": True}, test_mode=True).critic
    with pytest.raises(NotImplementedError, match="CelebA critic"):
        CelebADefenseGAN(cfg={"USE_BN": False}, test_mode=True).critic
    assert K.penalty_axes_id("reference") == 0 and K.penalty_axes_id("image") == 1 and K.penalty_axes_id(1) == 1
    for bad in ("height", 2, True, 0.0):
        with pytest.raises(ValueError, match="penalty_axes"):
            K.penalty_axes_id(bad)
    c = K.mnist_discriminator(net_dim=2)
    with pytest.raises(ValueError, match="lack"):
        c.set_named_weights({"Discriminator.1.Filters": np.zeros((5, 5, 1, 2))})
    bad = c.tflib_init(0)
    bad["Discriminator.Output.W"] = np.zeros((3, 1), np.float32)
    with pytest.raises(ValueError, match="Discriminator.Output.W: shape"):
        c.set_named_weights(bad)


def test_binding_declares_the_critic_symbols():
    names = {n for n, _, _ in _native.SYMBOLS}
    assert {"dg_critic_gradient", "dg_critic_step", "dg_clf_set_adam"} <= names and _native.ABI_VERSION == 2
    lib = _native.load()
    assert lib.dg_critic_gradient(None, None, None, None, 1, 10.0, 0, None, None, None, None) == -1       # DG_E_INVALID before any HIP call
    assert lib.dg_critic_step(None, None, None, None, 1, 10.0, 0, 1e-4, 1.5, 0.9, None, None) == -1
    assert b"betas" in lib.dg_last_error()
