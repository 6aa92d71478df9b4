"""-m gpu: the WGAN-GP critic on the device (DG_LAYER_LEAKY_RELU, dg_critic_gradient, dg_critic_step, gan.train(phase=...)) against
the float64 restatement in tests/support/critic_reference.py, whose penalty gradient is autograd's double backward.

Tolerances are the project's (tests/test_gpu_train.py, tests/test_gpu_train_shapes.py): every gradient tensor within 1e-4 of its own
reference's largest entry, 1e-5 relative on a cost term, 1e-6 on an Adam step, 1e-2 relative along a 30-step trajectory.  The
slopes s are norms of input-gradient entries and take the gradient tensors' bound, 1e-4 of the largest reference slope.  Inputs are
redrawn (critic_reference.safe_batch) until every LeakyReLU input of the float64 forward is 1e-6 from zero: closer than that,
float32 and float64 may decide a slope differently and the comparison says nothing (DESIGN.md section 7 has the same note for ReLU).
"""
import numpy as np
import pytest

from defensegan_amd import _native, critic as K
from defensegan_amd import network_builder as nb
from defensegan_amd import utils_tf
from tests.support import critic_reference as R
from tests.support.critic_cases import _check_all, _check_grads, _check_terms, _critic, _draw, _safe  # noqa: F401  (shared with test_gpu_critic_shapes.py)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------- 1. the layer kind
def test_leaky_relu_forward_backward_and_weight_gradient_with_an_exact_zero():
    """The upper half of image 0 is zero and the first convolution has zero biases, so its pre-activations there are exactly 0 on
    both sides: the value is 0 and the slope 0.2 (TF's MaximumGrad).  A slope of 1 or 0 at the tie changes the first layer's bias
    gradient and the input gradient by O(1)."""
    import torch
    c, params = _critic(net_dim=4, seed=3)
    params[0] = (params[0][0], np.zeros_like(params[0][1]))
    c.set_weights(params)
    layers = R.describe(c)
    def zero_half(batch):
        batch[0][0, :14] = 0.0
        return batch

    real, fake, alpha = _safe(c, params, 3, seed=5, lam=0.0, axes=(0,), change=zero_half)
    pre = []
    R.forward(layers, R.as_params(params), torch.as_tensor(real.astype(np.float64)), pre=pre)
    assert int((pre[0][0] == 0).sum()) >= 4 * 5 * 14                     # exact zeros reach the activation
    d = c.discriminate(real)
    want = R.discriminate(layers, params, real)
    assert np.abs(d - want).max() <= 1e-5 * np.abs(want).max()
    x = torch.tensor(real.astype(np.float64), requires_grad=True)
    (gx,) = torch.autograd.grad(R.forward(layers, R.as_params(params), x).sum(), x)
    got = c.backward(real, np.ones((3, 1), np.float32))
    assert np.abs(got - gx.numpy()).max() <= 1e-4 * np.abs(gx.numpy()).max()
    assert np.abs(gx.numpy()[0, :10]).max() > 0                          # the tie's slope is 0.2, not 0: gradient reaches the zero rows
    _check_all(c, params, (real, fake, alpha), lam=0.0, what="tie")
    c.close()


# ---------------------------------------------------------------------- 2. dg_critic_gradient against the reference
@pytest.mark.parametrize("B", [1, 3, 50])
def test_gradient_matches_reference_net_dim_8(B):
    c, params = _critic(net_dim=8, seed=B)
    for axes in (0, 1):
        _check_all(c, params, _safe(c, params, B, seed=10 + B), axes=axes, what="nd8 B%d axes%d" % (B, axes))
    c.close()


def test_gradient_matches_reference_net_dim_128():
    c, params = _critic(net_dim=128, seed=7)
    batch = _safe(c, params, 4, seed=NET128_SEED, axes=(0,))
    np.testing.assert_array_equal(batch[0], _draw((28, 28, 1), 4, NET128_SEED)[0])      # the first draw: no search in the test
    _check_all(c, params, batch, what="nd128")
    c.close()


NET128_SEED = 48            # the first seed from 40 that _safe accepts at net_dim 128, B = 4 (searched on the CPU)


@pytest.mark.parametrize("axes", [0, 1])
def test_gradient_on_a_nine_by_six_by_two_input(axes):
    """H = 9, W = 6, C = 2 through two SAME convolutions of stride 2: summing the columns over W instead of H, or padding an odd
    size on the wrong side, is an O(1) error in s and in every gradient."""
    c, params = _critic(small=True, seed=2)
    batch = _safe(c, params, 5, seed=77)
    _, _, slopes = _check_all(c, params, batch, axes=axes, what="9x6x2 axes%d" % axes)
    assert slopes.shape == ((5, 6, 2) if axes == 0 else (5,))
    c.close()


# ---------------------------------------------------------------------- 3. the double backward in isolation
def test_lambda_zero_is_the_wasserstein_gradient_and_equal_batches_leave_the_penalty():
    c, params = _critic(net_dim=8, seed=4)
    layers = R.describe(c)
    def one_image(batch):
        fake1 = batch[0].copy()
        fake1[2] = batch[1][2]
        return batch[0], fake1, batch[2]

    real, fake, alpha = _safe(c, params, 6, seed=21, lam=0.0, axes=(0,))
    # lambda = 0: the two-batch Wasserstein gradient (seeds +1/B on fake, -1/B on real), by plain autograd
    _, g0, _ = _check_all(c, params, (real, fake, alpha), lam=0.0, what="lambda0")
    import torch
    p = R.as_params(params, requires_grad=True)
    w = R.forward(layers, p, torch.as_tensor(fake.astype(np.float64))).mean() - R.forward(layers, p, torch.as_tensor(real.astype(np.float64))).mean()
    gw = torch.autograd.grad(w, [t for pair in p for t in pair])
    _check_grads(g0, [(gw[2 * i].numpy(), gw[2 * i + 1].numpy()) for i in range(len(p))], 6, what="wasserstein")
    # real == fake: w and its gradient vanish, the penalty alone remains and has no bias gradient
    half = torch.autograd.grad(R.forward(layers, p, torch.as_tensor(real.astype(np.float64))).mean(), [b for _, b in p])
    cost, g, _ = _check_all(c, params, (real, real.copy(), alpha), what="equal", bias_scales=[float(h.abs().max()) for h in half])
    assert cost[1] == 0.0 and abs(cost[0] - 10.0 * cost[2]) <= 1e-6 * cost[0]
    assert all(np.abs(db).max() <= 1e-6 * np.abs(dW).max() for dW, db in g)      # the two Wasserstein halves cancel to rounding
    assert all(np.abs(dW).max() > 0 for dW, _ in g)
    # one image with fake != real: xhat differs from real in that image only
    _check_all(c, params, _safe(c, params, 6, seed=22, axes=(0,), change=one_image), what="one image")
    c.close()


# ---------------------------------------------------------------------- 4. dg_critic_step
def test_adam_steps_one_to_six_value_for_value():
    """Before step t the weights and moments are read; a twin with those weights gives the step's gradient (dg_critic_gradient);
    TF Adam at beta 0.5 / 0.9 restated in float32 is applied and compared with what dg_critic_step left: lr_t at every t, both
    moments, the step counter.  Each step starts from the device's own state, so nothing accumulates."""
    c, params = _critic(net_dim=8, seed=5)
    twin, _ = _critic(net_dim=8, seed=5)
    c.adam_reset()
    lr = 1e-4
    for t in range(1, 7):
        before_w, before_a = c.get_weights(), c.adam_state()
        assert all(a[2] == t - 1 for a in before_a)
        batch = _draw((28, 28, 1), 8, 100 + t)
        twin.set_weights(before_w)
        gcost, grads, _ = twin.gradient(*batch)
        cost = c.step(*batch, learning_rate=lr).cpu().numpy()
        np.testing.assert_array_equal(cost, gcost)                      # the same kernels on the same state: the same bits
        after_w, after_a = c.get_weights(), c.adam_state()
        for i in range(len(before_w)):
            mm, vv, tt = after_a[i]
            assert tt == t
            for k in range(2):
                want, wm, wv = R.adam_update(before_w[i][k], grads[i][k], before_a[i][0][k], before_a[i][1][k], t, lr, 0.5, 0.9, dtype=np.float32)
                for what, got, w in (("p", after_w[i][k], want), ("m", mm[k], wm), ("v", vv[k], wv)):
                    np.testing.assert_allclose(got, w, rtol=1e-6, atol=1e-6 * np.abs(w).max(), err_msg="step %d layer %d %s %s" % (t, i, "Wb"[k], what))
            assert np.abs(after_w[i][0] - before_w[i][0]).max() > 0
    # the critic's steps left classifier training alone: a classifier handle that refused a critic call trains to the bits of one
    # that never saw one (the kernels' values against float64 are tests/test_gpu_train*.py's business)
    out = []
    for touched in (True, False):
        m = nb.MODELS["A"]()
        m.init_like_reference(seed=1)
        x = np.random.RandomState(3).uniform(0, 1, (16, 28, 28, 1)).astype(np.float32)
        y = (np.arange(16) % 10).astype(np.int32)
        if touched:
            import torch
            dev = torch.device("cuda", 0)
            xt, a, cost = torch.from_numpy(x[:4]).to(dev), torch.zeros(4, device=dev), torch.zeros(3, device=dev)
            rc = _native.load().dg_critic_step(m._handle, xt.data_ptr(), xt.data_ptr(), a.data_ptr(), 4, 10.0, 0, lr, 0.5, 0.9, cost.data_ptr(), None)
            assert rc == -1 and b"Dropout or Softmax" in _native.load().dg_last_error()
        losses = utils_tf.model_train(m, x, y, args={"nb_epochs": 2, "batch_size": 8, "learning_rate": 0.001}, rng=np.random.RandomState(1),
                                      return_losses=True)
        out.append((losses, m.get_weights(), [utils_tf.adam_state(m, i) for i in range(len(m.param_shapes()))]))
        m.close()
    (l0, w0, a0), (l1, w1, a1) = out
    np.testing.assert_array_equal(l0, l1)
    for (W, b), (W2, b2) in zip(w0, w1):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    for (mm, vv, t), (mm2, vv2, t2) in zip(a0, a1):
        assert t == t2
        for p, q in zip(mm + vv, mm2 + vv2):
            np.testing.assert_array_equal(p, q)
    c.close()
    twin.close()


def test_invalid_arguments_are_refused():
    import torch
    c, _ = _critic(net_dim=2, seed=1)
    c._ensure()
    dev = torch.device("cuda", 0)
    x, a = torch.zeros(2, 28, 28, 1, device=dev), torch.zeros(2, device=dev)
    g, cost = torch.zeros(c.n_params(), device=dev), torch.zeros(3, device=dev)
    lib = _native.load()
    call = lambda h, B, axes: lib.dg_critic_gradient(h, x.data_ptr(), x.data_ptr(), a.data_ptr(), B, 10.0, axes, g.data_ptr(), cost.data_ptr(), None, None)
    assert call(c._handle, 2, 0) == 0
    assert call(c._handle, 0, 0) == -1 and call(c._handle, 2, 2) == -1 and b"penalty_axes" in lib.dg_last_error()
    two = K.Critic([nb.Flatten(), nb.Linear(2)], (None, 28, 28, 1), [("W", "b")])
    two.init_like_tflib(0)
    assert call(two._handle, 2, 0) == -1 and b"one output" in lib.dg_last_error()
    c.close()
    two.close()


# ---------------------------------------------------------------------- 5. determinism
def test_two_identical_ten_step_runs_give_identical_bits():
    out = []
    for _ in range(2):
        c, _ = _critic(net_dim=8, seed=6)
        c.adam_reset()
        costs = [c.step(*_draw((28, 28, 1), 16, 300 + k)).cpu().numpy() for k in range(10)]
        out.append((np.stack(costs), c.get_weights(), c.adam_state()))
        c.close()
    (c0, w0, a0), (c1, w1, a1) = out
    np.testing.assert_array_equal(c0, c1)
    for (W, b), (W2, b2) in zip(w0, w1):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    for (mm, vv, t), (mm2, vv2, t2) in zip(a0, a1):
        assert t == t2 == 10
        for p, q in zip(mm + vv, mm2 + vv2):
            np.testing.assert_array_equal(p, q)


# ---------------------------------------------------------------------- 6. trajectory and learning
TRAJ_SEED, TRAJ_LR = 11, 1e-4


def _gan(net_dim=8, batch_size=16, **kw):
    from defensegan_amd import synth
    from defensegan_amd.gan import MnistDefenseGAN
    g = MnistDefenseGAN(cfg={"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": 64, "BATCH_SIZE": batch_size}, test_mode=True, device=0, **kw)
    assert g.set_weights(synth.make_weights("mnist", seed=1234, gain=2.0, bias_range=0.1)) == []
    g._critic = K.mnist_discriminator(net_dim=net_dim)
    return g


def _real_set(n, seed=0, noise=0.25):
    """A separable set: each of 10 classes a fixed seeded binary 28 x 28 pattern plus clipped Gaussian noise (tests/test_gpu_train.py's)."""
    pats = (np.random.RandomState(1234).uniform(0, 1, (10, 28, 28, 1)) > 0.5).astype(np.float32)
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 10, n)
    return np.clip(pats[y] + rs.standard_normal((n, 28, 28, 1)).astype(np.float32) * np.float32(noise), 0, 1).astype(np.float32)


def test_thirty_steps_track_float64_and_150_steps_learn():
    """net_dim 8, batch 16, lr 1e-4, beta 0.5 / 0.9, lambda 10, the reference's penalty axes; real = the separable set, fake = G(z)
    of synth.make_weights("mnist") at z ~ N(0, 1), alpha handed in.  The float64 reference alone (run on the CPU, its fakes from the
    oracle generator) meets both learning conditions with room: first cost 5.681, mean of its last ten costs -7.353; mean D(real) -
    mean D(fake) over 128 images 0.360 before and 9.236 after the 150 steps.  Only the first 30 steps are compared with it here
    (batches chosen by critic_reference.train_safe); the other 120 run on the device alone."""
    g = _gan()
    c = g.critic
    w = c.init_like_tflib(TRAJ_SEED)
    params = [(w[a], w[b]) for a, b in c.param_names]
    layers = R.describe(c)
    real_set = _real_set(512, seed=TRAJ_SEED)
    z = np.random.RandomState(TRAJ_SEED + 1).standard_normal((151 * 4 * 16, 128)).astype(np.float32)
    fakes = g.generate(z)                                                  # every fake batch any draw may ask for, made once

    def draw(k, attempt):
        rs = np.random.RandomState([TRAJ_SEED, k, attempt])
        j = (k * 4 + min(attempt, 3)) * 16
        return real_set[rs.permutation(512)[:16]], fakes[j:j + 16], rs.uniform(0, 1, 16).astype(np.float32)

    ref, _, batches = R.train_safe(layers, params, draw, 30, lr=TRAJ_LR)
    c.adam_reset()
    sep0 = float(c.discriminate(real_set[:128]).mean() - c.discriminate(fakes[:128]).mean())
    costs = [c.step(*b, learning_rate=TRAJ_LR) for b in batches]
    costs += [c.step(*draw(k, 0), learning_rate=TRAJ_LR) for k in range(30, 150)]
    costs = np.stack([t.cpu().numpy() for t in costs])
    rel = np.abs(costs[:30, 0] - ref[:, 0]) / np.abs(ref[:, 0])
    print("30-step trajectory: max relative cost difference %.3g at step %d" % (rel.max(), int(rel.argmax())))
    assert rel.max() <= 1e-2, "max relative cost difference %g at step %d" % (rel.max(), int(rel.argmax()))
    sep1 = float(c.discriminate(real_set[:128]).mean() - c.discriminate(fakes[:128]).mean())
    print("cost first %.6g, mean of last ten %.6g; D(real) - D(fake): %.6g -> %.6g" % (costs[0, 0], costs[-10:, 0].mean(), sep0, sep1))
    assert costs[-10:, 0].mean() < costs[0, 0]
    assert sep1 > sep0
    g.close()


# ---------------------------------------------------------------------- 7. gan.train(phase="disc")
def test_gan_train_phase_disc_is_the_schedule_driven_by_hand(tmp_path):
    import torch
    images = _real_set(100, seed=3)
    seed, iters = 77, 3
    g = _gan(net_dim=4, critic_iters=2)
    w0 = g.critic.init_like_tflib(9)
    with pytest.raises(NotImplementedError, match="generator step"):
        g.train(images, phase=None, train_iters=1)
    g.critic.adam_reset()
    costs = g.train(images, phase="disc", train_iters=iters, seed=seed)
    assert costs.shape == (iters, 3)
    # by hand: the documented schedule, latents and alpha stream, through the C ABI
    h = _gan(net_dim=4, critic_iters=2)
    h.critic.set_named_weights(w0)
    h.critic.adam_reset()
    h._ensure_handle()
    lib, dev = _native.load(), torch.device("cuda", 0)
    sched = h.critic_schedule(100, iters * 2, seed)
    assert sched.shape == (6, 16) and len(set(sched.reshape(-1).tolist())) == 96        # one epoch: six disjoint full batches of 100 images
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    x = torch.from_numpy(images).to(dev)
    hand = torch.zeros(iters * 2, 3, device=dev)
    for k in range(iters * 2):
        fake = h.generate(h.init_latents(16, seed=seed, first_row=k * 16, std=1.0))
        alpha = torch.rand(16, generator=gen, device=dev, dtype=torch.float32)
        real = x[torch.from_numpy(sched[k]).to(dev)].contiguous()
        _native.check(lib.dg_critic_step(h.critic._handle, real.data_ptr(), fake.data_ptr(), alpha.data_ptr(), 16, 10.0, 0, 1e-4, 0.5, 0.9,
                                         hand[k].data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    np.testing.assert_array_equal(costs, hand.cpu().numpy()[1::2])
    for (W, b), (W2, b2) in zip(g.critic.get_weights(), h.critic.get_weights()):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    # save / load: weights, moments and t, bit for bit
    path = str(tmp_path / "critic.npz")
    g.save_discriminator(path)
    r = _gan(net_dim=4)
    r.load_discriminator(path)
    for (W, b), (W2, b2) in zip(g.critic.get_weights(), r.critic.get_weights()):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    for (mm, vv, t), (mm2, vv2, t2) in zip(g.critic.adam_state(), r.critic.adam_state()):
        assert t == t2 == iters * 2
        for p, q in zip(mm + vv, mm2 + vv2):
            np.testing.assert_array_equal(p, q)
    # discriminator_cost is dg_critic_gradient's cost
    real, fake, alpha = images[:16], _real_set(16, seed=8), np.linspace(0, 1, 16).astype(np.float32)
    want, _, _ = g.critic.gradient(real, fake, alpha)
    assert g.discriminator_cost(real, fake, alpha, return_terms=True) == tuple(float(v) for v in want)
    assert np.isfinite(g.discriminator_cost(real, seed=5))
    np.testing.assert_array_equal(g.discriminator_fn(real), g.critic.discriminate(real))
    for q in (g, h, r):
        q.close()
