"""-m gpu: the generator's training step (defensegan_amd/csrc/dg_gen_train.hip) against the float64 reference of
tests/support/generator_reference.py: the seeded backward with every weight gradient, the crop of Generator.2, row isolation, Adam
value for value from the device's own state, the on-device refresh of the derived weight layouts, and train_gan.

Bounds are the project's: every gradient tensor within 1e-4 of its reference's largest entry (a bias: of the sum of its absolute
terms, generator_reference.bias_scales), 1e-5 relative on a cost, rtol 1e-6 / atol 1e-6 max on an Adam step computed from the
device's own state.  Inputs are the first accepted draw of generator_reference.find_seed (found on the CPU; SEEDS below)."""
import numpy as np
import pytest

from tests.support import generator_reference as GR

pytestmark = pytest.mark.gpu

GRAD_TOL, COST_TOL = 1e-4, 1e-5
# (latent, net_dim, N) -> the first seed generator_reference.find_seed accepts (tests/test_gen_train_cpu.py re-derives every entry)
SEEDS = GR.SEEDS


def make(latent=128, nd=64, weights=None, **cfg):
    from defensegan_amd.gan import MnistDefenseGAN
    c = {"USE_BN": False, "LATENT_DIM": latent, "NET_DIM": nd}
    c.update(cfg)
    g = MnistDefenseGAN(cfg=c, test_mode=True, rec_rr=2, rec_iters=3)
    p = weights if weights is not None else GR.weights(latent, nd)
    assert g.set_weights(p) == []
    return g, p


def inputs(latent, nd, N):
    """The recorded draw; asserted to be one the seed search accepts (tests/test_gen_train_cpu.py pins that each is the FIRST)."""
    z, dy = GR.draw(SEEDS[(latent, nd, N)], N, latent)
    assert GR.accepted(GR.weights(latent, nd), z)
    return z, dy


def check_grads(dev, ref, scales, what):
    worst = 0.0
    for name in GR.NAMES:
        scale = scales.get(name, float(np.abs(ref[name]).max()))
        err = float(np.abs(dev[name].astype(np.float64) - ref[name]).max())
        used = err / (GRAD_TOL * scale) if scale > 0 else (0.0 if err == 0 else np.inf)
        print("%s %-22s err %.3e scale %.3e uses %.3f of the bound" % (what, name, err, scale, used))
        worst = max(worst, used)
        assert used <= 1.0, (what, name, err, scale)
    return worst


@pytest.mark.parametrize("latent,nd,N", [(128, 64, 1), (128, 64, 3), (128, 64, 33), (128, 64, 50), (64, 64, 3), (128, 128, 3)])
def test_seeded_backward_with_an_explicit_dy(latent, nd, N):
    """dg_gen_param_gradient with a random dy: the eight gradient tensors, dz and y against float64.  N = 33 crosses a 32-row block,
    N = 50 is the reference's batch.  Measured (one MI355X, one run): the worst tensor of the six cases uses 0.021 of the 1e-4 bound; every use is printed."""
    import ctypes as C
    import torch
    g, p = make(latent, nd)
    z, dy = inputs(latent, nd, N)
    ref = GR.gradient(p, z, dy)
    cost, grads, dz = g.generator_gradient(z, dy)
    assert cost is None
    check_grads(grads, ref["grads"], GR.bias_scales(p, z, dy), "N=%d" % N)
    assert np.abs(dz - ref["dz"]).max() <= GRAD_TOL * np.abs(ref["dz"]).max()
    # y through out_y of the C entry
    h = g._ensure_handle()
    zz, dd = g._to_device(z), g._to_device(dy)
    flat = torch.empty(g.n_params(), dtype=torch.float32, device=zz.device)
    y = torch.empty(N, 28, 28, 1, dtype=torch.float32, device=zz.device)
    g._check(g._lib().dg_gen_param_gradient(h, zz.data_ptr(), dd.data_ptr(), N, flat.data_ptr(), y.data_ptr(), None,
                                            torch.cuda.current_stream(zz.device).cuda_stream))
    assert np.abs(y.cpu().numpy() - ref["y"]).max() <= COST_TOL
    assert np.array_equal(y.cpu().numpy(), g.generate(z))
    # out_dz NULL changes nothing else; a repeated call returns the same bits
    assert np.array_equal(flat.cpu().numpy(), np.concatenate([grads[n].reshape(-1) for n in GR.NAMES]))
    g.close()


def test_dz_agrees_with_the_projection_path():
    """dy = 2 (y - x) / P is the projection loss's own seed (image_rec_loss = mean over H, W, C of (y - x)^2, summed over rows): out_dz
    then agrees with dg_loss_grad's dz within the gradient bound -- the new tail backward tied to the value-checked one.  Measured
    (one MI355X, one run): 3.97e-7 of the largest entry, 0.004 of the 1e-4 bound."""
    g, p = make()
    N = 4
    z, x = inputs(128, 64, N)
    x = (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    y, _, dz_loop = g.loss_grad(x, z)
    dy = (2.0 * (y - x) / 784.0).astype(np.float32)
    _, _, dz = g.generator_gradient(z, dy)
    err = np.abs(dz - dz_loop).max() / np.abs(dz_loop).max()
    print("dz vs loss_grad: %.3e of the largest entry" % err)
    assert err <= GRAD_TOL
    g.close()


def test_the_crop_of_generator_2():
    """A dy that is non-zero only where Generator.3's taps reach h2's last kept row and column (image rows / columns >= 21): dF2 and
    db2 against float64 -- the valid-tap set is that of an 8x8 output with row and column 7 removed.  Measured (one MI355X, one
    run): the worst of the eight tensors uses 0.020 of the 1e-4 bound."""
    g, p = make()
    N = 3
    z, dy = inputs(128, 64, N)
    mask = np.zeros((28, 28), bool)
    mask[21:, :] = True
    mask[:, 21:] = True
    dy = dy * mask[None, :, :, None]
    ref = GR.gradient(p, z, dy)
    _, grads, _ = g.generator_gradient(z, dy)
    check_grads(grads, ref["grads"], GR.bias_scales(p, z, dy), "crop")
    g.close()


def test_zero_and_one_hot_seeds():
    """dy = 0 gives exactly zero gradients; a dy with one non-zero pixel in one image gives the float64 gradient of that row alone,
    and the other rows' dz stay exactly zero: rows do not leak into each other.  Measured (one MI355X, one run): the worst tensor
    uses 0.016 of the 1e-4 bound."""
    g, p = make()
    N = 3
    z, _ = inputs(128, 64, N)
    _, grads, dz = g.generator_gradient(z, np.zeros((N, 28, 28, 1), np.float32))
    assert all(not v.any() for v in grads.values()) and not dz.any()
    dy = np.zeros((N, 28, 28, 1), np.float32)
    dy[1, 13, 9, 0] = 1.5
    ref = GR.gradient(p, z, dy)
    _, grads, dz = g.generator_gradient(z, dy)
    check_grads(grads, ref["grads"], GR.bias_scales(p, z, dy), "one-hot")
    assert not dz[0].any() and not dz[2].any()
    assert np.abs(dz[1] - ref["dz"][1]).max() <= GRAD_TOL * np.abs(ref["dz"]).max()
    ref1 = GR.gradient(p, z[1:2], dy[1:2])
    for n in GR.NAMES:
        assert np.abs(ref1["grads"][n] - ref["grads"][n]).max() <= 1e-12 * max(1.0, np.abs(ref["grads"][n]).max())
    g.close()


def critic_of(g, net_dim, seed=0):
    from defensegan_amd import critic
    c = critic.mnist_discriminator(net_dim=net_dim)
    g._ensure_handle()
    c._device = g._device
    w = c.init_like_tflib(seed=seed)
    rs = np.random.RandomState(seed + 1)
    for k in list(w):                                      # tflib's zero biases would hide the bias path
        if k.endswith(".Biases") or k.endswith(".b"):
            w[k] = rs.uniform(-0.1, 0.1, w[k].shape).astype(np.float32)
    c.set_named_weights(w)
    if g._critic is not None:
        g._critic.close()
    g._critic = c
    return c, [(w[a], w[b]) for a, b in c.param_names]


@pytest.mark.parametrize("cnd,B", [(8, 1), (8, 4), (8, 50), (64, 4)])
def test_the_critic_seeded_gradient(cnd, B):
    """generator_gradient(z) with dy = None: cost = -mean D(G(z)) and the eight tensors against the float64 composition of
    TorchGenerator and critic_reference.forward.  Measured (one MI355X, one run): at most 0.021 of the gradient bound, the cost within
    2.7e-6 relative (bound 1e-5)."""
    from tests.support import critic_reference as CR
    g, p = make()
    c, cparams = critic_of(g, cnd)
    layers = CR.describe(c)
    z, _ = inputs(128, 64, B)
    assert GR.accepted(p, z, (layers, cparams))
    ref = GR.gradient(p, z, critic=(layers, cparams))
    cost, grads, dz = g.generator_gradient(z)
    print("cost dev %.9g ref %.9g" % (cost, ref["cost"]))
    assert abs(cost - ref["cost"]) <= COST_TOL * max(abs(ref["cost"]), 1e-3)
    assert abs(g.generator_cost(z) - cost) == 0.0
    check_grads(grads, ref["grads"], GR.bias_scales(p, z, ref["dy"]), "critic %d B=%d" % (cnd, B))
    assert np.abs(dz - ref["dz"]).max() <= GRAD_TOL * np.abs(ref["dz"]).max()
    g.close()


def test_adam_steps_one_to_six_value_for_value():
    """Six dg_gen_step calls; before each the gradient comes from a TWIN handle holding the device's own weights (and is the same
    bits as the stepping handle's own), float32 Adam is restated on the host, and parameters, both moments and the counter are
    compared (rtol 1e-6, atol 1e-6 max).  Measured (one MI355X, one run): under 0.0005 of that bound at every
    step -- the host restatement reproduces the kernel's float32 arithmetic; the use is printed per step."""
    lr, b1, b2 = 1e-4, 0.5, 0.9
    g, p = make()
    N = 4
    worst = 0.0
    for t in range(1, 7):
        z, dy = GR.draw(100 + t, N, 128)
        w0 = g.get_weights()
        m0, v0, t0 = g.generator_adam_state()
        assert t0 == t - 1
        twin, _ = make(weights=w0)
        _, gt, _ = twin.generator_gradient(z, dy)
        _, go, _ = g.generator_gradient(z, dy)
        twin.close()
        assert g.generator_step(z, dy, learning_rate=lr, beta1=b1, beta2=b2) is None
        w1 = g.get_weights()
        m1, v1, t1 = g.generator_adam_state()
        assert t1 == t
        for n in GR.NAMES:
            assert np.array_equal(gt[n], go[n]), n
            pw, pm, pv = GR.adam_f32(w0[n], gt[n], m0[n], v0[n], t, lr, b1, b2)
            for got, want in ((w1[n], pw), (m1[n], pm), (v1[n], pv)):
                bound = 1e-6 * float(np.abs(want).max()) + 1e-6 * np.abs(want)
                worst = max(worst, float((np.abs(got - want) / bound).max()))
                assert np.allclose(got, want, rtol=1e-6, atol=1e-6 * float(np.abs(want).max())), (t, n)
            assert not np.array_equal(w1[n], w0[n]), n
        print("Adam step %d: worst use of the rtol 1e-6 / atol 1e-6 max bound so far %.3f" % (t, worst))
    g.generator_adam_reset()
    m, v, t = g.generator_adam_state()
    assert t == 0 and all(not a.any() for a in m.values()) and all(not a.any() for a in v.values())
    g.close()


@pytest.mark.parametrize("option", [None, ("frag_path", 1), ("turn_fused", 1)])
def test_the_refresh_of_the_derived_layouts(option):
    """After three steps every derived layout holds the new weights: generate(z) and reconstruct (B = 3, R = 2, L = 3) are
    bit-identical to a FRESH handle given get_weights() -- on the default path, with frag_path = 1 and with turn_fused = 1."""
    g, p = make()
    if option:
        g.set_option(*option)
    N = 4
    zs = GR.draw(7, 6, 128)[0]
    x = g.generate(zs[:3])
    before = g.generate(zs)
    for t in range(3):
        z, dy = GR.draw(200 + t, N, 128)
        g.generator_step(z, dy, learning_rate=1e-2)
    w = g.get_weights()
    fresh, _ = make(weights=w)
    if option:
        fresh.set_option(*option)
    after = g.generate(zs)
    assert not np.array_equal(after, before)
    assert np.array_equal(after, fresh.generate(zs))
    a = g.reconstruct(x, seed=5, return_details=True)
    b = fresh.reconstruct(x, seed=5, return_details=True)
    for k in ("rec", "loss", "z", "idx"):
        assert np.array_equal(a[k], b[k]), k
    # a set_weights after training replaces the parameters and leaves Adam's moments alone
    m0, v0, t0 = g.generator_adam_state()
    g.set_weights(p)
    m1, v1, t1 = g.generator_adam_state()
    assert t1 == t0 == 3 and all(np.array_equal(m0[n], m1[n]) for n in GR.NAMES)
    assert np.array_equal(g.generate(zs), before)
    g.close()
    fresh.close()


def small_gan(seed=0):
    g, p = make(BATCH_SIZE=4, CRITIC_ITERS=2)
    critic_of(g, 4, seed)
    rs = np.random.RandomState(3)
    images = rs.uniform(0, 1, (24, 28, 28, 1)).astype(np.float32)
    return g, images


def state_of(g):
    m, v, t = g.generator_adam_state()
    c = g.critic
    return (g.get_weights(), m, v, t, c.named_weights(), c.adam_state())


def same_state(a, b):
    for da, db in ((a[0], b[0]), (a[1], b[1]), (a[2], b[2]), (a[4], b[4])):
        for k in da:
            assert np.array_equal(da[k], db[k]), k
    assert a[3] == b[3]
    for (ma, va, ta), (mb, vb, tb) in zip(a[5], b[5]):
        assert ta == tb
        for p, q in zip(ma + va, mb + vb):
            assert np.array_equal(p, q)


def test_train_gan_is_deterministic_and_resumes(tmp_path):
    """Two identical five-iteration train_gan runs leave identical bits in both networks, in all four Adam states and in the costs;
    iteration 0 has no generator step (NaN) and train_iters = 1 equals train(phase="disc", train_iters=1) bit for bit; saving after
    two iterations and resuming for three more gives the bits of five in one go."""
    runs = []
    for _ in range(2):
        g, images = small_gan()
        costs = g.train_gan(images, train_iters=5, seed=9)
        runs.append((costs, state_of(g)))
        g.close()
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True)
    same_state(runs[0][1], runs[1][1])
    assert np.isnan(runs[0][0][0, 3]) and np.isfinite(runs[0][0][1:, 3]).all() and np.isfinite(runs[0][0][:, :3]).all()
    # one iteration: the critic alone
    g, images = small_gan()
    c1 = g.train_gan(images, train_iters=1, seed=9)
    g2, _ = small_gan()
    c2 = g2.train(images, phase="disc", train_iters=1, seed=9)
    assert np.array_equal(c1[:, :3], c2)
    for k, v in g.critic.named_weights().items():
        assert np.array_equal(v, g2.critic.named_weights()[k]), k
    g.close()
    g2.close()
    # save after two, resume for three
    g, images = small_gan()
    ca = g.train_gan(images, train_iters=2, seed=9)
    gp, dp = str(tmp_path / "generator.npz"), str(tmp_path / "discriminator.npz")
    g.save_generator(gp)
    g.save_discriminator(dp)
    g.close()
    g, _ = small_gan(seed=5)
    g.load_generator_state(gp)
    g.load_discriminator(dp)
    cb = g.train_gan(images, train_iters=3, seed=9, start_iter=2)
    assert np.array_equal(np.concatenate([ca, cb]), runs[0][0], equal_nan=True)
    same_state(state_of(g), runs[0][1])
    g.close()


def test_refusals_on_the_device():
    """CelebA and use_bn handles are refused with "not implemented for"; null pointers, N < 1, incomplete weights and unknown names
    are errors, not faults."""
    import ctypes as C
    from defensegan_amd import _native
    lib = _native.load()
    for arch, bn in ((1, 0), (0, 1)):
        h = C.c_void_p()
        assert lib.dg_create(arch, 128, 64, bn, 0, C.byref(h)) == 0
        one = (C.c_float * 1)()
        assert lib.dg_gen_step(h, one, one, 1, 1e-4, 0.5, 0.9, None) == -1
        assert b"not implemented for" in lib.dg_last_error()
        assert lib.dg_gen_adam_reset(h) == -1 and b"not implemented for" in lib.dg_last_error()
        lib.dg_destroy(h)
    h = C.c_void_p()
    assert lib.dg_create(0, 128, 64, 0, 0, C.byref(h)) == 0
    one = (C.c_float * 1)()
    assert lib.dg_gen_param_gradient(h, None, one, 1, one, None, None, None) == -1
    assert lib.dg_gen_param_gradient(h, one, one, 1, None, None, None, None) == -1
    assert lib.dg_gen_param_gradient(h, one, one, 1, one, None, None, None) == -2          # weights incomplete
    assert lib.dg_get_weights(h, b"Generator.9.Filters", one, 0) == -1
    assert lib.dg_get_weights(h, b"Generator.Input.b", one, 0) == -2
    assert lib.dg_gen_get_adam(h, b"nope", None, None, None, 0) == -1
    lib.dg_destroy(h)
    g, _ = make()
    g._ensure_handle()
    assert lib.dg_gen_param_gradient(g._handle, one, one, 0, one, None, None, None) == -1
    assert lib.dg_gen_param_gradient(g._handle, one, one, (1 << 24) + 1, one, None, None, None) == -1
    g.close()


def test_it_learns_against_a_fixed_critic():
    """20 generator steps at lr 1e-4 against a FIXED critic (net_dim 8), fresh z per step, batch 16, lower generator_cost on a
    held-out batch of 128.  The float64 reference alone (generator_reference.learning_reference, run on the CPU first and re-run by
    tests/test_gen_train_cpu.py, which pins LEARNING_REFERENCE) goes from 0.146382 to -1.815263; the device follows that trajectory
    within the project's 1e-2 relative.  Measured (one MI355X, one run): 0.146382 -> -1.815758, 0.0000 and 0.027 of the bound."""
    g, p = make()
    layers, cparams, w = GR.fixed_critic()
    from defensegan_amd import critic
    c = critic.mnist_discriminator(net_dim=8)
    g._ensure_handle()
    c._device = g._device
    c.set_named_weights(w)
    g._critic = c
    zh = GR.draw(999, 128, 128)[0]
    before = g.generator_cost(zh)
    for t in range(1, 21):
        g.generator_step(GR.draw(300 + t, 16, 128)[0], learning_rate=1e-4)
    after = g.generator_cost(zh)
    ref_before, ref_after = GR.LEARNING_REFERENCE
    print("held-out cost %.6f -> %.6f (float64 %.6f -> %.6f): uses %.4f and %.4f of the 1e-2 relative bound"
          % (before, after, ref_before, ref_after, abs(before - ref_before) / (1e-2 * abs(ref_before)),
             abs(after - ref_after) / (1e-2 * abs(ref_after))))
    assert after < before
    assert abs(before - ref_before) <= 1e-2 * abs(ref_before)
    assert abs(after - ref_after) <= 1e-2 * abs(ref_after)
    for k, v in c.named_weights().items():                 # the critic did not move
        assert np.array_equal(v, w[k]), k
    g.close()


# ---------------------------------------------------------------------- train_gan against something that is not train_gan
REPLAY_ITERS, REPLAY_SEED = 3, 9


def _ptr(t):
    return t.data_ptr()


def hand_driven_run(g, images, iters, seed, lr=1e-4, b1=0.5, b2=0.9):
    """The schedule of train_gan driven by hand through the C ABI, written from the issue's description: iteration it > 0 starts
    with dg_init_latents(seed + 1, first_row = it * batch, std 1), dg_generate, dg_clf_backward (dlogits = -1/B) and dg_gen_step;
    then critic_iters times dg_init_latents(seed, first_row = k * batch, std 1), dg_generate, the next `batch` uniforms of the alpha
    stream and dg_critic_step on images[schedule[k]].  Returns (costs [iters, 4], what every step was fed: z of the generator steps,
    z of the critic steps, alphas, schedule)."""
    import torch
    from defensegan_amd import _native
    lib = _native.load()
    h = g._ensure_handle()
    c = g.critic
    c._device = g._device
    c._ensure()
    dev = torch.device("cuda", g._device)
    s = torch.cuda.current_stream(dev).cuda_stream
    bs, ci, lat = int(g.batch_size), int(g.critic_iters), int(g.latent_dim)
    x = torch.from_numpy(images).to(dev)
    sched = g.critic_schedule(len(images), iters * ci, seed)
    agen = torch.Generator(device=dev)
    agen.manual_seed(seed)
    costs = torch.full((iters, 4), float("nan"), dtype=torch.float32, device=dev)
    zs_gen, zs_critic, alphas = {}, [], []
    z = torch.empty(bs, lat, dtype=torch.float32, device=dev)
    y = torch.empty(bs, 28, 28, 1, dtype=torch.float32, device=dev)
    dy = torch.empty_like(y)
    dl = torch.full((bs, 1), -1.0 / bs, dtype=torch.float32, device=dev)
    cost3 = torch.empty(3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for it in range(iters):
            if it > 0:
                _native.check(lib.dg_init_latents(h, _ptr(z), bs, seed + 1, it * bs, 1.0, s))
                _native.check(lib.dg_generate(h, _ptr(z), bs, _ptr(y), s))
                costs[it, 3] = -c.discriminate(y).mean()
                _native.check(lib.dg_clf_backward(c._handle, _ptr(y), _ptr(dl), bs, _ptr(dy), s))
                _native.check(lib.dg_gen_step(h, _ptr(z), _ptr(dy), bs, lr, b1, b2, s))
                zs_gen[it] = z.cpu().numpy()
            for i in range(ci):
                k = it * ci + i
                _native.check(lib.dg_init_latents(h, _ptr(z), bs, seed, k * bs, 1.0, s))
                _native.check(lib.dg_generate(h, _ptr(z), bs, _ptr(y), s))
                alpha = torch.rand(bs, generator=agen, device=dev, dtype=torch.float32)
                real = x[torch.from_numpy(sched[k]).to(dev)].contiguous()
                _native.check(lib.dg_critic_step(c._handle, _ptr(real), _ptr(y), _ptr(alpha), bs, float(g.gradient_penalty_lambda), 0,
                                                 lr, b1, b2, _ptr(cost3), s))
                if i == ci - 1:
                    costs[it, :3] = cost3
                zs_critic.append(z.cpu().numpy())
                alphas.append(alpha.cpu().numpy())
    return costs.cpu().numpy(), (zs_gen, zs_critic, alphas, sched)


def test_train_gan_equals_the_schedule_driven_by_hand_through_the_c_abi():
    """train_iters = 3 with BATCH_SIZE 4, CRITIC_ITERS 2 and a net_dim 4 critic: train_gan's costs, both networks and all four Adam
    states equal, bit for bit, the same schedule issued call by call through the C ABI (hand_driven_run) -- which z goes to which
    step, the seed + 1 / first_row = it * batch latents of the generator steps, fake batches from the current weights and the
    generator-before-critic order are thereby pinned by something that is not train_gan."""
    g, images = small_gan()
    costs = g.train_gan(images, train_iters=REPLAY_ITERS, seed=REPLAY_SEED)
    want = state_of(g)
    g.close()
    g, _ = small_gan()
    by_hand, _ = hand_driven_run(g, images, REPLAY_ITERS, REPLAY_SEED)
    assert np.array_equal(costs, by_hand, equal_nan=True)
    same_state(state_of(g), want)
    g.close()


def test_train_gan_follows_the_float64_trajectory():
    """The costs train_gan returns (last critic cost, w and P of every iteration, the generator cost from iteration 1 on) against
    generator_reference.train_gan_reference -- float64 autograd for both networks, critic_reference's Adam -- fed the latents and
    alphas the device drew (hand_driven_run records them; the test above shows they are train_gan's): each within 1e-2 relative,
    the project's bound along a trajectory.  Measured (one MI355X, one run): at most 0.0014 of the bound (w of iteration 1 and the
    generator cost of iteration 2); the use is printed per entry."""
    from tests.support import critic_reference as CR
    g, images = small_gan()
    costs = g.train_gan(images, train_iters=REPLAY_ITERS, seed=REPLAY_SEED)
    g.close()
    g, _ = small_gan()
    p0 = g.get_weights()
    c = g.critic
    layers = CR.describe(c)
    cparams = [(c.named_weights()[a], c.named_weights()[b]) for a, b in c.param_names]
    _, (zs_gen, zs_critic, alphas, sched) = hand_driven_run(g, images, REPLAY_ITERS, REPLAY_SEED)
    g.close()
    ref = GR.train_gan_reference(p0, layers, cparams, images, sched, zs_gen, zs_critic, alphas, 2)
    assert np.isnan(costs[0, 3]) and np.isnan(ref[0, 3])
    used = np.abs(costs - ref) / (1e-2 * np.abs(ref))
    print("train_gan vs float64, use of the 1e-2 relative bound per (iteration; cost, w, P, generator cost):\n%s" % used)
    assert np.nanmax(used) <= 1.0, (costs, ref)


def _write_idx(dirname, n, seed=0):
    import os
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (n, 28, 28)).astype(np.uint8)
    lab = rs.randint(0, 10, n).astype(np.uint8)
    os.makedirs(dirname, exist_ok=True)
    for key, header, body in (("train_images", 16, img), ("train_labels", 8, lab), ("test_images", 16, img[:8]), ("test_labels", 8, lab[:8])):
        from defensegan_amd import datasets
        with open(os.path.join(dirname, datasets.IDX_FILES[key]), "wb") as fh:
            fh.write(bytes(header))
            fh.write(body.tobytes())


def test_the_command_line_trains_saves_and_resumes(tmp_path):
    """python -m defensegan_amd.train_gan's main() on a tiny idx fixture (72 images, 60 of them the training split, the shipped
    batch of 50): --train_iters 2 --save_every 1 writes generator.npz, discriminator.npz and train_state.json; --resume to 3
    iterations leaves the files of 3 iterations in one go, bit for bit; the generator file loads through load_generator."""
    import json
    import os
    from defensegan_amd import train_gan as T
    from defensegan_amd.gan import MnistDefenseGAN
    data = str(tmp_path / "data")
    _write_idx(data, 72)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert T.main(["--data_dir", data, "--out_dir", a, "--train_iters", "2", "--save_every", "1"]) == 0
    assert json.load(open(os.path.join(a, "train_state.json")))["iterations"] == 2
    assert T.main(["--data_dir", data, "--out_dir", a, "--train_iters", "3", "--save_every", "1", "--resume"]) == 0
    assert json.load(open(os.path.join(a, "train_state.json")))["iterations"] == 3
    assert T.main(["--data_dir", data, "--out_dir", b, "--train_iters", "3"]) == 0
    for name in ("generator.npz", "discriminator.npz"):
        with np.load(os.path.join(a, name)) as fa, np.load(os.path.join(b, name)) as fb:
            assert sorted(fa.files) == sorted(fb.files)
            for k in fa.files:
                assert np.array_equal(fa[k], fb[k]), (name, k)
    with np.load(os.path.join(a, "generator.npz")) as fa:
        assert int(fa["adam_t"]) == 2                       # iterations 1 and 2 took a generator step
    g = MnistDefenseGAN(cfg={"USE_BN": False}, test_mode=True)
    assert g.load_generator(os.path.join(a, "generator.npz"))
    assert np.isfinite(g.generate(GR.draw(0, 2, 128)[0])).all()
    g.close()
