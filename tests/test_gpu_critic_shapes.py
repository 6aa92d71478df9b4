"""-m gpu: the critic beyond the MNIST layout (tests/support/critic_cases.py) against the float64 reference of
tests/support/critic_reference.py -- ReLU critics folded and unfolded, hidden Linear layers, Flatten first, VALID / 1x1 / non-square
convolutions, more than 256 columns, H = 1, exact zero norms, 65537 images -- then the tangent pass alone, Adam steps at other betas
and with cost = NULL, workspace regrowth on one handle, and LeakyReLU in the classifier entry points.

The bounds are the project's (tests/test_gpu_critic.py): 1e-4 of the largest reference entry on slopes and gradient tensors, 1e-5
relative on a cost term, 1e-6 on an Adam step; what float32 alone uses of them is measured in tests/test_critic_cases_cpu.py.  Every
batch is the draw recorded in the table: no search runs here.  Each test prints the figures it asserts (pytest -s)."""
import numpy as np
import pytest

from defensegan_amd import _native
from defensegan_amd import network_builder as nb
from defensegan_amd import utils_tf
from tests.support import blackbox_reference as BR
from tests.support import critic_cases as T
from tests.support import critic_reference as R
from tests.support import pgd_reference as P
from tests.support import train_reference as TR
from tests.support.critic_cases import _check_all

pytestmark = pytest.mark.gpu

SMALL = [(name, B, axes) for name, case in T.CASES.items() if name != "many_images" for B in case.Bs for axes in case.axes]


def _finite(cost, grads, slopes):
    return bool(np.isfinite(cost).all() and np.isfinite(slopes).all() and all(np.isfinite(g).all() for pair in grads for g in pair))


# ---------------------------------------------------------------------- 1. every case, every axes value
@pytest.mark.parametrize("name,B,axes", SMALL)
def test_case_matches_reference(name, B, axes):
    case = T.CASES[name]
    c, params = T.critic_of(case)
    batch = T.case_batch(case, B)
    H, W, Cc = case.shape
    cost, grads, slopes = _check_all(c, params, batch, axes=axes, what="%s B%d axes%d" % (name, B, axes))
    assert slopes.shape == ((B, W, Cc) if axes == 0 else (B,))
    assert _finite(cost, grads, slopes)
    if name == "wide":
        # columns 256..259 are the second trip of critic_norm_kernel<false>'s column loop
        _, _, rs = R.param_gradient(R.describe(c), params, *batch, axes=axes)
        if axes == 0:
            got, want = slopes.reshape(B, W * Cc)[:, 256:], rs.reshape(B, W * Cc)[:, 256:]
            assert got.shape == (B, 4)
            err = np.abs(got - want).max()
            print("wide: columns 256..259: max|dev - ref| = %.3g, smallest reference slope there %.3g" % (err, want.min()))
            assert want.min() > 1e-3
            assert err <= 1e-4 * np.abs(rs).max(), "columns 256..259 (the column loop's second trip): max|dev - ref| = %g" % err
    if name == "zero_columns":
        if axes == 0:
            assert (slopes[:, :, 1] == 0.0).all() and slopes[:, :, 0].min() > 1e-3
        # the rows of the zeroed filter slice: the penalty's gradient there is exactly 0 (its input v is 0 in channel 1), so the rows
        # are the Wasserstein term's alone, bit for bit those of lambda = 0 (the Wasserstein term's own rows there are no zeros:
        # d w / dK[:, :, 1, :] sums inputs times a_1 whatever K holds; tests/test_critic_cases_cpu.py has the same on the reference)
        _, g0, _ = c.gradient(*batch, gp_lambda=0.0, penalty_axes=axes)
        np.testing.assert_array_equal(grads[0][0][:, :, 1, :], g0[0][0][:, :, 1, :])
        assert np.abs(grads[0][0][:, :, 0, :] - g0[0][0][:, :, 0, :]).max() > 1e-3
    if name == "dead_image":
        assert (slopes[T.DEAD] == 0.0).all()
        others = [b for b in range(B) if b != T.DEAD]
        assert slopes[others].min() > 1e-3
    if name == "mixed" and axes == 0:
        assert (slopes[:, 7, :] == 0.0).all()               # the stride-2 VALID convolution never reads column 7
    c.close()


# ---------------------------------------------------------------------- 2. the tangent pass in isolation
@pytest.mark.parametrize("name", ["mixed", "mlp"])
def test_equal_batches_leave_the_penalty_gradient_alone(name):
    """real == fake: the Wasserstein halves cancel, what is left is the tangent pass and its weight gradients -- through a ReLU folded
    into a Linear, a hidden Linear's tangent map (mixed) and two of them with Flatten first (mlp)."""
    import torch
    case = T.CASES[name]
    c, params = T.critic_of(case)
    layers = R.describe(c)
    B = case.Bs[-1]
    real, _, alpha = T.case_batch(case, B)
    p = R.as_params(params, requires_grad=True)
    half = torch.autograd.grad(R.forward(layers, p, torch.as_tensor(real.astype(np.float64))).mean(), [b for _, b in p])
    for axes in case.axes:
        cost, g, _ = _check_all(c, params, (real, real.copy(), alpha), axes=axes, what="%s equal axes%d" % (name, axes),
                                bias_scales=[float(h.abs().max()) for h in half])
        assert cost[1] == 0.0 and abs(cost[0] - 10.0 * cost[2]) <= 1e-6 * cost[0]
        assert all(np.abs(db).max() <= 1e-6 * np.abs(dW).max() for dW, db in g)      # the penalty has no bias gradient
        assert all(np.abs(dW).max() > 0 for dW, _ in g)
    c.close()


# ---------------------------------------------------------------------- 3. dg_critic_step on the new layouts
def _state(c):
    return c.get_weights(), c.adam_state()


def _assert_same_state(a, b):
    (w0, a0), (w1, a1) = a, b
    for (W, bb), (W2, b2) in zip(w0, w1):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(bb, b2)
    for (mm, vv, t), (mm2, vv2, t2) in zip(a0, a1):
        assert t == t2
        for p, q in zip(mm + vv, mm2 + vv2):
            np.testing.assert_array_equal(p, q)


@pytest.mark.parametrize("betas", [(0.5, 0.9), (0.9, 0.999), (0.0, 0.0)])
@pytest.mark.parametrize("name", ["relu_fused", "mlp"])
def test_adam_steps_one_and_two_value_for_value(name, betas):
    """tests/test_gpu_critic.py's form at t = 1 and 2: a twin with the weights before the step gives the step's gradient, TF Adam
    restated in float32 with the given betas is applied and compared with what dg_critic_step left.  Betas (0, 0), the allowed edge:
    m = g, v = g^2, lr_t = lr."""
    case = T.CASES[name]
    c, _ = T.critic_of(case)
    twin, _ = T.critic_of(case)
    c.adam_reset()
    B, lr, (b1, b2) = case.Bs[-1], 1e-4, betas
    for t in (1, 2):
        before_w, before_a = _state(c)
        assert all(a[2] == t - 1 for a in before_a)
        batch = T.draw_case(case, B, 10 + t)
        twin.set_weights(before_w)
        gcost, grads, _ = twin.gradient(*batch)
        cost = c.step(*batch, learning_rate=lr, beta1=b1, beta2=b2).cpu().numpy()
        np.testing.assert_array_equal(cost, gcost)
        after_w, after_a = _state(c)
        for i in range(len(before_w)):
            mm, vv, tt = after_a[i]
            assert tt == t
            for k in range(2):
                want, wm, wv = R.adam_update(before_w[i][k], grads[i][k], before_a[i][0][k], before_a[i][1][k], t, lr, b1, b2, dtype=np.float32)
                for what, got, w in (("p", after_w[i][k], want), ("m", mm[k], wm), ("v", vv[k], wv)):
                    np.testing.assert_allclose(got, w, rtol=1e-6, atol=1e-6 * np.abs(w).max(), err_msg="%s step %d layer %d %s %s" % (name, t, i, "Wb"[k], what))
            assert np.abs(after_w[i][0] - before_w[i][0]).max() > 0
    c.close()
    twin.close()


def test_step_with_a_null_cost_leaves_the_same_bits():
    """dg_critic_step(cost = NULL) writes the cost into the workspace's own slot; weights and moments equal the run that was handed a
    buffer, bit for bit."""
    import torch
    case = T.CASES["relu_fused"]
    B, lib, dev = case.Bs[-1], _native.load(), torch.device("cuda", 0)
    out = []
    for with_cost in (True, False):
        c, _ = T.critic_of(case)
        c.adam_reset()
        cost = torch.zeros(3, device=dev)
        for t in (1, 2):
            r, f, a = (torch.from_numpy(v).to(dev) for v in T.draw_case(case, B, 10 + t))
            _native.check(lib.dg_critic_step(c._handle, r.data_ptr(), f.data_ptr(), a.data_ptr(), B, 10.0, 0, 1e-4, 0.5, 0.9,
                                             cost.data_ptr() if with_cost else None, torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        out.append(_state(c))
        assert all(a[2] == 2 for a in out[-1][1])
        if not with_cost:
            assert not cost.cpu().numpy().any()
        c.close()
    _assert_same_state(*out)
    fresh, _ = T.critic_of(case)
    assert np.abs(out[0][0][0][0] - fresh.get_weights()[0][0]).max() > 0          # the steps moved the weights
    fresh.close()


# ---------------------------------------------------------------------- 4. workspace regrowth on one handle
def test_one_handle_across_growing_and_shrinking_batches():
    """ensure() re-allocates every per-layer buffer when B grows and keeps them when it shrinks; slices are addressed with the
    current B inside the larger buffers.  Every sum has a fixed order that depends on B alone, so each result equals a fresh
    handle's at that B, bit for bit."""
    case = T.CASES["mixed"]
    c, _ = T.critic_of(case)
    for B in (3, 11, 3, 1):
        batch = T.draw_case(case, B, 20 + B)
        for axes in case.axes:
            fresh, _ = T.critic_of(case)
            want = fresh.gradient(*batch, penalty_axes=axes)
            got = c.gradient(*batch, penalty_axes=axes)
            np.testing.assert_array_equal(got[0], want[0], err_msg="cost at B = %d" % B)
            np.testing.assert_array_equal(got[2], want[2], err_msg="slopes at B = %d" % B)
            for (dW, db), (rW, rb) in zip(got[1], want[1]):
                np.testing.assert_array_equal(dW, rW, err_msg="B = %d" % B)
                np.testing.assert_array_equal(db, rb, err_msg="B = %d" % B)
            assert _finite(*got) and all(np.abs(dW).max() > 0 for dW, _ in got[1])
            fresh.close()
    c.close()


# ---------------------------------------------------------------------- 5. 65537 images
@pytest.mark.parametrize("axes", [0, 1])
def test_many_images(axes):
    """One image more than the norm kernels' grid holds: workgroup 0 takes image 65536 on its second trip.  Both weight-gradient calls
    of both layers run 256 slots.  All 65537 * (4 or 1) slopes, the cost terms and the gradients at the project's bounds (the
    float32 restatement uses 0.101 of the gradient bound at this draw, tests/support/critic_cases.py)."""
    case = T.CASES["many_images"]
    B = case.Bs[0]
    c, params = T.critic_of(case)
    batch = T.case_batch(case, B)
    cost, grads, slopes = _check_all(c, params, batch, axes=axes, what="many_images axes%d" % axes)
    assert slopes.shape == ((B, 2, 1) if axes == 0 else (B,)) and _finite(cost, grads, slopes)
    _, _, rs = R.param_gradient(R.describe(c), params, *batch, axes=axes)
    last = np.abs(slopes[65536:] - rs[65536:]).max()
    print("many_images: image 65536 (the grid loop's second trip): max|dev - ref| = %.3g" % last)
    assert last <= 1e-4 * np.abs(rs).max() and rs[65536:].min() > 0
    c.close()


# ---------------------------------------------------------------------- 6. LeakyReLU in the classifier entry points
@pytest.fixture(scope="module")
def leaky():
    """tests/support/critic_cases.py's 3-class LeakyReLU classifier on the device, with its recorded inputs (no search here)."""
    m, params, layers = T.leaky_classifier()
    x, y = T.leaky_inputs(T.LEAKY_ATTEMPT)
    m.set_weights(params)
    yield dict(m=m, params=params, layers=layers, x=x, y=y)
    m.close()


def test_leakyrelu_classifier_training_step(leaky):
    """dg_clf_param_gradient and one dg_clf_train step (tests/test_gpu_train.py's forms and bounds): loss 1e-5, gradients 1e-4 of the
    largest entry, the Adam update 1e-6."""
    from tests.test_gpu_train import SEED, _IdentityRng, _check_grads, _device_gradient
    m, params, x, y = leaky["m"], leaky["params"], leaky["x"], leaky["y"]
    m.set_weights(params)
    loss, grads, _ = _device_gradient(m, x, y, step=0)
    rl, rg, _ = TR.param_gradient(leaky["layers"], params, x, y, SEED, 0)
    print("leakyrelu classifier: loss dev %.9g ref %.9g" % (loss, rl))
    assert abs(loss - rl) <= 1e-5 * abs(rl), (loss, rl)
    _check_grads(grads, rg)
    lr = 0.01
    losses = utils_tf.model_train(m, x, y, args={"nb_epochs": 1, "batch_size": 5, "learning_rate": lr}, rng=_IdentityRng(), return_losses=True)
    assert losses.shape == (1,) and abs(float(losses[0]) - rl) <= 1e-5 * abs(rl)
    for i, ((W, b), (gW, gb), (nW, nb_)) in enumerate(zip(params, grads, m.get_weights())):
        for p, g, new in ((W, gW, nW), (b, gb, nb_)):
            want, _, _ = TR.adam_update(p, g, np.zeros_like(p), np.zeros_like(p), 1, lr, dtype=np.float32)
            np.testing.assert_allclose(new, want, rtol=1e-6, atol=1e-6 * np.abs(want).max(), err_msg="layer %d" % i)
        (mW, mb), (vW, vb), t = utils_tf.adam_state(m, i)
        assert t == 1
        np.testing.assert_allclose(mW, np.float32(0.1) * gW, rtol=1e-6, atol=0)
    m.set_weights(params)


def test_leakyrelu_classifier_input_and_class_gradients(leaky):
    """dg_fgsm's input gradient, dg_clf_class_gradient and dg_clf_jacobian against float64 autograd (tests/test_gpu_blackbox.py's
    bound: rtol 1e-5, atol 1e-5 of the reference's largest element)."""
    import torch
    m, params, layers, x, y = leaky["m"], leaky["params"], leaky["layers"], leaky["x"], leaky["y"]
    m.set_weights(params)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    ce = torch.nn.functional.cross_entropy(TR.logits(layers, TR.as_params(params), xt), torch.as_tensor(y, dtype=torch.long), reduction="sum")
    (gref,) = torch.autograd.grad(ce, xt)
    gref = gref.numpy()
    g = m.input_gradient(x, y)
    np.testing.assert_allclose(g, gref, rtol=1e-5, atol=1e-5 * np.abs(gref).max())
    adv = nb.FastGradientMethod(m).generate(x, eps=0.1, y=y, clip_min=0.0, clip_max=1.0)
    f = np.float32
    np.testing.assert_array_equal(adv, np.clip(x + f(0.1) * np.sign(g).astype(f), f(0), f(1)))
    decided = np.abs(gref) > 1e-4 * np.abs(gref).max()
    assert decided.mean() >= 0.99 and (np.sign(g)[decided] == np.sign(gref)[decided]).all()
    for of_probs in (True, False):
        jac = m.jacobian(x, of_probs=of_probs)
        assert jac.shape == (5, 3, 8, 8, 1)
        for k in range(3):
            ref = BR.class_gradient(layers, params, x, np.full(5, k), of_probs=of_probs)
            scale = np.abs(ref).max()
            np.testing.assert_allclose(jac[:, k], ref, rtol=1e-5, atol=1e-5 * scale, err_msg="class %d of_probs %s" % (k, of_probs))
            np.testing.assert_array_equal(m.class_gradient(x, np.full(5, k), of_probs=of_probs), jac[:, k])
        ref = BR.class_gradient(layers, params, x, y, of_probs=of_probs)
        np.testing.assert_allclose(m.class_gradient(x, y, of_probs=of_probs), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_leakyrelu_classifier_pgd_teacher_forced(leaky):
    """Three PGD iterations against tests/support/pgd_reference.py in tests/test_gpu_pgd.py's form: x_{k+1} from the reference's x_k on
    the decided pixels (|g_ref| > 1e-4 max|g_ref|, at least 99 % of all) within 1e-6."""
    from tests.support import bpda_reference as B
    m, params, x, y = leaky["m"], leaky["params"], leaky["x"], leaky["y"]
    m.set_weights(params)
    kw = dict(eps=0.3, eps_iter=0.05, clip_min=0.0, clip_max=1.0)
    ref = P.pgd(P.classifier_ops(B.layers_of(m), params, y), x, y, 0.3, 0.05, 3, 0.0, 1.0)
    atk = nb.ProjectedGradientDescent(m)
    for k in range(3):
        g = ref["grads"][k]
        decided = np.abs(g) > 1e-4 * np.abs(g).max()
        adv = atk.generate(x, y, nb_iter=1, x_init=ref["iterates"][k].astype(np.float32), **kw)
        d = np.abs(adv.astype(np.float64) - ref["iterates"][k + 1])
        print("leakyrelu k %d: undecided %.5f, max |dx| on decided pixels %.3e" % (k, 1 - decided.mean(), d[decided].max()))
        assert 1 - decided.mean() <= 0.01
        assert d[decided].max() <= 1e-6
    assert np.abs(ref["iterates"][3] - ref["iterates"][0]).max() > 0.05
