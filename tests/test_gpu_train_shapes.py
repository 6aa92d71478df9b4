"""-m gpu: classifier training on the device at the sizes it ships with.  tests/test_gpu_train.py compares gradients at 3 .. 7
images; here dg_clf_param_gradient and dg_clf_train are compared value for value with the float64 restatement
(tests/support/train_reference.py) over the batch sizes, models and input shapes at which the weight-gradient kernel changes
regime (train_reference.REGIMES, asserted in tests/test_train_cpu.py), with batches in which one dropped or doubled term of a
sum is an O(1) error, over Adam steps 1 .. 6, and across batch sizes on one handle.

Tolerances are the project's: 1e-4 of a gradient tensor's own largest element, 1e-5 relative on a loss, 1e-6 on an Adam step.
Measured on an MI355X over every case here: gradients within 1.7e-6 of the largest element, losses within 1.1e-6.
Each test prints the figure it is about to assert (pytest -s shows them).

What each kind of test is there to catch (checked by breaking dg_clf_train.hip one way at a time): a slot's last term dropped,
Kc rounded down, the last slot left out of the reduction, or a slot's tail chunk adding the next slot's first terms to db fail
test_weight_gradients_match_float64 and the isolated-image tests; lr_t without its sqrt term and a Dropout step counter stuck
at 0 fail test_adam_steps_one_to_six_value_for_value and the handle test; a label given to an index outside the set fails
test_an_index_outside_the_set_is_a_zero_image_without_a_label alone.  (A bias row of ones beyond a slot's end changes nothing:
the gradient column is zero there.)"""
import numpy as np
import pytest

from defensegan_amd import _native
from defensegan_amd import network_builder as nb
from defensegan_amd import utils_tf
from oracle import classifier_oracle as CO
from tests.support import train_reference as R

pytestmark = pytest.mark.gpu

SEED = 11241990


def _set_biases(m, params, seed, width=0.1):
    """init_like_reference leaves every bias zero: give the forward's bias path and the db rows something to carry."""
    rs = np.random.RandomState(seed)
    params = [(W, rs.uniform(-width, width, size=b.shape).astype(np.float32)) for W, b in params]
    m.set_weights(params)
    return params


def _images(m, n, rs):
    shape = (n,) + tuple(m.input_shape[1:])
    if shape[-1] == 1:
        return np.clip(rs.uniform(-0.5, 1.5, shape), 0, 1).astype(np.float32)
    return rs.uniform(-1, 1, shape).astype(np.float32)


def _batch(m, n, seed):
    """Seeded inputs in the model's range ([0, 1] with exact zeros and ones for 28 x 28 x 1, [-1, 1] for colour) and labels."""
    rs = np.random.RandomState(seed)
    x = _images(m, n, rs)
    m._ensure()
    return x, rs.randint(0, m.nb_classes, n).astype(np.int32)


# A ReLU input within float32 rounding of zero is decided differently in float64 and float32, and the two gradients then differ by
# that activation's whole term (measured on model F: an input of -3.65e-8 at B = 130 moved the first convolution's dK by 7e-3 of
# its largest element, exactly g * patch; one of 9.3e-8 at B = 100 moved the second's by 9e-4).  Among the 1.6 million ReLU inputs
# of such a batch the smallest is about 1e-7 to 1e-6, so the value checks draw their batches so that the float64 forward keeps
# every ReLU input at least MARGIN from zero: about ten times the float32 rounding of these sums (unit-norm weight columns,
# inputs in [-1, 1]: a few 1e-8 to 1e-7).  The choice looks at the float64 reference alone.
MARGIN = 1e-6


def _conditioned(m, params, x, seed, step=0, pass_=0):
    """x with every image redrawn whose float64 training-phase forward has a ReLU input closer than MARGIN to zero."""
    layers, shape = R.describe(m), tuple(m.input_shape[1:])
    masks = R.step_masks(layers, shape, len(x), SEED, step, pass_)
    rs = np.random.RandomState(seed + 77777)
    for _ in range(40):
        bad = R.relu_margins(layers, params, x, masks) < MARGIN
        if not bad.any():
            return x
        x = x.copy()
        x[bad] = _images(m, int(bad.sum()), rs)
    raise AssertionError("no batch with every ReLU input %g from zero" % MARGIN)


def _clip(m):
    return (0.0, 1.0) if m.input_shape[-1] == 1 else (-1.0, 1.0)


def _device_gradient(m, x, y, adv_eps=0.0, lo=0.0, hi=1.0, seed=SEED, step=0):
    import torch
    m._ensure()
    dev = torch.device("cuda", m._device)
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    yt = torch.from_numpy(np.asarray(y, np.int32)).to(dev)
    shapes = m.param_shapes()
    total = sum(int(np.prod(ws)) + int(np.prod(bs)) for ws, bs in shapes)
    grads = torch.empty(total, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    xadv = torch.empty_like(xt)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _native.check(_native.load().dg_clf_param_gradient(m._handle, xt.data_ptr(), yt.data_ptr(), len(x), float(adv_eps), lo, hi, seed,
                                                           step, grads.data_ptr(), loss.data_ptr(), xadv.data_ptr(), stream))
    torch.cuda.synchronize(dev)
    return float(loss.item()), _split(grads.cpu().numpy(), shapes), (xadv.cpu().numpy() if adv_eps > 0 else None)


def _split(flat, shapes):
    out, off = [], 0
    for ws, bs in shapes:
        nw, nbias = int(np.prod(ws)), int(np.prod(bs))
        out.append((flat[off:off + nw].reshape(ws), flat[off + nw:off + nw + nbias]))
        off += nw + nbias
    return out


def _train(m, X, y, idx, n_steps, batch_size, lr, adv_eps=0.0, lo=0.0, hi=1.0, seed=SEED):
    """dg_clf_train through the C ABI (no Adam reset, unlike utils_tf.model_train): the per-step losses."""
    import torch
    m._ensure()
    dev = torch.device("cuda", m._device)
    Xt = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(dev)
    yt = torch.from_numpy(np.asarray(y, np.int32)).to(dev)
    it = torch.from_numpy(np.asarray(idx, np.int32)).to(dev)
    assert it.numel() >= n_steps * batch_size
    loss = torch.empty(max(n_steps, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _native.check(_native.load().dg_clf_train(m._handle, Xt.data_ptr(), yt.data_ptr(), len(X), it.data_ptr(), n_steps, batch_size, lr,
                                                  float(adv_eps), lo, hi, seed, loss.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return loss.cpu().numpy()[:n_steps]


def _adam(m):
    return [utils_tf.adam_state(m, i) for i in range(len(m.param_shapes()))]


def _same_adam(a, b):
    for (m0, v0, t0), (m1, v1, t1) in zip(a, b):
        assert t0 == t1
        for p, q in zip(m0 + v0, m1 + v1):
            np.testing.assert_array_equal(p, q)


def _check_grads(dev, ref, what, bound=1e-4, weights_only=False):
    """Every tensor within bound * its own reference's largest element (tests/test_gpu_train.py's form)."""
    for i, ((dW, db), (rW, rb)) in enumerate(zip(dev, ref)):
        for name, d, r in (("W", dW, rW),) + (() if weights_only else (("b", db, rb),)):
            scale = np.abs(r).max()
            err = np.abs(d - r).max()
            print("%s layer %d d%s: max|dev - ref| = %.3g = %.3g of max|ref| = %.3g" % (what, i, name, err, err / max(scale, 1e-300), scale))
            assert err <= bound * scale + 1e-12, "%s layer %d d%s: max|dev - ref| = %g, max|ref| = %g" % (what, i, name, err, scale)


def _check_loss(loss, ref, what):
    print("%s loss: dev %.9g ref %.9g relative %.3g" % (what, loss, ref, abs(loss - ref) / abs(ref)))
    assert abs(loss - ref) <= 1e-5 * abs(ref), (what, loss, ref)


# ---------------------------------------------------------------------- weight gradients over batch sizes, models and shapes
# Batch sizes 1 .. 200 on E (Linear only) and F (convolutions), clean and adversarial at 128; D, Y, Q, Z at a small batch and at
# the shipped 128 (the float64 reference of the widest, Z at 128, takes about a second); model A on 64 x 64 x 3 with 2 classes
# and the adversarial half clipped to [-1, 1].  Which regime of the kernel each case reaches: train_reference.regimes.
@pytest.mark.parametrize("key,B,adv", R.GRADIENT_CASES)
def test_weight_gradients_match_float64(key, B, adv):
    m = R.shape_model(key)
    params = _set_biases(m, m.init_like_reference(seed=sum(map(ord, key))), seed=B)
    x, y = _batch(m, B, seed=B + 1)
    lo, hi = _clip(m)
    step = B % 5
    layers = R.describe(m)
    for attempt in range(10):
        x = _conditioned(m, params, x, seed=B + attempt, step=step)
        loss, grads, xadv = _device_gradient(m, x, y, adv_eps=adv, lo=lo, hi=hi, step=step)
        if adv == 0:
            break
        # the adversarial inputs are the device's: the images whose x_adv lands next to a kink are drawn again
        near = R.relu_margins(layers, params, xadv, R.step_masks(layers, tuple(x.shape[1:]), B, SEED, step, 2)) < MARGIN
        if not near.any():
            break
        x[near] = _images(m, int(near.sum()), np.random.RandomState(1000 * B + attempt))
    else:
        raise AssertionError("no batch whose adversarial inputs keep every ReLU input %g from zero" % MARGIN)
    # the adversarial half on the device's own x_adv: float64 and float32 differ in the sign of near-zero input gradients
    rl, rg, _ = R.param_gradient(R.describe(m), params, x, y, SEED, step, adv_eps=adv, lo=lo, hi=hi, x_adv=xadv)
    what = "%s B=%d adv=%g" % (key, B, adv)
    _check_loss(loss, rl, what)
    _check_grads(grads, rg, what)
    if adv > 0:
        assert xadv.min() >= lo and xadv.max() <= hi and np.abs(xadv - x).max() <= adv + 1e-6
        _, _, ref_xadv = R.param_gradient(R.describe(m), params, x, y, SEED, step, adv_eps=adv, lo=lo, hi=hi)
        same = (np.abs(xadv - ref_xadv) <= 1e-6).mean()
        print("%s: x_adv equals the float64 FGSM on %.5f of the pixels" % (what, same))
        assert same > 0.99
    m.close()


# ---------------------------------------------------------------------- input gradient and seeded backward for the rest of the zoo
def _oracle_backward(layers, params, x, seed):
    """d(sum seed * logits)/dx by the oracle's layer functions (the form of tests/test_gpu_cw.py; Dropout is the identity)."""
    acts, used, it = [x], [], iter(params)
    body = [L for L in layers if L[0] != "softmax"]
    for L in body:
        h = acts[-1]
        if L[0] == "conv":
            W, b = next(it); used.append(W); h = CO.conv2d(h, W, b, L[3], L[4])
        elif L[0] == "linear":
            W, b = next(it); used.append(W); h = h @ W + b
        elif L[0] == "relu":
            h = np.maximum(h, 0)
        elif L[0] == "flatten":
            h = h.reshape(len(h), -1)
        acts.append(h)
    g, pi = seed, len(used)
    for li in range(len(body) - 1, -1, -1):
        L, xin, out = body[li], acts[li], acts[li + 1]
        if L[0] == "conv":
            pi -= 1; g = CO.conv2d_backward_input(g, used[pi], xin.shape, L[3], L[4])
        elif L[0] == "linear":
            pi -= 1; g = g @ used[pi].T
        elif L[0] == "relu":
            g = g * (out > 0)
        elif L[0] == "flatten":
            g = g.reshape(xin.shape)
    return g


def _oracle_layers(m):
    return [L if L[0] != "dropout" else ("dropout",) for L in R.describe(m)]


@pytest.mark.parametrize("name", ["C", "D", "Y", "Q", "Z"])
def test_input_gradient_and_fgsm_vs_oracle_rest_of_the_zoo(name):
    """tests/test_classifier.py::test_input_gradient_and_fgsm_vs_oracle for the models it leaves out."""
    m = nb.MODELS[name]()
    params = _set_biases(m, m.init_like_reference(seed=11), seed=12)
    rs = np.random.RandomState(12)
    x = rs.uniform(0, 1, size=(6, 28, 28, 1)).astype(np.float32)
    labels = rs.randint(0, 10, size=6).astype(np.int32)
    p64 = [(W.astype(np.float64), b.astype(np.float64)) for W, b in params]
    for lab in (labels, None):
        g = m.input_gradient(x, lab)
        xo, go = CO.fgsm(_oracle_layers(m), p64, x.astype(np.float64), 0.3, 0.0, 1.0, lab)
        print("%s input gradient: max|dev - oracle| = %.3g of max|oracle|" % (name, np.abs(g - go).max() / np.abs(go).max()))
        np.testing.assert_allclose(g, go, rtol=0, atol=2e-5 * np.abs(go).max())
        xa = nb.FastGradientMethod(m).generate(x, eps=0.3, clip_min=0.0, clip_max=1.0, y=lab)
        assert xa.min() >= 0.0 and xa.max() <= 1.0 and np.abs(xa - x).max() <= 0.3 + 1e-6
        decided = np.abs(go) > 1e-4 * np.abs(go).max()           # sign() is only comparable away from 0
        assert decided.mean() > 0.5
        np.testing.assert_allclose(xa[decided], xo[decided], rtol=0, atol=1e-6)
    m.close()


@pytest.mark.parametrize("name", ["C", "D", "Y", "Q", "Z"])
def test_seeded_backward_matches_oracle_rest_of_the_zoo(name):
    """tests/test_gpu_cw.py::test_seeded_backward_matches_oracle_and_ce_seed_is_bitwise_fgsm for the models it leaves out."""
    m = nb.MODELS[name]()
    params = _set_biases(m, m.init_like_reference(seed=ord(name)), seed=13)
    rs = np.random.RandomState(11)
    x = rs.uniform(0, 1, (5, 28, 28, 1)).astype(np.float32)
    seed = rs.standard_normal((5, 10)).astype(np.float32)
    g = m.backward(x, seed)
    p64 = [(W.astype(np.float64), b.astype(np.float64)) for W, b in params]
    want = _oracle_backward(_oracle_layers(m), p64, x.astype(np.float64), seed.astype(np.float64))
    print("%s seeded backward: max|dev - oracle| = %.3g of max|oracle|" % (name, np.abs(g - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(g, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # the CE seed, bit for bit as dg_clf_input_gradient forms it: the input gradient of an identity Linear on the logits
    logits = m.get_logits(x)
    ident = nb.MLP([nb.Flatten(), nb.Linear(10), nb.Softmax()], input_shape=(None, 1, 1, 10))
    ident.set_weights([(np.eye(10, dtype=np.float32), np.zeros(10, np.float32))])
    labels = rs.randint(0, 10, 5).astype(np.int32)
    ce_seed = ident.input_gradient(logits.reshape(5, 1, 1, 10), labels=labels).reshape(5, 10)
    assert m.backward(x, ce_seed).tobytes() == m.input_gradient(x, labels=labels).tobytes()
    ident.close()
    m.close()


# ---------------------------------------------------------------------- batches in which one term is the whole gradient
# With zero biases an all-zero image adds exactly nothing to any dW (tests/test_train_cpu.py checks that on the reference), so a
# batch whose only non-zero image is s makes image s's terms the whole of every dW: a term the kernel drops, or counts twice, is
# an error of the order of the gradient itself, not of 1 / K of it.  The images are those next to the slot boundaries of the
# planner (train_reference.boundary_images): E at 130 has slots [0, 65) and [65, 130) in every layer; F at 128 has 256 slots of
# 98 terms cutting every image of the first convolution in two, 13 slots of 247 cutting images 9 and 118 of the second, and two
# slots of 64 in the last two layers.
ISOLATED = [("E", 130), ("F", 128)]


def _zero_bias_model(name):
    m = nb.MODELS[name]()
    params = m.init_like_reference(seed=ord(name) + 1)
    assert not any(b.any() for _, b in params)
    return m, params


@pytest.mark.parametrize("name,B", ISOLATED)
def test_one_nonzero_image_gives_its_own_term(name, B):
    m, params = _zero_bias_model(name)
    layers = R.describe(m)
    x, y = _batch(m, B, seed=B + 7)
    x = _conditioned(m, params, x, seed=B + 7)
    chosen = R.boundary_images(layers, (28, 28, 1), B)
    assert chosen == ([0, 64, 65, 129] if name == "E" else [0, 9, 63, 64, 118, 127])
    for s in chosen:
        xs = np.zeros_like(x)
        xs[s] = x[s]
        loss, grads, _ = _device_gradient(m, xs, y)
        rl, rg, _ = R.param_gradient(layers, params, xs, y, SEED, 0)
        assert all(np.abs(rW).max() > 0 for rW, _ in rg)
        _check_loss(loss, rl, "%s B=%d image %d alone" % (name, B, s))
        _check_grads(grads, rg, "%s B=%d image %d alone" % (name, B, s), weights_only=True)
    m.close()


def test_corner_pixels_put_the_signal_on_the_first_and_last_term():
    """Model F, B = 128, SAME padding 3 before and 3 after an 8 x 8 stride-2 kernel.  Image 0 non-zero at its top-left pixel only:
    it meets the kernel at rows a in {3, 1} for output rows {0, 1}, so dK[3, 3] of the first convolution is the single term
    k = 0.  Image 127 non-zero at its bottom-right pixel only: rows a in {4, 6} for output rows {13, 12}, so dK[4, 4] is the single
    term k = K - 1, the last term of the last slot."""
    m, params = _zero_bias_model("F")
    layers = R.describe(m)
    B = 128
    _, y = _batch(m, B, seed=3)
    for s, (py, px), (a, c) in ((0, (0, 0), (3, 3)), (B - 1, (27, 27), (4, 4))):
        xs = np.zeros((B, 28, 28, 1), np.float32)
        xs[s, py, px, 0] = 0.75
        loss, grads, _ = _device_gradient(m, xs, y)
        rl, rg, _ = R.param_gradient(layers, params, xs, y, SEED, 0)
        rK = rg[0][0]
        assert np.abs(rK[a, c]).max() > 0.1 * np.abs(rK).max()            # the single-term entries carry the tensor's scale
        touched = np.abs(rK).reshape(8, 8, -1).max(axis=2) > 0
        assert touched.sum() == 4 and touched[a, c]
        _check_loss(loss, rl, "F corner pixel of image %d" % s)
        _check_grads(grads, rg, "F corner pixel of image %d" % s, weights_only=True)
        np.testing.assert_array_equal(grads[0][0][~touched], 0)            # nothing leaks into the kernel rows the pixel never meets
    m.close()


@pytest.mark.parametrize("name,B", ISOLATED)
def test_full_batch_minus_its_complement_is_the_isolated_gradient(name, B):
    """Every image non-zero except the chosen ones, differenced against the full batch on the device: per-image terms add, so the
    difference is the gradient of the chosen images alone.  A term counted twice, or leaking from a neighbour, shows here.
    Tolerance: each of the two large sums may differ from float64 by the project's 1e-4 of its largest element (asserted for
    these very batch sizes above), so their difference is within 2e-4 of the full gradient's largest element; the isolated
    gradient is asserted to be at least 20 times that, so one doubled image of the six (four) stands far outside it."""
    m, params = _zero_bias_model(name)
    layers = R.describe(m)
    x, y = _batch(m, B, seed=B + 9)
    x = _conditioned(m, params, x, seed=B + 9)
    chosen = R.boundary_images(layers, (28, 28, 1), B)
    alone, rest = np.zeros_like(x), x.copy()
    alone[chosen] = x[chosen]
    rest[chosen] = 0
    _, g_full, _ = _device_gradient(m, x, y)
    _, g_rest, _ = _device_gradient(m, rest, y)
    _, g_alone, _ = _device_gradient(m, alone, y)
    _, r_full, _ = R.param_gradient(layers, params, x, y, SEED, 0)
    _, r_alone, _ = R.param_gradient(layers, params, alone, y, SEED, 0)
    for i in range(len(r_full)):
        tol = 2e-4 * np.abs(r_full[i][0]).max()
        scale = np.abs(r_alone[i][0]).max()
        assert scale >= 20 * tol, (i, scale, tol)
        diff = g_full[i][0] - g_rest[i][0]
        err_ref, err_dev = np.abs(diff - r_alone[i][0]).max(), np.abs(diff - g_alone[i][0]).max()
        print("%s B=%d layer %d: (full - rest) - alone: %.3g vs float64, %.3g vs device, tolerance %.3g, max|alone| %.3g"
              % (name, B, i, err_ref, err_dev, tol, scale))
        assert err_ref <= tol and err_dev <= tol, (i, err_ref, err_dev, tol)
    m.close()


# ---------------------------------------------------------------------- Adam steps 1 .. 6 and the step counter
def _twin(name):
    a, b = nb.MODELS[name](), nb.MODELS[name]()
    params = _set_biases(a, a.init_like_reference(seed=ord(name)), seed=5)
    b.set_weights(params)
    return a, b, params


@pytest.mark.parametrize("name,adv", [("A", 0.0), ("F", 0.15)])
def test_adam_steps_one_to_six_value_for_value(name, adv):
    """dg_clf_train one step per call.  Before step t the trained model's weights and moments are read; a second model with those
    weights gives the step's gradient (dg_clf_param_gradient with the Dropout step t - 1); TF Adam restated in float32 is applied
    to it and compared with what the step left: lr_t at every t, both moments' accumulation, and the step counter that draws
    model A's Dropout masks.  Each step starts from the device's own state, so nothing accumulates over the six."""
    m, twin, _ = _twin(name)
    bs, lr = 8, 0.001
    X, y = _batch(m, 6 * bs, seed=21)
    idx = np.random.RandomState(3).permutation(6 * bs).astype(np.int32)
    _native.check(_native.load().dg_clf_adam_reset(m._handle))
    losses = []
    for t in range(1, 7):
        before_w, before_a = m.get_weights(), _adam(m)
        assert all(a[2] == t - 1 for a in before_a)
        sel = idx[(t - 1) * bs:t * bs]
        twin.set_weights(before_w)
        gl, grads, _ = _device_gradient(twin, X[sel], y[sel], adv_eps=adv, step=t - 1)
        loss = _train(m, X, y, sel, 1, bs, lr, adv_eps=adv)
        assert loss[0] == np.float32(gl)                        # the same kernels on the same state: the same bits
        losses.append(loss[0])
        after_w, after_a = m.get_weights(), _adam(m)
        for i in range(len(before_w)):
            (mm, vv, tt) = after_a[i]
            assert tt == t
            for k in range(2):                                  # W, b
                want, wm, wv = R.adam_update(before_w[i][k], grads[i][k], before_a[i][0][k], before_a[i][1][k], t, lr, dtype=np.float32)
                for what, got, w in (("p", after_w[i][k], want), ("m", mm[k], wm), ("v", vv[k], wv)):
                    np.testing.assert_allclose(got, w, rtol=1e-6, atol=1e-6 * np.abs(w).max(),
                                               err_msg="step %d layer %d %s %s" % (t, i, "Wb"[k], what))
                assert np.abs(after_w[i][k] - before_w[i][k]).max() > 0
    # one call of six steps is the six calls, bit for bit
    m6, _, params = _twin(name)
    _native.check(_native.load().dg_clf_adam_reset(m6._handle))
    losses6 = _train(m6, X, y, idx, 6, bs, lr, adv_eps=adv)
    np.testing.assert_array_equal(losses6, np.asarray(losses, np.float32))
    for (W, b), (W6, b6) in zip(m.get_weights(), m6.get_weights()):
        np.testing.assert_array_equal(W, W6)
        np.testing.assert_array_equal(b, b6)
    _same_adam(_adam(m), _adam(m6))
    # a reset returns t to 0 and clears the moments; the weights stay
    trained = m.get_weights()
    _native.check(_native.load().dg_clf_adam_reset(m._handle))
    for (mm, vv, tt) in _adam(m):
        assert tt == 0 and not any(p.any() for p in mm + vv)
    for (W, b), (W2, b2) in zip(trained, m.get_weights()):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    for q in (m, twin, m6):
        q.close()


# ---------------------------------------------------------------------- one handle across batch sizes, the gather, the last batch
def _small_a():
    m, twin = nb.model_a(nb_filters=16), nb.model_a(nb_filters=16)
    params = _set_biases(m, m.init_like_reference(seed=8), seed=9)
    twin.set_weights(params)
    return m, twin, params


def test_one_handle_across_batch_sizes_keeps_results_and_adam_state():
    """B = 5 -> 130 -> 5 -> 64 on one handle (the workspace grows once, the slots are planned anew for every B), each against
    float64, the two B = 5 results bit-identical; the Adam state of an earlier step is untouched by the gradient calls, and a
    training step at batch 32 on the same handle continues from it."""
    m, twin, _ = _small_a()
    layers = R.describe(m)
    lr = 0.001
    X, y = _batch(m, 130, seed=31)
    _native.check(_native.load().dg_clf_adam_reset(m._handle))
    _train(m, X, y, np.arange(8, dtype=np.int32), 1, 8, lr)
    params, state = m.get_weights(), _adam(m)
    assert all(a[2] == 1 and a[0][0].any() for a in state)
    got = {}
    for visit, B in enumerate((5, 130, 5, 64)):
        loss, grads, _ = _device_gradient(m, X[:B], y[:B], step=2)
        rl, rg, _ = R.param_gradient(layers, params, X[:B], y[:B], SEED, 2)
        _check_loss(loss, rl, "visit %d B=%d" % (visit, B))
        _check_grads(grads, rg, "visit %d B=%d" % (visit, B))
        got[visit] = (loss, grads)
    assert got[0][0] == got[2][0]
    for (W0, b0), (W2, b2) in zip(got[0][1], got[2][1]):
        np.testing.assert_array_equal(W0, W2)
        np.testing.assert_array_equal(b0, b2)
    _same_adam(state, _adam(m))
    for (W, b), (W2, b2) in zip(params, m.get_weights()):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    # the step at batch 32: Adam's step 2 from the state of step 1
    sel = np.arange(40, 72, dtype=np.int32)
    twin.set_weights(params)
    _, grads, _ = _device_gradient(twin, X[sel], y[sel], step=1)
    _train(m, X, y, sel, 1, 32, lr)
    after_w, after_a = m.get_weights(), _adam(m)
    for i in range(len(params)):
        assert after_a[i][2] == 2
        for k in range(2):
            want, wm, wv = R.adam_update(params[i][k], grads[i][k], state[i][0][k], state[i][1][k], 2, lr, dtype=np.float32)
            for what, g, w in (("p", after_w[i][k], want), ("m", after_a[i][0][k], wm), ("v", after_a[i][1][k], wv)):
                np.testing.assert_allclose(g, w, rtol=1e-6, atol=1e-6 * np.abs(w).max(), err_msg="layer %d %s %s" % (i, "Wb"[k], what))
    m.close()
    twin.close()


def test_an_index_outside_the_set_is_a_zero_image_without_a_label():
    """include/defensegan_hip.h: "an index outside [0, n) reads a zero image that contributes nothing".  Indices -1, n and n + 1000
    in three slots of a batch of 16: the step's loss and gradients are those of the batch with these rows replaced by a zero
    image carrying no label, the divisor staying 16.  The gradients are read from Adam's first moment after the first step
    (m = 0.1 g from zero moments)."""
    m, _, params = _small_a()
    n, bs = 40, 16
    X, y = _batch(m, n, seed=41)
    idx = np.random.RandomState(5).permutation(n)[:bs].astype(np.int32)
    idx[[1, 6, 15]] = [-1, n, n + 1000]
    _native.check(_native.load().dg_clf_adam_reset(m._handle))
    loss = _train(m, X, y, idx, 1, bs, 0.001)
    ok = (idx >= 0) & (idx < n)
    xb = np.where(ok[:, None, None, None], X[np.clip(idx, 0, n - 1)], 0).astype(np.float32)
    yb = np.where(ok, y[np.clip(idx, 0, n - 1)], -1)
    rl, rg, _ = R.param_gradient(R.describe(m), params, xb, yb, SEED, 0)
    _check_loss(float(loss[0]), rl, "three rows outside the set")
    grads = [(mm[0] / np.float32(0.1), mm[1] / np.float32(0.1)) for mm, _, _ in _adam(m)]
    _check_grads(grads, rg, "three rows outside the set")
    # and it is not the gradient of the batch that gives those rows a label
    _, wrong, _ = R.param_gradient(R.describe(m), params, xb, np.where(ok, yb, 0), SEED, 0)
    assert np.abs(wrong[-1][1] - rg[-1][1]).max() > 1e-2 * np.abs(rg[-1][1]).max()
    m.close()


def test_model_train_shifts_the_last_batch_back():
    """n = 100 images in batches of 16: seven steps, the last on images 84 .. 99 of the permutation (cleverhans' batch_indices).
    Per-step losses against the float64 run on the same indices: the first step to the loss tolerance, the rest to the 1e-2 of
    tests/test_gpu_train.py's trajectory test (Adam's normalised steps amplify rounding where a gradient is near zero)."""
    m, _, params = _small_a()
    X, y = _batch(m, 100, seed=51)
    idx = utils_tf.epoch_indices(np.random.RandomState(7), 100, 16)
    perm = list(range(100))
    np.random.RandomState(7).shuffle(perm)
    assert idx.shape == (112,) and idx[96:].tolist() == perm[84:100]
    losses = utils_tf.model_train(m, X, y, args={"nb_epochs": 1, "batch_size": 16, "learning_rate": 0.001}, rng=np.random.RandomState(7),
                                  return_losses=True)
    ref, _ = R.train(R.describe(m), params, X, y, idx, 16, 0.001, SEED)
    assert losses.shape == ref.shape == (7,)
    rel = np.abs(losses - ref) / np.abs(ref)
    print("per-step relative loss differences:", rel)
    assert rel[0] <= 1e-5 and rel.max() <= 1e-2
    assert _adam(m)[0][2] == 7
    m.close()
