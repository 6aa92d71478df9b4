"""-m gpu: the classifier kernels on anisotropic geometry and on layer orders the zoo does not have.  Every other GPU test of
dg_clf.hip and dg_clf_train.hip runs a model of network_builder.MODELS: square images, kernels and strides, every ReLU folded into
its producer, always a Softmax.  Here the four cases of tests/support/geometry_cases.py (whose properties tests/test_geometry_cpu.py
asserts) go through every entry point that walks those kernels -- dg_clf_forward, dg_eval_batch, dg_clf_input_gradient,
dg_clf_backward, dg_clf_class_gradient, dg_clf_jacobian, dg_clf_param_gradient, dg_clf_train -- at batch sizes 1, 5 and 11, value
for value against float64 (oracle/classifier_oracle.py, tests/support/train_reference.py, tests/support/blackbox_reference.py).

Tolerances are the project's: logits 2e-5 of max(1, max|ref|), probabilities 2e-6, input gradients 2e-5 of the reference's largest
element, weight gradients 1e-4 of each tensor's largest element, losses 1e-5 relative, Adam-updated weights rtol 1e-6 and 1e-6 of
the tensor's largest element.  Batches are drawn so that every float64 ReLU input stays MARGIN from zero, as in
tests/test_gpu_train_shapes.py.  Each test prints the figure it is about to assert (pytest -s shows them).

Measured on an MI355X, the largest deviation over every case and batch size: logits 2.2e-7 of max(1, max|ref|), probabilities
2.5e-7, dg_eval_batch's diffs 1.3e-7 relative, input gradients (with labels, own argmax, seeded, class gradients) 4.1e-7 of the
largest element, weight gradients 5.6e-7 of the largest element, gradient and training losses 9.7e-8 relative, weights after three
Adam steps within 1e-6 relative plus 3e-10 element by element (the absolute term allows 5e-8 and more); every Jacobian slice and
every result on a reused handle bit-identical.  The 54 tests take about three seconds.

Which test catches which break (each made alone in a scratch copy of the kernels, reads kept in bounds, this file run on it; the
parametrised cases that failed in brackets; "all" = every case):

    break                                    clf_conv2d_kernel            clf_conv2d_bwd_kernel        tr_wgrad_kernel
    pad_t and pad_l swapped                  forward, input, weight,      input, weight(adv)           weight, training
                                             training [G3, G4]            [G3, G4]                     [G3, G4]
    kh for kw in the weight index            forward, input, weight,      input, weight(adv)           weight, training
                                             training [G1, G2, G3]        [G1, G2, G3]                 [all]
    sh and sw swapped                        all four tests [all]         input, weight, training      weight, training [all]
                                                                          [all]
    the decode's extents swapped (oh / ow;   all four tests [all]         input, weight, training      weight, training [all]
    ih / iw where threads run over inputs)                                [all]
    pad_before = total - total / 2           forward, input, weight,      input, weight(adv)           weight, training
                                             training [G1, G3, G4]        [G1, G3, G4]                 [G1, G3, G4]

    forward = test_forward_and_eval_batch_match_float64, input = test_input_gradients_match_float64, weight =
    test_weight_gradients_match_float64 (adv: its adversarial half only, unless a convolution lies below another parameter layer),
    training = test_three_training_steps_track_float64.  G1's pads before are 1 and 1, so it cannot see the first row; G4's first
    kernel has kh = 1, where a * kh + c is a * kw + c; G2 is VALID and has no pad.

    clf_relu_bwd_kernel passing g unmasked   input [G4], weight(adv) [G4]: the ReLU in front of G4's first convolution.  G2's second
                                             ReLU cannot show it: the fused ReLU of the convolution below applies the same mask again.
    a ReLU fused into every Conv2D           all four tests [G4]: its second convolution has none.
    no fold across Dropout                   no test fails, and none should: ReLU(Dropout(x)) and Dropout(ReLU(x)) are the same
                                             float32 values and gradients (the mask is 0 or 1, keep > 0), so G4's ReLU run stand-alone
                                             behind the Dropout gives the results of the fold, which are those of float64.
"""
import functools

import numpy as np
import pytest

from defensegan_amd import _native
from defensegan_amd import network_builder as nb
from oracle import classifier_oracle as CO
from tests.support import blackbox_reference as BR
from tests.support import geometry_cases as G
from tests.support import train_reference as R
from tests.test_gpu_train_shapes import MARGIN, SEED, _adam, _check_grads, _check_loss, _device_gradient, _train

pytestmark = pytest.mark.gpu

STEP = {1: 0, 5: 2, 11: 3}                       # the Dropout step each batch size is differentiated at
CASES = [(name, B) for name in G.NAMES for B in G.BATCH_SIZES]
G2_UNREAD_ROWS, G2_UNREAD_COLUMN = [2, 5, 8, 11], 7


@functools.lru_cache(maxsize=None)
def _params(name):
    return tuple(G.params(name))


@functools.lru_cache(maxsize=None)
def _p64(name):
    return tuple((W.astype(np.float64), b.astype(np.float64)) for W, b in _params(name))


def _classes(name):
    return _params(name)[-1][1].size


def _device_model(name):
    m = G.model(name)
    m.set_weights(list(_params(name)))
    return m


def _margins(name, x, step, pass_=0):
    """Per image: the smallest |ReLU input| of the float64 forward, at evaluation and in the training phase of (step, pass_)."""
    layers = G.layers(name)
    masks = R.step_masks(layers, G.input_shape(name), len(x), SEED, step, pass_)
    return np.minimum(R.relu_margins(layers, _p64(name), x), R.relu_margins(layers, _p64(name), x, masks))


def _conditioned(name, x, step, rs):
    """x with every image redrawn whose float64 forward has a ReLU input closer than MARGIN to zero."""
    for _ in range(40):
        bad = _margins(name, x, step) < MARGIN
        if not bad.any():
            return x
        x = x.copy()
        x[bad] = G.images(name, int(bad.sum()), rs)
    raise AssertionError("no batch with every ReLU input %g from zero" % MARGIN)


@functools.lru_cache(maxsize=None)
def _batch(name, B):
    """The case's conditioned inputs and labels at batch size B: drawn once and shared by every test, which leave them unchanged."""
    rs = np.random.RandomState(1000 * B + sum(map(ord, name)))
    x = _conditioned(name, G.images(name, B, rs), STEP[B], rs)
    y = rs.randint(0, _classes(name), B).astype(np.int32)
    return x, y


def _close(what, got, ref, bound, floor=0.0):
    """max|got - ref| <= bound * max(floor, max|ref|), printed first."""
    scale = max(floor, float(np.abs(ref).max()))
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    print("%s: max|dev - f64| = %.3g = %.3g of %.3g" % (what, err, err / scale, scale))
    assert got.shape == ref.shape and scale > 0 and err <= bound * scale, (what, err, scale)


# ---------------------------------------------------------------------- forward
@pytest.mark.parametrize("name,B", CASES)
def test_forward_and_eval_batch_match_float64(name, B):
    m = _device_model(name)
    x, _ = _batch(name, B)
    lo, po = CO.forward(G.layers(name), _p64(name), x.astype(np.float64))
    out = m.fprop(x)
    assert out["logits"].shape == (B, _classes(name))
    _close("%s B=%d logits" % (name, B), out["logits"], lo, 2e-5, floor=1.0)
    err = np.abs(out["probs"] - po).max()
    print("%s B=%d probs: max|dev - f64| = %.3g" % (name, B, err))
    assert err <= 2e-6
    if G.layers(name)[-1][0] == "softmax":
        np.testing.assert_allclose(out["probs"].sum(axis=1), 1.0, atol=1e-6)
    else:
        np.testing.assert_array_equal(out["probs"], out["logits"])          # no Softmax: the probabilities are the logits
    # dg_eval_batch as tests/test_classifier.py::test_color_input_and_eval_batch_vs_oracle
    rs = np.random.RandomState(B)
    orig = np.clip(x + 0.1 * rs.standard_normal(x.shape), -1, 1).astype(np.float32)
    labels = po.argmax(axis=1).astype(np.int32)
    labels[::5] = (labels[::5] + 1) % _classes(name)                        # some wrong on purpose
    n_ok, preds, diffs = m.eval_batch(x, orig, labels)
    want_ok, want_preds, want_diffs = CO.eval_batch(po, labels, x.astype(np.float64), orig.astype(np.float64))
    assert n_ok == want_ok and np.array_equal(preds.cpu().numpy(), want_preds)
    print("%s B=%d diffs: relative %.3g" % (name, B, np.abs(diffs.cpu().numpy() / want_diffs - 1).max()))
    np.testing.assert_allclose(diffs.cpu().numpy(), want_diffs, rtol=2e-6)
    n2, p2, d2 = m.eval_batch(x)
    assert n2 == 0 and d2 is None and np.array_equal(p2.cpu().numpy(), want_preds)
    m.close()


# ---------------------------------------------------------------------- input gradients
def _seeded_reference(name, x, seed):
    """d(sum seed * logits)/dx by autograd, Dropout the identity."""
    import torch
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    z = R.logits(G.layers(name), R.as_params(_p64(name)), xt)
    (g,) = torch.autograd.grad(z, xt, torch.as_tensor(np.asarray(seed, np.float64)))
    return g.numpy()


def _g2_unread_is_zero(g):
    assert not g[:, G2_UNREAD_ROWS].any() and not g[:, :, G2_UNREAD_COLUMN].any()
    assert g[:, 0].any() and g[:, :, 0].any()


@pytest.mark.parametrize("name,B", CASES)
def test_input_gradients_match_float64(name, B):
    m = _device_model(name)
    x, labels = _batch(name, B)
    layers, x64, n = G.layers(name), x.astype(np.float64), _classes(name)
    what = "%s B=%d " % (name, B)
    got, cg = [], {}
    for lab in (labels, None):
        g = m.input_gradient(x, None if lab is None else np.array(lab))
        _close(what + ("input gradient" if lab is not None else "input gradient, own argmax"), g,
               CO.input_gradient(layers, _p64(name), x64, lab), 2e-5)
        got.append(g)
    rs = np.random.RandomState(B + 3)
    seed = rs.standard_normal((B, n)).astype(np.float32)
    g = m.backward(x, seed)
    _close(what + "seeded backward", g, _seeded_reference(name, x, seed), 2e-5)
    got.append(g)
    classes = rs.randint(0, n, B)
    for of_probs in (False, True):
        g = m.class_gradient(x, classes, of_probs=of_probs)
        _close(what + "class gradient of_probs=%d" % of_probs, g, BR.class_gradient(layers, _p64(name), x, classes, of_probs=of_probs), 2e-5)
        got.append(g)
        cg[of_probs] = g
        if B == 5:
            jac = m.jacobian(x, of_probs=of_probs)
            assert jac.shape == (B, n) + x.shape[1:]
            for k in range(n):                                       # slice k is the class gradient of class k, bit for bit
                np.testing.assert_array_equal(jac[:, k], m.class_gradient(x, np.full(B, k), of_probs=of_probs), err_msg="class %d" % k)
            np.testing.assert_array_equal(jac[np.arange(B), classes], g)
            got.append(jac.reshape((B * n,) + x.shape[1:]))
    if name == "G2":
        onehot = np.eye(n, dtype=np.float32)[classes]                # no Softmax: of_probs changes nothing, the seed is one-hot
        np.testing.assert_array_equal(cg[False], cg[True])
        np.testing.assert_array_equal(cg[False], m.backward(x, onehot))
        for g in got:
            _g2_unread_is_zero(g)
    m.close()


# ---------------------------------------------------------------------- weight gradients
@pytest.mark.parametrize("adv", [0.0, 0.15])
@pytest.mark.parametrize("name,B", CASES)
def test_weight_gradients_match_float64(name, B, adv):
    m = _device_model(name)
    layers, params, step = G.layers(name), list(_p64(name)), STEP[B]
    x, y = _batch(name, B)
    rs = np.random.RandomState(7000 + B)
    for attempt in range(10):
        loss, grads, xadv = _device_gradient(m, x, y, adv_eps=adv, lo=-1.0, hi=1.0, step=step)
        if adv == 0:
            break
        # the adversarial inputs are the device's: the images whose x_adv lands next to a kink are drawn again
        # (as are those whose inner FGSM forward, with the masks of pass 1, has one)
        near = (_margins(name, xadv, step, pass_=2) < MARGIN) | (_margins(name, x, step, pass_=1) < MARGIN)
        if not near.any():
            break
        x = x.copy()
        x[near] = G.images(name, int(near.sum()), rs)
        x = _conditioned(name, x, step, rs)
    else:
        raise AssertionError("no batch whose adversarial inputs keep every ReLU input %g from zero" % MARGIN)
    rl, rg, _ = R.param_gradient(layers, params, x, y, SEED, step, adv_eps=adv, lo=-1.0, hi=1.0, x_adv=xadv)
    what = "%s B=%d adv=%g" % (name, B, adv)
    assert all(np.abs(rW).max() > 0 and np.abs(rb).max() > 0 for rW, rb in rg)
    _check_loss(loss, rl, what)
    _check_grads(grads, rg, what)
    if adv > 0:
        assert xadv.min() >= -1.0 and xadv.max() <= 1.0 and np.abs(xadv - x).max() <= adv + 1e-6
        # against the float64 FGSM of the training-phase model where the sign of its input gradient is decided
        import torch
        p = R.as_params(params)
        masks = R.step_masks(layers, G.input_shape(name), B, SEED, step, 1)
        xin = torch.tensor(x.astype(np.float64), requires_grad=True)
        z = R.logits(layers, p, xin, masks)
        (gin,) = torch.autograd.grad(torch.nn.functional.cross_entropy(z, z.detach().argmax(dim=1), reduction="sum"), xin)
        gin = gin.numpy()
        decided = np.abs(gin) > 1e-4 * np.abs(gin).max()
        want = np.clip(x.astype(np.float64) + adv * np.sign(gin), -1.0, 1.0)
        # exact zeros are expected (dead ReLUs, dropped or unread pixels: G4 reads half its rows and passes half of those pixels
        # through its first ReLU); of the rest, nearly every sign is decided
        print("%s: the inner input gradient is non-zero on %.3f of the pixels, its sign decided on %.3f" % (what, (gin != 0).mean(), decided.mean()))
        assert (gin != 0).mean() > 0.1 and decided.sum() >= 0.9 * (gin != 0).sum()
        np.testing.assert_allclose(xadv[decided], want[decided], rtol=0, atol=1e-6)
        np.testing.assert_array_equal(xadv[gin == 0], x[gin == 0])          # sign(0) = 0: masked and unread pixels stay
        if name == "G2":
            _g2_unread_is_zero(xadv - x)
        if name == "G3":
            assert (gin == 0).mean() > 0.05                                  # the input Dropout's mask reaches the gradient
    m.close()


# ---------------------------------------------------------------------- three Adam steps
def _training_set(name, bs, n_steps, lr):
    """n_steps * bs images whose float64 trajectory keeps every ReLU input of every step MARGIN from zero (a redrawn image
    changes the weights of the later steps, so the steps are gone through again until none is left)."""
    layers, params = G.layers(name), list(_p64(name))
    rs = np.random.RandomState(sum(map(ord, name)) + 31)
    n = n_steps * bs
    X, y = G.images(name, n, rs), rs.randint(0, _classes(name), n).astype(np.int32)
    idx = rs.permutation(n).astype(np.int32)
    for _ in range(40):
        clean = True
        for s in range(n_steps):
            _, before = R.train(layers, params, X, y, idx[:s * bs], bs, lr, SEED)
            sel = idx[s * bs:(s + 1) * bs]
            masks = R.step_masks(layers, G.input_shape(name), bs, SEED, s, 0)
            bad = R.relu_margins(layers, before, X[sel], masks) < MARGIN
            if bad.any():
                X[sel[bad]] = G.images(name, int(bad.sum()), rs)
                clean = False
                break
        if clean:
            return X, y, idx
    raise AssertionError("no training set with every ReLU input %g from zero" % MARGIN)


@pytest.mark.parametrize("name", ["G1", "G4"])
def test_three_training_steps_track_float64(name):
    """dg_clf_train, three steps at B = 5, against train_reference.train: each step's loss to the loss tolerance, the final weights
    to the tolerances of test_gpu_train_shapes.py::test_adam_steps_one_to_six_value_for_value."""
    bs, n_steps, lr = 5, 3, 0.001
    X, y, idx = _training_set(name, bs, n_steps, lr)
    m = _device_model(name)
    _native.check(_native.load().dg_clf_adam_reset(m._handle))
    losses = _train(m, X, y, idx, n_steps, bs, lr, lo=-1.0, hi=1.0)
    ref_losses, ref_params = R.train(G.layers(name), list(_p64(name)), X, y, idx, bs, lr, SEED)
    assert losses.shape == ref_losses.shape == (n_steps,)
    for s in range(n_steps):
        _check_loss(float(losses[s]), float(ref_losses[s]), "%s step %d" % (name, s + 1))
    assert all(a[2] == n_steps for a in _adam(m))
    for i, ((W, b), (rW, rb), (W0, b0)) in enumerate(zip(m.get_weights(), ref_params, _params(name))):
        for k, got, want, start in (("W", W, rW, W0), ("b", b, rb, b0)):
            excess = np.abs(got - want) - 1e-6 * np.abs(want)
            print("%s layer %d %s after %d steps: max(|dev - f64| - 1e-6 |f64|) = %.3g, allowed %.3g; moved by %.3g"
                  % (name, i, k, n_steps, excess.max(), 1e-6 * np.abs(want).max(), np.abs(got - start).max()))
            assert np.abs(got - start).max() > 0.5 * lr
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max(), err_msg="layer %d %s" % (i, k))
    m.close()


# ---------------------------------------------------------------------- one handle across batch sizes
def _everything(m, name, B):
    """Every entry point's result at batch size B, as bytes."""
    x, y = _batch(name, B)
    rs = np.random.RandomState(B)
    classes = rs.randint(0, _classes(name), B)
    out = m.fprop(x)
    res = [out["logits"], out["probs"], m.eval_batch(x)[1].cpu().numpy(), m.input_gradient(x, np.array(y)), m.input_gradient(x, None),
           m.backward(x, rs.standard_normal((B, _classes(name))).astype(np.float32)), m.class_gradient(x, classes, of_probs=True)]
    for adv in (0.0, 0.15):
        loss, grads, xadv = _device_gradient(m, x, y, adv_eps=adv, lo=-1.0, hi=1.0, step=STEP[B])
        res += [np.float32(loss)] + [t for pair in grads for t in pair] + ([xadv] if adv > 0 else [])
    return [np.asarray(r).tobytes() for r in res]


@pytest.mark.parametrize("name", G.NAMES)
def test_one_handle_across_batch_sizes_is_bitwise_a_fresh_handle(name):
    """B = 11, then 1, then 5 on one handle (its workspaces sized for 11, the weight gradient's slots planned anew for every B):
    every result is that of a handle that has seen nothing else."""
    reused = _device_model(name)
    for B in (11, 1, 5):
        fresh = _device_model(name)
        want, got = _everything(fresh, name, B), _everything(reused, name, B)
        fresh.close()
        same = [a == b for a, b in zip(want, got)]
        print("%s B=%d: %d of %d results bit-identical" % (name, B, sum(same), len(same)))
        assert all(same), (name, B, same)
    reused.close()
