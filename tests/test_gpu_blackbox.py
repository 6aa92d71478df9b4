"""-m gpu: the black-box substitute attack on the device (dg_clf_class_gradient, dg_clf_jacobian, dg_jacobian_augment,
blackbox.train_sub, blackbox.blackbox) against the float64 restatement of tests/support/blackbox_reference.py, which
tests/test_blackbox_cpu.py pins on its own.

Tolerance of the class gradient: the project's for dg_clf_backward, rtol 1e-5 and atol 1e-5 of the reference's largest element.
Each test prints the figure it is about to assert (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

from defensegan_amd import _native, attacks_tf, blackbox, gan_defense as gd, network_builder as nb, utils_tf
from tests.support import blackbox_reference as BR
from tests.support import train_reference as R

pytestmark = pytest.mark.gpu

MARGIN = 1e-6          # as tests/test_gpu_train_shapes.py: float64 ReLU inputs stay this far from zero


def _model(key, seed=0):
    if key == "A64":
        m = nb.model_a(nb_classes=2, input_shape=(None, 64, 64, 3))
    else:
        m = nb.MODELS[key]()
    return m, m.init_like_reference(seed=seed)


def _images(m, n, rs):
    return rs.uniform(0, 1, (n,) + tuple(m.input_shape[1:])).astype(np.float32)


def _conditioned(m, params, n, seed):
    """n images whose float64 evaluation forward keeps every ReLU input at least MARGIN from zero."""
    rs = np.random.RandomState(seed)
    layers = R.describe(m)
    x = _images(m, n, rs)
    for _ in range(40):
        bad = R.relu_margins(layers, params, x) < MARGIN
        if not bad.any():
            return x
        x[bad] = _images(m, int(bad.sum()), rs)
    raise AssertionError("no batch with every ReLU input %g from zero" % MARGIN)


# ---------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("key,B", [("A", 5), ("C", 5), ("E", 5), ("F", 5), ("A64", 3)])
def test_class_gradient_matches_float64(key, B):
    m, params = _model(key)
    x = _conditioned(m, params, B, seed=11)
    classes = np.random.RandomState(5).randint(0, m.nb_classes, B)
    layers = R.describe(m)
    for of_probs in (True, False):
        g = m.class_gradient(x, classes, of_probs=of_probs)
        ref = BR.class_gradient(layers, params, x, classes, of_probs=of_probs)
        scale = np.abs(ref).max()
        assert scale > 0
        print("%s of_probs=%d: max|dev - f64| = %.3g of max|f64| (%.3g)" % (key, of_probs, np.abs(g - ref).max() / scale, scale))
        np.testing.assert_allclose(g, ref, rtol=1e-5, atol=1e-5 * scale)
    m.close()


# ---------------------------------------------------------------------- 2. the logits' seed is onehot
@pytest.mark.parametrize("key", ["A", "F"])
def test_logit_class_gradient_is_bitwise_backward_of_onehot(key):
    m, params = _model(key)
    x = _images(m, 4, np.random.RandomState(1))
    c = np.array([3, 0, 9, 3])
    onehot = np.zeros((4, m.nb_classes), np.float32)
    onehot[np.arange(4), c] = 1
    np.testing.assert_array_equal(m.class_gradient(x, c, of_probs=False), m.backward(x, onehot))
    assert not np.array_equal(m.class_gradient(x, c, of_probs=True), m.backward(x, onehot))
    m.close()


def test_a_model_without_softmax_is_differentiated_at_its_logits():
    m = nb.MLP([nb.Flatten(), nb.Linear(16), nb.ReLU(), nb.Linear(3)], (None, 6, 5, 2))
    m.init_like_reference(seed=2)
    x = _images(m, 3, np.random.RandomState(1))
    c = np.array([2, 0, 1])
    onehot = np.eye(3, dtype=np.float32)[c]
    np.testing.assert_array_equal(m.class_gradient(x, c, of_probs=True), m.backward(x, onehot))
    m.close()


def test_host_classes_are_checked_and_device_classes_out_of_range_give_zero():
    import torch
    m, _ = _model("E")
    x = _images(m, 3, np.random.RandomState(1))
    for bad in ([0, 1, 10], [0, -1, 2], [0, 1], [0.5, 1, 2]):
        with pytest.raises(ValueError, match="class indices"):
            m.class_gradient(x, bad)
    with pytest.raises(ValueError, match="x must be"):
        m.class_gradient(x[:, :27], [0, 1, 2])
    with pytest.raises(ValueError, match="x must be"):
        m.jacobian(x.reshape(3, 784))
    xt = torch.from_numpy(x).cuda()
    for of_probs in (True, False):
        g = m.class_gradient(xt, torch.tensor([4, 10, -1], dtype=torch.int32).cuda(), of_probs=of_probs).cpu().numpy()
        assert np.abs(g[0]).max() > 0 and (g[1] == 0).all() and (g[2] == 0).all()
    m.close()


# ---------------------------------------------------------------------- 3. the Jacobian
@pytest.mark.parametrize("key", ["E", "F", "A64"])
def test_jacobian_slices_are_bitwise_class_gradients(key):
    m, _ = _model(key)
    x = _images(m, 3, np.random.RandomState(2))
    for of_probs in (True, False):
        jac = m.jacobian(x, of_probs=of_probs)
        assert jac.shape == (3, m.nb_classes) + x.shape[1:]
        for k in range(m.nb_classes):
            np.testing.assert_array_equal(jac[:, k], m.class_gradient(x, np.full(3, k), of_probs=of_probs), err_msg="class %d" % k)
        np.testing.assert_array_equal(jac, m.jacobian(x, of_probs=of_probs))          # reproducible from call to call
    if m.nb_classes == 10:
        # the probabilities sum to 1: their gradients sum to zero, up to the 1e-5 of the largest element each of the ten may be off by
        jp = m.jacobian(x, of_probs=True).astype(np.float64)
        assert np.abs(jp.sum(axis=1)).max() <= 1e-4 * np.abs(jp).max()
    m.close()


# ---------------------------------------------------------------------- 4. the augmentation
def _augment_native(m, X, labels, lmbda, batch_size, in_place=False):
    import torch
    n = len(X)
    dev = torch.device("cuda", m._device)
    y = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
    if in_place:
        buf = torch.zeros((2 * n,) + X.shape[1:], dtype=torch.float32, device=dev)
        buf[:n] = torch.from_numpy(X)
        src = out = buf
    else:
        src = torch.from_numpy(X).to(dev)
        out = torch.full((2 * n,) + X.shape[1:], 7.0, dtype=torch.float32, device=dev)
    _native.check(_native.load().dg_jacobian_augment(m._handle, src.data_ptr(), y.data_ptr(), n, float(lmbda), int(batch_size),
                                                     out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out.cpu().numpy()


@pytest.mark.parametrize("key,n,batch_size", [("F", 5, 2), ("E", 130, 128), ("F", 130, 128)])
def test_augmentation_is_the_sign_step_and_independent_of_the_chunking(key, n, batch_size):
    m, _ = _model(key)
    rs = np.random.RandomState(n)
    X = _images(m, n, rs)
    X[0] = rs.randint(0, 2, X[0].shape)                     # pixels at 0 and at 1: the step must leave [0, 1]
    labels = rs.randint(0, m.nb_classes, n)
    lmbda = 0.1
    out = attacks_tf.jacobian_augmentation(m, X, labels, lmbda, batch_size=batch_size)
    assert out.shape == (2 * n,) + X.shape[1:] and out.dtype == np.float32
    np.testing.assert_array_equal(out[:n], X)
    g = m.class_gradient(X, labels, of_probs=True)
    np.testing.assert_array_equal(out[n:], X + np.float32(lmbda) * np.sign(g))
    assert (np.sign(g) != 0).mean() > 0.5
    assert out[n].min() < 0 and out[n].max() > 1            # not clipped
    np.testing.assert_array_equal(out, attacks_tf.jacobian_augmentation(m, X, labels, lmbda, batch_size=n))       # one chunk
    np.testing.assert_array_equal(out, _augment_native(m, X, labels, lmbda, batch_size))
    np.testing.assert_array_equal(out, _augment_native(m, X, labels, lmbda, batch_size, in_place=True))
    # torch in, torch out
    import torch
    t = attacks_tf.jacobian_augmentation(m, torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda(), lmbda, batch_size=batch_size)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    np.testing.assert_array_equal(t.cpu().numpy(), out)
    m.close()


def test_a_saturated_row_is_returned_unchanged():
    """The last Linear layer scaled until p_label rounds to 1 and the other classes' exp underflows: the seed (delta_kc - p_c) * p_k
    is exactly 0 in every component, so sign() is 0 everywhere and the new image is the old one; the unsaturated model moves it."""
    m, params = _model("E")
    X = _images(m, 4, np.random.RandomState(3))
    layers = R.describe(m)
    import torch
    z = R.logits(layers, R.as_params(params), torch.as_tensor(X.astype(np.float64))).numpy()
    srt = np.sort(z, axis=1)
    scale = 400.0 / (srt[:, -1] - srt[:, -2]).min()
    labels = z.argmax(axis=1)
    moved = attacks_tf.jacobian_augmentation(m, X, labels, 0.1)
    assert (moved[4:] != X).mean() > 0.5
    m.set_weights(params[:-1] + [(params[-1][0] * np.float32(scale), params[-1][1])])
    assert (m.get_probs(X)[np.arange(4), labels] == 1).all()
    out = attacks_tf.jacobian_augmentation(m, X, labels, 0.1)
    np.testing.assert_array_equal(out[4:], X)
    np.testing.assert_array_equal(out[:4], X)
    assert (m.class_gradient(X, labels) == 0).all()
    m.close()


def test_augment_refuses_a_partial_overlap():
    import torch
    m, _ = _model("E")
    buf = torch.zeros(12, 28, 28, 1, device="cuda")
    y = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = _native.load().dg_jacobian_augment(m._handle, buf[2:].data_ptr(), y.data_ptr(), 4, 0.1, 2, buf.data_ptr(), None)
    assert rc == -1 and b"overlaps" in _native.load().dg_last_error()
    m.close()


# ---------------------------------------------------------------------- 5. train_sub
class _RecordingOracle(object):
    """A fixed model F whose argmax is the label; keeps every query and its answer."""

    def __init__(self):
        self.model = nb.model_f()
        self.model.init_like_reference(seed=9)
        self.queries = []

    def __call__(self, X):
        labels = utils_tf.batch_eval_labels(self.model.get_probs, X, 4)
        self.queries.append((np.array(X), labels))
        return labels


def _train_sub_run():
    sub = nb.model_e()
    sub.init_like_reference(seed=1)
    oracle = _RecordingOracle()
    rs = np.random.RandomState(0)
    X0, Y0 = rs.uniform(0, 1, (8, 28, 28, 1)).astype(np.float32), rs.randint(0, 10, 8)
    _, X, Y = blackbox.train_sub(sub, oracle, X0, Y0, nb_epochs_s=2, batch_size=4, learning_rate=0.001, data_aug=3, lmbda=0.1,
                                 rng=np.random.RandomState(utils_tf.WHITEBOX_RNG_SEED), seed=77)
    return sub, oracle, X0, Y0, X, Y


def test_train_sub_is_deterministic_labels_by_the_oracle_and_resets_adam_only():
    sub, oracle, X0, Y0, X, Y = _train_sub_run()
    sub2, _, _, _, X2, Y2 = _train_sub_run()
    assert X.shape == (32, 28, 28, 1) and Y.shape == (32,)
    np.testing.assert_array_equal(X, X2)
    np.testing.assert_array_equal(Y, Y2)
    for (W, b), (W2, b2) in zip(sub.get_weights(), sub2.get_weights()):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    # the first halves are the earlier sets; each new half was sent to the oracle and carries its answer
    np.testing.assert_array_equal(X[:8], X0)
    np.testing.assert_array_equal(Y[:8], Y0)
    assert [len(q[0]) for q in oracle.queries] == [8, 16]
    for (qx, qy), lo in zip(oracle.queries, (8, 16)):
        np.testing.assert_array_equal(qx, X[lo:2 * lo])
        np.testing.assert_array_equal(qy, Y[lo:2 * lo])
        np.testing.assert_array_equal(qy, oracle.model.get_probs(qx).argmax(axis=1))
    # each round's new half is the sign step of the substitute as it stood after that round: replay the loop by hand
    twin = nb.model_e()
    twin.init_like_reference(seed=1)
    rng = np.random.RandomState(utils_tf.WHITEBOX_RNG_SEED)
    args = {"nb_epochs": 2, "batch_size": 4, "learning_rate": 0.001}
    for rho, n in enumerate((8, 16, 32)):
        utils_tf.model_train(twin, X[:n], Y[:n], args=args, rng=rng, seed=77 + rho)          # a fresh Adam inside, the weights carried
        if rho < 2:
            g = twin.class_gradient(X[:n], Y[:n])
            np.testing.assert_array_equal(X[n:2 * n], X[:n] + np.float32(0.1) * np.sign(g))
    for (W, b), (Wt, bt) in zip(sub.get_weights(), twin.get_weights()):
        np.testing.assert_array_equal(W, Wt)
        np.testing.assert_array_equal(b, bt)
    # Adam's step count is the last round's alone (2 epochs of 32 / 4 steps), not the 4 + 8 + 16 of all three
    assert utils_tf.adam_state(sub, 0)[2] == 16
    fresh = nb.model_e()
    fresh.init_like_reference(seed=1)
    utils_tf.model_train(fresh, X, Y, args=args, rng=np.random.RandomState(0), seed=79)
    assert not np.array_equal(fresh.get_weights()[0][0], sub.get_weights()[0][0])            # the weights were NOT reset
    for mm in (sub, sub2, twin, fresh, oracle.model):
        mm.close()


# ---------------------------------------------------------------------- 6. blackbox() end to end
NCLS = 10


def _separable(n, seed):
    """28 x 28 x 1 images: noise U(0, 0.3) and a 7 x 7 block raised by 0.4 whose position is the class."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, NCLS, n)
    x = rs.uniform(0, 0.3, (n, 28, 28, 1)).astype(np.float32)
    for i, c in enumerate(y):
        r, col = 2 + 9 * (c // 4), 1 + 7 * (c % 4)
        x[i, r:r + 7, col:col + 7] += np.float32(0.4)
    return x, y


_DATA = {}


def _data():
    if not _DATA:
        _DATA["d"] = _separable(512, 1) + _separable(232, 2)
    return _DATA["d"]


KW = dict(batch_size=16, learning_rate=0.001, nb_epochs=3, holdout=32, data_aug=4, nb_epochs_s=5, lmbda=0.1, num_tests=232, fgsm_eps=0.3)


def _agreement(sub, oracle, X):
    return float((sub.get_probs(X).argmax(axis=1) == oracle.get_probs(X).argmax(axis=1)).mean())


def test_blackbox_without_defense_trains_a_substitute_that_transfers():
    data = _data()
    bb, sub = nb.model_f(nb_classes=NCLS), nb.model_e(nb_classes=NCLS)
    bb.init_like_reference(seed=0)
    sub0 = sub.init_like_reference(seed=1)
    acc = blackbox.blackbox(None, bb, sub, data, defense_type="none", **KW)
    assert sorted(acc) == ["bbox", "bbox_on_sub_adv_ex", "sub"] and acc["sub"] == 0
    X_test = data[2][32:]
    untrained = nb.model_e(nb_classes=NCLS)
    untrained.set_weights(sub0)
    before, after = _agreement(untrained, bb, X_test), _agreement(sub, bb, X_test)
    print("oracle accuracy %.4f clean, %.4f on the substitute's FGSM images; agreement with the oracle %.4f before, %.4f after training"
          % (acc["bbox"], acc["bbox_on_sub_adv_ex"], before, after))
    assert after > before
    assert acc["bbox_on_sub_adv_ex"] < acc["bbox"]
    # 'bbox' is the bare oracle's accuracy on the 200 test images behind the holdout
    assert acc["bbox"] == float((bb.get_probs(X_test).argmax(axis=1) == data[3][32:]).mean())
    for mm in (bb, sub, untrained):
        mm.close()


def test_blackbox_with_defense_gan_returns_the_roc_triple_of_model_eval_gan():
    from tests.helpers import make_gan
    data = _data()
    gan, _ = make_gan("mnist", gain=2.0, bias_range=0.1, rec_rr=2, rec_iters=3)
    bb, sub = nb.model_f(nb_classes=NCLS), nb.model_e(nb_classes=NCLS)
    kw = dict(KW, nb_epochs=1, data_aug=2, nb_epochs_s=2)
    acc = blackbox.blackbox(gan, bb, sub, data, defense_type="defense_gan", **kw)
    assert sorted(acc) == ["bbox", "bbox_on_sub_adv_ex", "roc_info", "sub"] and acc["sub"] == 0
    X_test, y_test = data[2][32:], data[3][32:]
    labels, preds, diffs = acc["roc_info"]
    assert labels.shape == preds.shape == diffs.shape == (200,) and diffs.dtype == np.float32
    np.testing.assert_array_equal(labels, y_test)
    assert acc["bbox_on_sub_adv_ex"] == float((preds == labels).mean())
    # a direct model_eval_gan call on the same adversarial images
    import torch
    fgsm = nb.FastGradientMethod(sub)
    x_adv = utils_tf.batch_eval(lambda xb: fgsm.generate(xb, eps=0.3, clip_min=0.0, clip_max=1.0), torch.from_numpy(X_test).cuda(), 16)
    assert float((x_adv.cpu().numpy() - X_test).__abs__().max()) <= 0.3 + 1e-6
    c, n, roc = gd.model_eval_gan(gan.reconstruct, bb, x_adv, y_test, 16, rec_rr=2, seed=blackbox.SEED)
    assert n == 200 and c / 200.0 == acc["bbox_on_sub_adv_ex"]
    for a, b in zip(roc, acc["roc_info"]):
        np.testing.assert_array_equal(a, b)
    rec = gan.reconstruct(x_adv[:16], seed=blackbox.SEED, first_row=0)
    np.testing.assert_allclose(diffs[:16], ((x_adv[:16] - rec) ** 2).mean(dim=(1, 2, 3)).cpu().numpy(), rtol=1e-5)
    for mm in (bb, sub):
        mm.close()


def test_with_a_gan_the_queries_go_through_the_projection_even_without_defense():
    """blackbox.py:509-514 builds model(reconstruct(x)) unconditionally: with a gan given, defense_type 'none' still labels the new
    halves through gan.reconstruct (and evaluates WITHOUT it); label_through_rec=False never calls it."""
    import types
    from tests.helpers import make_gan
    data = _data()
    gan, _ = make_gan("mnist", gain=2.0, bias_range=0.1, rec_rr=2, rec_iters=3)
    inner, calls = gan.reconstruct, []

    def recording(self, images, *a, **kw):
        calls.append((np.array(images.cpu().numpy() if hasattr(images, "cpu") else images), kw.get("first_row")))
        return inner(images, *a, **kw)
    gan.reconstruct = types.MethodType(recording, gan)           # bound, so that model_eval_gan still sees an engine model
    kw = dict(KW, nb_epochs=1, data_aug=3, nb_epochs_s=2)
    accs = {}
    for through in (None, False):
        del calls[:]
        bb, sub = nb.model_f(nb_classes=NCLS), nb.model_e(nb_classes=NCLS)
        accs[through] = blackbox.blackbox(gan, bb, sub, data, defense_type="none", label_through_rec=through, **kw)
        assert sorted(accs[through]) == ["bbox", "bbox_on_sub_adv_ex", "sub"]                 # no roc_info without defense_gan
        if through is False:
            assert calls == []
        else:
            # the two new halves, 32 and 64 images, and nothing else (the final evaluation of 'none' sees the bare images);
            # image i of the adversary's queries draws the latent rows of image i: first_row counts on across the queries
            seen = np.concatenate([c[0] for c in calls])
            assert seen.shape == (96, 28, 28, 1)
            done = 0
            for x, first_row in calls:
                assert first_row == done * 2
                done += len(x)
            # each new half is a sign step of lmbda from the set before it: [X0 + s0 | X0 + s1, (X0 + s0) + s2]
            X0 = data[2][:32]
            for new, old in ((seen[:32], X0), (seen[32:64], X0), (seen[64:], seen[:32])):
                step = np.abs(new - old)
                assert step.max() <= 0.1 + 1e-6 and (step > 0.09).mean() > 0.5
        for mm in (bb, sub):
            mm.close()
    assert accs[None]["bbox"] == accs[False]["bbox"]             # the oracle's training does not depend on the labelling
