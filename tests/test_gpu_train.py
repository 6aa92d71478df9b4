"""-m gpu: classifier training on the device (dg_clf_param_gradient, dg_clf_train, utils_tf.model_train) against the float64
restatement in tests/support/train_reference.py, and a classifier that learns."""
import numpy as np
import pytest

from defensegan_amd import _native
from defensegan_amd import network_builder as nb
from defensegan_amd import utils_tf
from tests.support import train_reference as R

pytestmark = pytest.mark.gpu

SEED = 11241990


def _model(name, seed=None):
    m = nb.MODELS[name]()
    params = m.init_like_reference(seed=ord(name) if seed is None else seed)
    return m, params


def _synthetic(n, seed=0, noise=0.25, patterns_seed=1234):
    """A separable 10-class 28x28 set: each class a fixed seeded binary pattern, plus clipped Gaussian noise."""
    pats = (np.random.RandomState(patterns_seed).uniform(0, 1, (10, 28, 28, 1)) > 0.5).astype(np.float32)
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 10, n).astype(np.int32)
    x = np.clip(pats[y] + rs.standard_normal((n, 28, 28, 1)).astype(np.float32) * np.float32(noise), 0, 1).astype(np.float32)
    return x, y


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
    _native.check(_native.load().dg_clf_param_gradient(m._handle, xt.data_ptr(), yt.data_ptr(), len(x), float(adv_eps), lo, hi, seed, step,
                                                       grads.data_ptr(), loss.data_ptr(), xadv.data_ptr(), stream))
    torch.cuda.synchronize(dev)
    g, out, off = grads.cpu().numpy(), [], 0
    for ws, bs in shapes:
        nw, nbias = int(np.prod(ws)), int(np.prod(bs))
        out.append((g[off:off + nw].reshape(ws), g[off + nw:off + nw + nbias]))
        off += nw + nbias
    return float(loss.item()), out, (xadv.cpu().numpy() if adv_eps > 0 else None)


def _check_grads(dev, ref, bound=1e-4):
    for i, ((dW, db), (rW, rb)) in enumerate(zip(dev, ref)):
        for name, d, r in (("W", dW, rW), ("b", db, rb)):
            scale = np.abs(r).max()
            err = np.abs(d - r).max()
            assert err <= bound * scale + 1e-12, "layer %d %s: max|dev - ref| = %g, max|ref| = %g" % (i, name, err, scale)


# every Dropout position of the zoo: A / C after Flatten and after the hidden Linear, B on the input and before Flatten
@pytest.mark.parametrize("name,B,step", [("A", 3, 0), ("B", 5, 1), ("C", 3, 2), ("E", 7, 0), ("F", 5, 3)])
def test_param_gradient_matches_reference(name, B, step):
    m, params = _model(name)
    x, y = _synthetic(B, seed=B)
    loss, grads, _ = _device_gradient(m, x, y, step=step)
    rl, rg, _ = R.param_gradient(R.describe(m), params, x, y, SEED, step)
    assert abs(loss - rl) <= 1e-5 * abs(rl), (loss, rl)
    _check_grads(grads, rg)


def test_param_gradient_adversarial_with_dropout_matches_reference():
    m, params = _model("B")
    x, y = _synthetic(3, seed=9)
    loss, grads, xadv = _device_gradient(m, x, y, adv_eps=0.15, step=4)
    layers = R.describe(m)
    rl, rg, _ = R.param_gradient(layers, params, x, y, SEED, 4, adv_eps=0.15, x_adv=xadv)
    assert abs(loss - rl) <= 1e-5 * abs(rl)
    _check_grads(grads, rg)
    # the device's x_adv is the FGSM of the training-phase model with the inner pass's masks, up to the float32 sum x + 0.15f (the
    # float64 reference rounds x + 0.15 once: 1 ulp) and float64 / float32 signs of near-zero input gradients
    _, _, ref_xadv = R.param_gradient(layers, params, x, y, SEED, 4, adv_eps=0.15)
    assert (np.abs(xadv - ref_xadv) <= 1e-6).mean() > 0.99


@pytest.mark.parametrize("name,layer,B", [("B", 0, 5), ("B", 7, 3), ("A", 5, 3), ("A", 8, 7)])
def test_dropout_masks_are_the_python_restatement(name, layer, B):
    import torch
    m, _ = _model(name)
    assert isinstance(m.layers[layer], nb.Dropout)
    feats = R.feature_counts(R.describe(m), (28, 28, 1))[layer]
    dev = torch.device("cuda", 0)
    for step, pass_ in ((0, 0), (12, 1), (2 ** 33 + 5, 2)):
        mask = torch.empty(B * feats, dtype=torch.float32, device=dev)
        _native.check(_native.load().dg_clf_dropout_mask(m._handle, layer, B, SEED, step, pass_, mask.data_ptr(),
                                                         torch.cuda.current_stream(dev).cuda_stream))
        want = R.dropout_mask(m.layers[layer].prob, B * feats, SEED, step, pass_, layer)
        np.testing.assert_array_equal(mask.cpu().numpy(), want)


def test_one_adam_step_from_the_device_gradients():
    """dg_clf_train's first step = TF Adam (float32 restatement) applied to dg_clf_param_gradient's gradients of the same batch."""
    m, params = _model("A")
    x, y = _synthetic(6, seed=2)
    _, grads, _ = _device_gradient(m, x, y, step=0)
    lr = 0.01
    losses = utils_tf.model_train(m, x, y, args={"nb_epochs": 1, "batch_size": 6, "learning_rate": lr}, rng=_IdentityRng(),
                                  return_losses=True)
    assert losses.shape == (1,)
    got = m.get_weights()
    for i, ((W, b), (gW, gb), (nW, nb_)) in enumerate(zip(params, grads, got)):
        for p, g, new in ((W, gW, nW), (b, gb, nb_)):
            want, mm, vv = R.adam_update(p, g, np.zeros_like(p), np.zeros_like(p), 1, lr, dtype=np.float32)
            np.testing.assert_allclose(new, want, rtol=1e-6, atol=1e-6 * np.abs(want).max(), err_msg="layer %d" % i)
        (mW, mb), (vW, vb), t = utils_tf.adam_state(m, i)
        assert t == 1
        np.testing.assert_allclose(mW, np.float32(0.1) * gW, rtol=1e-6, atol=0)
        np.testing.assert_allclose(vW, np.float32(0.001) * gW * gW, rtol=1e-5, atol=1e-30)


class _IdentityRng(object):
    """An rng whose shuffle leaves the order alone: the epoch's one batch is the set in order."""

    def shuffle(self, a):
        pass


def test_adversarial_step_uses_dg_fgsm_on_a_model_without_dropout():
    m, params = _model("F")
    x, y = _synthetic(5, seed=4)
    loss, grads, xadv = _device_gradient(m, x, y, adv_eps=0.3, step=0)
    want = nb.FastGradientMethod(m).generate(x, eps=0.3, clip_min=0.0, clip_max=1.0)
    np.testing.assert_array_equal(xadv, want)
    rl, rg, _ = R.param_gradient(R.describe(m), params, x, y, SEED, 0, adv_eps=0.3, x_adv=xadv)
    assert abs(loss - rl) <= 1e-5 * abs(rl)
    _check_grads(grads, rg)


# Losses along 30 Adam steps against the float64 run on the same batches, masks and initial weights.  The device sums in float32
# (relative rounding ~1e-6 per gradient); Adam normalises each update, so these differences stay at the rounding level except
# where a gradient is near zero and its normalised step is noise, which moves the loss far less than 1e-2.
@pytest.mark.parametrize("name,adv", [("A", 0.0), ("F", 0.15)])
def test_thirty_step_trajectory_tracks_float64(name, adv):
    m, params = _model(name)
    x, y = _synthetic(480, seed=5)
    idx = utils_tf.epoch_indices(np.random.RandomState(7), 480, 16)
    losses = utils_tf.model_train(m, x, y, args={"nb_epochs": 1, "batch_size": 16, "learning_rate": 0.001},
                                  rng=np.random.RandomState(7), adv_eps=adv, return_losses=True)
    ref, _ = R.train(R.describe(m), params, x, y, idx, 16, 0.001, SEED, adv_eps=adv)
    assert losses.shape == (30,)
    rel = np.abs(losses - ref) / np.abs(ref)
    assert rel.max() <= 1e-2, "max relative loss difference %g at step %d" % (rel.max(), int(rel.argmax()))
    assert ref[-5:].mean() < ref[:5].mean()                  # it trains


def test_model_train_is_bit_reproducible():
    x, y = _synthetic(256, seed=6)
    out = []
    for _ in range(2):
        m, _ = _model("B")
        losses = utils_tf.model_train(m, x, np.eye(10, dtype=np.float32)[y], args={"nb_epochs": 2, "batch_size": 64, "learning_rate": 0.001},
                                      rng=np.random.RandomState([11, 24, 1990]), adv_eps=0.15, return_losses=True)
        out.append((losses, m.get_weights(), [utils_tf.adam_state(m, i) for i in range(len(m.param_shapes()))]))
    (l0, w0, a0), (l1, w1, a1) = out
    np.testing.assert_array_equal(l0, l1)
    for (W, b), (W2, b2) in zip(w0, w1):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    for (mm, vv, t), (mm2, vv2, t2) in zip(a0, a1):
        assert t == t2 == 8
        for p, q in zip(mm + vv, mm2 + vv2):
            np.testing.assert_array_equal(p, q)


def _accuracy(m, x, y):
    c, _, _ = m.eval_batch(x, labels=y)
    return c / float(len(x))


def test_model_f_learns_and_fgsm_finally_has_a_target(tmp_path):
    x, y = _synthetic(2500, seed=8)
    xtr, ytr, xte, yte = x[:2000], y[:2000], x[2000:], y[2000:]
    args = {"nb_epochs": 3, "batch_size": 128, "learning_rate": 0.001}
    m, _ = _model("F", seed=0)
    before = _accuracy(m, xte, yte)
    assert before < 0.3, before
    utils_tf.model_train(m, xtr, ytr, args=args)
    clean = _accuracy(m, xte, yte)
    assert clean >= 0.95, clean
    adv = nb.FastGradientMethod(m).generate(xte, eps=0.3, clip_min=0.0, clip_max=1.0)
    assert _accuracy(m, adv, yte) < clean
    # the trained parameters round-trip through the .npz file
    path = str(tmp_path / "f.npz")
    m.save_weights(path)
    m2 = nb.model_f()
    m2.load_weights(path)
    for (W, b), (W2, b2) in zip(m.get_weights(), m2.get_weights()):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    np.testing.assert_array_equal(m.get_logits(xte[:16]), m2.get_logits(xte[:16]))
    ma, _ = _model("F", seed=0)
    utils_tf.model_train(ma, xtr, ytr, args=args, adv_eps=0.15)
    assert _accuracy(ma, xte, yte) >= 0.9


def test_train_classifier_cli_writes_weights_load_weights_accepts(tmp_path, capsys):
    from defensegan_amd import datasets, train_classifier
    x, y = _synthetic(300, seed=10)
    d = tmp_path / "mnist"
    d.mkdir()
    for split, (xs, ys) in (("train", (x[:240], y[:240])), ("test", (x[240:], y[240:]))):
        img = np.round(xs * 255).astype(np.uint8)
        with open(str(d / datasets.IDX_FILES[split + "_images"]), "wb") as f:
            f.write(np.array([2051, len(img), 28, 28], ">i4").tobytes() + img.tobytes())
        with open(str(d / datasets.IDX_FILES[split + "_labels"]), "wb") as f:
            f.write(np.array([2049, len(ys)], ">i4").tobytes() + ys.astype(np.uint8).tobytes())
    out = str(tmp_path / "clf.npz")
    assert train_classifier.main(["--data_dir", str(d), "--model", "B", "--nb_epochs", "2", "--batch_size", "32", "--adv_tr",
                                  "--out", out]) == 0
    text = capsys.readouterr().out
    assert text.count("Test accuracy on legitimate examples:") == 2
    m = nb.model_b()
    m.load_weights(out)
    assert len(m.get_weights()) == 4
