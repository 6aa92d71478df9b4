"""-m gpu: one classifier handle carries three workspaces (evaluation buffers, the Carlini-Wagner workspace, the training
workspace with Adam's state).  A sequence of calls on ONE handle, whose image count goes 3 -> 70 -> 5 -> 3 so that every buffer
grows and is then reused larger than needed, must give bit for bit what each call gives on a fresh handle with the same weights."""
import numpy as np
import pytest

from defensegan_amd import network_builder as nb
from defensegan_amd import utils_tf

pytestmark = pytest.mark.gpu

BATCH = 70          # crosses the 64-image block of the per-image kernels (softmax, cross-entropy seeds)
CW = dict(binary_search_steps=2, max_iterations=5, batch_size=2)      # on 5 images: a trailing partial chunk


def _model_b():
    """Input Dropout, SAME and VALID convolutions, fused ReLUs, Dropout before Flatten."""
    return nb.model_b()


def _model_small():
    """Every layer kind in a small model: a ReLU on the input (it follows no Conv2D / Linear), a ReLU after an already
    fused ReLU (a kernel of its own), SAME and VALID convolutions, Dropout, Linear with and without a fused ReLU."""
    return nb.MLP([nb.ReLU(), nb.Conv2D(4, (3, 3), (2, 2), "SAME"), nb.ReLU(), nb.ReLU(), nb.Conv2D(6, (4, 4), (1, 1), "VALID"),
                   nb.Dropout(0.5), nb.Flatten(), nb.Linear(16), nb.ReLU(), nb.Linear(10), nb.Softmax()])


def _images(n, seed, shift):
    rs = np.random.RandomState(seed)
    return (rs.uniform(0, 1, (n, 28, 28, 1)).astype(np.float32) - np.float32(shift)), rs.randint(0, 10, n).astype(np.int32)


def _forward(m, x):
    out = m.fprop(x)
    return [out["logits"], out["probs"]]


def _train(m, x, y):
    """Three Adam steps of adversarial training at BATCH images: the losses, the weights and Adam's state afterwards."""
    losses = utils_tf.model_train(m, x, y, args={"nb_epochs": 1, "batch_size": BATCH, "learning_rate": 0.001},
                                  rng=np.random.RandomState(3), adv_eps=0.15, return_losses=True)
    assert losses.shape == (3,)
    out = [losses]
    for W, b in m.get_weights():
        out += [W, b]
    for i in range(len(m.param_shapes())):
        (mW, mb), (vW, vb), t = utils_tf.adam_state(m, i)
        assert t == 3
        out += [mW, mb, vW, vb]
    return out


def _fgsm(m, x):
    return [nb.FastGradientMethod(m).generate(x, eps=0.1, clip_min=0.0, clip_max=1.0)]


def _cw(m, x):
    return list(nb.CarliniWagnerL2(m).generate(x, return_info=True, return_search=True, **CW))


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i)
        assert g.tobytes() == w.tobytes(), "%s, output %d: differs from the fresh handle's" % (what, i)


@pytest.mark.parametrize("make,shift", [(_model_b, 0.0), (_model_small, 0.3)], ids=["B", "small"])
def test_calls_on_one_handle_equal_calls_on_fresh_handles(make, shift):
    x3, _ = _images(3, 1, shift)
    xt, yt = _images(3 * BATCH, 2, shift)
    x5, _ = _images(5, 3, shift)
    one = make()
    start = one.init_like_reference(seed=5)

    def fresh(weights):
        m = make()
        m.set_weights(weights)
        return m

    _same(_forward(one, x3), _forward(fresh(start), x3), "first forward (3 images)")
    _same(_train(one, xt, yt), _train(fresh(start), xt, yt), "training (batches of %d)" % BATCH)
    trained = one.get_weights()
    _same(_fgsm(one, xt[:BATCH]), _fgsm(fresh(trained), xt[:BATCH]), "FGSM (%d images)" % BATCH)
    _same(_cw(one, x5), _cw(fresh(trained), x5), "Carlini-Wagner (5 images)")
    _same(_forward(one, x3), _forward(fresh(trained), x3), "last forward (3 images)")
