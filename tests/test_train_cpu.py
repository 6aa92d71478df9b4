"""-m "not gpu": the CPU restatement of classifier training (tests/support/train_reference.py) against finite differences and
hand-computed values, cleverhans' batch schedule (defensegan_amd.utils_tf), model_train's argument checks and the .npz weight
files."""
import numpy as np
import pytest

from defensegan_amd import network_builder as nb
from defensegan_amd import utils_tf
from tests.support import train_reference as R


def _tiny():
    """Every layer kind training meets: a SAME stride-2 conv, a VALID conv, Dropout before and after Flatten, Linear, Softmax."""
    layers = [nb.Conv2D(3, (3, 3), (2, 2), "SAME"), nb.ReLU(), nb.Conv2D(4, (2, 2), (1, 1), "VALID"), nb.ReLU(), nb.Dropout(0.5),
              nb.Flatten(), nb.Dropout(0.7), nb.Linear(5), nb.ReLU(), nb.Linear(3), nb.Softmax()]
    return nb.MLP(layers, input_shape=(None, 6, 6, 2))


def _tiny_params(rs):
    return [(rs.standard_normal((3, 3, 2, 3)) * 0.5, rs.standard_normal(3) * 0.1),
            (rs.standard_normal((2, 2, 3, 4)) * 0.5, rs.standard_normal(4) * 0.1),
            (rs.standard_normal((16, 5)) * 0.5, rs.standard_normal(5) * 0.1),
            (rs.standard_normal((5, 3)) * 0.5, rs.standard_normal(3) * 0.1)]


def test_param_shapes_follow_the_layers():
    assert _tiny().param_shapes() == [((3, 3, 2, 3), (3,)), ((2, 2, 3, 4), (4,)), ((16, 5), (5,)), ((5, 3), (3,))]
    assert nb.model_f().param_shapes() == [((8, 8, 1, 64), (64,)), ((6, 6, 64, 128), (128,)), ((5, 5, 128, 128), (128,)),
                                           ((128, 10), (10,))]


def test_reference_gradients_match_central_differences():
    rs = np.random.RandomState(3)
    layers = R.describe(_tiny())
    params = _tiny_params(rs)
    x = rs.uniform(0, 1, (3, 6, 6, 2))
    y = np.array([0, 2, 1])
    masks = R.step_masks(layers, (6, 6, 2), 3, seed=5, step=7, pass_=0)
    assert set(masks) == {4, 6} and masks[4].shape == (3, 16) and masks[6].shape == (3, 16)
    _, grads, _ = R.param_gradient(layers, params, x, y, seed=5, step=7)
    h = 1e-6
    for i, (W, b) in enumerate(params):
        for which, arr in ((0, W), (1, b)):
            flat = arr.reshape(-1)
            for e in rs.choice(flat.size, min(flat.size, 6), replace=False):
                def at(d):
                    p = [(np.array(a), np.array(c)) for a, c in params]
                    p[i][which].reshape(-1)[e] += d
                    return R.loss_of(layers, p, x, y, masks)
                fd = (at(h) - at(-h)) / (2 * h)
                assert abs(grads[i][which].reshape(-1)[e] - fd) <= 1e-6 + 1e-5 * abs(fd), (i, which, e)


def test_dropout_keeps_keep_prob_and_scales_by_its_inverse():
    """tf.nn.dropout(x, prob) in TF 1.x: prob is the KEEP probability (Dropout(0.25) keeps a quarter, scaled by 4)."""
    import torch
    layers = [("dropout", 0.25)]
    masks = {0: R.dropout_mask(0.25, 8, seed=1, step=0, pass_=0, layer=0).reshape(1, 8)}
    y = R.logits(layers, [], torch.ones(1, 8, dtype=torch.float64), masks).numpy()
    assert set(np.unique(y)) <= {0.0, 4.0}
    np.testing.assert_array_equal(y, masks[0] * 4.0)


def test_adversarial_step_averages_the_two_losses():
    rs = np.random.RandomState(4)
    layers = R.describe(_tiny())
    params = _tiny_params(rs)
    x = rs.uniform(0, 1, (2, 6, 6, 2))
    y = np.array([1, 0])
    loss, grads, xa = R.param_gradient(layers, params, x, y, seed=2, step=0, adv_eps=0.1)
    assert xa.min() >= 0 and xa.max() <= 1 and np.abs(xa - x).max() <= 0.1 + 1e-12
    lc, gc, _ = R.param_gradient(layers, params, x, y, seed=2, step=0)
    la = R.loss_of(layers, params, xa, y, R.step_masks(layers, (6, 6, 2), 2, 2, 0, 2))
    assert abs(loss - (lc + la) / 2) < 1e-12


def test_adam_steps_one_and_two_by_hand():
    lr = 0.001
    p, m, v = np.array([1.0, -2.0, 0.5]), np.zeros(3), np.zeros(3)
    g1, g2 = np.array([0.5, -1.0, 0.0]), np.array([0.1, 2.0, -3.0])
    p1, m1, v1 = R.adam_update(p, g1, m, v, 1, lr)
    # step 1: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001) / 0.1: p -= lr * g / (|g| + 1e-8 / sqrt(0.001)) ~ lr sign(g)
    np.testing.assert_allclose(m1, [0.05, -0.1, 0.0])
    np.testing.assert_allclose(v1, [0.00025, 0.001, 0.0])
    lr1 = lr * np.sqrt(0.001) / 0.1
    np.testing.assert_allclose(p1, [1.0 - lr1 * 0.05 / (np.sqrt(0.00025) + 1e-8), -2.0 + lr1 * 0.1 / (np.sqrt(0.001) + 1e-8), 0.5], rtol=0,
                               atol=1e-15)
    assert abs(p1[0] - (1.0 - 0.001)) < 1e-9 and abs(p1[1] - (-2.0 + 0.001)) < 1e-9
    p2, m2, v2 = R.adam_update(p1, g2, m1, v1, 2, lr)
    m2w = 0.9 * m1 + 0.1 * g2
    v2w = 0.999 * v1 + 0.001 * g2 * g2
    lr2 = lr * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    np.testing.assert_allclose(m2, m2w)
    np.testing.assert_allclose(v2, v2w)
    np.testing.assert_allclose(p2, p1 - lr2 * m2w / (np.sqrt(v2w) + 1e-8), rtol=0, atol=1e-15)
    assert abs(m2[0] - 0.055) < 1e-15 and abs(v2[0] - (0.999 * 0.00025 + 0.001 * 0.01)) < 1e-15


def test_batch_indices_shift_the_last_batch_back():
    assert [utils_tf.batch_indices(b, 5, 2) for b in range(3)] == [(0, 2), (2, 4), (3, 5)]
    assert [utils_tf.batch_indices(b, 6, 3) for b in range(2)] == [(0, 3), (3, 6)]
    assert utils_tf.batch_indices(3, 10, 4) == (6, 10)


def test_epoch_permutation_is_cleverhans_schedule():
    rng = np.random.RandomState([11, 24, 1990])
    idx = utils_tf.epoch_indices(rng, 5, 2)
    perm = list(range(5))
    np.random.RandomState([11, 24, 1990]).shuffle(perm)
    assert idx.dtype == np.int32
    assert idx.tolist() == perm[0:2] + perm[2:4] + perm[3:5]
    # a second epoch continues the same generator
    perm2 = list(range(5))
    r2 = np.random.RandomState([11, 24, 1990])
    r2.shuffle(list(range(5)))
    r2.shuffle(perm2)
    assert utils_tf.epoch_indices(rng, 5, 2).tolist() == perm2[0:2] + perm2[2:4] + perm2[3:5]


def test_philox_known_answers():
    """Random123's known-answer vectors of Philox4x32-10."""
    out = R.philox4x32_10(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint64),
                          (0, 0))
    assert [hex(int(w)) for w in out[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    out = R.philox4x32_10(np.array([[0xFFFFFFFF] * 4], np.uint64), (0xFFFFFFFF, 0xFFFFFFFF))
    assert [hex(int(w)) for w in out[0]] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    out = R.philox4x32_10(np.array([[0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint64), (0xA4093822, 0x299F31D0))
    assert [hex(int(w)) for w in out[0]] == ["0xd16cfe09", "0x94fdcceb", "0x5001e420", "0x24126ea1"]


def test_mask_counters_and_keep_fraction():
    u = R.uniforms(10, seed=0, step=0, pass_=0, layer=0)
    words = R.philox4x32_10(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]], np.uint64), (0, 0)).reshape(-1)[:10]
    np.testing.assert_array_equal(u, (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24))
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    # (step, pass, layer) each give other draws
    a = R.uniforms(64, 9, 3, 1, 4)
    for other in (R.uniforms(64, 9, 4, 1, 4), R.uniforms(64, 9, 3, 2, 4), R.uniforms(64, 9, 3, 1, 5), R.uniforms(64, 8, 3, 1, 4)):
        assert not np.array_equal(a, other)
    for keep in (0.2, 0.25, 0.5):
        m = R.dropout_mask(keep, 10 ** 6, seed=11241990, step=0, pass_=0, layer=1)
        assert set(np.unique(m)) == {0.0, 1.0}
        assert abs(m.mean() - keep) < 2e-3, (keep, m.mean())


def test_model_train_rejects_bad_arguments_before_touching_the_device():
    m = nb.model_f()
    x = np.zeros((8, 28, 28, 1), np.float32)
    y = np.arange(8) % 10
    ok = {"nb_epochs": 1, "batch_size": 4, "learning_rate": 0.001}
    with pytest.raises(ValueError, match="args"):
        utils_tf.model_train(m, x, y)
    with pytest.raises(ValueError, match="batch_size was not given"):
        utils_tf.model_train(m, x, y, args={"nb_epochs": 1, "learning_rate": 0.001})
    with pytest.raises(ValueError, match="batch_size > 0"):
        utils_tf.model_train(m, x, y, args=dict(ok, batch_size=0))
    with pytest.raises(ValueError, match="X_train must be"):
        utils_tf.model_train(m, np.zeros((8, 28, 28, 3), np.float32), y, args=ok)
    with pytest.raises(ValueError, match="smaller than one batch"):
        utils_tf.model_train(m, x, y, args=dict(ok, batch_size=16))
    onehot = np.eye(10)[y]
    bad = onehot.copy()
    bad[3, 0] = 0.5
    with pytest.raises(ValueError, match="row 3 is not one-hot"):
        utils_tf.model_train(m, x, bad, args=ok)
    two = onehot.copy()
    two[5, (y[5] + 1) % 10] = 1
    with pytest.raises(ValueError, match="row 5 is not one-hot"):
        utils_tf.model_train(m, x, two, args=ok)
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        utils_tf.model_train(m, x, y + 5, args=ok)
    with pytest.raises(ValueError, match="one-hot labels must be"):
        utils_tf.model_train(m, x, np.eye(9)[y % 9], args=ok)
    with pytest.raises(ValueError, match="adv_clip"):
        utils_tf.model_train(m, x, y, args=ok, adv_eps=0.1, adv_clip=(1.0, 0.0))


def test_model_train_through_the_reconstruction_layer_is_not_implemented():
    m = nb.model_f()
    m.rec_layer = object()            # what add_rec_model installs; training through it is out of scope
    with pytest.raises(NotImplementedError, match="reconstruction layer"):
        utils_tf.model_train(m, np.zeros((4, 28, 28, 1), np.float32), np.zeros(4, np.int32),
                             args={"nb_epochs": 1, "batch_size": 4, "learning_rate": 0.001})


def test_labels_of_accepts_one_hot_and_indices():
    y = np.array([3, 0, 9])
    assert utils_tf.labels_of(np.eye(10)[y], 3, 10).tolist() == [3, 0, 9]
    assert utils_tf.labels_of(y, 3, 10).dtype == np.int32
    assert utils_tf.labels_of(y.astype(np.float32), 3, 10).tolist() == [3, 0, 9]
    with pytest.raises(ValueError, match="integers"):
        utils_tf.labels_of(np.array([0.5, 1, 2]), 3, 10)


def test_weight_file_round_trips(tmp_path, monkeypatch):
    """save_weights writes get_weights() as W0, b0, ...; load_weights checks the names and shapes and installs them (the device
    side, dg_clf_get_weights / dg_clf_set_weights, is replaced by a recorder here; tests/test_gpu_train.py runs it for real)."""
    m = _tiny()
    rs = np.random.RandomState(0)
    params = [(W.astype(np.float32), b.astype(np.float32)) for W, b in _tiny_params(rs)]
    got = []
    monkeypatch.setattr(m, "get_weights", lambda: params)
    monkeypatch.setattr(m, "set_weights", lambda p: got.append(p))
    path = str(tmp_path / "clf.npz")
    m.save_weights(path)
    with np.load(path) as f:
        assert sorted(f.files) == ["W0", "W1", "W2", "W3", "b0", "b1", "b2", "b3"]
    m.load_weights(path)
    for (W, b), (W2, b2) in zip(params, got[0]):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    np.savez(path, W0=params[0][0], b0=params[0][1])
    with pytest.raises(ValueError, match="this model needs"):
        m.load_weights(path)
    wrong = {("W%d" % i): W for i, (W, _) in enumerate(params)}
    wrong.update({("b%d" % i): b for i, (_, b) in enumerate(params)})
    wrong["W1"] = np.zeros((2, 2, 3, 5), np.float32)
    np.savez(path, **wrong)
    with pytest.raises(ValueError, match="parameter pair 1"):
        m.load_weights(path)


# ---------------------------------------------------------------------- the cases of tests/test_gpu_train_shapes.py
def test_slot_plan_restatement_worked_by_hand():
    """dg_clf_train.hip's slot_plan on cases worked by hand: (tiles, S, Kc, slots)."""
    assert R.slot_plan(784, 200, 128) == (52, 2, 64, 2)            # model E first Linear, B = 128
    assert R.slot_plan(784, 200, 100) == (52, 1, 100, 1)           # one slot, the last chunk holds 4 terms
    assert R.slot_plan(784, 200, 130) == (52, 2, 65, 2)            # slot 1 starts at k = 65
    assert R.slot_plan(64, 64, 128 * 196) == (2, 256, 98, 256)     # model F first convolution at the cap, Kc cuts an image in two
    assert R.slot_plan(64, 64, 200 * 196) == (2, 256, 154, 255)    # ceil(K / Kc) < S
    assert R.slot_plan(9 * 128, 128, 128) == (19 * 2, 2, 64, 2)    # model Z's last convolution: 19 M-tiles
    m = nb.model_f()
    assert R.wgrad_shapes(R.describe(m), (28, 28, 1)) == [("conv", 64, 64, 196), ("conv", 2304, 128, 25), ("conv", 3200, 128, 1),
                                                          ("linear", 128, 10, 1)]
    assert R.boundary_images(R.describe(nb.model_e()), (28, 28, 1), 130) == [0, 64, 65, 129]
    # F at 128: Kc = 98 cuts images 0 and 127 of the first convolution, Kc = 247 cuts images 9 (k 225 .. 249) and 118 of the second
    assert R.boundary_images(R.describe(m), (28, 28, 1), 128) == [0, 9, 63, 64, 118, 127]


def test_gradient_cases_reach_every_regime_of_the_weight_gradient_kernel():
    """Each regime of tr_wgrad_kernel / slot_plan is reached by a layer of a case that tests/test_gpu_train_shapes.py compares
    with float64.  A planner change that moves the regimes shows here as the regime that lost its case."""
    reached = {r: [] for r in R.REGIMES}
    for key, B, _ in R.GRADIENT_CASES:
        m = R.shape_model(key)
        for i, (kind, M, N, pos) in enumerate(R.wgrad_shapes(R.describe(m), m.input_shape[1:])):
            for r in R.regimes(kind, M, N, pos, B):
                reached[r].append((key, B, i))
    missing = [r for r in R.REGIMES if not reached[r]]
    assert not missing, "no gradient case reaches: %s" % "; ".join(missing)
    # the cases the regimes were chosen by
    assert ("E", 128, 0) in reached["linear layer with >= 2 slots of >= 2 chunks"]
    assert ("F", 128, 0) in reached["256-slot cap"] and ("F", 128, 0) in reached["slot start off a chunk boundary"]
    assert ("E", 130, 0) in reached["slot start off a chunk boundary"]
    assert ("F", 200, 0) in reached["slots < S"]
    assert ("E", 1, 0) in reached["K < 16"] and ("E", 16, 0) in reached["K a multiple of 16"]
    assert ("Z", 128, 5) in reached["ragged last M-tile"] and ("Z", 128, 7) in reached["ragged last N-tile"]
    assert ("A16c", 37, 3) in reached["N < 4"]
    # every model of the zoo is differentiated at a batch size of at least 128 or by the older small-batch tests
    assert {k for k, _, _ in R.GRADIENT_CASES} >= set("DEFYQZ") and set(nb.MODELS) == set("ABCDEFYQZ")


def test_reference_gives_zero_weight_gradients_for_zero_images_with_zero_biases():
    """What the isolated-image GPU tests rest on: with zero biases and ReLU, an all-zero image has zero activations in every layer
    and a zero masked gradient in every ReLU layer, so it adds exactly nothing to any dW (db of the logits layer still sums over
    all images).  Checked on the float64 reference alone, for a Linear-only and a convolutional model."""
    for name in ("E", "F"):
        m = nb.MODELS[name]()
        layers = R.describe(m)
        rs = np.random.RandomState(1)
        params = [(rs.standard_normal(ws) * 0.1, np.zeros(bs)) for ws, bs in m.param_shapes()]
        y = rs.randint(0, 10, 4)
        x = np.zeros((4, 28, 28, 1))
        _, grads, _ = R.param_gradient(layers, params, x, y, seed=1, step=0)
        for dW, _ in grads:
            assert not dW.any()
        assert grads[-1][1].any() and not any(db.any() for _, db in grads[:-1])
        # one non-zero image among zeros: its gradient is that image's own term of the sum, whatever the zero images' labels are
        x[2] = rs.uniform(0, 1, (28, 28, 1))
        _, g1, _ = R.param_gradient(layers, params, x, y, seed=1, step=0)
        y2 = y.copy()
        y2[[0, 1, 3]] = (y2[[0, 1, 3]] + 1) % 10
        _, g2, _ = R.param_gradient(layers, params, x, y2, seed=1, step=0)
        for (dW, _), (dW2, _) in zip(g1, g2):
            assert dW.any()
            np.testing.assert_array_equal(dW, dW2)


def test_reference_loss_ignores_an_image_without_a_label_and_keeps_the_divisor():
    import torch
    z = torch.tensor([[1.0, 2.0, 0.5], [0.3, -1.0, 2.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    full = float(R.mean_ce(z, [2, 0, 1]))
    part = float(R.mean_ce(z, [2, -1, 1]))
    ce = -torch.log_softmax(z, dim=1).numpy()
    assert abs(full - (ce[0, 2] + ce[1, 0] + ce[2, 1]) / 3) < 1e-15
    assert abs(part - (ce[0, 2] + ce[2, 1]) / 3) < 1e-15
