"""-m "not gpu": the black-box substitute flow's host side.  The float64 restatement of the class gradient
(tests/support/blackbox_reference.py) is pinned on its own -- finite differences, a hand-computed model, the saturated case --
so that tests/test_gpu_blackbox.py compares the device with something checked; train_sub's schedule, batch_eval, the command
line's defaults and the result file names are checked against the reference's blackbox.py:143-213, 596-630, 663-674, 723-759."""
import argparse
import os

import numpy as np
import pytest

from defensegan_amd import attacks_tf, blackbox, network_builder as nb, utils_tf
from tests.support import blackbox_reference as BR
from tests.support import train_reference as R


# ---------------------------------------------------------------------- the restatement, pinned
def _every_layer_kind():
    """Conv2D SAME and VALID with strides, ReLU, Dropout (identity at evaluation), Flatten, Linear, Softmax on 9 x 8 x 2."""
    m = nb.MLP([nb.Dropout(0.8), nb.Conv2D(3, (3, 3), (1, 1), "SAME"), nb.ReLU(), nb.Conv2D(4, (3, 2), (2, 1), "VALID"), nb.ReLU(),
                nb.Flatten(), nb.Dropout(0.5), nb.Linear(6), nb.ReLU(), nb.Linear(4), nb.Softmax()], (None, 9, 8, 2))
    rs = np.random.RandomState(3)
    params = [(rs.standard_normal(w) * 0.5, rs.standard_normal(b) * 0.1) for w, b in m.param_shapes()]
    return m, params, rs


def test_class_gradient_matches_central_finite_differences():
    m, params, rs = _every_layer_kind()
    layers = R.describe(m)
    x = rs.uniform(-1, 1, (3, 9, 8, 2))
    classes = np.array([0, 3, 1])
    assert R.relu_margins(layers, params, x).min() > 1e-4          # no kink within the difference step
    g = BR.class_gradient(layers, params, x, classes)
    h, worst = 1e-6, 0.0
    for idx in [tuple(rs.randint(0, s) for s in x.shape) for _ in range(40)]:
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        b = idx[0]
        fd = (BR.prob_of_class(layers, params, xp, classes)[b] - BR.prob_of_class(layers, params, xm, classes)[b]) / (2 * h)
        worst = max(worst, abs(fd - g[idx]))
    assert worst <= 1e-8 * max(1.0, np.abs(g).max()), worst
    # the logits' gradient is another thing: of_probs=False differentiates z_c
    gl = BR.class_gradient(layers, params, x, classes, of_probs=False)
    assert np.abs(gl - g).max() > 1e-3


def test_class_gradient_of_a_hand_computed_two_class_linear_model():
    """Flatten, Linear(2), Softmax on a 1 x 1 x 2 image: z = x W + b, p = softmax(z), dp_0/dx = p_0 p_1 (W[:, 0] - W[:, 1])."""
    m = nb.MLP([nb.Flatten(), nb.Linear(2), nb.Softmax()], (None, 1, 1, 2))
    W, b = np.array([[1.0, -2.0], [0.5, 3.0]]), np.array([0.25, -0.75])
    x = np.array([[[[0.2, -0.4]]]])
    z = x.reshape(1, 2) @ W + b
    p = np.exp(z) / np.exp(z).sum()
    want0 = p[0, 0] * p[0, 1] * (W[:, 0] - W[:, 1])
    layers = R.describe(m)
    np.testing.assert_allclose(BR.class_gradient(layers, [(W, b)], x, [0]).reshape(2), want0, rtol=1e-13)
    np.testing.assert_allclose(BR.class_gradient(layers, [(W, b)], x, [1]).reshape(2), -want0, rtol=1e-13)
    np.testing.assert_allclose(BR.class_gradient(layers, [(W, b)], x, [1], of_probs=False).reshape(2), W[:, 1], rtol=1e-13)
    # augmentation: the old half, then x + lmbda * sign, outside [0, 1] when it leads there
    out = BR.jacobian_augmentation(layers, [(W, b)], x, [0], 0.1)
    assert out.shape == (2, 1, 1, 2)
    np.testing.assert_array_equal(out[0], x[0])
    np.testing.assert_allclose(out[1].reshape(2), x.reshape(2) + 0.1 * np.sign(want0), rtol=0, atol=1e-16)
    assert out[1].min() < 0


def test_saturated_class_has_an_exactly_zero_seed():
    """Once p_c rounds to 1 and the other classes' exp underflows, (delta_kc - p_c) * p_k is exactly 0 in every component: the
    gradient is exactly 0 and the augmented image equals the original."""
    z = np.array([[1000.0, -1000.0, 0.0]])
    assert (BR.softmax_seed(z, [0]) == 0).all()
    assert BR.softmax_seed(z, [1])[0, 1] == 0 and (BR.softmax_seed(z, [1]) == 0).all()      # p_1 = 0: nothing flows either
    m = nb.MLP([nb.Flatten(), nb.Linear(2), nb.Softmax()], (None, 1, 1, 2))
    W, b = np.array([[1.0, -2.0], [0.5, 3.0]]) * 1e4, np.zeros(2)
    x = np.array([[[[0.2, -0.4]]]])
    layers = R.describe(m)
    c = int((x.reshape(1, 2) @ W).argmax())
    assert (BR.class_gradient(layers, [(W, b)], x, [c]) == 0).all()
    out = BR.jacobian_augmentation(layers, [(W, b)], x, [c], 0.1)
    np.testing.assert_array_equal(out[1], x[0])


# ---------------------------------------------------------------------- train_sub's schedule
class _Recorder(object):
    """Stands in for model_train and jacobian_augmentation: records the calls; augmentation appends X + 1000 * (round + 1)."""

    def __init__(self, rng):
        self.rng, self.events, self.round = rng, [], 0

    def model_train(self, model, X, Y, args=None, rng=None, seed=None, **kw):
        assert rng is self.rng and kw == {}
        self.events.append(("train", len(X), np.array(X), np.array(Y), dict(args), seed, rng.randint(0, 1 << 30)))
        return True

    def augment(self, model, X, Y, lmbda, batch_size=128):
        self.events.append(("augment", len(X), lmbda, batch_size, np.array(Y)))
        self.round += 1
        return np.vstack([X, X + 1000.0 * self.round])


def _run_schedule(monkeypatch, holdout, data_aug, batch_size=128):
    rng = np.random.RandomState(utils_tf.WHITEBOX_RNG_SEED)
    rec = _Recorder(rng)
    monkeypatch.setattr(utils_tf, "model_train", rec.model_train)
    monkeypatch.setattr(attacks_tf, "jacobian_augmentation", rec.augment)
    X0 = np.arange(holdout, dtype=np.float64).reshape(holdout, 1, 1, 1)
    Y0 = np.arange(holdout) % 10

    def oracle_labels(X):
        rec.events.append(("label", len(X), np.array(X)))
        return (np.asarray(X).reshape(-1).astype(np.int64) // 1000) % 7 + 10          # labels no Y0 holds: 11 .. 16

    _, X, Y = blackbox.train_sub(object(), oracle_labels, X0, Y0, 10, batch_size, 0.001, data_aug, 0.1, rng, seed=500)
    return rec, X0, Y0, X, Y, oracle_labels


def test_train_sub_schedule_sizes_halves_labels_and_rng_order(monkeypatch):
    rec, X0, Y0, X, Y, oracle_labels = _run_schedule(monkeypatch, 150, 6)
    kinds = [e[0] for e in rec.events]
    assert kinds == ["train", "augment", "label"] * 5 + ["train"]               # no augmentation after the last round
    trains = [e for e in rec.events if e[0] == "train"]
    assert [e[1] for e in trains] == [150, 300, 600, 1200, 2400, 4800]
    assert len(X) == len(Y) == 4800
    assert [e[1] for e in rec.events if e[0] == "label"] == [150, 300, 600, 1200, 2400]   # only the new half is queried
    assert [e[5] for e in trains] == [500 + rho for rho in range(6)]            # Dropout seed + rho
    assert all(e[4] == {"nb_epochs": 10, "batch_size": 128, "learning_rate": 0.001} for e in trains)
    # one rng, drawn from in round order: the recorder's draws are the first six of a fresh RandomState([11, 24, 1990])
    fresh = np.random.RandomState(utils_tf.WHITEBOX_RNG_SEED)
    assert [e[6] for e in trains] == [fresh.randint(0, 1 << 30) for _ in range(6)]
    prevX, prevY = X0, Y0
    for t in trains[1:]:
        n = len(prevX)
        np.testing.assert_array_equal(t[2][:n], prevX)                          # the first half of X_sub is untouched
        np.testing.assert_array_equal(t[3][:n], prevY)                          # ... and of Y_sub: hstack, second half overwritten
        np.testing.assert_array_equal(t[3][n:], oracle_labels(t[2][n:]))        # the new half carries the oracle's labels
        assert not np.array_equal(t[3][n:], prevY)
        prevX, prevY = t[2], t[3]
    # the augmentation saw the labels of the set it was given
    aug = [e for e in rec.events if e[0] == "augment"]
    assert [e[1] for e in aug] == [150, 300, 600, 1200, 2400] and all(e[2] == 0.1 and e[3] == 128 for e in aug)
    for a, t in zip(aug, trains):
        np.testing.assert_array_equal(a[4], t[3])


def test_train_sub_schedule_equals_the_restatement(monkeypatch):
    rec, X0, Y0, X, Y, oracle_labels = _run_schedule(monkeypatch, 8, 3, batch_size=4)
    k = [0]

    def augment(Xs, Ys):
        k[0] += 1
        return np.vstack([Xs, Xs + 1000.0 * k[0]])

    Xr, Yr, log = BR.train_sub_schedule(lambda *a: None, augment, oracle_labels, X0, Y0, 3)
    np.testing.assert_array_equal(X, Xr)
    np.testing.assert_array_equal(Y, Yr)
    assert [(e[0], e[2]) for e in log] == [("train", 8), ("augment", 8), ("label", 8), ("train", 16), ("augment", 16), ("label", 16),
                                           ("train", 32)]


def test_train_sub_refuses_a_holdout_smaller_than_a_batch():
    with pytest.raises(ValueError, match="holdout .* smaller than batch_size"):
        blackbox.train_sub(object(), lambda X: None, np.zeros((100, 28, 28, 1), np.float32), np.zeros(100, np.int64), 10, 128, 0.001, 6,
                           0.1, np.random.RandomState(0))


def test_blackbox_refuses_online_training_and_recs_that_are_not_there():
    data = (np.zeros((4, 28, 28, 1), np.float32), np.zeros(4, np.int64)) * 2
    with pytest.raises(NotImplementedError, match="online_training"):
        blackbox.blackbox(None, nb.model_f(), nb.model_e(), data, defense_type="defense_gan", online_training=True)
    with pytest.raises(ValueError, match="train_on_recs"):
        blackbox.blackbox(None, nb.model_f(), nb.model_e(), data, defense_type="defense_gan", train_on_recs=True)


def test_class_gradient_and_augmentation_refuse_the_reconstruction_layer():
    m = nb.model_e()
    m.add_rec_model(object(), None, 4)
    x = np.zeros((2, 28, 28, 1), np.float32)
    for call in (lambda: m.class_gradient(x, [0, 1]), lambda: m.jacobian(x), lambda: attacks_tf.jacobian_augmentation(m, x, [0, 1], 0.1)):
        with pytest.raises(NotImplementedError, match="reconstruction layer"):
            call()


# ---------------------------------------------------------------------- batch_eval
def test_batch_eval_runs_consecutive_batches_with_a_partial_last_one():
    X = np.arange(11 * 3, dtype=np.float32).reshape(11, 3)
    seen = []

    def fn(xb):
        seen.append(np.array(xb))
        return xb * 2

    out = utils_tf.batch_eval(fn, X, 4)
    np.testing.assert_array_equal(out, X * 2)
    assert [len(s) for s in seen] == [4, 4, 3]                          # NOT shifted back as model_train's last batch is
    np.testing.assert_array_equal(np.concatenate(seen), X)
    np.testing.assert_array_equal(utils_tf.batch_eval_labels(fn, X, 4), np.full(11, 2))
    np.testing.assert_array_equal(utils_tf.batch_eval_labels(lambda xb: -xb, X + 1, 5), np.zeros(11, np.int64))
    with pytest.raises(ValueError):
        utils_tf.batch_eval(fn, X, 0)
    with pytest.raises(ValueError):
        utils_tf.batch_eval(fn, X[:0], 4)


# ---------------------------------------------------------------------- the command line and the result files
def test_cli_defaults_are_the_reference_flags():
    """blackbox.py:723-759."""
    a = blackbox.build_parser().parse_args(["--data_dir", "d"])
    want = dict(nb_classes=10, learning_rate=0.001, nb_epochs=10, holdout=150, data_aug=6, nb_epochs_s=10, lmbda=0.1, fgsm_eps=0.3,
                fgsm_eps_tr=0.15, rec_path=None, num_tests=2000, random_test_iter=-1, online_training=False, defense_type="none",
                results_dir=None, train_on_recs=False, num_train=-1, bb_model="F", sub_model="E", debug_dir=None, debug=False,
                override=False)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    # and blackbox()'s own defaults (blackbox.py:370-374)
    import inspect
    d = {k: p.default for k, p in inspect.signature(blackbox.blackbox).parameters.items()}
    for k, v in dict(batch_size=128, learning_rate=0.001, nb_epochs=10, holdout=150, data_aug=6, nb_epochs_s=10, lmbda=0.1,
                     online_training=False, train_on_recs=False, test_on_dev=True, defense_type="none").items():
        assert d[k] == v, k


def _flags(**kw):
    base = dict(data_aug=6, fgsm_eps=0.3, fgsm_eps_tr=0.15, defense_type="none", dataset_name="mnist", rec_path=None, train_on_recs=False,
                num_tests=-1, num_train=-1, bb_model="F", sub_model="E")
    base.update(kw)
    return argparse.Namespace(**base)


class _Gan(object):
    checkpoint_dir, rec_rr, rec_lr, rec_iters = "output/gans/mnist", 10, 10.0, 200


def test_result_file_names_are_the_reference():
    """blackbox.py:596-630."""
    f = blackbox.get_results_dir_filename
    assert f(_flags(), _Gan()) == (os.path.join("results", "none_mnist"), "bbModel=F_subModel=E_sub=6_eps=0.30.txt")
    assert f(_flags(defense_type="adv_tr", bb_model="A", sub_model="B"), _Gan()) == (
        os.path.join("results", "adv_tr_mnist"), "bbModel=A_subModel=B_sub=6_trEps=0.15_eps=0.30.txt")
    rp = "output/gans/mnist/recs_rr10_lr10.00000_iters200"
    assert f(_flags(defense_type="defense_gan", rec_path=rp, train_on_recs=True), _Gan()) == (
        "results/gans/mnist", "bbModel=F_subModel=E_teRR=10_teLR=10.0000_teIter=200_sub=6_eps=0.30.txt")
    assert f(_flags(defense_type="defense_gan", rec_path=rp), _Gan()) == (
        "results/gans/mnist", "bbModel=F_subModel=E_orig_teRR=10_teLR=10.0000_teIter=200_sub=6_eps=0.30.txt")
    # defense_gan without rec_path keeps the plain name; rec_path without defense_gan too
    assert f(_flags(defense_type="defense_gan"), _Gan())[1] == "bbModel=F_subModel=E_sub=6_eps=0.30.txt"
    assert f(_flags(rec_path=rp), _Gan()) == (os.path.join("results", "none_mnist"), "bbModel=F_subModel=E_sub=6_eps=0.30.txt")
    assert f(_flags(num_tests=2000), _Gan())[1] == "bbModel=F_subModel=E_numtest=2000_sub=6_eps=0.30.txt"
    assert f(_flags(num_tests=2000, num_train=500), _Gan())[1] == "bbModel=F_subModel=E_numtrain=500_numtest=2000_sub=6_eps=0.30.txt"
    assert f(_flags(num_tests=0), _Gan())[1] == "bbModel=F_subModel=E_numtest=0_sub=6_eps=0.30.txt"


def test_result_counter_accuracy_line_and_roc_pickle(tmp_path):
    """blackbox.py:663-699."""
    import pickle
    d = str(tmp_path / "results")
    p0 = blackbox.result_path(d, "name.txt", "run")
    assert p0 == os.path.join(d, "run", "0_name.txt")
    acc = {"bbox": 0.99, "sub": 0, "bbox_on_sub_adv_ex": 0.25}
    blackbox.write_results(p0, acc)
    assert open(p0).read() == "0.99 0 0.25 \n"
    assert not os.path.exists(p0.replace(".txt", "_roc.pkl"))
    p1 = blackbox.result_path(d, "name.txt", "run")
    assert p1 == os.path.join(d, "run", "1_name.txt")                    # the counter never overwrites
    roc = [np.arange(3), np.arange(3)[::-1].copy(), np.array([0.5, 0.25, 0.125], np.float32)]
    blackbox.write_results(p1, dict(acc, roc_info=roc))
    raw = open(p1.replace(".txt", "_roc.pkl"), "rb").read()
    assert b"numpy.core" in raw and b"numpy._core" not in raw            # readable by the Python-2 reference (py2pickle)
    back = pickle.loads(raw)
    for a, b in zip(back, roc):
        np.testing.assert_array_equal(a, b)
    assert blackbox.result_path(d, "name.txt") == os.path.join(d, "0_name.txt")


# ---------------------------------------------------------------------- the cached reconstructions (--rec_path)
def test_load_recs_reads_back_the_cache_reconstruct_dataset_writes(tmp_path):
    """--rec_path names <checkpoint_dir>/recs_rr{R}_lr{lr}_iters{L}; its per-image pickles (the layout DefenseGANBase.reconstruct_dataset
    writes, gan.py:504-557) are read back without one projection, and what is missing is reconstructed and cached."""
    from defensegan_amd import config
    from defensegan_amd.gan import MnistDefenseGAN
    rs = np.random.RandomState(0)
    splits = {"train": (rs.rand(7, 28, 28, 1).astype(np.float32), np.arange(7) % 3),
              "test": (rs.rand(5, 28, 28, 1).astype(np.float32), np.arange(5) % 4)}

    def gan_with(reconstruct, **rec):
        g = MnistDefenseGAN(cfg={"USE_BN": False}, test_mode=True, **rec)
        g.reconstruct = reconstruct
        return g
    half = lambda images, **kw: np.asarray(images) * 0.5
    writer = gan_with(half, rec_rr=2, rec_iters=5, rec_lr=10.0)
    writer.reconstruct_dataset(splits, str(tmp_path), batch_size=3)
    rec_path = tmp_path / "recs_rr2_lr10.00000_iters5"
    assert len(list((rec_path / "train" / "pickles").iterdir())) == 7 and not (rec_path / "train" / "feats.pkl").exists()

    # the command line's way: the projection parameters come from the directory's name, whatever the cfg says
    args = blackbox.build_parser().parse_args(["--data_dir", "d", "--rec_path", str(rec_path) + os.sep, "--defense_type", "defense_gan"])
    rp = config.resolve_rec_params({"REC_RR": 10, "REC_LR": 1.0, "REC_ITERS": 200}, args)
    assert (rp["rec_rr"], rp["rec_lr"], rp["rec_iters"]) == (2, 10.0, 5)

    def refuse(images, **kw):
        raise AssertionError("the cache is complete: nothing is to be reconstructed")
    reader = gan_with(refuse, rec_rr=rp["rec_rr"], rec_iters=rp["rec_iters"], rec_lr=rp["rec_lr"])
    tr, ytr, te, yte = blackbox.load_recs(reader, args.rec_path, splits, batch_size=4)
    assert tr.dtype == np.float32 and tr.shape == (7, 28, 28, 1) and te.shape == (5, 28, 28, 1)
    np.testing.assert_array_equal(tr, splits["train"][0] * 0.5)
    np.testing.assert_array_equal(te, splits["test"][0] * 0.5)
    np.testing.assert_array_equal(ytr, splits["train"][1])
    np.testing.assert_array_equal(yte, splits["test"][1])
    # --num_train / --debug truncate the originals first: the reconstructions are then truncated with them
    tr3 = blackbox.load_recs(reader, args.rec_path, {"train": (splits["train"][0][:3], splits["train"][1][:3]), "test": splits["test"]}, 4)[0]
    np.testing.assert_array_equal(tr3, splits["train"][0][:3] * 0.5)
    # an image missing from the cache: its batch is reconstructed and cached again
    missing = rec_path / "test" / "pickles" / "rec_0000004_l0.pkl"
    missing.unlink()
    with pytest.raises(AssertionError, match="nothing is to be reconstructed"):
        blackbox.load_recs(reader, args.rec_path, splits, batch_size=4)
    te2 = blackbox.load_recs(gan_with(half, rec_rr=2, rec_iters=5, rec_lr=10.0), args.rec_path, splits, batch_size=4)[2]
    np.testing.assert_array_equal(te2, te)
    assert missing.exists()
