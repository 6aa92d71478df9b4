"""-m "not gpu": the white-box driver (defensegan_amd/whitebox.py) on stub model, gan and attack objects -- flags, result files,
the ``rand`` bookkeeping, the refusals, the order of calls -- and the PGD definition as restated in tests/support/pgd_reference.py,
with the host side of network_builder.ProjectedGradientDescent and dg_pgd's argument checks.  The device kernels are
tests/test_gpu_pgd.py's, the flow on the device tests/test_gpu_whitebox.py's."""
import argparse
import inspect
import os
import pickle

import numpy as np
import pytest

from defensegan_amd import _native, network_builder as nb, whitebox as wb
from tests.support import bpda_reference as R
from tests.support import pgd_reference as P


# ---------------------------------------------------------------------- the command line and the result files
def test_cli_defaults_are_the_reference_flags():
    """whitebox.py:347-349, 367-392."""
    a = wb.build_parser().parse_args(["--data_dir", "d"])
    want = dict(alpha=0.05, nb_classes=10, learning_rate=0.001, nb_epochs=10, lmbda=0.1, fgsm_eps=0.3, rec_path=None, num_tests=-1,
                random_test_iter=-1, online_training=False, defense_type="none", attack_type="none", results_dir=None, same_init=False,
                model="F", debug_dir="temp", num_train=-1, debug=False, override=False, train_on_recs=False,
                eps_iter=None, nb_iter=None, eot_samples=None)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    # and whitebox()'s own defaults (whitebox.py:56-59; defense_type as the flag's)
    d = {k: p.default for k, p in inspect.signature(wb.whitebox).parameters.items()}
    for k, v in dict(rec_data_path=None, batch_size=128, learning_rate=0.001, nb_epochs=10, eps=0.3, alpha=0.05, online_training=False,
                     train_on_recs=False, test_on_dev=True, attack_type="fgsm", defense_type="none", num_tests=-1, num_train=-1,
                     fgsm_eps_tr=0.15, same_init=False, recs=None, attack_params=None, init_seed=0, phases=None).items():
        assert d[k] == v, k
    assert wb.ITERATIVE_DEFAULTS == {"eps_iter": 0.05, "nb_iter": 10, "eot_samples": 1}
    assert wb.CW_PARAMS == {"binary_search_steps": 1, "max_iterations": 100, "learning_rate": 10.0, "initial_const": 100}


def _flags(**kw):
    base = dict(fgsm_eps_tr=0.15, defense_type="none", attack_type="fgsm", dataset_name="mnist", rec_path=None, train_on_recs=False,
                num_tests=-1, num_train=-1, model="F")
    base.update(kw)
    return argparse.Namespace(**base)


class _Gan(object):
    checkpoint_dir, rec_rr, rec_lr, rec_iters = "output/gans/mnist", 10, 10.0, 200


def test_result_file_names_are_the_reference():
    """whitebox.py:309-341, branch by branch."""
    f = wb.get_results_dir_filename
    assert f(_flags(), _Gan()) == (os.path.join("results", "whitebox_none_mnist"), "model=F_nodefense_attack=fgsm.txt")
    assert f(_flags(defense_type="adv_tr", model="A", attack_type="pgd"), None) == (
        os.path.join("results", "whitebox_adv_tr_mnist"), "model=A_advTrEps=0.15attack=pgd.txt")
    # defense_gan without rec_path, and rec_path without defense_gan, fall to the last branch
    assert f(_flags(defense_type="defense_gan", attack_type="bpda"), _Gan()) == (
        os.path.join("results", "whitebox_defense_gan_mnist"), "model=F_nodefense_attack=bpda.txt")
    rp = "output/gans/mnist/recs_rr10_lr10.00000_iters200"
    assert f(_flags(rec_path=rp), _Gan())[1] == "model=F_nodefense_attack=fgsm.txt"
    assert f(_flags(num_tests=500), _Gan())[1] == "model=F_numtest=500_nodefense_attack=fgsm.txt"
    assert f(_flags(num_tests=500, num_train=1000, attack_type="cw"), _Gan())[1] == "model=F_numtrain=1000_numtest=500_nodefense_attack=cw.txt"
    assert f(_flags(num_tests=0), _Gan())[1] == "model=F_numtest=0_nodefense_attack=fgsm.txt"


def test_rec_path_name_is_the_one_the_reference_meant():
    """whitebox.py:317-323 formats 'Iter={}_RR={:d}_LR={:.4f}' with (rec_rr, rec_lr, rec_iters): rec_lr is a float after main's
    float(tr_lr), and a float under '{:d}' raises in Python -- the reference cannot name this file.  Written here: Iter = rec_iters,
    RR = rec_rr, LR = rec_lr."""
    g = _Gan()
    with pytest.raises(ValueError):
        "Iter={}_RR={:d}_LR={:.4f}_defense=gan".format(g.rec_rr, g.rec_lr, g.rec_iters, "fgsm")
    rp = "output/gans/mnist/recs_rr10_lr10.00000_iters200"
    f = wb.get_results_dir_filename
    assert f(_flags(defense_type="defense_gan", rec_path=rp, train_on_recs=True), g) == (
        "results/gans/mnist", "model=F_Iter=200_RR=10_LR=10.0000_defense=ganattack=fgsm.txt")
    assert f(_flags(defense_type="defense_gan", rec_path=rp, attack_type="bpda", num_tests=64), g) == (
        "results/gans/mnist", "model=F_numtest=64_orig_Iter=200_RR=10_LR=10.0000_defense=ganattack=bpda.txt")


def test_result_counter_accuracy_line_and_roc_pickle(tmp_path):
    """whitebox.py:269-306."""
    d = str(tmp_path / "results")
    p0 = wb.result_path(d, "name.txt", "run")
    assert p0 == os.path.join(d, "run", "0_name.txt")
    wb.write_results(p0, (0.25, 0, None))
    assert open(p0).read() == "0.25 0 \n"
    assert not os.path.exists(p0.replace(".txt", "_roc.pkl"))
    p1 = wb.result_path(d, "name.txt", "run")
    assert p1 == os.path.join(d, "run", "1_name.txt")                    # the counter never overwrites
    roc = [np.arange(3), np.arange(3)[::-1].copy(), np.array([0.5, 0.25, 0.125], np.float32)]
    wb.write_results(p1, (0.5, 0, roc))
    assert open(p1).read() == "0.5 0 \n"
    raw = open(p1.replace(".txt", "_roc.pkl"), "rb").read()
    assert b"numpy.core" in raw and b"numpy._core" not in raw            # readable by the Python-2 reference (py2pickle)
    for a, b in zip(pickle.loads(raw), roc):
        np.testing.assert_array_equal(a, b)
    assert wb.result_path(d, "name.txt") == os.path.join(d, "0_name.txt")


# ---------------------------------------------------------------------- whitebox() on stubs
class _StubModel(object):
    _device, _weights_set = 0, True

    def __init__(self, log):
        self.log, self.rec_layer = log, None

    def _ensure(self):
        pass

    def add_rec_model(self, gan, z_init, batch_size):
        self.log.append(("add_rec_model", None if z_init is None else tuple(z_init.shape), batch_size))
        self.rec_layer = (gan, z_init)


class _StubGan(object):
    dataset_name, arch_name, rec_rr, latent_dim = "mnist", "mnist", 2, 8

    def reconstruct(self, *a, **kw):
        raise AssertionError("the stubbed evaluation never projects")


def _stubs(monkeypatch, log, epochs_seen=None):
    """model_train, the accuracy, the attacks and the evaluation replaced by recorders; returns the data."""
    def model_train(model, X, Y, args=None, rng=None, adv_eps=None, adv_clip=None, evaluate=None, seed=None):
        log.append(("train", len(X), args["nb_epochs"], adv_eps, adv_clip, model.rec_layer is not None))
        assert rng.randint(0, 2 ** 31) == np.random.RandomState([11, 24, 1990]).randint(0, 2 ** 31)
        for _ in range(args["nb_epochs"]):
            evaluate()

    def accuracy(model, X, Y, batch_size):
        log.append(("accuracy", float(np.asarray(X).ravel()[0]), len(X)))
        return 0.75

    def attack_class(name):
        class Attack(object):
            def __init__(self, model, **kw):
                log.append(("build " + name, model.rec_layer is not None))

            def generate(self, x, *a, **kw):
                log.append(("generate " + name, len(x), float(np.asarray(x).min()), float(np.asarray(x).max()),
                            {k: v for k, v in kw.items() if k != "y"}, [np.asarray(v).tolist() for v in a]))
                return np.asarray(x) + 1.0
        Attack.DEFAULTS = nb.CarliniWagnerL2.DEFAULTS
        return Attack

    def model_eval_gan(reconstruct, model, X, Y, batch_size, rec_rr=1, compute_diffs=True, seed=None, same_init_z=None):
        log.append(("eval", reconstruct is not None, len(X), float(np.asarray(X).ravel()[0]), rec_rr, compute_diffs,
                    None if same_init_z is None else tuple(same_init_z.shape)))
        return 3, len(X), (["labels", "preds", "diffs"] if reconstruct is not None else None)

    monkeypatch.setattr(wb.utils_tf, "model_train", model_train)
    monkeypatch.setattr(wb, "_accuracy", accuracy)
    monkeypatch.setattr(wb.gan_defense, "model_eval_gan", model_eval_gan)
    for cls, name in (("FastGradientMethod", "fgsm"), ("CarliniWagnerL2", "cw"), ("ProjectedGradientDescent", "pgd"), ("BPDA", "bpda")):
        monkeypatch.setattr(wb.network_builder, cls, attack_class(name))
    x_tr, x_te = np.full((12, 2, 2, 1), 0.5, np.float32), np.full((6, 2, 2, 1), 0.5, np.float32)
    return x_tr, np.arange(12) % 3, x_te, np.arange(6) % 3


def test_flow_order_without_defense(monkeypatch):
    log = []
    data = _stubs(monkeypatch, log)
    out = wb.whitebox(None, _StubModel(log), data, batch_size=4, nb_epochs=2, attack_type="pgd", defense_type="adv_tr", num_tests=5,
                      num_train=10, attack_params={"nb_iter": 4, "eot_samples": None})
    assert out == (3 / 5.0, 0, None)
    assert [e[0] for e in log] == ["train", "accuracy", "accuracy", "accuracy", "build pgd", "generate pgd", "eval"]
    assert log[0] == ("train", 10, 2, 0.15, (0.0, 1.0), False)
    assert log[1] == log[2] == ("accuracy", 0.5, 5)                    # evaluate() per epoch, on the (truncated) test split
    assert log[3] == ("accuracy", 0.5, 10)                             # the training accuracy
    assert log[5][1] == 5 and log[5][4] == dict(eps=0.3, eps_iter=0.05, nb_iter=4, clip_min=0.0, clip_max=1.0, seed=wb.SEED,
                                                batch_size=wb.PGD_CALL_IMAGES)
    assert log[5][5] == [[0, 1, 2, 0, 1]]                              # the true labels
    assert log[6] == ("eval", False, 5, 1.5, 1, False, None)           # the attack's images, bare


def test_no_attack_returns_the_training_accuracy(monkeypatch):
    for none in (None, "none"):
        log = []
        data = _stubs(monkeypatch, log)
        assert wb.whitebox(None, _StubModel(log), data, batch_size=4, nb_epochs=1, attack_type=none) == (0.75, 0, None)
        assert [e[0] for e in log] == ["train", "accuracy", "accuracy"]


@pytest.mark.parametrize("attack,same_init", [("fgsm", True), ("bpda", False)])
def test_flow_order_with_defense_gan_attaches_the_projection_after_training(monkeypatch, attack, same_init):
    log = []
    data = _stubs(monkeypatch, log)
    recs = (np.full((12, 2, 2, 1), 0.25, np.float32), data[1], np.full((6, 2, 2, 1), 0.125, np.float32), data[3])
    acc, zero, roc = wb.whitebox(_StubGan(), _StubModel(log), data, batch_size=4, nb_epochs=1, attack_type=attack,
                                 defense_type="defense_gan", train_on_recs=True, recs=recs, same_init=same_init,
                                 attack_params={"eot_samples": 3})
    assert (acc, zero, roc) == (0.5, 0, ["labels", "preds", "diffs"])
    assert [e[0] for e in log] == ["train", "accuracy", "accuracy", "add_rec_model", "build " + attack] + \
        ["generate " + attack] * (2 if attack == "fgsm" else 1) + ["eval"]
    assert log[0] == ("train", 12, 1, None, (0.0, 1.0), False)         # trained bare, on the reconstructions
    assert log[1] == ("accuracy", 0.125, 6) and log[2] == ("accuracy", 0.25, 12)
    assert log[3] == ("add_rec_model", (8, 8) if same_init else None, 4)          # [batch_size * rec_rr, latent_dim], sigma = 1
    assert log[4] == ("build " + attack, True)                         # built on the defended model
    gen = log[5]
    assert (gen[2], gen[3]) == (0.5, 0.5)                              # the attack starts from the ORIGINAL test images
    if attack == "fgsm":
        assert (log[5][1], log[6][1]) == (4, 2) and gen[4] == dict(eps=0.3, ord=np.inf, clip_min=0.0, clip_max=1.0)
    else:
        assert gen[1] == 6 and gen[4] == dict(eps=0.3, eps_iter=0.05, nb_iter=10, eot_samples=3, clip_min=0.0, clip_max=1.0,
                                              seed=wb.SEED, batch_size=4)
    assert log[-1] == ("eval", True, 6, 1.5, 2, True, (8, 8) if same_init else None)


def test_cw_on_defense_gan_is_built_before_the_projection_is_attached(monkeypatch, capsys):
    log = []
    data = _stubs(monkeypatch, log)
    out = wb.whitebox(_StubGan(), _StubModel(log), data, batch_size=4, nb_epochs=1, attack_type="cw", defense_type="defense_gan",
                      attack_params={"max_iterations": 7, "nb_iter": 3})
    assert out[2] == ["labels", "preds", "diffs"]
    assert [e[0] for e in log] == ["train", "accuracy", "accuracy", "build cw", "add_rec_model", "generate cw", "eval"]
    assert log[3] == ("build cw", False)
    assert log[5][4] == dict(binary_search_steps=1, max_iterations=7, learning_rate=10.0, initial_const=100, batch_size=4)
    assert log[6][:3] == ("eval", True, 6)
    assert "BARE classifier" in capsys.readouterr().out
    # without the defense the attack is built where the reference builds it
    del log[:]
    wb.whitebox(None, _StubModel(log), data, batch_size=4, nb_epochs=1, attack_type="cw")
    assert [e[0] for e in log] == ["train", "accuracy", "accuracy", "build cw", "generate cw", "eval"]
    assert log[4][4]["max_iterations"] == 100


@pytest.mark.parametrize("attack_type", ["rand_fgsm", "rand+fgsm"])
def test_rand_takes_alpha_off_the_budget(monkeypatch, attack_type):
    """whitebox.py:192-196: x' = clip(x + alpha sign(N(0, 1)), min_val, 1) and eps - alpha reach the attack."""
    log = []
    data = _stubs(monkeypatch, log)
    wb.whitebox(None, _StubModel(log), data, batch_size=6, nb_epochs=1, eps=0.3, alpha=0.125, attack_type=attack_type)
    gen = [e for e in log if e[0] == "generate fgsm"]
    assert len(gen) == 1 and gen[0][4]["eps"] == pytest.approx(0.175, abs=1e-12)
    assert (gen[0][2], gen[0][3]) == (0.375, 0.625)                    # every pixel moved by +- alpha, both signs drawn
    assert wb.attack_kind("fgsm") == ("fgsm", False) and wb.attack_kind(attack_type) == ("fgsm", True)
    assert wb.attack_kind("rand_pgd") == ("pgd", True) and wb.attack_kind("cw") == ("cw", False) and wb.attack_kind("none") is None


def test_pairing_errors_and_refusals():
    data = (np.zeros((4, 28, 28, 1), np.float32), np.zeros(4, np.int64)) * 2
    with pytest.raises(ValueError, match="bpda"):
        wb.whitebox(_StubGan(), nb.model_f(), data, attack_type="pgd", defense_type="defense_gan")
    for defense in ("none", "adv_tr"):
        with pytest.raises(ValueError, match="is pgd"):
            wb.whitebox(None, nb.model_f(), data, attack_type="bpda", defense_type=defense)
    with pytest.raises(ValueError, match="same_init"):
        wb.whitebox(_StubGan(), nb.model_f(), data, attack_type="bpda", defense_type="defense_gan", same_init=True)
    with pytest.raises(ValueError, match="unknown attack_type"):
        wb.whitebox(None, nb.model_f(), data, attack_type="deepfool")
    with pytest.raises(ValueError, match="unknown attack_type"):
        wb.whitebox(None, nb.model_f(), data, attack_type="rand_cw")
    with pytest.raises(ValueError, match="unknown attack_params"):
        wb.whitebox(None, nb.model_f(), data, attack_type="pgd", attack_params={"steps": 3})
    with pytest.raises(ValueError, match="needs a gan"):
        wb.whitebox(None, nb.model_f(), data, defense_type="defense_gan")
    with pytest.raises(ValueError, match="defense_type"):
        wb.whitebox(None, nb.model_f(), data, defense_type="gan")
    with pytest.raises(NotImplementedError, match="never trains through the projection either"):
        wb.whitebox(_StubGan(), nb.model_f(), data, defense_type="defense_gan", online_training=True)
    with pytest.raises(ValueError, match="train_on_recs"):
        wb.whitebox(_StubGan(), nb.model_f(), data, defense_type="defense_gan", train_on_recs=True)


# ---------------------------------------------------------------------- the PGD definition
LINEAR2 = [("flatten",), ("linear", 2), ("softmax",)]


def test_pgd_rule_by_hand_on_a_two_pixel_example():
    """Two pixels, two classes, logits = x W + b with W = [[1, -1], [-2, 2]]: for y = 0 the gradient is p_1 (W[:, 1] - W[:, 0]) =
    p_1 (-2, 4), so every step is (-eps_iter, +eps_iter) until the ball's face.  logit_1 - logit_0 = -2 x_0 + 4 x_1 - b_0 with
    b = (1.9, 0): -0.9 at x_0 = (0.5, 0.5), -0.3 at (0.4, 0.6), +0.3 at (0.3, 0.7): iterate 2 is the first success."""
    W, b = np.array([[1.0, -1.0], [-2.0, 2.0]]), np.array([1.9, 0.0])
    x, y = np.full((1, 1, 2, 1), 0.5), np.array([0])
    ops = P.classifier_ops(LINEAR2, [(W, b)], y)
    out = P.pgd(ops, x, y, eps=0.25, eps_iter=0.1, nb_iter=4, lo=0.0, hi=1.0)
    want = [[0.5, 0.5], [0.4, 0.6], [0.3, 0.7], [0.25, 0.75], [0.25, 0.75]]          # the third step lands on the ball's face
    np.testing.assert_allclose(np.array(out["iterates"]).reshape(5, 2), want, rtol=0, atol=1e-15)
    assert np.sign(out["grads"][0]).ravel().tolist() == [-1.0, 1.0]
    assert out["first_success"].tolist() == [2]
    np.testing.assert_allclose(out["x_adv"].ravel(), [0.3, 0.7], rtol=0, atol=1e-15)
    assert [out["preds"][j].tolist() for j in (1, 2, 3, 4)] == [[0], [1], [1], [1]]
    # the range clips after the ball: from x = (0.05, 0.95) the same steps stop at 0 and 1
    out = P.pgd(ops, np.array([0.05, 0.95]).reshape(1, 1, 2, 1), y, eps=0.25, eps_iter=0.1, nb_iter=2, lo=0.0, hi=1.0)
    np.testing.assert_allclose(out["iterates"][2].ravel(), [0.0, 1.0], rtol=0, atol=1e-15)
    # a zero gradient (W = 0) leaves x_0, projected onto the ball and the range
    flat = P.classifier_ops(LINEAR2, [(np.zeros((2, 2)), b)], y)
    out = P.pgd(flat, x, y, eps=0.25, eps_iter=0.1, nb_iter=2, lo=0.0, hi=1.0, x_init=np.array([0.9, 0.5]).reshape(1, 1, 2, 1))
    np.testing.assert_allclose(out["iterates"][2].ravel(), [0.75, 0.5], rtol=0, atol=1e-15)


def test_pgd_is_bpda_with_the_identity_projection_and_one_sample():
    calls = []

    class Ops(object):
        def gradient(self, x_k):
            calls.append(("gradient", float(x_k.ravel()[0])))
            return np.ones_like(x_k)

        def predict(self, x_k):
            calls.append(("predict", float(x_k.ravel()[0])))
            return np.zeros(len(x_k), np.int64)
    out = P.pgd(Ops(), np.zeros((2, 1, 1, 1)), np.zeros(2, np.int64), eps=1.0, eps_iter=0.25, nb_iter=3, lo=0.0, hi=1.0)
    # nb_iter gradients, and one prediction per iterate 1 .. nb_iter, each on the iterate itself
    assert calls == [("gradient", 0.0), ("predict", 0.25), ("gradient", 0.25), ("predict", 0.5), ("gradient", 0.5), ("predict", 0.75)]
    assert out["seeds"] == [0, 1, 2, 3] and out["first_success"].tolist() == [-1, -1]
    assert out["x_adv"].ravel().tolist() == [0.75, 0.75]                # no success: the last iterate


def test_pgd_tracking_on_a_prescribed_prediction_sequence():
    labels = np.array([3, 3, 3, 3])
    seq = {0.25: np.array([3, 5, 3, 3]),                                # image 1 succeeds at iterate 1
           0.5: np.array([4, 3, 3, 3]),                                 # image 0 at 2; image 1 "fails" again: not undone
           0.75: np.array([3, 3, 3, 9])}                                # image 3 at the last iterate; image 2 never

    class Ops(object):
        def gradient(self, x_k):
            return np.ones_like(x_k)

        def predict(self, x_k):
            return seq[float(x_k.ravel()[0])]
    out = P.pgd(Ops(), np.zeros((4, 1, 1, 2)), labels, eps=1.0, eps_iter=0.25, nb_iter=3, lo=0.0, hi=1.0)
    assert out["first_success"].tolist() == [2, 1, -1, 3]
    assert out["x_adv"][:, 0, 0, 0].tolist() == [0.5, 0.25, 0.75, 0.75]


def test_pgd_argument_checks():
    x, y = np.zeros((2, 28, 28, 1), np.float32), np.zeros(2, np.int32)
    atk = nb.ProjectedGradientDescent(nb.model_e())
    with pytest.raises(ValueError, match="nb_iter"):
        atk.generate(x, y, nb_iter=0)
    with pytest.raises(ValueError, match="eps"):
        atk.generate(x, y, eps=-0.1)
    with pytest.raises(ValueError, match="eps"):
        atk.generate(x, y, eps_iter=-0.1)
    with pytest.raises(ValueError, match="clip_min"):
        atk.generate(x, y, clip_min=1.0, clip_max=0.0)
    with pytest.raises(ValueError, match="not both"):
        atk.generate(x, y, rand_init=True, x_init=x)
    with pytest.raises(ValueError, match="batch_size"):
        atk.generate(x, y, batch_size=0)
    defended = nb.model_e()
    defended.add_rec_model(object(), None, 4)
    with pytest.raises(ValueError, match="use BPDA"):
        nb.ProjectedGradientDescent(defended).generate(x, y)
    with pytest.raises(ValueError, match="PGD-on-bare.*ProjectedGradientDescent"):
        nb.BPDA(nb.model_e()).generate(x, y)
    d = {k: p.default for k, p in inspect.signature(atk.generate).parameters.items()}
    assert (d["eps"], d["eps_iter"], d["nb_iter"], d["rand_init"], d["return_info"]) == (0.3, 0.05, 10, False, False)


def test_dg_pgd_refuses_bad_arguments_on_the_host():
    """The value checks come before any device call: they answer without a GPU, with dg_last_error's text."""
    lib = _native.load()
    for args, text in (((0.3, 0.05, 0, 0.0, 1.0), b"nb_iter"), ((-0.1, 0.05, 1, 0.0, 1.0), b"eps"), ((0.3, -1.0, 1, 0.0, 1.0), b"eps"),
                       ((0.3, 0.05, 1, 1.0, 0.0), b"clip_min"), ((float("nan"), 0.05, 1, 0.0, 1.0), b"eps"),
                       ((0.3, 0.05, 1, 0.0, 1.0), b"bad argument")):
        eps, eps_iter, nb_iter, lo, hi = args
        assert lib.dg_pgd(None, None, None, None, 1, eps, eps_iter, nb_iter, lo, hi, None, None, None) == -1
        assert text in lib.dg_last_error(), (args, lib.dg_last_error())


# ---------------------------------------------------------------------- what the GPU cases' choice of seeds promises
@pytest.mark.parametrize("name", sorted(P.CASES))
def test_gpu_cases_have_few_undecided_pixels_on_the_reference_alone(name):
    """tests/test_gpu_pgd.py compares x_{k+1} on the decided pixels, |g| > 1e-4 max|g|; the cases' seeds are chosen so that the float64
    reference leaves at most 1 % of the pixels undecided at every teacher-forced iterate."""
    c = P.CASES[name]
    x = P.case_inputs(name)[0]
    out = P.case_reference(name)
    assert len(out["grads"]) == 3 and out["iterates"][0].shape == (c["B"],) + c["shape"]
    for g in out["grads"]:
        print("%s: undecided %.5f" % (name, R.undecided_fraction(g)))
        assert R.undecided_fraction(g) <= 0.01
    for xk in out["iterates"]:
        assert np.abs(xk - x).max() <= c["eps"] + 1e-12 and xk.min() >= c["lo"] and xk.max() <= c["hi"]
    assert not np.array_equal(out["iterates"][1], out["iterates"][0])
