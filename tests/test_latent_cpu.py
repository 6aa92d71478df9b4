"""-m "not gpu": the latent-space attack's float64 reference (tests/support/latent_reference.py) checked on its own -- the margin's
tie rule, the hinge's seed, the tracker's rules, the gradient against central differences, the recorded draws -- and the host side
of network_builder.LatentAttack and of the whitebox driver on stand-in operations.  The device is tests/test_gpu_latent.py's."""
import numpy as np
import pytest

from defensegan_amd import network_builder as nb, whitebox as wb
from tests.support import generator_reference as GR
from tests.support import latent_reference as LR


def test_the_runner_up_takes_the_first_maximum_on_ties():
    Z = np.array([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [5.0, 1.0, 0.0, 5.0]])
    m, o = LR.margin_of(Z, [0, 1, 0])
    assert o.tolist() == [1, 0, 3] and m.tolist() == [-2.0, 0.0, 0.0]


def test_the_seed_is_zero_exactly_when_the_hinge_is_off():
    m, o, lab = np.array([-0.5, -0.5, 0.25, -1.0]), np.array([1, 1, 0, 2]), [0, 0, 2, 1]
    g = LR.hinge_seed(m, o, lab, 3, 2.0, 0.5)
    assert not g[0].any() and not g[1].any() and not g[3].any()              # m + kappa = 0 is off
    assert g[2].tolist() == [-2.0, 0.0, 2.0]
    assert LR.hinge_seed(m, o, lab, 3, 2.0, 0.75)[0].tolist() == [2.0, -2.0, 0.0]


def test_the_trackers_tie_rules_and_its_no_success_branch():
    # image 0: successes (k, r) = (0, 1), (1, 0), (1, 1) at equal distance -> the earliest k; image 1: two successes in one
    # iterate at equal distance -> the smallest r; image 2: a later, strictly smaller distance wins; image 3: no success -> the
    # FINAL iterate's smallest margin, smallest r on ties
    m = np.array([[[1, -1], [-1, -1], [-1, 1], [3, 2]],
                  [[-1, -1], [1, 1], [-2, 1], [1, 1]]], np.float64)
    d = np.array([[[9, 5], [4, 4], [6, 1], [7, 7]],
                  [[5, 5], [1, 1], [5, 0], [8, 8]]], np.float64)
    bd, bm, bi, br = LR.track(m, d, 0.0)
    assert bi.tolist() == [0, 0, 1, -1] and br.tolist() == [1, 0, 0, 0]
    assert bd.tolist() == [5, 4, 5, 8] and bm.tolist() == [-1, -1, -2, 1]
    # kappa moves the success line: m < -kappa
    assert LR.track(m, d, 1.0)[2].tolist() == [-1, -1, 1, -1]
    assert LR.track(m, d, 1.0)[3].tolist() == [0, 0, 0, 0]


def test_autograd_against_central_differences():
    """d(sum_j f_j)/dz at a decided point (a recorded draw: every gate, o_j and the hinge's sign are away from their kinks)."""
    name = "conv_3x2"
    latent, kind, B, R, c, kappa = LR.CASES[name]
    gp, clf, x, labels, z0 = LR.case_inputs(name, *LR.SEEDS[name])
    z = z0.astype(np.float64)
    it = LR.iteration(gp, clf, x, labels, R, z, c, kappa)
    assert (it["margin"] + kappa > 0).any()                                  # the classification term is in play
    f = lambda zz: LR.iteration(gp, clf, x, labels, R, zz, c, kappa)["f"].sum()
    rs, h = np.random.RandomState(0), 1e-6
    for _ in range(4):
        j, i = rs.randint(z.shape[0]), rs.randint(z.shape[1])
        e = np.zeros_like(z)
        e[j, i] = h
        num = (f(z + e) - f(z - e)) / (2 * h)
        assert abs(num - it["dz"][j, i]) <= 1e-6 * max(1.0, np.abs(it["dz"]).max()), (j, i, num, it["dz"][j, i])
    # dy is the classifier's input gradient for the hinge's seed plus 2 (y - x) / 784
    import torch
    y = torch.as_tensor(it["y"]).requires_grad_(True)
    (LR.logits(clf[0], clf[1], y) * torch.as_tensor(it["dlogits"])).sum().backward()
    want = y.grad.numpy() + 2.0 * (it["y"] - np.repeat(x.astype(np.float64), R, axis=0)) / 784.0
    assert np.abs(want - it["dy"]).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_the_recorded_draws_are_accepted_by_the_reference_alone(name):
    s = LR.accepted_case(name, *LR.SEEDS[name])
    assert s is not None, "the recorded (classifier seed, draw seed) of %s is no longer accepted" % name
    print("%s: float32 on the CPU uses %.3f / %.3f / %.3f of the dz / margin / dist bounds" % ((name,) + s))
    assert max(s) <= LR.MAX_SHARE


def test_the_attack_seed_succeeds_in_float64():
    ref = LR.attack_reference(LR.ATTACK_SEED)
    assert int((ref["best_iter"] >= 0).sum()) >= 6
    _, clf, x, labels, _ = LR.attack_inputs(LR.ATTACK_SEED)
    import torch
    pred = LR.logits(clf[0], clf[1], torch.as_tensor(ref["x_adv"])).argmax(dim=1).numpy()
    assert (pred[ref["best_iter"] >= 0] != labels[ref["best_iter"] >= 0]).all()


# ---------------------------------------------------------------------- the host side
class _Gan(object):
    rec_rr, latent_dim, use_bn = 3, 8, False

    class _arch(object):
        arch_id = 0


def test_latent_attack_takes_the_gan_of_the_reconstruction_layer_and_refuses_by_name():
    from defensegan_amd.gan import CelebADefenseGAN, MnistDefenseGAN
    model = nb.model_f()
    with pytest.raises(ValueError, match="needs the generator"):
        nb.LatentAttack(model)
    gan = MnistDefenseGAN(cfg={"USE_BN": False}, test_mode=True)
    model.add_rec_model(gan, None, 4)
    assert nb.LatentAttack(model).gan is gan
    x = np.zeros((1, 28, 28, 1), np.float32)
    with pytest.raises(NotImplementedError, match="not implemented for the CelebA generator"):
        nb.LatentAttack(model, CelebADefenseGAN(cfg={"USE_BN": False}, test_mode=True)).generate(x, [0])
    with pytest.raises(NotImplementedError, match="not implemented for use_bn"):
        nb.LatentAttack(model, MnistDefenseGAN(cfg={"USE_BN": True}, test_mode=True)).generate(x, [0])
    with pytest.raises(ValueError, match="rec_rr"):
        nb.LatentAttack(model, gan).generate(x, [0], rec_rr=0)
    with pytest.raises(ValueError, match="confidence"):
        nb.LatentAttack(model, gan).generate(x, [0], confidence=-1.0)


# ---------------------------------------------------------------------- the driver on stand-in operations
def _stubs(monkeypatch, log):
    class Attack(object):
        def __init__(self, model, gan=None):
            log.append(("build latent", model.rec_layer is not None, gan))

        def generate(self, x, y, **kw):
            log.append(("generate latent", len(x), np.asarray(y).tolist(), kw))
            return np.asarray(x) + 1.0

    def model_eval_gan(reconstruct, model, X, Y, batch_size, rec_rr=1, compute_diffs=True, seed=None, same_init_z=None):
        log.append(("eval", reconstruct is not None, len(X), float(np.asarray(X).ravel()[0]), rec_rr))
        return 2, len(X), ["labels", "preds", "diffs"]

    monkeypatch.setattr(wb.utils_tf, "model_train", lambda *a, **kw: None)
    monkeypatch.setattr(wb, "_accuracy", lambda *a: 0.75)
    monkeypatch.setattr(wb.gan_defense, "model_eval_gan", model_eval_gan)
    monkeypatch.setattr(wb.network_builder, "LatentAttack", Attack)
    return np.full((8, 2, 2, 1), 0.5, np.float32), np.arange(8) % 3, np.full((4, 2, 2, 1), 0.5, np.float32), np.arange(4) % 3


class _Model(object):
    _device, _weights_set, rec_layer = 0, True, None

    def _ensure(self):
        pass

    def add_rec_model(self, gan, z_init, batch_size):
        self.rec_layer = (gan, z_init)


class _StubGan(object):
    dataset_name, arch_name, rec_rr, latent_dim = "mnist", "mnist", 5, 8

    def reconstruct(self, *a, **kw):
        raise AssertionError("the stubbed evaluation never projects")


def test_driver_flag_plumbing_and_the_refusal_without_the_defense(monkeypatch):
    log = []
    data = _stubs(monkeypatch, log)
    gan = _StubGan()
    out = wb.whitebox(gan, _Model(), data, batch_size=4, nb_epochs=1, attack_type="latent", defense_type="defense_gan",
                      attack_params={"latent_iters": 7, "latent_c": 2.5, "nb_iter": None})
    assert out == (0.5, 0, ["labels", "preds", "diffs"])
    assert [e[0] for e in log] == ["build latent", "generate latent", "eval"]
    assert log[0] == ("build latent", True, gan)                                  # built on the defended model, with its gan
    assert log[1][1:3] == (4, [0, 1, 2, 0])                                       # the original test images, the true labels
    assert log[1][3] == dict(rec_rr=5, nb_iter=7, learning_rate=0.05, c=2.5, seed=wb.SEED, batch_size=4)
    assert log[2] == ("eval", True, 4, 1.5, 5)                                    # x_adv through model_eval_gan's projection
    for defense in ("none", "adv_tr"):
        with pytest.raises(ValueError, match="needs the projection"):
            wb.whitebox(None, _Model(), data, attack_type="latent", defense_type=defense)
    assert wb.attack_kind("latent") == ("latent", False)
    for bad in ("rand_latent", "deepfool"):
        with pytest.raises(ValueError, match="^unknown attack_type"):
            wb.attack_kind(bad)
    assert wb.LATENT_DEFAULTS == {"latent_iters": 100, "latent_lr": 0.05, "latent_c": 1.0}
    # the command line and the result file
    a = wb.build_parser().parse_args(["--data_dir", "d", "--attack_type", "latent", "--defense_type", "defense_gan", "--latent_iters", "9",
                                      "--latent_lr", "0.1", "--latent_c", "3"])
    assert (a.latent_iters, a.latent_lr, a.latent_c) == (9, 0.1, 3.0)
    b = wb.build_parser().parse_args(["--data_dir", "d"])
    assert (b.latent_iters, b.latent_lr, b.latent_c) == (None, None, None)
    a.dataset_name, a.fgsm_eps_tr = "mnist", 0.15
    # the naming rule, branch by branch: defense_gan without rec_path falls to the last branch, as for every attack; with
    # rec_path the defended run's own name
    assert wb.get_results_dir_filename(a, gan)[1] == "model=F_nodefense_attack=latent.txt"
    a.rec_path, gan.checkpoint_dir, gan.rec_iters, gan.rec_lr = "output/gans/mnist/recs_rr5_lr10.00000_iters200", "output/gans/mnist", 200, 10.0
    assert wb.get_results_dir_filename(a, gan) == ("results/gans/mnist", "model=F_orig_Iter=200_RR=5_LR=10.0000_defense=ganattack=latent.txt")
