"""-m "not gpu": the elastic-net attack's float64 restatement (tests/support/ead_reference.py) against hand-computed cases, the front
end of attacks.ElasticNetMethod and of whitebox --attack_type ead without a device, and the recorded seeds of the GPU tests."""
import numpy as np
import pytest
import torch

from defensegan_amd import attacks, network_builder as nb, whitebox
from tests.support import ead_reference as E

# one Linear layer on P = 4 pixels, two classes: Z_0 - Z_1 = v . x + b_0, so with the label 0 and the hinge active dloss1/dx = v
LAYERS = [("flatten",), ("linear", 2)]
V = np.array([2.0, -2.0, 0.1, -3.0])


def _params(b0):
    return [(np.stack([V, np.zeros(4)], axis=1), np.array([b0, 0.0]))]


def _img(*rows):
    return torch.as_tensor(np.array(rows, np.float64).reshape(len(rows), 2, 2, 1))


def test_rate_and_extrapolation_weight():
    f32 = lambda v: float(np.float32(v))
    assert E.rate(0, 10, 0.1) == f32(0.1)
    assert E.rate(1, 10, 0.1) == f32(0.1 * 0.9 ** 0.5)
    assert E.rate(9, 10, 0.1) == f32(0.1 * 0.1 ** 0.5)
    assert E.rate(9, 10, 0.1) > 0                                     # the decay reaches 0 only past the last iteration
    assert [E.zt_of(i, True) for i in (0, 1, 9)] == [f32(1 / 4), f32(2 / 5), f32(10 / 13)]
    assert [E.zt_of(i, False) for i in (0, 1, 9)] == [0.0, 0.0, 0.0]


def test_every_shrinkage_branch_and_both_clips():
    """lr = 0.1, const = 1, beta = 0.05, X = Y = x0: S - x0 = -0.1 v = (-0.2, 0.2, -0.01, 0.3)."""
    x0 = _img([0.1, 0.9, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5])
    Xn, Yn, S = E.ista_step(LAYERS, _params(5.0), x0, x0, x0, np.array([0, 0]), np.array([1.0, 1.0]), 0.0, False, 0.05, 0.1, 0.25, 0.0, 1.0)
    np.testing.assert_allclose(S.reshape(2, 4).numpy(), [[-0.1, 1.1, 0.49, 0.8], [0.3, 0.7, 0.49, 0.8]], atol=1e-15)
    want = np.array([[0.0, 1.0, 0.5, 0.75],                           # lower branch clipped at lo, upper clipped at hi, middle, upper
                     [0.35, 0.65, 0.5, 0.75]])                        # lower and upper branch unclipped, middle, upper
    np.testing.assert_allclose(Xn.reshape(2, 4).numpy(), want, atol=1e-15)
    assert Xn.reshape(2, 4)[0, 2].item() == 0.5 and Xn.reshape(2, 4)[0, 0].item() == 0.0 and Xn.reshape(2, 4)[0, 1].item() == 1.0   # exact
    x0n = x0.reshape(2, 4).numpy()
    np.testing.assert_allclose(Yn.reshape(2, 4).numpy(), want + 0.25 * (want - x0n), atol=1e-15)
    assert Yn.min().item() < 0.0 and Yn.max().item() > 1.0            # the slack is not clipped
    # without fista the slack is the iterate
    Xi, Yi, _ = E.ista_step(LAYERS, _params(5.0), x0, x0, x0, np.array([0, 0]), np.array([1.0, 1.0]), 0.0, False, 0.05, 0.1, E.zt_of(0, False),
                            0.0, 1.0)
    assert torch.equal(Xi, Yi) and torch.equal(Xi, Xn)
    # the threshold itself belongs to the middle branch
    S = torch.tensor([0.55, 0.45, 0.5500001, 0.4499999], dtype=torch.float64)
    got = E.shrink(S, torch.full((4,), 0.5, dtype=torch.float64), 0.05, 0.0, 1.0)
    assert got[0].item() == 0.5 and got[1].item() == 0.5 and got[2].item() > 0.5 and got[3].item() < 0.5


def test_a_slack_outside_the_box_moves_the_next_step():
    """The second iteration starts from the unclipped slack: with X' = (0, 1, ...) and Y' outside [0, 1] the L2 term 2 (Y - x0) uses Y."""
    x0 = _img([0.1, 0.9, 0.5, 0.5])
    t, c = np.array([0]), np.array([1.0])
    X1, Y1, _ = E.ista_step(LAYERS, _params(5.0), x0, x0, x0, t, c, 0.0, False, 0.05, 0.1, 0.25, 0.0, 1.0)
    g = E.slack_gradient(LAYERS, _params(5.0), Y1, x0, t, c, 0.0, False).reshape(4).numpy()
    np.testing.assert_allclose(g, V + 2 * (Y1 - x0).reshape(4).numpy(), atol=1e-15)
    assert Y1.reshape(4)[0].item() == pytest.approx(-0.025) and Y1.reshape(4)[1].item() == pytest.approx(1.025)


def test_one_iteration_whole_run():
    """b_0 = 1.6.  Image 0: Z_0 - Z_1 = -1.45 at x0, the hinge is off, g = 0, X' = x0, a success at distance 0.  Image 1: 0.15 at x0, one
    step to (0.35, 0.65, 0.5, 0.75) where it is -1.2: a success with l1 = 0.55, l2 = 0.1075."""
    x = np.array([[0.1, 0.9, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5]]).reshape(2, 2, 2, 1)
    kw = dict(labels=np.array([0, 0]), batch_size=2, beta=0.05, learning_rate=0.1, binary_search_steps=1, max_iterations=1, initial_const=1.0)
    beta = float(np.float32(0.05))
    out = E.ead(LAYERS, _params(1.6), x, **kw)
    np.testing.assert_array_equal(out["best_class"], [1, 1])
    lr = E.rate(0, 1, 0.1)
    want = 0.5 + np.array([-lr * 2 + beta, lr * 2 - beta, 0.0, lr * 3 - beta])
    np.testing.assert_allclose(out["x_adv"].reshape(2, 4), [[0.1, 0.9, 0.5, 0.5], want], atol=1e-12)
    e = want - 0.5
    np.testing.assert_allclose(out["best_dist"], [0.0, (e * e).sum() + beta * np.abs(e).sum()], atol=1e-12)
    np.testing.assert_allclose(out["best_dist"][1], 0.135, atol=1e-6)
    np.testing.assert_allclose(out["const"], [0.5, 0.5])              # success: upper = 1, const = (0 + 1) / 2
    assert out["kept"].tolist() == [[True] * 4, [False, False, True, False]]
    l1 = E.ead(LAYERS, _params(1.6), x, decision_rule="L1", **kw)
    np.testing.assert_allclose(l1["best_dist"], [0.0, np.abs(e).sum()], atol=1e-12)
    # a constant too small to leave the threshold: nothing moves, image 1 fails, the constant grows tenfold
    small = E.ead(LAYERS, _params(1.6), x, **dict(kw, initial_const=0.1))
    assert small["best_class"].tolist() == [1, -1] and small["best_dist"][1] == 1e10
    assert small["x_adv"].tobytes() == x.astype(np.float64).tobytes()
    np.testing.assert_allclose(small["const"], [0.05, 1.0])


def test_the_two_rules_pick_different_bests():
    """a = one pixel moved by 0.5 (l1 0.5, l2 0.25), b = three pixels moved by 0.2 (l1 0.6, l2 0.12), beta = 0.1: EN 0.30 against 0.18."""
    x0 = _img([0.2, 0.2, 0.2, 0.2], [0.2, 0.2, 0.2, 0.2])
    X = _img([0.7, 0.2, 0.2, 0.2], [0.4, 0.4, 0.4, 0.2])
    l1, l2, en = E.distances(X, x0, 0.1, "EN")
    np.testing.assert_allclose(l1.numpy(), [0.5, 0.6]); np.testing.assert_allclose(l2.numpy(), [0.25, 0.12])
    np.testing.assert_allclose(en.numpy(), [0.30, 0.18])
    assert int(en.argmin()) == 1 and int(E.distances(X, x0, 0.1, "L1")[2].argmin()) == 0


# ---------------------------------------------------------------------------------------------------- the front end, no device
def test_defaults_and_argument_checks_need_no_device():
    D = attacks.ElasticNetMethod.DEFAULTS
    assert D == dict(batch_size=1, confidence=0.0, beta=1e-3, decision_rule="EN", fista=True, learning_rate=1e-2, binary_search_steps=9,
                     max_iterations=1000, abort_early=False, initial_const=1e-3, clip_min=0.0, clip_max=1.0)
    assert nb.ElasticNetMethod is attacks.ElasticNetMethod
    m = nb.MODELS["F"]()
    ead = attacks.ElasticNetMethod(m)
    x = np.zeros((2, 28, 28, 1), np.float32)
    with pytest.raises(ValueError, match="decision_rule"):
        ead.generate(x, decision_rule="L2")
    with pytest.raises(ValueError, match="beta"):
        ead.generate(x, beta=-1e-3)
    with pytest.raises(ValueError, match="beta"):
        ead.generate(x, beta=float("nan"))
    with pytest.raises(ValueError, match="max_iterations"):
        ead.generate(x, max_iterations=0)
    with pytest.raises(ValueError, match="clip_min"):
        ead.generate(x, clip_min=1.0, clip_max=1.0)
    with pytest.raises(TypeError, match="unknown ElasticNetMethod parameters"):
        ead.generate(x, eps=0.3)
    with pytest.raises(ValueError, match="not both"):
        ead.generate(x, y=np.zeros(2, np.int64), y_target=np.ones(2, np.int64))
    m.rec_layer = object()
    with pytest.raises(NotImplementedError, match="reconstruction layer"):
        ead.generate(x)
    assert m._handle is None if hasattr(m, "_handle") else True       # nothing touched the device
    assert attacks.ElasticNetMethod.parse_params({"decision_rule": "L1"})["decision_rule"] == 1


def test_whitebox_front_end():
    assert whitebox.attack_kind("ead") == ("ead", False)
    assert "ead" in whitebox.ATTACKS
    with pytest.raises(ValueError, match="unknown attack_type"):
        whitebox.attack_kind("rand_ead")
    with pytest.raises(ValueError, match="unknown attack_type"):
        whitebox.attack_kind("rand+ead")
    assert whitebox.attack_ord_value("inf", "ead") == np.inf
    with pytest.raises(ValueError, match="ord must be"):              # exactly as cw: inf only
        whitebox.attack_ord_value("2", "ead")
    with pytest.raises(NotImplementedError):
        whitebox.attack_ord_value("1", "ead")
    for o in ("1", "2"):
        with pytest.raises(type(pytest.raises(Exception, whitebox.attack_ord_value, o, "cw").value)):
            whitebox.attack_ord_value(o, "ead")
    assert whitebox.EAD_PARAMS == {"binary_search_steps": 5, "max_iterations": 100, "learning_rate": 1e-2, "initial_const": 1.0}
    assert whitebox._attack_params("ead", None) == {"beta": 1e-3, "decision_rule": "EN"}
    assert whitebox._attack_params("ead", {"ead_beta": 0.05, "ead_rule": "L1", "nb_iter": 3, "max_iterations": 7}) == {
        "beta": 0.05, "decision_rule": "L1", "max_iterations": 7}
    a = whitebox.build_parser().parse_args(["--cfg", "mnist", "--data_dir", "d", "--attack_type", "ead"])
    assert a.ead_beta == 1e-3 and a.ead_rule == "EN"
    a = whitebox.build_parser().parse_args(["--cfg", "mnist", "--data_dir", "d", "--attack_type", "ead", "--ead_beta", "0.01", "--ead_rule", "L1"])
    assert a.ead_beta == 0.01 and a.ead_rule == "L1"


def test_result_line_gains_the_two_norms(tmp_path):
    p = str(tmp_path / "r.txt")
    whitebox.write_results(p, (0.25, 0, None), {"l1": 3.5, "l2": 0.75, "successes": 4})
    whitebox.write_results(p, (0.5, 0, None))
    assert open(p).read() == "0.25 0 l1=3.5 l2=0.75 \n0.5 0 \n"


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_recorded_seed_is_the_first_accepted(name):
    layers, params = E.case_model(name)
    assert E.find_seed(E.CASES[name], layers, params) == E.SEEDS[name]


def test_the_cases_show_what_they_are_named_for():
    """What the GPU tests assert on the reference again, checked here when the cases are chosen."""
    def run(name):
        layers, params = E.case_model(name)
        return E.run_case(E.CASES[name], E.SEEDS[name], layers, params)[2]
    sparse = run("sparse_F")
    assert 0.05 < sparse["kept"].mean() < 0.95
    clip = run("clip_F")
    assert min(clip["clamped"]) > 100
    en, l1 = run("rule_en_F"), run("rule_l1_F")
    assert (np.abs(en["x_adv"] - l1["x_adv"]).reshape(16, -1).max(axis=1) > 1e-3).any()
    assert not np.array_equal(run("five_F")["x_adv"], run("five_ista_F")["x_adv"])
    stops = run("abort_F")["abort_iters"][0]
    assert None not in stops and len(set(stops)) >= 2
    wide = run("wide_F")["abort_iters"][0]
    assert None not in wide and len(set(wide)) == 2
    c = run("search_F")["const"]
    assert (c < 6.0).any() and (c > 6.0).any()
    mixed = run("mixed_F")["best_class"]
    assert (mixed == -1).any() and (mixed != -1).mean() >= 0.25
