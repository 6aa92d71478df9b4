"""-m "not gpu": the saliency-map attack's definition as restated in tests/support/jsma_reference.py -- every input set the GPU tests
use is mostly decidable, a float32 run takes the decidable trajectories, the pair rule is cleverhans' [F, F] arg-max --, the host
side of attacks.SaliencyMapMethod, and whitebox's target draw and flags on stub objects.  The device kernels are
tests/test_gpu_jsma.py's."""
import os

import numpy as np
import pytest
import torch

from defensegan_amd import attacks, network_builder as nb, whitebox as wb
from tests.support import jsma_reference as JR
from tests.test_whitebox_cpu import _StubGan, _StubModel, _stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, c) for name, c in sorted(JR.RUN_CASES.items())] + [("step%d" % i, c) for i, c in enumerate(JR.STEP_CASES)] + [("tile", JR.TILE_CASE)]


# ---------------------------------------------------------------------- the input sets
@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_every_input_set_is_mostly_decidable(name, c):
    out = JR.case_run(c)
    dec = JR.decidable(out)
    m = out["score_margin"][np.isfinite(out["score_margin"])]
    print("%s: decidable %d/%d, iterations up to %d, smallest relative score margin %.3e" % (name, dec.sum(), dec.size, out["iters"].max(),
                                                                                           m.min() if m.size else np.nan))
    assert dec.mean() >= 0.75
    assert out["iters"].max() >= 1                                  # the case attacks something
    assert (out["n_changed"] <= 2 * out["iters"]).all()
    assert out["x_adv"].min() >= 0.0 and out["x_adv"].max() <= 1.0


@pytest.mark.parametrize("name", sorted(JR.RUN_CASES))
def test_the_float32_run_takes_the_decidable_trajectories(name):
    ref, f32 = JR.case_run(name), JR.float32_run(name)
    dec = JR.decidable(ref)
    assert (f32["choices"][:, dec] == ref["choices"][:, dec]).all()
    for k in ("iters", "final_class", "n_changed"):
        assert (f32[k][dec] == ref[k][dec]).all(), k
    assert np.array_equal(f32["x_adv"][dec], ref["x_adv"].astype(np.float32)[dec])          # +-theta and a clip: the same bits


def test_whole_runs_cover_both_endings():
    """Among the whole runs there are images that reach the target and images that run out of iterations or pairs."""
    ok = np.concatenate([JR.case_run(n)["final_class"] == JR.case_run(n)["target"] for n in JR.RUN_CASES])
    assert ok.any() and not ok.all()
    out = JR.case_run("r784")
    assert out["iters"].max() == 39 and out["choices"].shape == (39, 8, 2)


# ---------------------------------------------------------------------- the pair rule
@pytest.mark.parametrize("theta", [1.0, -1.0])
def test_the_pair_choice_is_cleverhans_flat_argmax_with_the_increase_coef_trick(theta):
    """Restricting the pairs to the domain picks the pair that cleverhans' shifted [F, F] tables pick, wherever an admissible pair exists
    (without one cleverhans returns (0, 0); the definition here stops the image)."""
    rs = np.random.RandomState(12)
    seen = 0
    for trial in range(200):
        F = int(rs.randint(2, 40))
        a, b = rs.standard_normal(F), rs.standard_normal(F)
        if trial % 3 == 0:
            b = -a                                                  # the softmax outputs' case
        if trial % 5 == 0:
            a[rs.randint(0, F)] = a[rs.randint(0, F)]               # an exact tie now and then
        dom = rs.uniform(0, 1, F) < 0.7
        p, q, best, second, _ = JR.pair_choice(a, b, dom, theta)
        if p < 0:
            continue
        seen += 1
        assert 0 <= p < q < F and dom[p] and dom[q] and best > 0 and second <= best
        assert (p, q) == JR.cleverhans_pair(a, b, dom, theta), trial
    assert seen > 100


def test_pair_choice_edges():
    a, b = np.array([1.0, 1.0, 1.0, np.nan]), np.array([-1.0, -1.0, -1.0, -1.0])
    dom = np.ones(4, bool)
    assert JR.pair_choice(a, b, dom, 1.0)[:3] == (0, 1, 4.0)                   # a three-way tie goes to (0, 1); the NaN pair never wins
    assert JR.pair_choice(a, b, dom, -1.0)[:2] == (-1, -1)                      # no admissible pair for the other sign
    assert JR.pair_choice(a, b, np.array([True, False, False, False]), 1.0)[:2] == (-1, -1)
    assert JR.pair_choice(np.zeros(4), np.zeros(4), dom, 1.0)[:2] == (-1, -1)   # zero gradients: nothing, not (0, 0)


def test_the_grid_caps_stand_where_the_tiled_case_was_chosen_for():
    for name, text in JR.CAP_SOURCES:
        with open(os.path.join(ROOT, "defensegan_amd", "csrc", name)) as fh:
            assert text in fh.read(), text
    assert JR.TILE_B > JR.IMAGE_CAP > JR.WAVE_CAP and JR.IMAGE_CAP % JR.TILE_CASE["B"] == 10


# ---------------------------------------------------------------------- the front end, before the device is touched
def test_front_end_refusals():
    m = nb.model_f()
    atk = attacks.SaliencyMapMethod(m)
    assert nb.SaliencyMapMethod is attacks.SaliencyMapMethod
    x, y = np.zeros((2, 28, 28, 1), np.float32), np.array([1, 2])
    with pytest.raises(ValueError, match="unknown SaliencyMapMethod parameters"):
        atk.generate(x, y_target=y, eps=0.3)
    with pytest.raises(ValueError, match="y_target is required"):
        atk.generate(x)
    for bad in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="theta"):
            atk.generate(x, y_target=y, theta=bad)
    with pytest.raises(ValueError, match="gamma"):
        atk.generate(x, y_target=y, gamma=-0.1)
    with pytest.raises(ValueError, match="clip_min must not exceed clip_max"):
        atk.generate(x, y_target=y, clip_min=1.0, clip_max=0.0)
    with pytest.raises(ValueError, match="batch_size"):
        atk.generate(x, y_target=y, batch_size=0)
    m.rec_layer = object()
    with pytest.raises(NotImplementedError, match="reconstruction layer"):
        atk.generate(x, y_target=y)
    assert atk.max_iters(784, 1.0) == 392 and atk.max_iters(784, 0.1) == 39 and atk.max_iters(25, 1.0) == 12 and atk.max_iters(16, 0.0) == 0
    p = atk.parse_params({})
    assert (p["theta"], p["gamma"], p["clip_min"], p["clip_max"], p["of_probs"], p["batch_size"], p["return_info"]) == (1.0, 1.0, 0.0, 1.0, True, None, False)


# ---------------------------------------------------------------------- whitebox: the target draw, the flags, the result line
def test_whitebox_targets_are_never_the_true_class_and_come_from_the_runs_generator():
    y = np.arange(1000) % 10
    t = wb.jsma_targets(y, 10, np.random.RandomState(3))
    assert t.dtype == np.int32 and (t != y).all() and t.min() == 0 and t.max() == 9
    assert np.array_equal(t, (y + 1 + np.random.RandomState(3).randint(0, 9, 1000)) % 10)
    assert len(set((t - y) % 10)) == 9                              # every other class is drawn
    assert (wb.jsma_targets([0, 1, 0], 2, np.random.RandomState(0)) == [1, 0, 1]).all()
    with pytest.raises(ValueError, match="at least 2 classes"):
        wb.jsma_targets(y, 1, np.random.RandomState(0))
    s = wb.jsma_summary([1, 2, 0, 0], [1, 2, 1, 0], [4, 8, 2, 6], 16)
    assert s == {"success_rate": 0.75, "l0": (4 + 8 + 6) / 3.0 / 16}
    assert np.isnan(wb.jsma_summary([0], [1], [2], 16)["l0"])


def test_whitebox_flow_and_flags(monkeypatch, tmp_path):
    log = []
    data = _stubs(monkeypatch, log)

    class Jsma(object):
        def __init__(self, model, **kw):
            log.append(("build jsma", model.rec_layer is not None))

        def generate(self, x, **kw):
            log.append(("generate jsma", len(x), kw))
            n = len(x)
            return np.asarray(x) + 1.0, np.full(n, 2, np.int32), np.asarray(kw["y_target"]) * np.array([1, 1, 1, 0, 1, 1][:n]), np.full(n, 4, np.int32)
    monkeypatch.setattr(wb.network_builder, "SaliencyMapMethod", Jsma, raising=False)
    model = _StubModel(log)
    model.nb_classes = 3
    norms = {}
    out = wb.whitebox(None, model, data, batch_size=4, nb_epochs=1, attack_type="jsma", defense_type="adv_tr", num_tests=5,
                      attack_params={"jsma_theta": -0.5, "jsma_gamma": 0.25, "nb_iter": 3}, norms=norms)
    assert out == (3 / 5.0, 0, None)
    assert [e[0] for e in log] == ["train", "accuracy", "accuracy", "build jsma", "generate jsma", "eval"]
    kw = log[4][2]
    rng = np.random.RandomState([11, 24, 1990])
    rng.randint(0, 2 ** 31)                                         # what the stubbed training drew
    want = wb.jsma_targets(np.arange(5) % 3, 3, rng)
    assert np.array_equal(kw.pop("y_target"), want) and (want != np.arange(5) % 3).all()
    assert kw == dict(theta=-0.5, gamma=0.25, clip_min=0.0, clip_max=1.0, return_info=True)
    # image 3's class is not its target unless the target is 0
    ok = (want * np.array([1, 1, 1, 0, 1])) == want
    assert norms == {"success_rate": ok.mean(), "l0": 4 / 4.0}
    p = str(tmp_path / "r.txt")
    wb.write_results(p, out, norms)
    assert open(p).read() == "0.6 0 success=%s l0=1.0 \n" % ok.mean()
    # the defaults, the flags, the refusals
    del log[:]
    wb.whitebox(None, model, data, batch_size=4, nb_epochs=1, attack_type="jsma")
    assert log[4][2]["theta"] == 1.0 and log[4][2]["gamma"] == 0.1
    a = wb.build_parser().parse_args(["--data_dir", "d", "--attack_type", "jsma", "--jsma_theta", "-1", "--jsma_gamma", "0.05"])
    assert (a.jsma_theta, a.jsma_gamma) == (-1.0, 0.05)
    a = wb.build_parser().parse_args(["--data_dir", "d"])
    assert (a.jsma_theta, a.jsma_gamma) == (1.0, 0.1)
    assert wb.attack_kind("jsma") == ("jsma", False)
    with pytest.raises(ValueError, match="unknown attack_type.*jsma"):
        wb.attack_kind("rand_jsma")
    with pytest.raises(ValueError, match="bare classifier"):
        wb.whitebox(_StubGan(), model, data, attack_type="jsma", defense_type="defense_gan")
    with pytest.raises(ValueError, match="attack_ord"):
        wb.whitebox(None, model, data, attack_type="jsma", attack_ord=2)
    assert wb.get_results_dir_filename(_flags(), None)[1] == "model=F_nodefense_attack=jsma.txt"


def _flags():
    import argparse
    return argparse.Namespace(fgsm_eps_tr=0.15, defense_type="none", attack_type="jsma", dataset_name="mnist", rec_path=None, train_on_recs=False,
                              num_tests=-1, num_train=-1, model="F")
