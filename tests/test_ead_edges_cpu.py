"""-m "not gpu": the elastic-net edge cases of tests/support/ead_reference.py (EDGE_CASES) without a device: every recorded seed is
the first that find_seed accepts, and each case shows on the float64 reference the property that tests/test_gpu_ead_edges.py needs of
it -- a case that lacks its property tests nothing."""
import functools

import numpy as np
import pytest

from tests.support import ead_reference as E
from tests.test_gpu_ead import DIST_RTOL


@functools.lru_cache(maxsize=None)
def _run(name, **override):
    layers, params = E.case_model(name)
    return E.run_case(E.CASES[name], E.SEEDS[name], layers, params, **override)


def test_the_edge_cases_are_cases_like_the_others():
    """They sit in CASES and SEEDS, so tests/test_ead_cpu.py::test_recorded_seed_is_the_first_accepted re-derives each of their seeds
    through find_seed / accepted, unchanged."""
    from tests import test_ead_cpu
    assert all(E.CASES[name] is case and name in E.SEEDS for name, case in E.EDGE_CASES.items())
    assert set(E.EDGE_CASES) == {"kappa_F", "kappa_targeted_F", "kappa_abort_F", "huge_chunk_tiny", "abort_every_F", "given_y_F", "beta0_F", "two_class_tiny"}
    marks = [m for m in test_ead_cpu.test_recorded_seed_is_the_first_accepted.pytestmark if m.name == "parametrize"]
    assert set(E.EDGE_CASES) <= set(marks[0].args[1])


@pytest.mark.parametrize("name", ["kappa_F", "kappa_targeted_F"])
def test_kappa_matters(name):
    """The same draw at confidence 0 ends elsewhere: another success set, or a best_dist further off than the GPU test's bound."""
    c = E.CASES[name]
    assert c["kw"]["confidence"] == E.KAPPA > 0 and c["B"] == 16 and c["kw"]["max_iterations"] == 10
    x, labels, out = _run(name)
    x0, labels0, zero = _run(name, confidence=0.0)
    assert np.array_equal(x, x0) and (labels is None or np.array_equal(labels, labels0))
    ok, ok0 = out["best_class"] != -1, zero["best_class"] != -1
    both = ok & ok0
    rel = np.abs(out["best_dist"][both] - zero["best_dist"][both]) / zero["best_dist"][both]
    print("%s: %d / %d succeed with / without kappa; best_dist moves by up to %.3f relative (bound %g)" %
          (name, ok.sum(), ok0.sum(), rel.max() if both.any() else np.nan, DIST_RTOL))
    assert not np.array_equal(ok, ok0) or rel.max() > DIST_RTOL
    assert (rel > DIST_RTOL).sum() >= 4                              # not one image alone
    if name == "kappa_F":                                           # both sides of the success rule's t == 0 branch
        assert labels is None and (out["labels"] == 0).any() and (out["labels"] != 0).any()
    else:
        assert E.CASES[name]["targeted"] and len(set(labels.tolist())) >= 4
    # a success under kappa holds the label's logit kappa clear of the rest: the margin kappa adds is used
    assert np.nanmin(out["success_margin"]) >= E.MIN_MARGIN


def test_kappa_reaches_the_abort_check(monkeypatch):
    """kappa_F and kappa_targeted_F run with abort_early off, where the iterate's hinge (loss1_X) feeds nothing that is returned.
    kappa_abort_F turns the check on: the chunks stop at other iterations at confidence 0, and also when kappa is dropped or
    negated in loss1_X ALONE, the seed and the success rule left right."""
    from tests.support import cw_reference as CW
    c = E.CASES["kappa_abort_F"]
    assert c["kw"]["confidence"] == E.KAPPA and c["kw"]["abort_early"] and c["kw"]["max_iterations"] == 10 and c["B"] == 32
    out = _run("kappa_abort_F")[2]
    zero = _run("kappa_abort_F", confidence=0.0)[2]
    stops = out["abort_iters"][0]
    assert None not in stops and all(s >= 1 for s in stops)
    assert zero["abort_iters"] != out["abort_iters"]
    ok = out["best_class"] != -1
    assert ok.any() and (~ok).any()                                 # and kappa decides who succeeds at all
    in_slack, slack_gradient, loss1_and_seed = [False], E.slack_gradient, CW.loss1_and_seed

    def slack(*a, **k):
        in_slack[0] = True
        try:
            return slack_gradient(*a, **k)
        finally:
            in_slack[0] = False
    got = {}
    for factor in (0.0, -1.0):
        monkeypatch.setattr(E, "slack_gradient", slack)
        monkeypatch.setattr(CW, "loss1_and_seed", lambda Z, t, const, confidence, targeted, f=factor:
                            loss1_and_seed(Z, t, const, confidence if in_slack[0] else f * confidence, targeted))
        layers, params = E.case_model("kappa_abort_F")
        got[factor] = E.run_case(c, E.SEEDS["kappa_abort_F"], layers, params)[2]["abort_iters"]
        monkeypatch.undo()
    print("kappa_abort_F: stops %s; at confidence 0 %s; with loss1_X's kappa dropped %s, negated %s" %
          (stops, zero["abort_iters"][0], got[0.0][0], got[-1.0][0]))
    assert got[0.0] != out["abort_iters"] and got[-1.0] != out["abort_iters"]


def test_huge_chunk_reaches_the_second_trip_of_the_chunk_kernel():
    c = E.CASES["huge_chunk_tiny"]
    assert c["B"] == 300 and c["kw"]["batch_size"] == 272 and c["kw"]["abort_early"] and c["kw"]["max_iterations"] == 10
    assert c["model"] == "tiny3" and E.case_model("huge_chunk_tiny")[1][-1][0].shape == (16, 3)
    out = _run("huge_chunk_tiny")[2]
    late = out["best_class"][256:272]                               # in-chunk indices 256 .. 271 of chunk 0: the loop's second trip
    print("huge_chunk_tiny: %d of the 16 images past in-chunk index 255 succeed; stops %s" % ((late != -1).sum(), out["abort_iters"]))
    assert (late != -1).any()
    assert len(out["abort_iters"]) == 1 and len(out["abort_iters"][0]) == 2
    assert None not in out["abort_iters"][0]                        # both chunks record a stop, as wide_F's do
    assert (out["best_class"][272:] != -1).any()                    # and the trailing partial chunk does something


def test_abort_every_iteration():
    c = E.CASES["abort_every_F"]
    assert c["kw"]["max_iterations"] == 6 and c["kw"]["abort_early"] and c["B"] == 32 and c["kw"]["batch_size"] == 16
    assert (c["kw"]["max_iterations"] // 10 or 1) == 1              # every iteration is a check, iteration 0 included
    out = _run("abort_every_F")[2]
    stops = out["abort_iters"][0]
    print("abort_every_F: stops %s" % (stops,))
    assert any(s is not None and s >= 1 for s in stops)


def test_given_labels_differ_from_the_models_own():
    x, labels, out = _run("given_y_F")
    import torch
    from tests.support import cw_reference as CW
    layers, params = E.case_model("given_y_F")
    with torch.no_grad():                                           # the labels a call without y would take
        own = CW.own_label(CW.logits(layers, E.params64(params), torch.as_tensor(x.astype(np.float64))).numpy())
    share = float((labels != own).mean())
    print("given_y_F: the given labels differ from the model's own on %.2f of the images" % share)
    assert not E.CASES["given_y_F"].get("targeted") and np.array_equal(out["labels"], labels)
    assert 0.25 <= share <= 0.75
    # a label the model does not predict is a success before anything moves: distance 0 exactly, there and nowhere else
    assert np.array_equal(out["best_dist"] == 0, labels != own) and (out["best_class"] != -1).all()


def test_beta_zero_and_two_classes():
    c = E.CASES["beta0_F"]
    assert c["kw"]["beta"] == 0.0
    out = _run("beta0_F")[2]
    assert out["near_threshold"] <= 1e-4 and (out["best_class"] != -1).mean() >= 0.25
    moved = ~out["kept"][out["best_class"] != -1]
    print("beta0_F: %.4f of the successful images' pixels moved" % moved.mean())
    assert moved.mean() > 0.9                                       # nothing is shrunk back to x0: the middle branch is d == 0 alone
    t = E.CASES["two_class_tiny"]
    assert t["model"] == "tiny2" and t["B"] == 16 and t["kw"]["max_iterations"] == 5
    assert E.case_model("two_class_tiny")[1][-1][0].shape == (16, 2)
    two = _run("two_class_tiny")[2]
    assert set(two["labels"].tolist()) == {0, 1} and set(two["best_class"].tolist()) <= {-1, 0, 1}
