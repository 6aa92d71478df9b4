"""Carlini-Wagner L2 (whitebox --attack_type cw) without a GPU: the CPU restatement's loss gradient, TF Adam, abort-check
schedule and constant search against hand-computed answers; the C entries and the Python surface reject what they must."""
import ctypes as C

import numpy as np
import pytest
import torch

from defensegan_amd import _native
from defensegan_amd import network_builder as nb
from tests.support import cw_reference as R


def _tiny_model_params(rs, tie=False):
    """Conv2D(3, 3x3, stride 2, SAME) + ReLU, Flatten, Linear(5) on 7x6x2 inputs; with ``tie`` classes 1 and 3 share a column."""
    layers = [("conv", 3, (3, 3), (2, 2), "SAME"), ("relu",), ("flatten",), ("linear", 5), ("softmax",)]
    K = rs.standard_normal((3, 3, 2, 3))
    b = rs.standard_normal(3) * 0.1
    W = rs.standard_normal((4 * 3 * 3, 5))
    if tie:
        W[:, 3] = W[:, 1]
    return layers, [(K, b), (W, np.zeros(5))]


def test_seed_matches_finite_differences_with_a_tie_in_oth():
    """dloss1/dZ by the TF rules equals central differences in logit space; at a tie the max's share is split evenly."""
    Z = torch.tensor([[0.3, 1.2, -0.4, 1.2, 0.1], [2.0, 0.5, 0.7, -1.0, 0.2]], dtype=torch.float64)
    t = np.array([0, 2])
    for targeted in (False, True):
        conf = 2.5 if not targeted else 0.4
        _, seed = R.loss1_and_seed(Z, t, [3.0, 0.5], conf, targeted)
        fd = torch.zeros_like(Z)
        h = 1e-6
        for b in range(2):
            for k in range(5):
                zp, zm = Z.clone(), Z.clone()
                zp[b, k] += h
                zm[b, k] -= h
                fd[b, k] = (R.loss1_and_seed(zp, t, [3.0, 0.5], conf, targeted)[0][b]
                            - R.loss1_and_seed(zm, t, [3.0, 0.5], conf, targeted)[0][b]) / (2 * h)
        np.testing.assert_allclose(seed.numpy(), fd.numpy(), atol=1e-6)
    _, seed = R.loss1_and_seed(Z, t, [3.0, 0.5], 2.5, False)
    assert seed[0, 1] == seed[0, 3] == -1.5 and seed[0, 0] == 3.0          # the tie: half each, the label none of it


def test_seed_is_zero_where_the_hinge_is_not_positive():
    Z = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64)
    loss1, seed = R.loss1_and_seed(Z, np.array([0]), [2.0], -1.0, False)       # real - oth + k = 0: TF's tie goes to the 0
    assert float(loss1[0]) == 0.0 and not seed.any()


@pytest.mark.parametrize("tie", [False, True])
def test_total_gradient_through_tanh_matches_finite_differences(tie):
    rs = np.random.RandomState(7 + tie)
    layers, params = _tiny_model_params(rs, tie)
    lo, hi = -1.0, 2.0
    x = torch.as_tensor(rs.uniform(lo, hi, (2, 7, 6, 2)))
    u = torch.clamp((x - lo) / (hi - lo), 0, 1)
    timg = torch.atanh((u * 2 - 1) * 0.999999)
    other = R.to_img(torch.tanh(timg), lo, hi)
    w = torch.as_tensor(rs.standard_normal(x.shape) * 0.3)
    t, const = np.array([0, 2]), np.array([5.0, 7.0])
    _, _, _, _, g = R.step_values(layers, params, w, timg, other, t, const, 10.0, False, lo, hi)
    h = 1e-6
    idx = [(0, 0, 0, 0), (0, 3, 2, 1), (1, 6, 5, 0), (1, 2, 4, 1), (0, 5, 1, 1)]
    for i in idx:
        wp, wm = w.clone(), w.clone()
        wp[i] += h
        wm[i] -= h
        fd = (R.total_loss(layers, params, wp, timg, other, t, const, 10.0, False, lo, hi)
              - R.total_loss(layers, params, wm, timg, other, t, const, 10.0, False, lo, hi)) / (2 * h)
        assert abs(float(g[i]) - fd) <= 1e-5 * max(1.0, abs(fd)), (i, float(g[i]), fd)


def test_tf_adam_first_three_steps():
    lr, w, m, v = 0.5, 1.0, 0.0, 0.0
    grads = [2.0, -1.0, 4.0]
    # by hand: m1 = .2, v1 = .004, lr_t1 = .5*sqrt(.001)/.1; m2 = .18 - .1 = .08, v2 = .003996 + .001 = .004996; ...
    m1, v1 = 0.2, 0.004
    w1 = 1.0 - 0.5 * np.sqrt(1 - 0.999) / (1 - 0.9) * m1 / (np.sqrt(v1) + 1e-8)
    m2, v2 = 0.9 * m1 - 0.1, 0.999 * v1 + 0.001
    w2 = w1 - 0.5 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2) * m2 / (np.sqrt(v2) + 1e-8)
    m3, v3 = 0.9 * m2 + 0.4, 0.999 * v2 + 0.016
    w3 = w2 - 0.5 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3) * m3 / (np.sqrt(v3) + 1e-8)
    assert abs(w1 - (1.0 - 0.5)) < 1e-6                         # the first step is lr * sign(g)
    for step, (g, want) in enumerate(zip(grads, [(w1, m1, v1), (w2, m2, v2), (w3, m3, v3)]), start=1):
        w, m, v = R.adam_step(w, m, v, g, lr, step)
        np.testing.assert_allclose([w, m, v], want, rtol=1e-12, atol=1e-15)


def test_abort_check_schedule():
    assert R.abort_check_iterations(100) == list(range(0, 100, 10))
    assert R.abort_check_iterations(1000) == list(range(0, 1000, 100))
    for n in range(1, 10):
        assert R.abort_check_iterations(n) == list(range(n))
    assert R.abort_check_iterations(25) == list(range(0, 25, 2))


def test_const_update_known_answers_over_four_outer_steps():
    t = np.array([3, 3, 3])
    const, lower, upper = np.full(3, 0.01), np.zeros(3), np.full(3, 1e10)
    # image 0 always succeeds, image 1 never, image 2 fails twice then succeeds
    scores = [[5, -1, -1], [5, -1, 3], [5, 3, 7], [5, 3, 7]]
    want = [[0.005, 0.1, 0.1], [0.0025, 1.0, 1.0], [0.00125, 10.0, 0.55], [0.000625, 100.0, 0.325]]
    for s, w in zip(scores, want):
        const, lower, upper = R.const_update(np.array(s), t, const, lower, upper, targeted=False)
        np.testing.assert_allclose(const, w, rtol=1e-12)
    np.testing.assert_allclose(upper, [0.00125, 1e10, 0.55])
    np.testing.assert_allclose(lower, [0.0, 10.0, 0.1])
    # targeted: success means the score IS the label
    c, lo_, up = R.const_update(np.array([3, 5]), np.array([3, 3]), [1.0, 1.0], [0.0, 0.0], [1e10, 1e10], targeted=True)
    np.testing.assert_allclose(c, [0.5, 10.0])


def test_repeat_sets_the_last_step_to_the_upper_bound():
    """binary_search_steps >= 10: the last outer step runs at const = upper_bound (1e10 for an image that never succeeded)."""
    layers, params = _tiny_model_params(np.random.RandomState(3))
    x = np.random.RandomState(4).uniform(0, 1, (2, 7, 6, 2))
    seen = []
    orig = R.loss1_and_seed

    def spy(Z, t, const, confidence, targeted):
        seen.append(np.array(const, np.float64).copy())
        return orig(Z, t, const, confidence, targeted)
    R.loss1_and_seed = spy
    try:
        R.cw_l2(layers, params, x, labels=np.array([0, 1]), batch_size=2, binary_search_steps=10, max_iterations=1, abort_early=False,
                confidence=1e6, initial_const=1.0)                  # confidence 1e6: nothing ever succeeds
    finally:
        R.loss1_and_seed = orig
    assert [float(c[0]) for c in seen] == [10.0 ** k for k in range(9)] + [1e10]


def test_native_entries_reject_a_null_handle_without_a_gpu():
    lib = _native.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dg_clf_backward(None, p, p, 1, p, None) == -1
    assert lib.dg_cw(None, p, None, 1, 0, 1, 0.0, 0.01, 1, 1, 1, 0.01, 0.0, 1.0, p, None, None, None, None, None) == -1
    assert b"dg_cw" in lib.dg_last_error()


def test_generate_on_a_defended_model_raises():
    m = nb.model_f()
    m.rec_layer = object()                                  # what add_rec_model installs; never entered
    with pytest.raises(NotImplementedError, match="ReconstructionLayer"):
        nb.CarliniWagnerL2(m).generate(np.zeros((1, 28, 28, 1), np.float32))
