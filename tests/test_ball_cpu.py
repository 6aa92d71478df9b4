"""-m "not gpu": the L1 / L2 attack definitions as restated in tests/support/ball_reference.py -- FGM ord 1 and 2, the L2 step, the
projected rand_init draw -- by hand, and the host side of ``ord``: argument checks, the BPDA driver loop for ord = 2 on CPU tensors
over stand-in operations, today's ``step`` signature for ord = inf, and the result names.  The device kernels are
tests/test_gpu_ball.py's."""
import argparse

import numpy as np
import pytest

from defensegan_amd import network_builder as nb, whitebox as wb
from tests.support import ball_reference as BR
from tests.test_bpda_cpu import _StandIn, _defended


# ---------------------------------------------------------------------- the definitions, by hand
def test_fgm_hand_computed_on_a_2x2x1_image():
    x = np.full((1, 2, 2, 1), 0.5)
    g = np.array([3.0, -4.0, 0.0, 0.0]).reshape(1, 2, 2, 1)
    # ord 1: sum|g| = 7, eps 0.7 -> 0.3, -0.4;   ord 2: ||g|| = 5, eps 0.5 -> 0.3, -0.4
    for ord, eps in ((1, 0.7), (2, 0.5)):
        np.testing.assert_allclose(BR.fgm(x, g, eps, ord, 0.0, 1.0).ravel(), [0.8, 0.1, 0.5, 0.5], rtol=0, atol=1e-15)
    # the range: eps 1 moves pixel 0 by 0.6 (ord 2) to 1.1 -> 1.0, pixel 1 by -0.8 to -0.3 -> 0.0
    np.testing.assert_allclose(BR.fgm(x, g, 1.0, 2, 0.0, 1.0).ravel(), [1.0, 0.0, 0.5, 0.5], rtol=0, atol=1e-15)
    # per image: a second image with another gradient keeps its own norm
    x2, g2 = np.concatenate([x, x]), np.concatenate([g, 2 * np.ones_like(g)])
    out = BR.fgm(x2, g2, 0.4, 1, 0.0, 1.0)
    np.testing.assert_allclose(out[0].ravel(), [0.5 + 0.4 * 3 / 7, 0.5 - 0.4 * 4 / 7, 0.5, 0.5], rtol=0, atol=1e-15)
    np.testing.assert_allclose(out[1].ravel(), [0.6] * 4, rtol=0, atol=1e-15)


def test_l2_step_inside_the_ball_projected_and_zero_gradient():
    x = np.full((1, 2, 2, 1), 0.5)
    g = np.array([3.0, -4.0, 0.0, 0.0]).reshape(1, 2, 2, 1)
    info = {}
    # from x itself: u = (0.6, -0.8), d = 0.05 u, ||d|| = 0.05 < eps: the step lands inside the ball and is kept
    out = BR.l2_step(x, x, g, eps=0.1, eps_iter=0.05, lo=0.0, hi=1.0, info=info)
    np.testing.assert_allclose(out.ravel(), [0.53, 0.46, 0.5, 0.5], rtol=0, atol=1e-15)
    assert info["projected"].tolist() == [False] and info["moved"][0] == pytest.approx(0.05, abs=1e-15)
    # from the ball's face, x + 0.1 u: d = 0.15 u is scaled back to 0.1 u
    xk = x + 0.1 * np.array([0.6, -0.8, 0.0, 0.0]).reshape(x.shape)
    out = BR.l2_step(x, xk, g, eps=0.1, eps_iter=0.05, lo=0.0, hi=1.0, info=info)
    np.testing.assert_allclose(out.ravel(), [0.56, 0.42, 0.5, 0.5], rtol=0, atol=1e-15)
    assert info["projected"].tolist() == [True] and info["moved"][0] == pytest.approx(0.15, abs=1e-15)
    # a zero gradient: a zero step, no NaN; the iterate is still projected onto the ball
    out = BR.l2_step(x, x, np.zeros_like(g), 0.1, 0.05, 0.0, 1.0)
    assert np.array_equal(out, x)
    far = x + np.array([0.3, 0.0, 0.0, -0.4]).reshape(x.shape)                     # ||.|| = 0.5
    np.testing.assert_allclose(BR.l2_step(x, far, np.zeros_like(g), 0.1, 0.05, 0.0, 1.0).ravel(), [0.56, 0.5, 0.5, 0.42], rtol=0, atol=1e-15)
    assert np.isfinite(BR.fgm(x, np.zeros_like(g), 0.3, 1, 0.0, 1.0)).all() and np.array_equal(BR.fgm(x, np.zeros_like(g), 0.3, 2, 0.0, 1.0), x)
    # eps = 0: nothing moves
    assert np.array_equal(BR.l2_step(x, x, g, 0.0, 0.05, 0.0, 1.0), x)


def test_eot_sum_enters_as_gsum_plus_g():
    x = np.full((1, 2, 2, 1), 0.5)
    gsum = np.array([1.0, 1.0, 0.0, 0.0]).reshape(x.shape)
    g = np.array([2.0, -5.0, 0.0, 0.0]).reshape(x.shape)
    a = BR.l2_step(x, x, g, 0.1, 0.05, 0.0, 1.0, gsum=gsum)
    assert np.array_equal(a, BR.l2_step(x, x, gsum + g, 0.1, 0.05, 0.0, 1.0))
    np.testing.assert_allclose(a.ravel(), [0.53, 0.46, 0.5, 0.5], rtol=0, atol=1e-15)
    # three samples: R.eot_sum's left-to-right order decides the direction when a small term is absorbed
    big, small = np.array([1e8, 0.0]).reshape(1, 2, 1, 1), np.array([1e-9, 0.0]).reshape(1, 2, 1, 1)            # small > TINY

    class Ops(object):
        def __init__(self, gs):
            self.gs = list(gs)

        def project(self, x_k, seed):
            return x_k

        def gradient(self, rec):
            return self.gs.pop(0)

        def predict(self, rec):
            return np.zeros(1, int)
    x1 = np.full((1, 2, 1, 1), 0.5)
    absorbed = BR.attack_l2(Ops([big, small, -big]), x1, [0], 0.1, 0.05, 1, 3, 0.0, 1.0, 0)
    kept = BR.attack_l2(Ops([big, -big, small]), x1, [0], 0.1, 0.05, 1, 3, 0.0, 1.0, 0)
    assert np.array_equal(absorbed["iterates"][1], x1)                             # (1e8 + 1e-9) - 1e8 = 0: no step
    np.testing.assert_allclose(kept["iterates"][1].ravel(), [0.55, 0.5], rtol=0, atol=1e-15)


def test_projected_rand_init_draw():
    noise = nb.bpda_rand_noise(3, 784, 0.3, seed=5)
    assert BR.row_norms(noise, 2).min() > 2.0                                       # the cube's draw lies far outside the ball
    got = nb.ball_project_noise(noise, 0.3)
    assert got.dtype == np.float32 and got.shape == noise.shape
    np.testing.assert_allclose(got, BR.project_noise(noise, 0.3), rtol=2e-7, atol=0)
    np.testing.assert_allclose(BR.row_norms(got, 2), 0.3, rtol=1e-6)
    inside = (noise * np.float32(0.001)).astype(np.float32)                                             # inside the ball already: unchanged
    assert nb.ball_project_noise(inside, 0.3).tobytes() == inside.tobytes()
    assert np.array_equal(nb.ball_project_noise(np.zeros((2, 8), np.float32), 0.3), np.zeros((2, 8), np.float32))


# ---------------------------------------------------------------------- argument checks
def test_ord_is_checked_before_anything_else():
    x, y = np.zeros((2, 28, 28, 1), np.float32), np.zeros(2, np.int32)
    for atk in (nb.ProjectedGradientDescent(nb.model_e()), nb.BPDA(_defended())):
        with pytest.raises(NotImplementedError, match="needs a sort"):
            atk.generate(x, y, ord=1)
        for bad in (3, 0, "two", 2.5, -np.inf):
            with pytest.raises(ValueError, match="ord must be one of np.inf, 2"):
                atk.generate(x, y, ord=bad)
    with pytest.raises(ValueError, match="ord must be one of np.inf, 1, 2"):
        nb.FastGradientMethod(nb.model_e()).generate(x, ord=3)
    assert nb._attack_ord("inf", (np.inf, 2), "t") == np.inf and nb._attack_ord(float("inf"), (np.inf,), "t") == np.inf
    assert nb._attack_ord(2.0, (np.inf, 2), "t") == 2 and nb._attack_ord("1", (np.inf, 1, 2), "t") == 1
    # ord = 2 keeps the other refusals
    with pytest.raises(ValueError, match="PGD-on-bare"):
        nb.BPDA(nb.model_e()).generate(x, y, ord=2)
    with pytest.raises(ValueError, match="nb_iter"):
        nb.BPDA(_defended()).generate(x, y, ord=2, nb_iter=0)


def test_whitebox_attack_ord_checks():
    data = (np.zeros((2, 2, 2, 1), np.float32), np.zeros(2, int), np.zeros((2, 2, 2, 1), np.float32), np.zeros(2, int))
    with pytest.raises(ValueError, match="not with same_init"):                    # as today, whatever the ord
        wb.whitebox(object(), None, data, attack_type="bpda", defense_type="defense_gan", same_init=True, attack_ord=2)
    with pytest.raises(NotImplementedError, match="needs a sort"):
        wb.whitebox(None, None, data, attack_type="pgd", attack_ord=1)
    with pytest.raises(NotImplementedError, match="needs a sort"):
        wb.whitebox(object(), None, data, attack_type="bpda", defense_type="defense_gan", attack_ord="1")
    with pytest.raises(ValueError, match="attack_type cw: ord must be one of np.inf"):
        wb.whitebox(None, None, data, attack_type="cw", attack_ord=2)
    with pytest.raises(ValueError, match="ord must be one of"):
        wb.whitebox(None, None, data, attack_type="fgsm", attack_ord=3)
    assert wb.attack_ord_value("2", "pgd") == 2 and wb.attack_ord_value(1, "fgsm") == 1 and wb.attack_ord_value("inf", "cw") == np.inf
    ap = wb.build_parser()
    assert ap.parse_args(["--data_dir", "d"]).attack_ord == "inf"
    assert ap.parse_args(["--data_dir", "d", "--attack_ord", "2"]).attack_ord == "2"
    with pytest.raises(SystemExit):
        ap.parse_args(["--data_dir", "d", "--attack_ord", "3"])


# ---------------------------------------------------------------------- the driver loop
class _BallStandIn(_StandIn):
    """tests/test_bpda_cpu.py's stand-in operations plus the two of ord = 2, by the restatement in float64."""

    def __init__(self, preds, R_):
        super().__init__(preds, R_)
        self.ball_calls, self.sign_calls = [], 0

    def step(self, *a):
        self.sign_calls += 1
        return super().step(*a)

    def step_ball(self, rec, labels, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, ord, lo, hi, x_next):
        import torch
        self.ball_calls.append((bool(accumulate_only), ord, gsum is not None))
        g = self.field(rec.numpy().astype(np.float64))
        if accumulate_only:
            gsum += torch.from_numpy(g.astype(np.float32))
            return
        out = BR.l2_step(x_orig.numpy(), x_cur.numpy(), g, eps, eps_iter, lo, hi, gsum=None if gsum is None else gsum.numpy())
        x_next.copy_(torch.from_numpy(out.astype(np.float32)))

    def dist(self, x_adv, x_orig):
        import torch
        return torch.from_numpy(BR.row_norms(x_adv.numpy(), 2, x_orig.numpy()).astype(np.float32))


def _loop_case():
    rs = np.random.RandomState(1)
    x = (rs.randint(8, 56, (5, 28, 28, 1)) / 64.0).astype(np.float32)
    preds = {1: np.array([1, 0, 3, 4, 5]), 2: np.array([0, 2, 3, 4, 5]), 3: np.array([1, 2, 3, 0, 5])}
    return x, np.array([1, 2, 3, 4, 5], np.int32), preds


def _judging(ops, seed, m_eot):
    def predict(rec, _p=ops.predict):
        ops.judged = (ops.log[-1][0] - seed) // m_eot
        return _p(rec)
    ops.predict = predict
    return ops


@pytest.mark.parametrize("m_eot,batch_size", [(1, None), (3, None), (2, 2)])
def test_driver_loop_for_ord_2_over_stand_in_operations(m_eot, batch_size, monkeypatch):
    """BPDA.generate(ord=2) on CPU tensors: the projections and seeds of ord = inf, every step through ``step_ball`` (the samples
    before the last accumulate), a third return value ``dist``, and the result against the restatement over the same stand-ins."""
    from defensegan_amd import gan_defense
    monkeypatch.setattr(gan_defense, "COALESCE_ROWS", 1)
    x, y, preds = _loop_case()
    n, nb_iter, R_, seed, eps, eps_iter = 5, 3, 2, 900, 0.875, 0.75
    ops = _judging(_BallStandIn(preds, R_), seed, m_eot)
    adv, first, dist = nb.BPDA(_defended(R_, batch_size=50), ops=ops).generate(
        x, y, eps=eps, eps_iter=eps_iter, nb_iter=nb_iter, eot_samples=m_eot, clip_min=0.0, clip_max=1.0, seed=seed, batch_size=batch_size,
        return_info=True, ord=2)
    cuts = 1 if batch_size is None else -(-n // batch_size)
    assert ops.sign_calls == 0 and len(ops.ball_calls) == nb_iter * m_eot * cuts
    assert ops.ball_calls[:m_eot * cuts] == [(s < m_eot - 1, 2, m_eot > 1) for s in range(m_eot) for _ in range(cuts)]
    assert [e[0] for e in ops.log] == [seed + k * m_eot + s for k in range(nb_iter) for s in range(m_eot) for _ in range(cuts)] + \
        [seed + nb_iter * m_eot] * cuts

    class RefOps(object):
        def project(self, x_k, s):
            self.judged = (s - seed) // m_eot
            return x_k

        def gradient(self, rec):
            return _StandIn.field(rec)

        def predict(self, rec):
            return preds[self.judged]
    ref = BR.attack_l2(RefOps(), x, y, eps, eps_iter, nb_iter, m_eot, 0.0, 1.0, seed)
    # the field turns with the iterate, so the steps add up like a random walk: 0.75, then about 0.75 sqrt(2) > eps
    assert not ref["projected"][0].any() and ref["projected"][1].all() and ref["projected"][2].all()
    assert first.tolist() == ref["first_success"].tolist() == [2, 1, -1, 3, -1]
    np.testing.assert_allclose(adv, ref["x_adv"], rtol=0, atol=1e-6)
    assert adv.dtype == np.float32 and dist.dtype == np.float32 and dist.shape == (n,)
    np.testing.assert_allclose(dist, BR.row_norms(adv, 2, x), rtol=1e-6)
    assert dist.max() <= eps * (1 + 1e-6) and adv.min() >= 0 and adv.max() <= 1


def test_ord_inf_calls_step_with_todays_signature_and_returns_two_values(monkeypatch):
    """A stand-in without ``step_ball`` / ``dist`` and with a ``step`` of exactly today's eleven positional parameters serves
    ord = np.inf, given or not: the same bits, (x_adv, first_success) from return_info."""
    x, y, preds = _loop_case()
    kw = dict(eps=0.125, eps_iter=0.0625, nb_iter=3, clip_min=0.0, clip_max=1.0, seed=900, return_info=True)
    runs = []
    for extra in ({}, {"ord": np.inf}, {"ord": "inf"}):
        ops = _judging(_StandIn(preds, 2), 900, 1)
        assert not hasattr(ops, "step_ball") and not hasattr(ops, "dist")
        out = nb.BPDA(_defended(2, batch_size=50), ops=ops).generate(x, y, **dict(kw, **extra))
        assert len(out) == 2
        runs.append(out)
    for adv, first in runs[1:]:
        assert adv.tobytes() == runs[0][0].tobytes() and first.tolist() == runs[0][1].tolist() == [2, 1, -1, 3, -1]
    # rand_init with ord = 2 starts inside the L2 ball: one iteration of step 0 and eps_iter 0 returns x_0 itself
    ops = _judging(_BallStandIn({1: y.copy()}, 2), 7, 1)
    x0, _, dist = nb.BPDA(_defended(2, batch_size=50), ops=ops).generate(x, y, eps=0.5, eps_iter=0.0, nb_iter=1, seed=7, rand_init=True,
                                                                         return_info=True, ord=2)
    want = x + nb.ball_project_noise(nb.bpda_rand_noise(5, 784, 0.5, 7), 0.5).reshape(x.shape)
    np.testing.assert_allclose(x0, want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(dist, 0.5, rtol=1e-5)


# ---------------------------------------------------------------------- result names
def test_result_names_with_and_without_attack_ord():
    base = dict(defense_type="none", dataset_name="mnist", rec_path=None, train_on_recs=False, num_tests=-1, num_train=-1, model="F",
                fgsm_eps_tr=0.15)
    name = lambda **kw: wb.get_results_dir_filename(argparse.Namespace(**dict(base, **kw)), None)[1]
    assert name(attack_type="pgd") == "model=F_nodefense_attack=pgd.txt"                      # a namespace without the flag: as before
    assert name(attack_type="pgd", attack_ord="inf") == name(attack_type="pgd", attack_ord=np.inf) == "model=F_nodefense_attack=pgd.txt"
    assert name(attack_type="pgd", attack_ord="2") == name(attack_type="pgd", attack_ord=2) == "model=F_nodefense_attack=pgd_ord=2.txt"
    assert name(attack_type="fgsm", attack_ord="1", defense_type="adv_tr") == "model=F_advTrEps=0.15attack=fgsm_ord=1.txt"
    assert name(attack_type="bpda", attack_ord=2, num_tests=8) == "model=F_numtest=8_nodefense_attack=bpda_ord=2.txt"
