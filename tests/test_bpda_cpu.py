"""-m "not gpu": the BPDA/EOT definition as restated in tests/support/bpda_reference.py -- step rule, EOT sum order, seed
schedule, best tracking, the rand_init draw -- and the host side of network_builder.BPDA: argument checks, the Philox draw, and
the driver loop itself run on CPU tensors over stand-in operations (which projections it asks for, in which order, and what it
tracks).  The device kernels are tests/test_gpu_bpda.py's."""
import numpy as np
import pytest

from defensegan_amd import network_builder as nb
from tests.support import bpda_reference as R


# ---------------------------------------------------------------------- the step rule, by hand
def test_step_rule_hand_computed_cases():
    x = np.array([0.50, 0.50, 0.50, 0.95, 0.02, 0.50])
    xk = np.array([0.50, 0.58, 0.50, 0.99, 0.00, 0.45])
    g = np.array([2.0, 3.0, 0.0, 1.0, -1.0, -0.5])
    out = R.step_rule(x, xk, g, eps=0.1, eps_iter=0.05, lo=0.0, hi=1.0)
    #                  +step   ball face  sign(0)=0   range     range     -step
    np.testing.assert_allclose(out, [0.55, 0.60, 0.50, 1.00, 0.00, 0.40], rtol=0, atol=1e-15)
    # sign(0) = 0: the iterate does not move, but is still projected onto the ball
    assert R.step_rule(np.array([0.5]), np.array([0.9]), np.array([0.0]), 0.1, 0.05, 0.0, 1.0)[0] == pytest.approx(0.6, abs=1e-15)
    # eps_iter > eps: one step lands on the ball's face
    out = R.step_rule(np.full(4, 0.5), np.full(4, 0.5), np.array([1.0, -1.0, 1e-30, -1e-30]), eps=0.1, eps_iter=0.25, lo=0.0, hi=1.0)
    np.testing.assert_allclose(out, [0.6, 0.4, 0.6, 0.4], rtol=0, atol=1e-15)


def test_step_rule_stays_in_ball_and_range():
    rs = np.random.RandomState(0)
    x = rs.uniform(-1, 1, 4000)
    for eps, eps_iter, lo, hi in ((0.3, 0.05, -1.0, 1.0), (0.1, 0.5, 0.0, 1.0), (0.0, 0.1, -1.0, 1.0)):
        xk = np.clip(x + rs.uniform(-eps, eps, x.shape), lo, hi)
        out = R.step_rule(x, xk, rs.standard_normal(x.shape), eps, eps_iter, lo, hi)
        assert out.min() >= lo and out.max() <= hi
        inside = (x >= lo) & (x <= hi)
        assert np.abs(out - x)[inside].max() <= eps + 1e-15


def test_eot_sum_is_a_left_to_right_sum_not_a_mean():
    a, b, c = np.array([1.0]), np.array([1e-16]), np.array([-1.0])
    assert R.eot_sum([a, b, c])[0] == (1.0 + 1e-16) - 1.0 == 0.0          # left to right: the small term is absorbed first
    assert R.eot_sum([a, c, b])[0] == 1e-16
    g = np.array([0.25, -3.0])
    assert np.array_equal(R.eot_sum([g]), g) and np.array_equal(R.eot_sum([g, g, g, g]), 4 * g)


def test_seed_schedule():
    sched, final = R.seed_schedule(100, nb_iter=3, m=4)
    assert sched == [[100, 101, 102, 103], [104, 105, 106, 107], [108, 109, 110, 111]] and final == 112
    assert R.seed_schedule(7, 2, 1) == ([[7], [8]], 9)
    for seed, k, m in ((100, 3, 4), (7, 2, 1), (0, 1, 1), (2 ** 40, 5, 3)):
        assert nb.bpda_seed_schedule(seed, k, m) == R.seed_schedule(seed, k, m)


# ---------------------------------------------------------------------- best tracking on a stubbed prediction sequence
def test_tracking_keeps_the_first_success():
    labels = np.array([3, 3, 3, 3])
    iterates = [np.full((4, 2), float(j)) for j in range(4)]              # x_0 .. x_3
    preds = {1: np.array([3, 5, 3, 3]),                                   # image 1 succeeds at iterate 1
             2: np.array([4, 3, 3, 3]),                                   # image 0 at 2; image 1 "fails" again: not undone
             3: np.array([3, 3, 3, 9])}                                   # image 3 at the last iterate; image 2 never
    x_adv, first = R.track(preds, labels, iterates)
    assert first.tolist() == [2, 1, -1, 3] and first.dtype == np.int32
    assert x_adv[:, 0].tolist() == [2.0, 1.0, 3.0, 3.0]                   # no success: the last iterate


# ---------------------------------------------------------------------- the rand_init draw
def test_philox_known_answers():
    out = R.philox4x32_10(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], np.uint64), (0, 0))
    assert [hex(int(v)) for v in out[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    out = R.philox4x32_10(np.array([[0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint64), (0xA4093822, 0x299F31D0))
    assert [hex(int(v)) for v in out[0]] == ["0xd16cfe09", "0x94fdcceb", "0x5001e420", "0x24126ea1"]


@pytest.mark.parametrize("n,P,first", [(3, 784, 0), (2, 25, 5), (1, 7, 2 ** 33)])
def test_rand_init_draw_is_its_numpy_restatement(n, P, first):
    got = nb.bpda_rand_noise(n, P, 0.3, seed=(11 << 32) | 7, first_image=first)
    want = R.rand_noise(n, P, 0.3, seed=(11 << 32) | 7, first_image=first)
    assert got.dtype == np.float32 and got.shape == (n, P) and got.tobytes() == want.tobytes()
    assert got.min() >= -np.float32(0.3) and got.max() < np.float32(0.3)
    if n > 1:
        assert not np.array_equal(got[0], got[1])
        # keyed by the global image index: any batching gives the same rows
        assert nb.bpda_rand_noise(1, P, 0.3, seed=(11 << 32) | 7, first_image=first + 1).tobytes() == got[1].tobytes()


def test_rand_init_draw_is_uniform_enough():
    u = nb.bpda_rand_noise(50, 784, 1.0, seed=3).ravel()
    assert abs(u.mean()) < 0.02 and abs(u.std() - 1 / np.sqrt(3)) < 0.01


# ---------------------------------------------------------------------- the host class
def _defended(R_=2, batch_size=50, use_bn=False, shape=(None, 28, 28, 1)):
    from defensegan_amd.gan import MnistDefenseGAN
    gan = MnistDefenseGAN(cfg={"USE_BN": use_bn, "LATENT_DIM": 128, "NET_DIM": 64}, test_mode=True, rec_rr=R_, rec_iters=5, rec_lr=10.0)
    m = nb.model_e(input_shape=shape)
    m.add_rec_model(gan, None, batch_size)
    return m


def test_argument_checks():
    x, y = np.zeros((2, 28, 28, 1), np.float32), np.zeros(2, np.int32)
    with pytest.raises(ValueError, match="PGD-on-bare"):
        nb.BPDA(nb.model_e()).generate(x, y)
    m = _defended()
    with pytest.raises(ValueError, match="nb_iter"):
        nb.BPDA(m).generate(x, y, nb_iter=0)
    with pytest.raises(ValueError, match="eot_samples"):
        nb.BPDA(m).generate(x, y, eot_samples=0)
    with pytest.raises(ValueError, match="eps"):
        nb.BPDA(m).generate(x, y, eps=-0.1)
    with pytest.raises(ValueError, match="not both"):
        nb.BPDA(m).generate(x, y, rand_init=True, x_init=x)
    m.rec_layer.z_init = np.zeros((4, 128), np.float32)
    with pytest.raises(ValueError, match="z_init"):
        nb.BPDA(m).generate(x, y)


def test_notes_point_at_bpda():
    assert "BPDA" in nb._CW_REC_NOTE and "BPDA" in nb._REC_GRADIENT_NOTE


class _StandIn(object):
    """The four operations of BpdaDeviceOps on CPU tensors: an identity 'projection' that records what it was asked for,
    a fixed gradient field, predictions read off a prescribed sequence, and step / track by the definition."""

    def __init__(self, preds_of_iterate, R_):
        import torch
        self.device, self.preds, self.R, self.log, self.judged = torch.device("cpu"), preds_of_iterate, R_, [], None

    @staticmethod
    def field(rec):
        return np.sin(37.0 * rec + 0.25)              # a gradient with both signs; never exactly 0 on the grid used below

    def project(self, x, seed, first_row):
        self.log.append((int(seed), int(first_row), int(x.shape[0])))
        self.cut = (int(first_row) // self.R, int(first_row) // self.R + int(x.shape[0]))
        return x.clone()

    def predict(self, rec):
        import torch
        return torch.from_numpy(np.asarray(self.preds[self.judged][self.cut[0]:self.cut[1]], np.int32))

    def step(self, rec, labels, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, lo, hi, x_next):
        import torch
        g = torch.from_numpy(self.field(rec.numpy().astype(np.float64)).astype(np.float32))
        if accumulate_only:
            gsum += g
            return
        t = g if gsum is None else gsum + g
        x_next.copy_(torch.clamp(x_orig + torch.clamp(x_cur + eps_iter * torch.sign(t) - x_orig, -eps, eps), lo, hi))

    def track(self, preds, labels, k, x_iter, x_best, first_success):
        open_ = first_success < 0
        x_best[open_] = x_iter[open_]
        first_success[open_ & (preds != labels)] = k


@pytest.mark.parametrize("m_eot,batch_size", [(1, None), (3, None), (2, 2)])
def test_driver_loop_over_stand_in_operations(m_eot, batch_size, monkeypatch):
    """network_builder.BPDA.generate on CPU tensors: the projections it asks for (seed + k m + s, then seed + nb_iter m; rows
    keyed by the global image), nb_iter m + 1 of them per cut, and its result against the restatement run over the same stand-ins."""
    from defensegan_amd import gan_defense
    monkeypatch.setattr(gan_defense, "COALESCE_ROWS", 1)          # one caller batch per engine call: batch_size really cuts
    n, nb_iter, R_, seed = 5, 3, 2, 900
    rs = np.random.RandomState(1)
    x = (rs.randint(8, 56, (n, 28, 28, 1)) / 64.0).astype(np.float32)       # on a grid: every step is exact in float32
    y = np.array([1, 2, 3, 4, 5], np.int32)
    preds = {1: np.array([1, 0, 3, 4, 5]), 2: np.array([0, 2, 3, 4, 5]), 3: np.array([1, 2, 3, 0, 5])}
    kw = dict(eps=0.125, eps_iter=0.0625, nb_iter=nb_iter, eot_samples=m_eot, clip_min=0.0, clip_max=1.0, seed=seed)

    ops = _StandIn(preds, R_)

    def predict(rec, _p=ops.predict):
        # the driver judges iterate k at iteration k's first projection and iterate nb_iter at the end: the seed says which
        s = ops.log[-1][0] - seed
        ops.judged = s // m_eot
        return _p(rec)
    ops.predict = predict
    m = _defended(R_, batch_size=50)
    adv, first = nb.BPDA(m, ops=ops).generate(x, y, batch_size=batch_size, return_info=True, **kw)

    cuts = [(0, n)] if batch_size is None else [(a, min(n, a + batch_size)) for a in range(0, n, batch_size)]
    want_log = [(seed + k * m_eot + s, a * R_, b - a) for k in range(nb_iter) for s in range(m_eot) for a, b in cuts]
    want_log += [(seed + nb_iter * m_eot, a * R_, b - a) for a, b in cuts]
    assert ops.log == want_log and len(ops.log) == (nb_iter * m_eot + 1) * len(cuts)

    class RefOps(object):
        def __init__(self):
            self.judged = None

        def project(self, x_k, s):
            self.judged = (s - seed) // m_eot
            return x_k

        def gradient(self, rec):
            return _StandIn.field(rec)

        def predict(self, rec):
            return preds[self.judged]
    ref = R.bpda(RefOps(), x, y, 0.125, 0.0625, nb_iter, m_eot, 0.0, 1.0, seed)
    assert ref["seeds"] == sorted(set(s for s, _, _ in want_log))
    assert first.tolist() == ref["first_success"].tolist() == [2, 1, -1, 3, -1]
    assert np.array_equal(adv.astype(np.float64), ref["x_adv"])
    assert adv.dtype == np.float32 and np.abs(adv - x).max() <= 0.125 and adv.min() >= 0 and adv.max() <= 1


def test_use_bn_generators_are_cut_on_batch_size_exactly():
    """Batchnorm couples the rows of an engine call: no coalescing, the caller's batch is the engine's."""
    n, R_ = 5, 2
    x = np.full((n, 28, 28, 1), 0.5, np.float32)
    ops = _StandIn({1: np.zeros(n, np.int32)}, R_)
    ops.judged = 1
    m = _defended(R_, use_bn=True)
    nb.BPDA(m, ops=ops).generate(x, np.zeros(n, np.int32), nb_iter=1, batch_size=2, clip_min=0.0, clip_max=1.0, seed=5)
    assert ops.log == [(5, 0, 2), (5, 4, 2), (5, 8, 1), (6, 0, 2), (6, 4, 2), (6, 8, 1)]


# ---------------------------------------------------------------------- what the GPU case's choice of seed promises
def test_gpu_case_has_few_undecided_pixels_on_the_reference_alone():
    """tests/test_gpu_bpda.py compares x_{k+1} on the decided pixels, |g| > 1e-4 max|g|, and needs the undecided ones to be at most
    2 % of all: the case (R.CASE) is chosen so that the float64 reference satisfies this at every teacher-forced iterate, for
    m = 1 and m = 3 -- here with latents drawn by NumPy (the device draws its own for the same seeds and asserts it again)."""
    c = R.CASE
    p, x, y, model, cp = R.case_inputs()
    assert x.shape == (c["B"], 28, 28, 1) and x.min() >= 0 and x.max() <= 1
    for m_eot in (1, 3):
        sched, final = R.seed_schedule(c["seed"], 3, m_eot)
        z0 = R.host_z0_blocks([s for row in sched for s in row] + [final], c["B"] * c["R"], 128)
        ops = R.oracle_ops(p, c["arch"], R.layers_of(model), cp, y, z0, c["R"], c["L"], c["lr"])
        out = R.bpda(ops, x, y, c["eps"], c["eps_iter"], 3, m_eot, c["lo"], c["hi"], c["seed"])
        for g in out["grads"]:
            assert R.undecided_fraction(g) <= 0.02, R.undecided_fraction(g)
        for xk in out["iterates"]:
            assert np.abs(xk - x).max() <= c["eps"] + 1e-12 and xk.min() >= c["lo"] and xk.max() <= c["hi"]
        assert not np.array_equal(out["iterates"][1], out["iterates"][0])
