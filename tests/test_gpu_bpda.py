"""-m gpu: the BPDA/EOT attack on the device (dg_bpda_step, dg_bpda_track, network_builder.BPDA) against the CPU restatement in
tests/support/bpda_reference.py, and its bitwise identities.  The case (R.CASE: MNIST generator at gain 2.0, R = 2, L = 5,
B = 7, classifier F with fixed random weights) is fixed on the CPU, tests/test_bpda_cpu.py."""
import warnings

import numpy as np
import pytest

from defensegan_amd import gan_defense, network_builder as nb
from tests.helpers import make_gan
from tests.support import bpda_reference as R

pytestmark = pytest.mark.gpu
C = R.CASE
KW = dict(eps=C["eps"], eps_iter=C["eps_iter"], clip_min=C["lo"], clip_max=C["hi"])


@pytest.fixture(scope="module")
def case():
    """The defended model of R.CASE on the device, and a cache of float64 reference runs (one per EOT count), never modified."""
    import torch
    p, x, y, model, cp = R.case_inputs()
    gan, p_dev = make_gan(C["arch"], wseed=C["wseed"], gain=C["gain"], bias_range=C["bias_range"], rec_rr=C["R"], rec_iters=C["L"],
                          rec_lr=C["lr"])
    model.set_weights(cp)
    model.add_rec_model(gan, None, 50)
    refs = {}

    def reference(m_eot, nb_iter=3):
        if (m_eot, nb_iter) not in refs:
            sched, final = R.seed_schedule(C["seed"], nb_iter, m_eot)
            z0 = {s: gan.init_latents(C["B"] * C["R"], seed=s, first_row=0).cpu().numpy() for row in sched for s in row}
            z0[final] = gan.init_latents(C["B"] * C["R"], seed=final, first_row=0).cpu().numpy()
            ops = R.oracle_ops(p, C["arch"], R.layers_of(model), cp, y, z0, C["R"], C["L"], C["lr"])
            refs[(m_eot, nb_iter)] = R.bpda(ops, x, y, C["eps"], C["eps_iter"], nb_iter, m_eot, C["lo"], C["hi"], C["seed"])
        return refs[(m_eot, nb_iter)]
    yield dict(x=x, y=y, model=model, gan=gan, reference=reference)
    torch.cuda.synchronize()
    model.close()
    gan.close()


# ---------------------------------------------------------------------- 1. one step, teacher-forced
@pytest.mark.parametrize("m_eot", [1, 3])
def test_one_step_teacher_forced(case, m_eot):
    """x_{k+1} from the reference's x_k, k = 0, 1, 2, on the decided pixels (|g_ref| > 1e-4 max|g_ref|, at least 98 % of all):
    1e-6 absolute -- the values are x +- a step and clips."""
    x, y, ref = case["x"], case["y"], case["reference"](m_eot)
    atk = nb.BPDA(case["model"])
    for k in range(3):
        g = ref["grads"][k]
        decided = np.abs(g) > 1e-4 * np.abs(g).max()
        adv = atk.generate(x, y, nb_iter=1, eot_samples=m_eot, x_init=ref["iterates"][k].astype(np.float32), seed=C["seed"] + k * m_eot, **KW)
        d = np.abs(adv.astype(np.float64) - ref["iterates"][k + 1])
        print("m %d k %d: undecided %.4f, max |dx| on decided pixels %.3e, pixels off by a sign %d" %
              (m_eot, k, 1 - decided.mean(), d[decided].max(), int((d[decided] > 1e-6).sum())))
        assert 1 - decided.mean() <= 0.02
        assert d[decided].max() <= 1e-6


@pytest.mark.parametrize("m_eot", [1, 3])
def test_accumulated_gradient_matches_reference(case, m_eot):
    """g_0 = the sum over the EOT samples of the classifier's gradient at the projections of x_0, through dg_bpda_step's
    accumulate form: dg_clf_backward's bound (the sum adds no new kind of arithmetic)."""
    import torch
    x, y, gan, ref = case["x"], case["y"], case["gan"], case["reference"](m_eot)
    ops = nb.BpdaDeviceOps(case["model"])
    x0 = torch.from_numpy(np.clip(x, C["lo"], C["hi"])).to(ops.device)
    lab = torch.from_numpy(y).to(ops.device)
    gsum = torch.zeros_like(x0)
    for s in range(m_eot):
        ops.step(ops.project(x0, C["seed"] + s, 0), lab, None, None, gsum, True, 0.0, 0.0, 0.0, 0.0, None)
    got, want = gsum.cpu().numpy(), ref["grads"][0]
    print("m %d: max |dg| %.3e of max |g| %.3e" % (m_eot, np.abs(got - want).max(), np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


# ---------------------------------------------------------------------- the step kernel alone: both vector widths
def _step32(g, xc, xo, eps, eps_iter, lo, hi):
    f = np.float32
    d = (xc + f(eps_iter) * np.sign(g).astype(f)) - xo
    return np.clip(xo + np.clip(d, -f(eps), f(eps)), f(lo), f(hi)).astype(f)


@pytest.mark.parametrize("shape,B", [((64, 64, 3), 3), ((5, 5, 1), 3), ((28, 28, 1), 7)])
def test_step_kernel_is_the_input_gradient_and_the_rule_bit_for_bit(shape, B):
    """CelebA-sized rows (float4 path, 3 x 12288 elements: more than one workgroup and a partial last one), 5 x 5 x 1 rows
    (25 elements: the scalar path) and the MNIST case's 7 x 784: g has dg_clf_input_gradient's bits; gsum accumulates in call
    order; x_next is the rule in float32, with and without gsum; eps_iter > eps lands on the ball's face; clip_min = -1."""
    import torch
    m = nb.MLP([nb.Conv2D(4, (3, 3), (2, 2), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(10), nb.Softmax()], input_shape=(None,) + shape)
    m.set_weights(R.init_params(m, 5))
    ops = nb.BpdaDeviceOps(m)
    rs = np.random.RandomState(B)
    rec, xo = (rs.uniform(-1, 1, (B,) + shape).astype(np.float32) for _ in range(2))
    xc = np.clip(xo + rs.uniform(-0.3, 0.3, xo.shape), -1, 1).astype(np.float32)
    y = rs.randint(0, 10, B).astype(np.int32)
    g = m.input_gradient(rec, labels=y)
    dev = lambda a: torch.from_numpy(a).to(ops.device)
    t_rec, t_xc, t_xo, t_y = dev(rec), dev(xc), dev(xo), dev(y)
    out = torch.empty_like(t_xc)
    ops.step(t_rec, t_y, t_xc, t_xo, None, False, 0.3, 0.05, -1.0, 1.0, out)
    assert out.cpu().numpy().tobytes() == _step32(g, xc, xo, 0.3, 0.05, -1.0, 1.0).tobytes()
    ops.step(t_rec, t_y, t_xc, t_xo, None, False, 0.1, 0.5, -1.0, 1.0, out)                    # eps_iter > eps
    face = out.cpu().numpy()
    assert face.tobytes() == _step32(g, xc, xo, 0.1, 0.5, -1.0, 1.0).tobytes()
    assert np.abs(face - xo).max() <= 0.1 + 1e-6 and face.min() >= -1 and face.max() <= 1
    prior = rs.standard_normal(xo.shape).astype(np.float32)
    gsum = dev(prior.copy())
    ops.step(t_rec, t_y, None, None, gsum, True, 0.0, 0.0, 0.0, 0.0, None)
    assert gsum.cpu().numpy().tobytes() == (prior + g).tobytes()
    ops.step(t_rec, t_y, t_xc, t_xo, gsum, False, 0.3, 0.05, 0.0, 1.0, out)
    assert out.cpu().numpy().tobytes() == _step32((prior + g) + g, xc, xo, 0.3, 0.05, 0.0, 1.0).tobytes()
    assert gsum.cpu().numpy().tobytes() == (prior + g).tobytes()                               # read, not written
    zero = dev(np.zeros_like(xo))                                                               # sign(0) = 0
    m0 = nb.MLP([nb.Flatten(), nb.Linear(10), nb.Softmax()], input_shape=(None,) + shape)
    m0.set_weights([(np.zeros((int(np.prod(shape)), 10), np.float32), np.zeros(10, np.float32))])
    nb.BpdaDeviceOps(m0).step(t_rec, t_y, t_xc, t_xo, None, False, 0.05, 0.2, -1.0, 1.0, zero)
    assert zero.cpu().numpy().tobytes() == np.clip(xo + np.clip(xc - xo, np.float32(-0.05), np.float32(0.05)), -1, 1).astype(np.float32).tobytes()
    torch.cuda.synchronize()
    m.close()
    m0.close()


def test_entry_argument_errors():
    from defensegan_amd import _native
    lib = _native.load()
    assert lib.dg_bpda_step(None, None, None, 1, None, None, None, 0, 0.1, 0.1, 0.0, 1.0, None, None) == -1
    assert lib.dg_bpda_track(None, None, 1, 0, None, None, None, 4, None) == -1
    m = nb.MLP([nb.Flatten(), nb.Linear(10), nb.Softmax()], input_shape=(None, 2, 2, 1))
    m.init_like_reference(0)
    import torch
    buf = torch.zeros(8, device="cuda")
    lab = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    assert lib.dg_bpda_step(m._handle, p, lab.data_ptr(), 2, None, None, None, 1, 0.1, 0.1, 0.0, 1.0, None, None) == -1       # no gsum
    assert lib.dg_bpda_step(m._handle, p, lab.data_ptr(), 2, p, p, None, 0, 0.1, 0.1, 0.0, 1.0, None, None) == -1             # no x_next
    assert lib.dg_bpda_step(m._handle, p, lab.data_ptr(), 2, p, p, None, 0, -0.1, 0.1, 0.0, 1.0, p, None) == -1               # eps < 0
    assert lib.dg_bpda_track(lab.data_ptr(), lab.data_ptr(), 2, 1, p, p, lab.data_ptr(), 4, None) == -1                      # x_best is x_iter
    assert b"dg_bpda_track" in lib.dg_last_error()
    m.close()


# ---------------------------------------------------------------------- 2. bitwise identities
def test_single_sample_is_input_gradient_on_the_projection_fed_to_the_step(case):
    x, y, gan, model = case["x"], case["y"], case["gan"], case["model"]
    x0 = np.clip(x, C["lo"], C["hi"])
    rec = gan.reconstruct(x0, seed=C["seed"], first_row=0)
    g = model.input_gradient(rec, labels=y, no_rec=True)
    assert np.abs(g).max() > 0
    adv = nb.BPDA(model).generate(x, y, nb_iter=1, seed=C["seed"], **KW)
    assert adv.tobytes() == _step32(g, x0, x, C["eps"], C["eps_iter"], C["lo"], C["hi"]).tobytes()


def _chain(atk, x, y, n_calls, m_eot, **kw):
    """n_calls chained nb_iter = 1 calls with the documented seeds: (iterates x_1 .. x_n, first success over the chain)."""
    outs, first, cur = [], np.full(len(x), -1, np.int32), None
    for j in range(n_calls):
        cur, fs = atk.generate(x, y, nb_iter=1, eot_samples=m_eot, seed=C["seed"] + j * m_eot, x_init=cur, return_info=True,
                               **dict(kw, rand_init=kw.get("rand_init", False) and j == 0))
        outs.append(cur)
        first[(first < 0) & (fs == 1)] = j + 1
    return outs, first


def test_three_iterations_are_three_chained_calls(case):
    x, y, atk = case["x"], case["y"], nb.BPDA(case["model"])
    adv, first = atk.generate(x, y, nb_iter=3, eot_samples=2, seed=C["seed"], return_info=True, **KW)
    outs, chain_first = _chain(atk, x, y, 3, 2, **KW)
    assert first.tolist() == chain_first.tolist()
    want = outs[2].copy()
    for j in (1, 2):
        want[first == j] = outs[j - 1][first == j]
    assert adv.tobytes() == want.tobytes()
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    # the judgement is the defended prediction on the iterate, from the projection with the next seed
    rec = case["gan"].reconstruct(outs[0], seed=C["seed"] + 2, first_row=0)
    _, preds, _ = case["model"].eval_batch(rec, None, y)
    assert ((preds.cpu().numpy() != y) == (chain_first == 1)).all()


def test_result_does_not_depend_on_batch_size_and_repeats_bit_for_bit(case, monkeypatch):
    monkeypatch.setattr(gan_defense, "COALESCE_ROWS", 1)          # one caller batch per engine call: batch_size really cuts
    x, y, atk = case["x"], case["y"], nb.BPDA(case["model"])
    kw = dict(KW, nb_iter=2, eot_samples=2, seed=C["seed"], rand_init=True, return_info=True)
    runs = [atk.generate(x, y, batch_size=bs, **kw) for bs in (2, 7, 50, 7)]
    for adv, first in runs[1:]:
        assert adv.tobytes() == runs[0][0].tobytes() and first.tobytes() == runs[0][1].tobytes()
    import torch
    t_adv, t_first = atk.generate(torch.from_numpy(x).cuda(), y, batch_size=3, **kw)          # tensors in, tensors out
    assert t_adv.is_cuda and t_first.dtype == torch.int32 and t_adv.cpu().numpy().tobytes() == runs[0][0].tobytes()


# ---------------------------------------------------------------------- 3. tracking
def test_tracking_on_a_prescribed_prediction_sequence(case):
    """The device's bookkeeping (dg_bpda_track) on predictions a recording stand-in hands out: first success kept, a later
    failure does not undo it, no success leaves the last iterate and -1 -- exactly the reference's track() on the same iterates."""
    import torch
    x, y, model = case["x"], case["y"], case["model"]
    wrong = (y + 1) % 10
    preds = {1: y.copy(), 2: y.copy(), 3: y.copy()}
    preds[1][1] = wrong[1]
    preds[2][0] = wrong[0]; preds[2][5] = wrong[5]
    preds[3][3] = wrong[3]; preds[3][5] = y[5]

    class Prescribed(nb.BpdaDeviceOps):
        def __init__(self, model):
            super().__init__(model)
            self.judged, self.asked = None, []

        def project(self, x_, seed, first_row):
            self.judged = seed - C["seed"]
            self.asked.append(seed)
            return super().project(x_, seed, first_row)

        def predict(self, rec):
            super().predict(rec)                                   # the real one runs too; its answer is replaced
            return torch.from_numpy(preds[self.judged].astype(np.int32)).to(self.device)
    ops = Prescribed(model)
    adv, first = nb.BPDA(model, ops=ops).generate(x, y, nb_iter=3, seed=C["seed"], return_info=True, **KW)
    assert ops.asked == [C["seed"] + j for j in range(4)]
    outs, _ = _chain(nb.BPDA(model), x, y, 3, 1, **KW)
    want_adv, want_first = R.track(preds, y, [np.clip(x, C["lo"], C["hi"])] + outs)
    assert first.tolist() == want_first.tolist() == [2, 1, -1, 3, -1, 2, -1]
    assert adv.tobytes() == want_adv.tobytes()


# ---------------------------------------------------------------------- 4. ball and range
def test_ball_and_range_hold_with_rand_init_and_negative_clip_min(case):
    x, y, atk = case["x"], case["y"], nb.BPDA(case["model"])
    xs = (2 * x - 1).astype(np.float32)                            # a [-1, 1] input
    for kw in (dict(eps=0.3, eps_iter=0.05, clip_min=-1.0, clip_max=1.0, rand_init=True),
               dict(eps=0.1, eps_iter=0.25, clip_min=-1.0, clip_max=0.5),
               dict(eps=0.3, eps_iter=0.05, clip_min=0.0, clip_max=1.0, rand_init=True)):
        src = x if kw["clip_min"] == 0.0 else xs
        adv = atk.generate(src, y, nb_iter=3, eot_samples=2, seed=C["seed"], **kw)
        base = np.clip(src, kw["clip_min"], kw["clip_max"])
        assert adv.min() >= kw["clip_min"] and adv.max() <= kw["clip_max"]
        assert np.abs(adv.astype(np.float64) - src).max() <= kw["eps"] + 1e-6
        assert np.abs(adv - base).max() > 0.5 * kw["eps"]
    # the rand_init start itself: with eps_iter = 0 the first iterate is x_0 = clip(x + noise) (to the rule's two roundings)
    adv = atk.generate(xs, y, nb_iter=1, eps=0.3, eps_iter=0.0, clip_min=-1.0, clip_max=1.0, rand_init=True, seed=77)
    x0 = np.clip(xs + R.rand_noise(len(xs), 784, 0.3, 77).reshape(xs.shape), -1.0, 1.0)
    np.testing.assert_allclose(adv, x0, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------- 5. end to end
def test_bpda_lowers_defended_accuracy_below_the_zero_gradient_fgsm():
    """Classifier F trained on a separable 10-class set drawn from the generator's own range (x = G(z_true), z_true a class
    prototype plus noise), defended by the projection (R = 2, L = 20): the reference's FGSM sees a zero gradient and returns
    clip(x); BPDA(eps = 0.3, nb_iter = 5) must leave strictly fewer of the 32 test images correctly classified.
    Measured on MI355X: see DESIGN.md section 7."""
    import torch
    from defensegan_amd import utils_tf
    gan, _ = make_gan("mnist", wseed=1234, gain=2.0, bias_range=0.1, rec_rr=2, rec_iters=20, rec_lr=10.0)
    rs = np.random.RandomState(3)
    protos = rs.standard_normal((10, 128))
    y = rs.randint(0, 10, 2032).astype(np.int32)
    z = ((protos[y] + 0.3 * rs.standard_normal((len(y), 128))) * np.sqrt(1.0 / 128)).astype(np.float32)
    x = gan.generate(z)
    x = x if isinstance(x, np.ndarray) else x.cpu().numpy()
    x = x.reshape(-1, 28, 28, 1).astype(np.float32)
    xtr, ytr, xte, yte = x[:2000], y[:2000], x[2000:], y[2000:]
    m = nb.model_f()
    m.init_like_reference(seed=1)
    utils_tf.model_train(m, xtr, ytr, args={"nb_epochs": 3, "batch_size": 128, "learning_rate": 0.001})
    bare, _, _ = m.eval_batch(xte, labels=yte)
    m.add_rec_model(gan, None, 32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x_fgsm = nb.FastGradientMethod(m).generate(xte, eps=0.3, y=yte, clip_min=0.0, clip_max=1.0)
    assert np.array_equal(x_fgsm, np.clip(xte, 0, 1))
    c_fgsm, n, _ = m.model_eval(x_fgsm, yte, 32)
    x_bpda, first = nb.BPDA(m).generate(xte, yte, eps=0.3, nb_iter=5, clip_min=0.0, clip_max=1.0, seed=777, return_info=True)
    c_bpda, _, _ = m.model_eval(x_bpda, yte, 32)
    print("bare accuracy %.3f; defended accuracy under zero-gradient FGSM %.3f, under BPDA(eps 0.3, nb_iter 5) %.3f; "
          "%d of %d images had a successful iterate" % (bare / 32.0, c_fgsm / float(n), c_bpda / float(n), int((first > 0).sum()), n))
    assert np.abs(x_bpda - xte).max() <= 0.3 + 1e-6
    assert c_bpda < c_fgsm
    torch.cuda.synchronize()
    m.close()
    gan.close()
