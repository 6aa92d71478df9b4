"""-m gpu: projected gradient descent on the bare classifier in one device call (dg_pgd, network_builder.ProjectedGradientDescent)
against the CPU restatement in tests/support/pgd_reference.py, and its bitwise identities.  The cases (P.CASES) are fixed on the
CPU, tests/test_whitebox_cpu.py.  Each test prints the figure it is about to assert (pytest -s shows them)."""
import numpy as np
import pytest

from defensegan_amd import network_builder as nb
from tests.support import bpda_reference as R
from tests.support import pgd_reference as P

pytestmark = pytest.mark.gpu


def _kw(c):
    return dict(eps=c["eps"], eps_iter=c["eps_iter"], clip_min=c["lo"], clip_max=c["hi"])


@pytest.fixture(scope="module")
def cases():
    """Every case's model on the device, with its inputs; the float64 runs are P.case_reference's cache."""
    import torch
    out = {}
    for name in P.CASES:
        x, y, model, cp = P.case_inputs(name)
        model.set_weights(cp)
        out[name] = dict(x=x, y=y, model=model, c=P.CASES[name], own=model.get_probs(x).argmax(axis=1).astype(np.int32))
    yield out
    torch.cuda.synchronize()
    for v in out.values():
        v["model"].close()


def _step32(g, xc, xo, eps, eps_iter, lo, hi):
    f = np.float32
    d = (xc + f(eps_iter) * np.sign(g).astype(f)) - xo
    return np.clip(xo + np.clip(d, -f(eps), f(eps)), f(lo), f(hi)).astype(f)


# ---------------------------------------------------------------------- 1. one step, teacher-forced
@pytest.mark.parametrize("name", sorted(P.CASES))
def test_one_step_teacher_forced(cases, name):
    """x_{k+1} from the reference's x_k, k = 0, 1, 2, on the decided pixels (|g_ref| > 1e-4 max|g_ref|, at least 99 % of all): 1e-6
    absolute, tests/test_gpu_bpda.py's bound -- the values are x +- a step and clips."""
    v = cases[name]
    ref = P.case_reference(name)
    atk = nb.ProjectedGradientDescent(v["model"])
    for k in range(3):
        g = ref["grads"][k]
        decided = np.abs(g) > 1e-4 * np.abs(g).max()
        adv = atk.generate(v["x"], v["y"], nb_iter=1, x_init=ref["iterates"][k].astype(np.float32), **_kw(v["c"]))
        d = np.abs(adv.astype(np.float64) - ref["iterates"][k + 1])
        print("%s k %d: undecided %.5f, max |dx| on decided pixels %.3e, pixels off by a sign %d" %
              (name, k, 1 - decided.mean(), d[decided].max(), int((d[decided] > 1e-6).sum())))
        assert 1 - decided.mean() <= 0.01
        assert d[decided].max() <= 1e-6


# ---------------------------------------------------------------------- 2. bitwise identities
@pytest.mark.parametrize("name", sorted(P.CASES))
def test_one_iteration_is_the_rule_on_input_gradient_bit_for_bit(cases, name):
    v, c = cases[name], cases[name]["c"]
    x0 = np.clip(v["x"], c["lo"], c["hi"])
    g = v["model"].input_gradient(x0, labels=v["y"])
    assert np.abs(g).max() > 0
    adv, first = nb.ProjectedGradientDescent(v["model"]).generate(v["x"], v["y"], nb_iter=1, return_info=True, **_kw(c))
    assert adv.tobytes() == _step32(g, x0, v["x"], c["eps"], c["eps_iter"], c["lo"], c["hi"]).tobytes()
    assert set(first.tolist()) <= {1, -1} and first.dtype == np.int32
    # eps_iter > eps lands on the ball's face
    face = nb.ProjectedGradientDescent(v["model"]).generate(v["x"], v["y"], nb_iter=1, eps=0.1, eps_iter=0.5, clip_min=c["lo"], clip_max=c["hi"])
    assert face.tobytes() == _step32(g, x0, v["x"], 0.1, 0.5, c["lo"], c["hi"]).tobytes()


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_three_iterations_are_three_chained_calls(cases, name):
    v, c = cases[name], cases[name]["c"]
    atk = nb.ProjectedGradientDescent(v["model"])
    y = v["own"]                                                        # the model's own predictions: nothing is misclassified at x_0
    adv, first = atk.generate(v["x"], y, nb_iter=3, return_info=True, **_kw(c))
    outs, chain_first, cur = [], np.full(len(y), -1, np.int32), None
    for j in range(3):
        cur, fs = atk.generate(v["x"], y, nb_iter=1, x_init=cur, return_info=True, **_kw(c))
        outs.append(cur)
        chain_first[(chain_first < 0) & (fs == 1)] = j + 1
    assert first.tolist() == chain_first.tolist()
    want = outs[2].copy()
    for j in (1, 2):
        want[first == j] = outs[j - 1][first == j]
    assert adv.tobytes() == want.tobytes()
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])


def test_result_does_not_depend_on_batch_size_and_repeats_bit_for_bit(cases):
    v, c = cases["F"], cases["F"]["c"]
    atk = nb.ProjectedGradientDescent(v["model"])
    kw = dict(_kw(c), nb_iter=3, rand_init=True, seed=5, return_info=True)
    runs = [atk.generate(v["x"], v["own"], batch_size=bs, **kw) for bs in (2, 7, None, None)]
    for adv, first in runs[1:]:
        assert adv.tobytes() == runs[0][0].tobytes() and first.tobytes() == runs[0][1].tobytes()
    import torch
    t_adv, t_first = atk.generate(torch.from_numpy(v["x"]).cuda(), v["own"], batch_size=3, **kw)          # tensors in, tensors out
    assert t_adv.is_cuda and t_first.dtype == torch.int32 and t_adv.cpu().numpy().tobytes() == runs[0][0].tobytes()
    assert t_first.cpu().numpy().tobytes() == runs[0][1].tobytes()


# ---------------------------------------------------------------------- 3. tracking
@pytest.mark.parametrize("name", ["F", "two64"])
def test_first_success_and_result_against_dg_eval_batch_on_every_iterate(cases, name):
    """Ten and two classes.  The labels are the model's own predictions, except image 0's, which is misclassified at x_0 already.
    Every iterate is rebuilt by chained one-iteration calls and judged by dg_eval_batch: first_success is the first iterate in
    1 .. nb_iter whose prediction is not the label, the returned image that iterate, or the last one."""
    v, c = cases[name], cases[name]["c"]
    atk = nb.ProjectedGradientDescent(v["model"])
    y = v["own"].copy()
    y[0] = (y[0] + 1) % c["classes"]
    nb_iter = 4
    kw = dict(_kw(c), eps_iter=0.01)                                    # small steps: the successes spread over the iterates
    adv, first = atk.generate(v["x"], y, nb_iter=nb_iter, return_info=True, **kw)
    iterates, cur = [], None
    for _ in range(nb_iter):
        cur = atk.generate(v["x"], y, nb_iter=1, x_init=cur, **kw)
        iterates.append(cur)
    preds = {j + 1: v["model"].eval_batch(it, None, y)[1].cpu().numpy() for j, it in enumerate(iterates)}
    want_adv, want_first = R.track(preds, y, [np.clip(v["x"], c["lo"], c["hi"])] + iterates)
    print("%s: first_success %s" % (name, first.tolist()))
    assert first.tolist() == want_first.tolist()
    assert adv.tobytes() == want_adv.astype(np.float32).tobytes()
    assert first[0] == 1                                                # misclassified from the start: the first iterate judged
    # eps = 0: no image ever moves or succeeds; the result is the last iterate, clip(x)
    adv0, first0 = atk.generate(v["x"], v["own"], nb_iter=3, eps=0.0, eps_iter=0.05, clip_min=c["lo"], clip_max=c["hi"], return_info=True)
    assert first0.tolist() == [-1] * len(y)
    assert adv0.tobytes() == np.clip(v["x"], c["lo"], c["hi"]).tobytes()


def test_argmax_takes_the_first_maximum_as_dg_eval_batch_does():
    """Equal logits (zero weights, a bias with its maximum three times, 70 classes: more than one class per lane; 5 and 69 share a lane,
    67 sits in another): the prediction is the FIRST maximum, class 5 -- label 5 never succeeds, labels 67 and 69 succeed at once."""
    m = nb.MLP([nb.Flatten(), nb.Linear(70), nb.Softmax()], input_shape=(None, 3, 3, 1))
    b = np.zeros(70, np.float32)
    b[[5, 67, 69]] = 1.0
    m.set_weights([(np.zeros((9, 70), np.float32), b)])
    x = np.random.RandomState(0).uniform(0, 1, (3, 3, 3, 1)).astype(np.float32)
    assert m.eval_batch(x, None, None)[1].cpu().numpy().tolist() == [5, 5, 5]
    _, first = nb.ProjectedGradientDescent(m).generate(x, np.array([5, 67, 69]), nb_iter=2, clip_min=0.0, clip_max=1.0, return_info=True)
    assert first.tolist() == [-1, 1, 1]
    m.close()


# ---------------------------------------------------------------------- 4. ball, range, labels, refusals
def test_ball_and_range_hold_with_rand_init(cases):
    for name, kw in (("F", dict(eps=0.3, eps_iter=0.05, clip_min=0.0, clip_max=1.0, rand_init=True)),
                     ("two64", dict(eps=0.3, eps_iter=0.05, clip_min=-1.0, clip_max=1.0, rand_init=True)),
                     ("two64", dict(eps=0.1, eps_iter=0.25, clip_min=-1.0, clip_max=0.5))):
        v = cases[name]
        adv = nb.ProjectedGradientDescent(v["model"]).generate(v["x"], v["own"], nb_iter=3, seed=9, **kw)
        base = np.clip(v["x"], kw["clip_min"], kw["clip_max"])
        assert adv.min() >= kw["clip_min"] and adv.max() <= kw["clip_max"]
        inside = (v["x"] >= kw["clip_min"]) & (v["x"] <= kw["clip_max"])          # a pixel the range moves may leave the ball
        assert not inside.all() or kw["clip_max"] == 1.0
        assert np.abs(adv.astype(np.float64) - v["x"])[inside].max() <= kw["eps"] + 1e-6
        assert np.abs(adv - base).max() > 0.5 * kw["eps"]
    # the rand_init start itself: with eps_iter = 0 the first iterate is x_0 = clip(x + noise) (to the rule's two roundings)
    v = cases["two64"]
    adv = nb.ProjectedGradientDescent(v["model"]).generate(v["x"], v["own"], nb_iter=1, eps=0.3, eps_iter=0.0, clip_min=-1.0, clip_max=1.0,
                                                           rand_init=True, seed=77)
    x0 = np.clip(v["x"] + R.rand_noise(len(v["x"]), v["x"][0].size, 0.3, 77).reshape(v["x"].shape), -1.0, 1.0)
    np.testing.assert_allclose(adv, x0, rtol=0, atol=1e-6)


def test_an_out_of_range_label_leaves_its_image_at_clip_x(cases):
    v, c = cases["F"], cases["F"]["c"]
    y = v["own"].copy()
    y[2], y[5] = 10, -1
    adv, first = nb.ProjectedGradientDescent(v["model"]).generate(v["x"], y, nb_iter=3, return_info=True, **_kw(c))
    x0 = np.clip(v["x"], c["lo"], c["hi"])
    for i in (2, 5):
        assert adv[i].tobytes() == x0[i].tobytes()
        assert first[i] == 1                                            # no prediction equals such a label
    ok = np.ones(len(y), bool)
    ok[[2, 5]] = False
    want = nb.ProjectedGradientDescent(v["model"]).generate(v["x"][ok], v["own"][ok], nb_iter=3, **_kw(c))
    assert adv[ok].tobytes() == want.tobytes() and not np.array_equal(want, x0[ok])


def test_refusals(cases):
    from defensegan_amd import _native
    import torch
    v = cases["convlin5"]
    with pytest.raises(ValueError, match="PGD-on-bare.*ProjectedGradientDescent"):
        nb.BPDA(v["model"]).generate(v["x"], v["y"])
    defended = nb.model_e()
    defended.init_like_reference(seed=0)
    defended.add_rec_model(object(), None, 4)
    with pytest.raises(ValueError, match="use BPDA"):
        nb.ProjectedGradientDescent(defended).generate(np.zeros((2, 28, 28, 1), np.float32), np.zeros(2, np.int32))
    defended.close()
    lib, h = _native.load(), v["model"]._handle
    buf = torch.zeros(3 * 25, device="cuda")
    out = torch.zeros(3 * 25, device="cuda")
    lab = torch.zeros(3, dtype=torch.int32, device="cuda")
    p, q, l = buf.data_ptr(), out.data_ptr(), lab.data_ptr()
    for args, text in (((0.3, 0.05, 0, 0.0, 1.0, q), b"nb_iter"), ((-0.3, 0.05, 1, 0.0, 1.0, q), b"eps"), ((0.3, 0.05, 1, 1.0, 0.0, q), b"clip_min"),
                       ((0.3, 0.05, 1, 0.0, 1.0, p), b"x_adv must not be")):
        eps, eps_iter, nb_iter, lo, hi, dst = args
        assert lib.dg_pgd(h, p, p, l, 3, eps, eps_iter, nb_iter, lo, hi, dst, l, None) == -1
        assert text in lib.dg_last_error()
