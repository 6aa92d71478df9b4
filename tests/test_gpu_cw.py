"""-m gpu: Carlini-Wagner L2 on the device (dg_cw, network_builder.CarliniWagnerL2) and the seeded classifier backward
(dg_clf_backward) against the CPU restatement in tests/support/cw_reference.py and the NumPy oracle."""
import numpy as np
import pytest

from defensegan_amd import network_builder as nb
from oracle import classifier_oracle as CO
from tests.support import cw_reference as R

pytestmark = pytest.mark.gpu


def _model(name, seed=None, input_shape=(None, 28, 28, 1)):
    m = nb.MODELS[name](input_shape=input_shape)
    params = m.init_like_reference(seed=ord(name) if seed is None else seed)
    return m, params


def _oracle_backward(layers, params, x, seed):
    """d(sum seed * logits)/dx by the oracle's layer functions (classifier_oracle.conv2d / conv2d_backward_input)."""
    acts, used, it = [x], [], iter(params)
    body = [L for L in layers if L[0] != "softmax"]
    for L in body:
        h = acts[-1]
        if L[0] == "conv":
            W, b = next(it); used.append(W); h = CO.conv2d(h, W, b, L[3], L[4])
        elif L[0] == "linear":
            W, b = next(it); used.append(W); h = h @ W.astype(h.dtype) + b.astype(h.dtype)
        elif L[0] == "relu":
            h = np.maximum(h, 0)
        elif L[0] == "flatten":
            h = h.reshape(len(h), -1)
        acts.append(h)
    g, pi = seed, len(used)
    for li in range(len(body) - 1, -1, -1):
        L, xin, out = body[li], acts[li], acts[li + 1]
        if L[0] == "conv":
            pi -= 1; g = CO.conv2d_backward_input(g, used[pi], xin.shape, L[3], L[4])
        elif L[0] == "linear":
            pi -= 1; g = g @ used[pi].astype(g.dtype).T
        elif L[0] == "relu":
            g = g * (out > 0)
        elif L[0] == "flatten":
            g = g.reshape(xin.shape)
    return g


@pytest.mark.parametrize("name", ["A", "E", "F"])
def test_seeded_backward_matches_oracle_and_ce_seed_is_bitwise_fgsm(name):
    import torch
    m, params = _model(name)
    rs = np.random.RandomState(11)
    x = rs.uniform(0, 1, (5, 28, 28, 1)).astype(np.float32)
    seed = rs.standard_normal((5, 10)).astype(np.float32)
    g = m.backward(x, seed)
    p64 = [(W.astype(np.float64), b.astype(np.float64)) for W, b in params]
    want = _oracle_backward(R.layers_of(m), p64, x.astype(np.float64), seed.astype(np.float64))
    np.testing.assert_allclose(g, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # the CE seed, bit for bit as dg_clf_input_gradient forms it: the input gradient of an identity Linear on the logits
    # (fmaf with exact zeros and ones passes the seed through unchanged)
    logits = m.get_logits(x)
    ident = nb.MLP([nb.Flatten(), nb.Linear(10), nb.Softmax()], input_shape=(None, 1, 1, 10))
    ident.set_weights([(np.eye(10, dtype=np.float32), np.zeros(10, np.float32))])
    labels = rs.randint(0, 10, 5).astype(np.int32)
    ce_seed = ident.input_gradient(logits.reshape(5, 1, 1, 10), labels=labels).reshape(5, 10)
    g_ce = m.backward(x, ce_seed)
    g_ref = m.input_gradient(x, labels=labels)
    assert g_ce.tobytes() == g_ref.tobytes()
    adv = nb.FastGradientMethod(m).generate(x, eps=0.1, y=labels, clip_min=0.0, clip_max=1.0)
    assert adv.tobytes() == np.clip(x + np.float32(0.1) * np.sign(g_ce), 0, 1).astype(np.float32).tobytes()
    ident.close()
    m.close()
    torch.cuda.synchronize()


def _ref(m, params, x, **kw):
    p64 = [(W.astype(np.float64), b.astype(np.float64)) for W, b in params]
    return R.cw_l2(R.layers_of(m), p64, x.astype(np.float64), **kw)


@pytest.mark.parametrize("name", ["A", "F"])
def test_one_adam_step_values(name):
    """Two iterations = one Adam step seen by the best tracking.  Adam's first step is about lr * sign(g): pixels whose float64
    gradient is below 1e-4 of the image's largest are left out of the pixel comparison."""
    import torch
    m, params = _model(name)
    x = np.random.RandomState(5).uniform(0, 1, (16, 28, 28, 1)).astype(np.float32)
    kw = dict(batch_size=16, learning_rate=0.1, binary_search_steps=1, max_iterations=2, abort_early=False, initial_const=100.0)
    adv, l2, cls = nb.CarliniWagnerL2(m).generate(x, return_info=True, **kw)
    ref = _ref(m, params, x, **kw)
    assert (ref["best_class"] != -1).sum() >= 8
    np.testing.assert_array_equal(cls, ref["best_class"])
    np.testing.assert_allclose(l2, ref["best_l2"], rtol=1e-3)
    # the float64 gradient at w = 0
    xt = torch.as_tensor(x.astype(np.float64))
    timg = torch.atanh((torch.clamp(xt, 0, 1) * 2 - 1) * 0.999999)
    other = R.to_img(torch.tanh(timg), 0.0, 1.0)
    p64 = [(W.astype(np.float64), b.astype(np.float64)) for W, b in params]
    *_, g = R.step_values(R.layers_of(m), p64, torch.zeros_like(xt), timg, other, ref["labels"], np.full(16, 100.0), 0.0, False, 0.0, 1.0)
    g = np.abs(g.numpy()).reshape(16, -1)
    keep = g >= 1e-4 * g.max(axis=1, keepdims=True)
    d = np.abs(adv - ref["x_adv"]).reshape(16, -1)
    assert keep.mean() > 0.9
    assert d[keep].max() < 1e-5, d[keep].max()
    m.close()


@pytest.mark.parametrize("name", ["A", "F"])
def test_five_iterations(name):
    m, params = _model(name)
    x = np.random.RandomState(5).uniform(0, 1, (16, 28, 28, 1)).astype(np.float32)
    kw = dict(batch_size=16, learning_rate=0.01, binary_search_steps=1, max_iterations=5, abort_early=False, initial_const=100.0)
    adv, l2, cls = nb.CarliniWagnerL2(m).generate(x, return_info=True, **kw)
    ref = _ref(m, params, x, **kw)
    assert (ref["best_class"] != -1).sum() >= 4
    np.testing.assert_array_equal(cls, ref["best_class"])
    np.testing.assert_allclose(l2, ref["best_l2"], rtol=1e-3)
    assert (np.abs(adv - ref["x_adv"]) <= 1e-4).mean() >= 0.999
    m.close()


def test_whitebox_setting_full_horizon():
    """whitebox.py:201-209: binary_search_steps 1, max_iterations 100, learning_rate 10, initial_const 100 (abort_early default)."""
    import torch
    m, params = _model("F")
    x = np.random.RandomState(0).uniform(0, 1, (64, 28, 28, 1)).astype(np.float32)
    kw = dict(batch_size=32, learning_rate=10.0, binary_search_steps=1, max_iterations=100, initial_const=100.0)
    adv, l2, cls = nb.CarliniWagnerL2(m).generate(x, return_info=True, **kw)
    ref = _ref(m, params, x, **kw)
    assert abs(int((cls != -1).sum()) - int((ref["best_class"] != -1).sum())) <= 1
    ok = cls != -1
    assert abs(np.median(l2[ok]) / np.median(ref["best_l2"][ref["best_class"] != -1]) - 1) < 0.05
    # self-consistency on the device: a successful x_adv is misclassified and sits at best_l2 from the tanh round trip of x
    t = m.get_logits(x).argmax(axis=1)
    pred = m.get_logits(adv).argmax(axis=1)
    assert (pred[ok] != t[ok]).all()
    x64 = x.astype(np.float64)
    other = (np.tanh(np.arctanh((np.clip(x64, 0, 1) * 2 - 1) * 0.999999)) + 1) / 2
    d2 = ((adv.astype(np.float64) - other) ** 2).reshape(64, -1).sum(axis=1)
    np.testing.assert_allclose(d2[ok], l2[ok], rtol=1e-5)
    assert adv[~ok].tobytes() == np.clip(x[~ok], 0, 1).tobytes()
    assert (l2[~ok] == np.float32(1e10)).all()
    m.close()
    torch.cuda.synchronize()


def test_abort_early_chunks():
    m, params = _model("F")
    x = np.random.RandomState(0).uniform(0, 1, (64, 28, 28, 1)).astype(np.float32)
    kw = dict(batch_size=16, learning_rate=0.05, binary_search_steps=1, max_iterations=100, abort_early=True, initial_const=1.0)
    ref = _ref(m, params, x, **kw)
    stops = ref["abort_iters"][0]
    assert None not in stops and len(set(stops)) >= 2, stops           # the chunks stop at different checks
    full = _ref(m, params, x, **dict(kw, abort_early=False))
    assert not np.array_equal(full["best_l2"], ref["best_l2"])          # and stopping changes the result
    cw = nb.CarliniWagnerL2(m)
    adv, l2, cls, _, stop = cw.generate(x, return_info=True, return_search=True, **kw)
    assert stop.tolist() == [stops]                                     # the device's chunks stop at the same checks
    np.testing.assert_array_equal(cls, ref["best_class"])
    np.testing.assert_allclose(l2, ref["best_l2"], rtol=1e-3)
    adv2, l22, cls2 = cw.generate(x, return_info=True, **kw)
    assert adv.tobytes() == adv2.tobytes() and l2.tobytes() == l22.tobytes() and cls.tobytes() == cls2.tobytes()
    a1, l1, c1 = cw.generate(x[16:32], return_info=True, **kw)         # chunk 1 alone
    assert a1.tobytes() == adv[16:32].tobytes() and l1.tobytes() == l2[16:32].tobytes() and c1.tobytes() == cls[16:32].tobytes()
    m.close()


def test_binary_search_steps():
    m, params = _model("F")
    x = np.random.RandomState(0).uniform(0, 1, (16, 28, 28, 1)).astype(np.float32)
    kw = dict(batch_size=8, learning_rate=0.05, binary_search_steps=3, max_iterations=20, abort_early=False, initial_const=0.01)
    adv, l2, cls, const, _ = nb.CarliniWagnerL2(m).generate(x, return_info=True, return_search=True, **kw)
    ref = _ref(m, params, x, **kw)
    assert (ref["const"] < 0.01).any() and (ref["const"] > 0.01).any()   # the search moved the constants both ways
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    np.testing.assert_array_equal(cls, ref["best_class"])
    np.testing.assert_allclose(l2, ref["best_l2"], rtol=1e-3)
    assert (np.abs(adv - ref["x_adv"]) <= 1e-4).mean() >= 0.999
    m.close()


def test_repeat_runs_the_last_step_at_the_upper_bound():
    """binary_search_steps >= 10: the last outer step runs at const = upper_bound (cw_reset_kernel's repeat branch)."""
    m, params = _model("F")
    x = np.random.RandomState(0).uniform(0, 1, (8, 28, 28, 1)).astype(np.float32)
    kw = dict(batch_size=4, learning_rate=0.05, binary_search_steps=10, max_iterations=3, abort_early=False, initial_const=0.01)
    adv, l2, cls, const, _ = nb.CarliniWagnerL2(m).generate(x, return_info=True, return_search=True, **kw)
    ref = _ref(m, params, x, **kw)
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    np.testing.assert_array_equal(cls, ref["best_class"])
    np.testing.assert_allclose(l2, ref["best_l2"], rtol=1e-3)
    m.close()


def test_abort_early_with_chunks_wider_than_a_wave():
    """batch_size 128 (four waves per chunk workgroup) with abort on and a trailing partial chunk: the stop iterations follow the
    reference, and every returned x_adv is the image its best_l2 was measured on."""
    m, params = _model("F")
    x = np.random.RandomState(0).uniform(0, 1, (192, 28, 28, 1)).astype(np.float32)
    kw = dict(batch_size=128, learning_rate=0.05, binary_search_steps=1, max_iterations=100, abort_early=True, initial_const=1.0)
    adv, l2, cls, _, stop = nb.CarliniWagnerL2(m).generate(x, return_info=True, return_search=True, **kw)
    ref = _ref(m, params, x, **kw)
    assert None not in ref["abort_iters"][0]
    assert stop.tolist() == ref["abort_iters"]
    np.testing.assert_array_equal(cls, ref["best_class"])
    np.testing.assert_allclose(l2, ref["best_l2"], rtol=1e-3)
    ok = cls != -1
    x64 = x.astype(np.float64)
    other = (np.tanh(np.arctanh((np.clip(x64, 0, 1) * 2 - 1) * 0.999999)) + 1) / 2
    d2 = ((adv.astype(np.float64) - other) ** 2).reshape(192, -1).sum(axis=1)
    np.testing.assert_allclose(d2[ok], l2[ok], rtol=1e-5)
    t = m.get_logits(x).argmax(axis=1)
    assert (m.get_logits(adv).argmax(axis=1)[ok] != t[ok]).all()
    assert adv[~ok].tobytes() == np.clip(x[~ok], 0, 1).tobytes()
    m.close()


def test_generate_rejects_a_wrongly_shaped_input():
    m, _ = _model("F")
    with pytest.raises(ValueError, match="x must be"):
        nb.CarliniWagnerL2(m).generate(np.zeros((2, 28, 27, 1), np.float32))
    with pytest.raises(ValueError, match="x must be"):
        m.backward(np.zeros((2, 784), np.float32), np.zeros((2, 10), np.float32))
    m.close()


def test_targeted_celeba_shape_and_torch_stream():
    import torch
    m, params = _model("F", seed=3, input_shape=(None, 64, 64, 3))
    rs = np.random.RandomState(9)
    x = rs.uniform(-1, 1, (8, 64, 64, 3)).astype(np.float32)
    kw = dict(batch_size=4, learning_rate=0.05, binary_search_steps=2, max_iterations=10, abort_early=False, initial_const=10.0,
              clip_min=-1.0, clip_max=1.0)
    own = m.get_logits(x).argmax(axis=1)
    yt = (own + 1 + rs.randint(0, 9, 8)) % 10
    onehot = np.eye(10, dtype=np.float32)[yt]
    cw = nb.CarliniWagnerL2(m)
    adv, l2, cls = cw.generate(x, y_target=onehot, return_info=True, **kw)
    ref = _ref(m, params, x, labels=yt, targeted=True, **kw)
    assert (ref["best_class"] != -1).sum() >= 2
    np.testing.assert_array_equal(cls, ref["best_class"])
    assert ((cls == -1) | (cls == yt)).all()
    # one image may record its best one iteration apart (a success decided by a float32 / float64 margin near zero): all but
    # one match pixel for pixel, that one stays close in l2 and in every pixel's mean square
    np.testing.assert_allclose(l2, ref["best_l2"], rtol=5e-3)
    d = np.abs(adv - ref["x_adv"]).reshape(8, -1)
    assert ((d <= 1e-4).mean(axis=1) >= 0.999).sum() >= 7
    assert np.sqrt((d ** 2).mean(axis=1)).max() < 2e-3
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xt = torch.from_numpy(x).cuda()
        at, lt, ct = cw.generate(xt, y_target=torch.from_numpy(yt), return_info=True, **kw)
    s.synchronize()
    assert at.cpu().numpy().tobytes() == adv.tobytes() and lt.cpu().numpy().tobytes() == l2.tobytes()
    assert ct.cpu().numpy().tobytes() == cls.tobytes()
    m.close()
