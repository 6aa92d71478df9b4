"""-m gpu: the Jacobian saliency-map attack in one device call (dg_jsma, attacks.SaliencyMapMethod) against the float64 restatement in
tests/support/jsma_reference.py, its rules, bitwise identities, strided loops and refusals.  The input sets are fixed on the CPU
(tests/test_jsma_cpu.py asserts that at least 75 % of the images of each are decidable); the decisions -- the (p, q) sequence, iters,
final_class, n_changed -- and x_adv, bit for bit (every change is +-theta followed by a clip: no tolerance), are compared on the
decidable images, the others are checked for finiteness and the clip range.  Each test prints the figure it is about to assert."""
import numpy as np
import pytest
import torch

from defensegan_amd import _native, attacks, network_builder as nb
from tests.support import jsma_reference as JR

pytestmark = pytest.mark.gpu

KEYS = ("x_adv", "iters", "final_class", "n_changed")


def call(m, x, target, theta=1.0, max_iters=1, lo=0.0, hi=1.0, of_probs=1, stream=None, x_off=0):
    """One dg_jsma call through the C ABI; x lies ``x_off`` floats into a 16-byte aligned buffer.  A dict of NumPy arrays (x_adv, iters,
    final_class, n_changed, choices [max_iters, B, 2])."""
    dev = nb._ready(m)
    xs = np.ascontiguousarray(x, np.float32)
    B = int(xs.shape[0])
    xbuf = torch.zeros(xs.size + x_off, dtype=torch.float32, device=dev)
    xbuf[x_off:] = torch.from_numpy(xs.reshape(-1)).to(dev)
    assert xbuf.data_ptr() % 16 == 0
    t = torch.from_numpy(np.ascontiguousarray(target, np.int32)).to(dev)
    out = {"x_adv": torch.empty(xs.shape, dtype=torch.float32, device=dev), "iters": torch.empty(B, dtype=torch.int32, device=dev),
           "final_class": torch.empty(B, dtype=torch.int32, device=dev), "n_changed": torch.empty(B, dtype=torch.int32, device=dev)}
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    lib = _native.load()
    with torch.cuda.stream(s):
        _native.check(lib.dg_jsma(m._handle, xbuf.data_ptr() + 4 * x_off, t.data_ptr(), B, theta, max_iters, lo, hi, int(of_probs),
                                  out["x_adv"].data_ptr(), out["iters"].data_ptr(), out["final_class"].data_ptr(), out["n_changed"].data_ptr(),
                                  s.cuda_stream), lib)
        if max_iters > 0:
            out["choices"] = torch.empty(max_iters, B, 2, dtype=torch.int32, device=dev)
            _native.check(lib.dg_jsma_choices(m._handle, B, max_iters, out["choices"].data_ptr(), s.cuda_stream), lib)
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, keys=KEYS + ("choices",)):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys if k in a or k in b)


def _case_call(c, m, x, t):
    F = int(np.prod(c["shape"]))
    it = c["max_iters"] if c["max_iters"] is not None else int(np.floor(F * c["gamma"] / 2))
    return call(m, x, t, c["theta"], it, 0.0, 1.0, c["of_probs"])


def _check(tag, got, ref, x):
    """The comparison of tests 1 and 2: decisions and x_adv's bits on the decidable images, range and finiteness on all."""
    dec = JR.decidable(ref)
    want = ref["x_adv"].astype(np.float32)
    diff = int((_bits(got["x_adv"])[dec] != _bits(want)[dec]).sum())
    print("%s: decidable %d/%d, iters up to %d, elements of x_adv that differ in bits on the decidable images: %d" %
          (tag, dec.sum(), dec.size, got["iters"].max(), diff))
    assert dec.mean() >= 0.75
    assert (got["choices"][:, dec] == ref["choices"][:, dec]).all()
    for k in ("iters", "final_class", "n_changed"):
        assert (got[k][dec] == ref[k][dec]).all(), k
    assert diff == 0
    assert (got["n_changed"] <= 2 * got["iters"]).all()
    assert np.isfinite(got["x_adv"]).all() and got["x_adv"].min() >= 0.0 and got["x_adv"].max() <= 1.0


# ---------------------------------------------------------------------- 1. one iteration, value for value
@pytest.mark.parametrize("c", JR.STEP_CASES, ids=lambda c: "%s-%dx%d-B%d-th%g-p%d" % (c["model"], c["shape"][0], c["shape"][1], c["B"], c["theta"], c["of_probs"]))
def test_one_iteration_value_for_value(c):
    m, p, x, t = JR.case_inputs(c)
    m.set_weights(p)
    got = _case_call(c, m, x, t)
    m.close()
    _check("one iteration", got, JR.case_run(c), x)
    assert (got["iters"] <= 1).all()


# ---------------------------------------------------------------------- 2. whole runs
@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, c in JR.RUN_CASES.items():
        m, p, x, t = JR.case_inputs(c)
        m.set_weights(p)
        out[name] = dict(model=m, x=x, t=t, c=c)
    yield out
    torch.cuda.synchronize()
    for v in out.values():
        v["model"].close()


@pytest.mark.parametrize("case", sorted(JR.RUN_CASES))
def test_whole_run(runs, case):
    v = runs[case]
    got = _case_call(v["c"], v["model"], v["x"], v["t"])
    _check(case, got, JR.case_run(case), v["x"])


# ---------------------------------------------------------------------- 3. the rules
def _lin(n, shape=(4, 4, 1)):
    return nb.MLP([nb.Flatten(), nb.Linear(n), nb.Softmax()], input_shape=(None,) + shape)


def test_a_tie_goes_to_the_lower_index():
    """Features 2, 5 and 9 share their weight row, the strongest towards the target (class 0's bias keeps every image away from it):
    the pairs (2, 5), (2, 9) and (5, 9) score the same bits -- in three lanes of two waves -- and (2, 5) is taken; the whole run is the
    reference's, ties included."""
    rs = np.random.RandomState(4)
    W = (0.1 * rs.standard_normal((16, 3))).astype(np.float32)
    W[2] = W[5] = W[9] = np.array([-1.0, 2.0, -1.5], np.float32)
    p = [(W, np.array([10.0, 0.0, 0.0], np.float32))]
    x = JR.images(12, (4, 4, 1), 3)
    t = np.ones(12, np.int32)
    m = _lin(3)
    m.set_weights(p)
    got = call(m, x, t, 0.25, 8, 0.0, 1.0, 0)
    m.close()
    ref = JR.run(m, p, x, t, 0.25, 8, 0.0, 1.0, False)
    print("first pairs %s" % got["choices"][0].tolist())
    moved = got["iters"] >= 1
    assert moved.any() and (got["choices"][0][moved] == (2, 5)).all()
    assert (got["choices"] == ref["choices"]).all() and (got["iters"] == ref["iters"]).all()
    assert np.array_equal(_bits(got["x_adv"]), _bits(ref["x_adv"].astype(np.float32)))


def test_images_that_take_no_step():
    rs = np.random.RandomState(5)
    x = JR.images(4, (4, 4, 1), 6)
    m = _lin(4)
    # a model with zero gradients: no admissible pair, the image stops where it is
    m.set_weights([(np.zeros((16, 4), np.float32), np.array([0.1, 0.4, 0.2, 0.3], np.float32))])
    for of_probs in (0, 1):
        got = call(m, x, np.zeros(4, np.int32), 1.0, 3, 0.0, 1.0, of_probs)
        assert np.array_equal(_bits(got["x_adv"]), _bits(x)) and (got["iters"] == 0).all() and (got["choices"] == -1).all()
        assert (got["final_class"] == 1).all() and (got["n_changed"] == 0).all()
    W = rs.standard_normal((16, 4)).astype(np.float32)
    m.set_weights([(W, np.zeros(4, np.float32))])
    own = (x.reshape(4, 16).astype(np.float64) @ W.astype(np.float64)).argmax(axis=1).astype(np.int32)
    # an image already of class t is untouched; its neighbour with another target moves
    t = own.copy()
    t[1] = (own[1] + 1) % 4
    got = call(m, x, t, 1.0, 8, 0.0, 1.0, 0)
    for i in (0, 2, 3):
        assert np.array_equal(_bits(got["x_adv"][i]), _bits(x[i])) and got["iters"][i] == 0 and (got["choices"][:, i] == -1).all()
    assert got["iters"][1] >= 1 and got["n_changed"][1] == 2 * got["iters"][1]
    # fewer than 2 features below clip_max: untouched, whatever the target
    sat = np.ones((2, 4, 4, 1), np.float32)
    sat[0, 1, 1, 0] = 0.25
    own_s = (sat.reshape(2, 16).astype(np.float64) @ W.astype(np.float64)).argmax(axis=1)
    got = call(m, sat, ((own_s + 1) % 4).astype(np.int32), 1.0, 8, 0.0, 1.0, 0)
    assert np.array_equal(_bits(got["x_adv"]), _bits(sat)) and (got["iters"] == 0).all() and (got["choices"] == -1).all()
    # max_iters = 0
    got = call(m, x, t, 1.0, 0, 0.0, 1.0, 1)
    m.close()
    assert np.array_equal(_bits(got["x_adv"]), _bits(x)) and (got["iters"] == 0).all() and (got["n_changed"] == 0).all()
    assert (got["final_class"] == own).all()


def test_a_nan_pixel_stops_its_image_and_leaves_the_others_alone(runs):
    v = runs["r784p"]
    x, t, c = v["x"][:3].copy(), v["t"][:3], v["c"]
    clean = call(v["model"], x, t, c["theta"], 39, 0.0, 1.0, c["of_probs"])
    x[1, 3, 3, 0] = np.nan
    got = call(v["model"], x, t, c["theta"], 39, 0.0, 1.0, c["of_probs"])
    for i in (0, 2):
        assert all(np.array_equal(_bits(got[k][i]), _bits(clean[k][i])) for k in KEYS) and (got["choices"][:, i] == clean["choices"][:, i]).all()
        assert np.isfinite(got["x_adv"][i]).all()
    assert got["iters"][1] == 0 and (got["choices"][:, 1] == -1).all() and got["n_changed"][1] == 0
    assert np.array_equal(_bits(got["x_adv"][1]), _bits(x[1]))


# ---------------------------------------------------------------------- 4. independence, bit for bit
def test_bitwise_identities():
    c = dict(JR.STEP_CASES[8], max_iters=5)                         # the two-layer model on 28 x 28, B = 65, softmax outputs
    assert c["B"] == 65 and c["shape"] == (28, 28, 1)
    m, p, x, t = JR.case_inputs(c)
    m.set_weights(p)
    full = _case_call(c, m, x, t)
    assert full["iters"].max() == 5
    assert _same(full, _case_call(c, m, x, t))                      # two identical calls
    for i in (0, 1, 37, 64):                                        # alone and inside B = 65
        one = _case_call(c, m, x[i:i + 1], t[i:i + 1])
        assert all(np.array_equal(_bits(one[k][0]), _bits(full[k][i])) for k in KEYS), i
        assert (one["choices"][:, 0] == full["choices"][:, i]).all()
    atk = attacks.SaliencyMapMethod(m)
    gamma = 0.013                                                   # floor(784 * 0.013 / 2) = 5
    assert atk.max_iters(784, gamma) == 5
    for bs in (None, 4, 64):                                        # generate's chunkings
        xa, it, fc, nc = atk.generate(x, y_target=t, gamma=gamma, batch_size=bs, return_info=True)
        assert _same(full, {"x_adv": xa, "iters": it, "final_class": fc, "n_changed": nc}, KEYS), bs
    side = torch.cuda.Stream()
    assert _same(full, call(m, x, t, c["theta"], 5, 0.0, 1.0, c["of_probs"], stream=side))          # a side stream, synchronised by the caller
    out = atk.generate(torch.from_numpy(x).cuda(), y_target=np.eye(10, dtype=np.float32)[t], gamma=gamma)          # one-hot targets, a device tensor
    assert isinstance(out, torch.Tensor) and np.array_equal(_bits(out.cpu().numpy()), _bits(full["x_adv"]))
    m.close()


# ---------------------------------------------------------------------- 5. strides, alignment, the feature cap
def test_tiled_past_both_grid_caps_every_tile_is_the_base_run():
    """67 images of a linear model on 4 x 4, two iterations, image 0 with its own class as the target (inactive: the early continue),
    first against the float64 reference, then tiled to B = 65538: workgroups 0 and 1 of the image-strided kernels take a second image
    (base images 10 and 11, on the LDS their first image left behind) and the wave-strided kernels make five trips.  Every image works
    alone, so every tile must be the base run bit for bit."""
    c = JR.TILE_CASE
    m, p, x, t = JR.case_inputs(c)
    ref0 = JR.run(m, p, x, t, c["theta"], 0, 0.0, 1.0, False)
    t = t.copy()
    t[0] = ref0["final_class"][0]
    ref = JR.run(m, p, x, t, c["theta"], c["max_iters"], 0.0, 1.0, False, shadow=torch.float32)
    m.set_weights(p)
    base = call(m, x, t, c["theta"], c["max_iters"], 0.0, 1.0, 0)
    _check("tile base", base, ref, x)
    assert base["iters"][0] == 0 and (base["choices"][:, 0] == -1).all() and base["iters"].max() == 2
    B, n = JR.TILE_B, len(x)
    sel = np.arange(B) % n
    got = call(m, x[sel], t[sel], c["theta"], c["max_iters"], 0.0, 1.0, 0)
    m.close()
    assert B > JR.IMAGE_CAP and B > JR.WAVE_CAP and JR.IMAGE_CAP % n == 10
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(base[k])[sel]), k
    assert np.array_equal(got["choices"], base["choices"][:, sel])


def test_an_unaligned_x_takes_the_scalar_path_to_the_same_bits(runs):
    v = runs["r784"]
    c = v["c"]
    a = call(v["model"], v["x"], v["t"], c["theta"], 39, 0.0, 1.0, c["of_probs"])
    b = call(v["model"], v["x"], v["t"], c["theta"], 39, 0.0, 1.0, c["of_probs"], x_off=1)          # 4 bytes off a 16-byte boundary
    assert a["iters"].max() > 1 and _same(a, b)


def test_the_feature_cap_runs_and_one_more_is_refused():
    """F = 5120 = JSMA_MAX_FEATURES, the largest LDS the pair kernel asks for: a two-class linear model whose target column is w and whose
    other column is -w, so a = w, b = -w and the score of (p, q) is (w_p + w_q)^2 -- the pair is the two largest w, put at the very end
    of the row (features 5117 and 5119).  One feature more is refused."""
    F = 5120
    rs = np.random.RandomState(7)
    w = rs.uniform(0.0, 1.0, F).astype(np.float32)
    w[5117], w[5119] = 3.0, 2.0
    m = _lin(2, (64, 80, 1))
    m.set_weights([(np.stack([-w, w], axis=1), np.array([50000.0, 0.0], np.float32))])
    x = JR.images(2, (64, 80, 1), 8)
    x[1].reshape(-1)[5119] = 1.0                                    # image 1: feature 5119 is outside the domain, 5118 is not
    w1 = w.copy()
    w1[5119] = -1.0
    second = int(np.argmax(np.where(np.arange(F) == 5117, -1.0, w1)))
    got = call(m, x, np.ones(2, np.int32), 1.0, 1, 0.0, 1.0, 0)
    m.close()
    print("pairs at F = 5120: %s (image 1 expects (%d, %d) in some order)" % (got["choices"][0].tolist(), 5117, second))
    assert got["choices"][0][0].tolist() == [5117, 5119]
    assert got["choices"][0][1].tolist() == sorted([5117, second])
    assert (got["iters"] == 1).all() and (got["n_changed"] == 2).all()
    big = _lin(2, (72, 72, 1))
    big.set_weights([(np.zeros((5184, 2), np.float32), np.zeros(2, np.float32))])
    lib = _native.load()
    xb = torch.zeros(1, 72, 72, 1, device="cuda")
    tb = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.dg_jsma(big._handle, xb.data_ptr(), tb.data_ptr(), 1, 1.0, 1, 0.0, 1.0, 0, xb.data_ptr(), None, None, None, None) == -1
    assert b"not implemented for more than" in lib.dg_last_error()
    big.close()


# ---------------------------------------------------------------------- 6. refusals
def test_refusals(runs):
    lib = _native.load()
    v = runs["r16"]
    m = v["model"]
    x = torch.from_numpy(v["x"][:3]).cuda()
    t = torch.from_numpy(v["t"][:3]).cuda()
    o = torch.empty_like(x)
    h, X, T, O = m._handle, x.data_ptr(), t.data_ptr(), o.data_ptr()

    def rc(handle=h, x=X, target=T, B=3, theta=1.0, it=2, lo=0.0, hi=1.0, probs=1, out=O):
        return lib.dg_jsma(handle, x, target, B, theta, it, lo, hi, probs, out, None, None, None, None)
    assert rc() == 0                                                # the optional outputs may be NULL
    torch.cuda.synchronize()
    for kw, word in ((dict(handle=None), b"null"), (dict(x=None), b"null"), (dict(target=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=0), b"B must be >= 1"), (dict(theta=0.0), b"theta"), (dict(theta=float("inf")), b"theta"),
                     (dict(theta=float("nan")), b"theta"), (dict(it=-1), b"max_iters"), (dict(lo=1.0, hi=0.0), b"clip_min"),
                     (dict(probs=2), b"of_probs"), (dict(probs=-1), b"of_probs")):
        assert rc(**kw) == -1 and word in lib.dg_last_error(), kw
    one = _lin(2, (1, 1, 1))                                        # F < 2
    one.set_weights([(np.ones((1, 2), np.float32), np.zeros(2, np.float32))])
    assert rc(handle=one._handle) == -1 and b"at least 2 features" in lib.dg_last_error()
    one.close()
    bare = JR.model_of("mlp10", (4, 4, 1))
    bare._ensure()
    assert rc(handle=bare._handle) == -2 and b"has no weights" in lib.dg_last_error()          # DG_E_STATE
    bare.close()
    ch = torch.empty(3, 3, 2, dtype=torch.int32, device="cuda")
    assert lib.dg_jsma_choices(h, 3, 3, ch.data_ptr(), None) == -2                              # the last call had max_iters = 2
    atk = attacks.SaliencyMapMethod(m)
    with pytest.raises(ValueError, match="outside"):
        atk.generate(v["x"][:3], y_target=np.array([0, 10, 1]))
    with pytest.raises(ValueError, match="class indices"):
        atk.generate(v["x"][:3], y_target=np.array([0, 1]))
    with pytest.raises(ValueError, match="x must be"):
        atk.generate(v["x"][:3, :3], y_target=np.array([0, 1, 2]))


# ---------------------------------------------------------------------- 7. it reaches the target
def test_success_rate_and_l0_on_model_f_are_the_references(runs):
    """Model F at synthetic weights, on its logits, theta 1, gamma 0.1: the success rate and the mean n_changed equal the float64
    reference's on the reference's image set (every image of it is decidable: tests/test_jsma_cpu.py)."""
    v = runs["F28"]
    ref = JR.case_run("F28")
    got = _case_call(v["c"], v["model"], v["x"], v["t"])
    ok, ok_ref = got["final_class"] == v["t"], ref["final_class"] == ref["target"]
    print("model F, logits, theta 1, gamma 0.1, %d images: success rate %.4f (reference %.4f), mean n_changed %.4f (reference %.4f), "
          "mean n_changed / F on the successful images %.5f" % (len(ok), ok.mean(), ok_ref.mean(), got["n_changed"].mean(), ref["n_changed"].mean(),
                                                               (got["n_changed"][ok] / 784.0).mean() if ok.any() else float("nan")))
    assert JR.decidable(ref).all()
    assert ok.mean() == ok_ref.mean() and got["n_changed"].mean() == ref["n_changed"].mean()
    assert ok.mean() > 0
