"""-m gpu: the parts of dg_jsma.hip that tests/test_gpu_jsma.py does not execute -- sparse search domains (a thread with an empty
chunk, a wave whose total is 0, two features at the far end of the row), ties across lanes, trips and waves at D in the thousands,
clip ranges other than [0, 1], channels and non-square images, 200 classes, the C ABI's promises (a target that is no class, x_adv ==
x, each optional output NULL, an infinite pixel), the handle's state across calls and other attacks, and the early exit.  The inputs
are fixed in tests/support/jsma_reference.py; tests/test_jsma_edges_cpu.py shows on the CPU that each has the property it is chosen
for.  Every comparison is exact: x_adv in bits, the decisions as integers.  The linear families of section 1 have an exact oracle
and are compared on every image; the sets compared with the float64 reference keep tests/test_gpu_jsma.py's rule (the decidable
images, at least 75 % of each set).  Each test prints the figure it asserts."""
import numpy as np
import pytest
import torch

from defensegan_amd import _native, attacks, network_builder as nb
from tests.support import bpda_reference as R
from tests.support import jsma_reference as JR
from tests.test_gpu_jsma import KEYS, _bits, _check, _same
from tests.test_gpu_jsma import call as base_call

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def call(m, x, target, theta=1.0, max_iters=1, lo=0.0, hi=1.0, of_probs=1, x_off=0, out_off=0, inplace=False, null=()):
    """tests/test_gpu_jsma.py's call with the pointers under the test's control: x (x_adv) lies ``x_off`` (``out_off``) floats into a
    16-byte aligned buffer of its own, or x_adv is x itself; the outputs named in ``null`` are passed as NULL and left out of the dict."""
    dev = nb._ready(m)
    xs = np.ascontiguousarray(x, np.float32)
    B, N = int(xs.shape[0]), xs.size
    xbuf = torch.zeros(N + x_off, dtype=torch.float32, device=dev)
    xbuf[x_off:] = torch.from_numpy(xs.reshape(-1)).to(dev)
    obuf = xbuf if inplace else torch.zeros(N + out_off, dtype=torch.float32, device=dev)
    if inplace:
        out_off = x_off
    assert xbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    t = torch.from_numpy(np.ascontiguousarray(target, np.int32)).to(dev)
    out = {k: torch.full((B,), -7, dtype=torch.int32, device=dev) for k in ("iters", "final_class", "n_changed") if k not in null}
    ptr = {k: out[k].data_ptr() if k in out else None for k in ("iters", "final_class", "n_changed")}
    s = torch.cuda.current_stream(dev)
    lib = _native.load()
    _native.check(lib.dg_jsma(m._handle, xbuf.data_ptr() + 4 * x_off, t.data_ptr(), B, theta, max_iters, lo, hi, int(of_probs),
                              obuf.data_ptr() + 4 * out_off, ptr["iters"], ptr["final_class"], ptr["n_changed"], s.cuda_stream), lib)
    if max_iters > 0:
        out["choices"] = torch.empty(max_iters, B, 2, dtype=torch.int32, device=dev)
        _native.check(lib.dg_jsma_choices(m._handle, B, max_iters, out["choices"].data_ptr(), s.cuda_stream), lib)
    s.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["x_adv"] = obuf[out_off:].cpu().numpy().reshape(xs.shape)
    return res


def _exact(tag, got, want):
    """Every image against an exact expectation: the decisions as integers, x_adv in bits."""
    diff = int((_bits(got["x_adv"]) != _bits(np.asarray(want["x_adv"]).astype(np.float32))).sum())
    pairs = int((got["choices"] != want["choices"]).any(axis=2).sum())
    print("%s: %d images, iters %s, pairs that differ %d, elements of x_adv that differ in bits %d" %
          (tag, len(got["iters"]), got["iters"].tolist(), pairs, diff))
    assert pairs == 0 and diff == 0
    for k in ("iters", "n_changed", "final_class"):
        assert np.array_equal(got[k], want[k]), k


def _check_range(tag, got, ref, lo, hi, inside=True):
    """tests/test_gpu_jsma.py's _check for a clip range other than [0, 1]; ``inside`` = False where the images start outside it."""
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
    assert (got["n_changed"] <= 2 * got["iters"]).all() and np.isfinite(got["x_adv"]).all()
    if inside:
        assert got["x_adv"].min() >= lo and got["x_adv"].max() <= hi


def _edge_call(name, **kw):
    c = JR.EDGE_CASES[name]
    m, p, x, t = JR.edge_inputs(name)
    m.set_weights(p)
    got = call(m, x, t, c["theta"], c["max_iters"], c["lo"], c["hi"], c["of_probs"], **kw)
    m.close()
    return got, x


# ---------------------------------------------------------------------- 1. the pair search against an exact oracle, every image
@pytest.mark.parametrize("theta", JR.TIE_THETAS)
@pytest.mark.parametrize("F", sorted(JR.TIE_SHAPES))
def test_all_ties_the_pairs_are_the_domain_in_index_order(F, theta):
    """Every pair in the domain scores 4.0: step k must take (d[2k], d[2k + 1]) of the sorted domain, whatever threads and waves the
    pattern leaves empty."""
    m, p, x, t, doms = JR.tie_case(F, theta)
    m.set_weights(p)
    got = base_call(m, x, t, theta, JR.TIE_ITERS, 0.0, 1.0, 0)
    m.close()
    _exact("all ties, F %d, theta %g" % (F, theta), got, JR.tie_expected(x, doms, theta, JR.TIE_ITERS))


@pytest.mark.parametrize("F,n,theta", JR.DYADIC_CASES, ids=["F%d-n%d-th%g" % c for c in JR.DYADIC_CASES])
def test_dyadic_weights_many_ties(F, n, theta):
    m, p, x, t = JR.dyadic_case(F, n, theta)
    m.set_weights(p)
    got = base_call(m, x, t, theta, JR.DYADIC_ITERS, 0.0, 1.0, 0)
    m.close()
    _exact("dyadic, F %d, %d classes, theta %g" % (F, n, theta), got, JR.dyadic_run(F, n, theta))


# ---------------------------------------------------------------------- 2. sparse domains on the two-layer model
@pytest.mark.parametrize("name", JR.SPARSE_CASES)
def test_sparse_domains(name):
    c = JR.EDGE_CASES[name]
    got, x = _edge_call(name)
    _check(name, got, JR.edge_run(name), x)
    xf = x.reshape(len(x), -1)
    bound = 1.0 if c["theta"] > 0 else 0.0
    at_bound = sum(int((xf[i, got["choices"][:, i][got["choices"][:, i] >= 0]] == bound).sum()) for i in range(len(x)))
    print("%s: chosen features that started at the excluding bound %d, n_changed %s" % (name, at_bound, got["n_changed"].tolist()))
    assert at_bound == 0
    assert (got["n_changed"] == 2 * got["iters"]).all()


# ---------------------------------------------------------------------- 3. clip ranges
@pytest.mark.parametrize("name", [n for n in JR.RANGE_CASES if not n.startswith("unbounded")])
def test_clip_ranges(name):
    c = JR.EDGE_CASES[name]
    got, x = _edge_call(name)
    _check_range(name, got, JR.edge_run(name), c["lo"], c["hi"], inside=not c["outside"] and c["lo"] < c["hi"])          # lo == hi: the images lie around the point
    moved = _bits(got["x_adv"]) != _bits(x)
    if c["lo"] == c["hi"]:
        print("%s: %d elements moved, all to %g: %s" % (name, moved.sum(), c["lo"], bool((got["x_adv"][moved] == c["lo"]).all())))
        assert moved.any() and (got["x_adv"][moved] == c["lo"]).all()
        assert ((x[moved] < c["hi"]) if c["theta"] > 0 else (x[moved] > c["lo"])).all()
    if c["outside"]:
        away = (x < c["lo"]) | (x > c["hi"])
        print("%s: of %d elements outside the range %d are moved, %d keep their bits" % (name, away.sum(), (away & moved).sum(), (away & ~moved).sum()))
        assert (away & ~moved).any() and (away & moved).any()
        assert ((got["x_adv"][away & moved] >= c["lo"]) & (got["x_adv"][away & moved] <= c["hi"])).all()


@pytest.mark.parametrize("name", [n for n in JR.RANGE_CASES if n.startswith("unbounded")])
def test_no_clip_range_through_the_front_end(name):
    """clip_min = clip_max = None: the front end passes -inf and +inf, the domain is every finite feature and nothing is clipped."""
    c = JR.EDGE_CASES[name]
    m, p, x, t = JR.edge_inputs(name)
    m.set_weights(p)
    atk = attacks.SaliencyMapMethod(m)
    assert atk.max_iters(x[0].size, 1.0) == c["max_iters"]
    xa, it, fc, nc = atk.generate(x, y_target=t, theta=c["theta"], gamma=1.0, clip_min=None, clip_max=None, of_probs=False, return_info=True)
    ch = torch.empty(c["max_iters"], len(x), 2, dtype=torch.int32, device="cuda")
    lib = _native.load()
    _native.check(lib.dg_jsma_choices(m._handle, len(x), c["max_iters"], ch.data_ptr(), torch.cuda.current_stream().cuda_stream), lib)
    torch.cuda.synchronize()
    m.close()
    got = {"x_adv": xa, "iters": it, "final_class": fc, "n_changed": nc, "choices": ch.cpu().numpy()}
    _check_range(name, got, JR.edge_run(name), -JR.INF, JR.INF)
    print("%s: x_adv in [%g, %g]" % (name, xa.min(), xa.max()))
    assert (xa.max() == 1.5) if c["theta"] > 0 else (xa.min() == -1.5)          # a feature at the old bound moved on


# ---------------------------------------------------------------------- 4. channels, non-square images; 5. many classes
@pytest.mark.parametrize("name", JR.CONV_CASES + JR.MANY_CLASS_CASES)
def test_channels_non_square_images_and_many_classes(name):
    """The (p, q) themselves are compared: a feature index taken in another flatten order is another pair."""
    got, x = _edge_call(name)
    _check(name, got, JR.edge_run(name), x)


# ---------------------------------------------------------------------- 6. the C ABI's promises
@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in ("r16", "r16p", "r784"):
        c = JR.RUN_CASES[name]
        m, p, x, t = JR.case_inputs(c)
        m.set_weights(p)
        out[name] = dict(model=m, x=x, t=t, c=c, n=10)
    yield out
    torch.cuda.synchronize()
    for v in out.values():
        v["model"].close()


@pytest.mark.parametrize("case", ["r16", "r784"])
def test_a_target_that_is_no_class_leaves_its_image_alone(runs, case):
    v = runs[case]
    m, x, t, c = v["model"], v["x"], v["t"].copy(), v["c"]
    clean = base_call(m, x, t, c["theta"], 6, 0.0, 1.0, c["of_probs"])
    at_x = base_call(m, x, t, c["theta"], 0, 0.0, 1.0, c["of_probs"])["final_class"]
    bad = np.array([1, 3, 4, 6])
    t[bad] = (-1, v["n"], INT32_MIN, INT32_MAX)
    got = base_call(m, x, t, c["theta"], 6, 0.0, 1.0, c["of_probs"])
    ok = np.setdiff1d(np.arange(len(x)), bad)
    same = all(np.array_equal(_bits(got[k][ok]), _bits(clean[k][ok])) for k in KEYS) and np.array_equal(got["choices"][:, ok], clean["choices"][:, ok])
    print("%s: targets %s: iters %s, n_changed %s, final_class %s (the arg-max at x %s); the other images equal the clean run: %s" %
          (case, t[bad].tolist(), got["iters"][bad].tolist(), got["n_changed"][bad].tolist(), got["final_class"][bad].tolist(), at_x[bad].tolist(), same))
    assert np.array_equal(_bits(got["x_adv"][bad]), _bits(x[bad]))
    assert (got["iters"][bad] == 0).all() and (got["n_changed"][bad] == 0).all() and (got["choices"][:, bad] == -1).all()
    assert np.array_equal(got["final_class"][bad], at_x[bad])
    assert same and clean["iters"][ok].max() >= 2


@pytest.mark.parametrize("case", ["r16", "r784"])
def test_in_place_and_null_outputs(runs, case):
    v = runs[case]
    m, x, t, c = v["model"], v["x"], v["t"], v["c"]
    kw = dict(theta=c["theta"], max_iters=6, of_probs=c["of_probs"])
    full = call(m, x, t, **kw)
    assert _same(full, base_call(m, x, t, c["theta"], 6, 0.0, 1.0, c["of_probs"])) and full["n_changed"].max() >= 4
    for x_off in (0, 1):                                            # the float4 path where F % 4 == 0 and the scalar path
        got = call(m, x, t, x_off=x_off, inplace=True, **kw)
        print("%s: x_adv == x, %d floats off a 16-byte boundary: equal to the out-of-place call %s, n_changed %s" %
              (case, x_off, _same(full, got), got["n_changed"].tolist()))
        assert _same(full, got)
    assert _same(full, call(m, x, t, out_off=1, **kw)) and _same(full, call(m, x, t, x_off=2, out_off=3, **kw))
    for name in ("iters", "final_class", "n_changed"):
        got = call(m, x, t, null=(name,), **kw)
        print("%s: %s NULL, the other outputs equal the full call: %s" % (case, name, _same(full, got, [k for k in KEYS + ("choices",) if k != name])))
        assert name not in got and _same(full, got, [k for k in KEYS + ("choices",) if k != name])


@pytest.mark.parametrize("of_probs", [0, 1])
@pytest.mark.parametrize("sign", [1, -1])
def test_an_infinite_pixel(sign, of_probs):
    """On the logits the image goes on (its infinite logits have a first arg-max that is not the target, its gradients are the weights,
    the pixel is outside the domain); on softmax its outputs are NaN and it stops where it is.  Its neighbours are the clean run's."""
    m, p, bad, x, t, theta = JR.inf_case(sign)
    i = JR.INF_PIXEL[0]
    ref = JR.run(m, p, bad, t, theta, JR.INF_ITERS, 0.0, 1.0, bool(of_probs))
    m.set_weights(p)
    clean = base_call(m, x, t, theta, JR.INF_ITERS, 0.0, 1.0, of_probs)
    got = base_call(m, bad, t, theta, JR.INF_ITERS, 0.0, 1.0, of_probs)
    m.close()
    print("pixel %g, of_probs %d: pairs %s (reference %s), iters %d, final_class %d (reference %d), n_changed %d" %
          (sign * JR.INF, of_probs, got["choices"][:, i].tolist(), ref["choices"][:, i].tolist(), got["iters"][i], got["final_class"][i],
           ref["final_class"][i], got["n_changed"][i]))
    assert (ref["iters"][i] == 0) if of_probs else (ref["iters"][i] >= 2)
    assert np.array_equal(got["choices"][:, i], ref["choices"][:, i])
    for k in ("iters", "final_class", "n_changed"):
        assert got[k][i] == ref[k][i], k
    assert np.array_equal(_bits(got["x_adv"][i]), _bits(ref["x_adv"][i].astype(np.float32)))
    assert got["x_adv"][i].reshape(-1)[JR.INF_PIXEL[1]] == sign * JR.INF
    for j in (0, 2, 3):
        assert all(np.array_equal(_bits(got[k][j]), _bits(clean[k][j])) for k in KEYS) and np.array_equal(got["choices"][:, j], clean["choices"][:, j])


# ---------------------------------------------------------------------- 7. the handle's state
def test_handle_state_across_calls_attacks_and_weights():
    shape = (28, 28, 1)
    m = JR.model_of("mlp10", shape)
    p, p2 = R.init_params(m, 7), R.init_params(m, 8)
    x = JR.sparse_images(65, shape, 31)
    t = JR.targets(m, p, x, 32)
    t2 = JR.targets(m, p2, x, 33)
    lib = _native.load()

    def fresh(params, *args):
        f = JR.model_of("mlp10", shape)
        f.set_weights(params)
        out = base_call(f, *args)
        f.close()
        return out
    m.set_weights(p)
    seen = []
    for B, it in ((65, 5), (3, 2)):                                 # a big call, then a small one on its stale dom, flags and choices
        args = (x[:B], t[:B], 1.0, it, 0.0, 1.0, 1)
        seen.append(_same(base_call(m, *args), fresh(p, *args)))
    attacks.DeepFool(m).generate(x[:4], max_iter=3)                 # rewrites the handle's activations and gradient buffer
    got = base_call(m, x[:3], t[:3], 1.0, 0, 0.0, 1.0, 1)
    seen.append(_same(got, fresh(p, x[:3], t[:3], 1.0, 0, 0.0, 1.0, 1)))
    ch = torch.empty(1, 3, 2, dtype=torch.int32, device="cuda")
    rc = lib.dg_jsma_choices(m._handle, 3, 1, ch.data_ptr(), None)
    assert rc == -2 and b"max_iters = 1" in lib.dg_last_error()     # DG_E_STATE: the last call had max_iters = 0
    attacks.CarliniWagnerL2(m).generate(x[:4], batch_size=4, binary_search_steps=1, max_iterations=1)
    args = (x[:8], t[:8], -1.0, 7, 0.0, 1.0, 0)
    seen.append(_same(base_call(m, *args), fresh(p, *args)))
    m.set_weights(p2)                                               # new weights on the used handle
    args = (x[:8], t2[:8], -1.0, 7, 0.0, 1.0, 0)
    after = base_call(m, *args)
    seen.append(_same(after, fresh(p2, *args)))
    m.close()
    print("every dg_jsma call on the used handle equals the same call on a fresh one: %s; iters after the new weights %s" % (seen, after["iters"].tolist()))
    assert all(seen) and len(seen) == 5 and after["iters"].max() >= 2


# ---------------------------------------------------------------------- 8. the early exit and the prefixes
@pytest.mark.parametrize("case", ["r16p", "r784"])
def test_a_shorter_run_is_a_prefix_of_a_longer_one(runs, case):
    v = runs[case]
    m, x, t, c = v["model"], v["x"], v["t"], v["c"]
    full = base_call(m, x, t, c["theta"], 6, 0.0, 1.0, c["of_probs"])
    assert full["iters"].max() == 6
    for k in range(1, 7):
        got = base_call(m, x, t, c["theta"], k, 0.0, 1.0, c["of_probs"])
        want = JR.replay(x, full["choices"][:k], c["theta"], 0.0, 1.0)
        diff = int((_bits(got["x_adv"]) != _bits(want)).sum())
        print("%s, max_iters %d: pairs equal to the first rows of the 6-iteration run %s, elements of x_adv off the host replay %d" %
              (case, k, np.array_equal(got["choices"], full["choices"][:k]), diff))
        assert np.array_equal(got["choices"], full["choices"][:k]) and diff == 0
        assert np.array_equal(got["iters"], (full["choices"][:k, :, 0] >= 0).sum(axis=0))
        assert np.array_equal(got["n_changed"], (want != x).reshape(len(x), -1).sum(axis=1))
    assert _same(got, full)


@pytest.mark.parametrize("steps", [1, 2])
def test_the_early_exit_on_either_parity(steps):
    """A batch whose images all reach their target after exactly ``steps`` steps: the loop reads the active count after iterations 2
    and 4, so the batch of 1 leaves at the first read and the batch of 2 at the second.  From max_iters = steps on nothing changes."""
    m, p, x, t, ref, bat = JR.exit_batches()
    idx = bat[steps]
    m.set_weights(p)
    out = [base_call(m, x[idx], t[idx], 1.0, k, 0.0, 1.0, 0) for k in range(1, 6)]
    m.close()
    first = out[steps - 1]
    print("%d images done after %d steps: iters by max_iters %s" % (len(idx), steps, [o["iters"].tolist() for o in out]))
    assert len(idx) >= 1
    for k in range(steps, 6):
        got = out[k - 1]
        assert all(np.array_equal(_bits(got[key]), _bits(first[key])) for key in KEYS), k
        assert np.array_equal(got["choices"][:steps], first["choices"]) and (got["choices"][steps:] == -1).all()
        assert np.array_equal(got["choices"], ref["choices"][:k, idx])
    for key in ("iters", "final_class", "n_changed"):
        assert np.array_equal(first[key], ref[key][idx]), key
    assert (first["iters"] == steps).all() and (first["final_class"] == t[idx]).all()
    assert np.array_equal(_bits(first["x_adv"]), _bits(ref["x_adv"][idx].astype(np.float32)))
    if steps == 2:
        assert (out[0]["iters"] == 1).all() and np.array_equal(out[0]["choices"], first["choices"][:1])
