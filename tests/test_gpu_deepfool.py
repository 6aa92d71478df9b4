"""-m gpu: DeepFool in one device call (dg_deepfool, attacks.DeepFool) against the float64 restatement in
tests/support/deepfool_reference.py, its degenerate inputs, bitwise identities and refusals.  The input sets are fixed on the CPU
(tests/test_deepfool_cpu.py asserts that at least 75 % of the images of each are decidable); decisions -- final_class, iters, the j*
sequence -- are compared on the decidable images, the others are checked for finiteness and the clip range.  Each test prints the
figure it is about to assert (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest
import torch

from defensegan_amd import _native, attacks, network_builder as nb
from tests.support import deepfool_reference as DR

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4          # tests/test_gpu_gen_train.py's gradient bound: of the largest entry of the reference
NORM_TOL = 1e-4          # r_norm against the reference, relative
# r_norm against ||x_adv - x||_2 recomputed on the host in float64: a float32 sum of P <= 784 squares in a fixed tree order carries
# at most about sqrt(P) half-ulps of relative error, and the square root halves it: 28 * 6e-8 / 2 < 1e-6; 1e-5 leaves a factor 10
HOST_NORM_TOL = 1e-5


def _device_model(name, shape, params):
    m = DR.model_of(name, shape)
    m.set_weights(params)
    return m


def call(m, x, nc=10, overshoot=0.02, max_iter=50, lo=0.0, hi=1.0, stream=None, choices=True, lib=None):
    """One dg_deepfool call through the C ABI; a dict of NumPy arrays (x_adv, r_norm, iters, final_class, choices [max_iter, B])."""
    dev = nb._ready(m)
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    B = int(t.shape[0])
    out = {"x_adv": torch.empty_like(t), "r_norm": torch.empty(B, dtype=torch.float32, device=dev),
           "iters": torch.empty(B, dtype=torch.int32, device=dev), "final_class": torch.empty(B, dtype=torch.int32, device=dev)}
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    lib = lib or _native.load()
    with torch.cuda.stream(s):
        _native.check(lib.dg_deepfool(m._handle, t.data_ptr(), B, nc, overshoot, max_iter, lo, hi, out["x_adv"].data_ptr(),
                                      out["r_norm"].data_ptr(), out["iters"].data_ptr(), out["final_class"].data_ptr(), s.cuda_stream), lib)
        if choices and max_iter > 0:
            out["choices"] = torch.empty(max_iter, B, dtype=torch.int32, device=dev)
            _native.check(lib.dg_deepfool_choices(m._handle, B, max_iter, out["choices"].data_ptr(), s.cuda_stream), lib)
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def runs():
    """The whole-run cases' models on the device with their inputs; the float64 runs are DR.case_run's cache."""
    out = {}
    for name, c in DR.RUN_CASES.items():
        m, p, x = DR.case_inputs(name)
        m.set_weights(p)
        out[name] = dict(model=m, x=x, nc=c["nc"])
    yield out
    torch.cuda.synchronize()
    for v in out.values():
        v["model"].close()


def _same(a, b, keys=("x_adv", "r_norm", "iters", "final_class")):
    return all(np.array_equal(a[k].view(np.int32) if a[k].dtype == np.float32 else a[k], b[k].view(np.int32) if b[k].dtype == np.float32 else b[k])
               for k in keys)


# ---------------------------------------------------------------------- 1. one step, value for value
@pytest.mark.parametrize("name,shape,B,nc", DR.STEP_CASES)
def test_one_step_value_for_value(name, shape, B, nc):
    """max_iter = 1, overshoot = 0: x_adv - x against the reference's step on the images whose candidates and j* are decidable,
    within GRAD_TOL of the largest entry of the reference's r."""
    m, p, x = DR.case_inputs(dict(model=name, shape=shape, B=B, **DR.STEP_SEEDS))
    m.set_weights(p)
    ref = DR.run(m, p, x, nc, 0.0, 1, 0.0, 1.0, shadow=torch.float32)
    dec = DR.decidable(ref)
    got = call(m, x, nc, 0.0, 1)
    m.close()
    bound = GRAD_TOL * np.abs(ref["r_tot"]).max()
    d = np.abs((got["x_adv"].astype(np.float64) - x) - (ref["x_adv"] - x))[dec].max()
    print("%s %s B %d nc %d: decidable %d/%d, max |d r| %.3e, bound %.3e, share of the bound used %.4f" %
          (name, shape, B, nc, dec.sum(), B, d, bound, d / bound))
    assert dec.mean() >= 0.75
    assert (got["choices"][0][dec] == ref["choices"][0][dec]).all() and (got["iters"][dec] == ref["iters"][dec]).all()
    assert d <= bound
    assert np.isfinite(got["x_adv"]).all() and got["x_adv"].min() >= 0.0 and got["x_adv"].max() <= 1.0


# ---------------------------------------------------------------------- 2. whole runs
@pytest.mark.parametrize("case", sorted(DR.RUN_CASES))
@pytest.mark.parametrize("max_iter", [50, 3])
def test_whole_run(runs, case, max_iter):
    v = runs[case]
    ref = DR.case_run(case, max_iter)
    dec = DR.decidable(ref)
    got = call(v["model"], v["x"], v["nc"], 0.02, max_iter)
    rel = np.abs(got["r_norm"][dec] - ref["r_norm"][dec]) / ref["r_norm"][dec]
    host = np.sqrt(np.square(got["x_adv"].astype(np.float64) - v["x"]).reshape(len(dec), -1).sum(axis=1))
    hrel = np.abs(got["r_norm"] - host) / np.maximum(host, 1e-30)
    print("%s max_iter %d: decidable %d/%d, max rel r_norm error %.3e (bound %.0e), against the host %.3e (bound %.0e), iters up to %d" %
          (case, max_iter, dec.sum(), dec.size, rel.max(), NORM_TOL, hrel.max(), HOST_NORM_TOL, got["iters"].max()))
    assert dec.mean() >= 0.75
    assert (got["final_class"][dec] == ref["final_class"][dec]).all()
    assert (got["iters"][dec] == ref["iters"][dec]).all()
    assert (got["choices"][:, dec] == ref["choices"][:, dec]).all()
    assert rel.max() <= NORM_TOL
    assert hrel.max() <= HOST_NORM_TOL
    assert np.isfinite(got["x_adv"]).all() and np.isfinite(got["r_norm"]).all()
    assert got["x_adv"].min() >= 0.0 and got["x_adv"].max() <= 1.0


# ---------------------------------------------------------------------- 3. ties and degenerate inputs
def _lin(n, shape=(4, 4, 1)):
    return nb.MLP([nb.Flatten(), nb.Linear(n), nb.Softmax()], input_shape=(None,) + shape)


def test_ties_and_a_zero_difference():
    """Classes 1 and 2 share their last-layer row.  An image whose orig is 0 sees pert_1 == pert_2 and takes the lower rank, 1; an
    image whose orig is 1 has class 2 at rank 1 with f = 0 and w exactly 0 (pert = +inf) and takes rank 2, class 0."""
    rs = np.random.RandomState(4)
    W = rs.standard_normal((16, 3)).astype(np.float32)
    W[:, 2] = W[:, 1]
    p = [(W, np.zeros(3, np.float32))]
    x = rs.uniform(0, 1, (12, 4, 4, 1)).astype(np.float32)
    m = _lin(3)
    m.set_weights(p)
    got = call(m, x, 3, 0.02, 50, -np.inf, np.inf)
    m.close()
    ref = DR.run(m, p, x, 3, 0.02, 50, -np.inf, np.inf)
    print("orig %s, first choices %s" % (ref["orig"].tolist(), got["choices"][0].tolist()))
    assert set(ref["orig"].tolist()) == {0, 1}                      # both situations occur
    assert (got["choices"][0][ref["orig"] == 0] == 1).all() and (got["choices"][0][ref["orig"] == 1] == 2).all()
    assert (got["choices"] == ref["choices"]).all() and (got["iters"] == ref["iters"]).all()
    assert (got["final_class"] == ref["final_class"]).all()
    assert (got["final_class"][ref["orig"] == 0] == 1).all() and (got["final_class"][ref["orig"] == 1] == 0).all()


def test_constant_model_max_iter_zero_and_overshoot():
    rs = np.random.RandomState(5)
    x = rs.uniform(-0.5, 1.5, (3, 4, 4, 1)).astype(np.float32)
    m = _lin(4)
    m.set_weights([(np.zeros((16, 4), np.float32), np.array([0.1, 0.4, 0.2, 0.3], np.float32))])
    got = call(m, x, 4, 0.02, 5)                                    # every w_j is zero: no step, one counted iteration, then inactive
    assert np.array_equal(got["x_adv"], np.clip(x, 0, 1)) and (got["iters"] == 1).all() and (got["choices"] == -1).all()
    assert (got["final_class"] == 1).all()
    m.set_weights([(rs.standard_normal((16, 4)).astype(np.float32), np.zeros(4, np.float32))])
    got = call(m, x, 4, 0.02, 0)                                    # max_iter = 0
    assert np.array_equal(got["x_adv"], np.clip(x, 0, 1)) and (got["iters"] == 0).all()
    a, b = call(m, x, 4, 0.0, 50, -np.inf, np.inf), call(m, x, 4, 0.02, 50, -np.inf, np.inf)
    m.close()
    assert (a["iters"] == b["iters"]).all() and (a["choices"] == b["choices"]).all() and (a["iters"] >= 1).all()
    ra, rb = a["x_adv"].astype(np.float64) - x, b["x_adv"].astype(np.float64) - x
    err = np.abs(rb - 1.02 * ra).max()
    print("overshoot 0.02 against 1.02 x overshoot 0: largest absolute difference %.3e (max |r| %.3f)" % (err, np.abs(ra).max()))
    # each x_adv is one float32 rounding of x + s r below 4 in magnitude (half an ulp: 2.4e-7), once times 1.02 and once plain, and
    # float32(1.02) is 3e-8 relative off: 2.02 * 2.4e-7 + 3e-8 max |r|
    assert np.abs(b["x_adv"]).max() < 4.0 and err <= 2.02 * 2.4e-7 + 3e-8 * np.abs(ra).max()
    assert (b["r_norm"] > a["r_norm"]).all()


def test_a_nan_pixel_stops_its_image_and_leaves_the_others_alone(runs):
    v = runs["lin70"]
    x = v["x"][:3].copy()
    clean = call(v["model"], x, v["nc"])
    x[1, 3, 3, 0] = np.nan
    got = call(v["model"], x, v["nc"])
    for i in (0, 2):
        assert all(np.array_equal(got[k][i].view(np.int32) if got[k].dtype == np.float32 else got[k][i],
                                  clean[k][i].view(np.int32) if clean[k].dtype == np.float32 else clean[k][i])
                   for k in ("x_adv", "r_norm", "iters", "final_class")) and (got["choices"][:, i] == clean["choices"][:, i]).all()
    nan = np.isnan(x[1])
    assert got["iters"][1] == 0 and (got["choices"][:, 1] == -1).all() and got["final_class"][1] == 0
    assert np.isnan(got["x_adv"][1][nan]).all() and np.array_equal(got["x_adv"][1][~nan], np.clip(x[1][~nan], 0, 1))


# ---------------------------------------------------------------------- 4. independence of the batch
def test_bitwise_identities(runs):
    v = runs["lin70"]
    m, x, nc = v["model"], v["x"], v["nc"]
    full = call(m, x, nc)
    assert _same(full, call(m, x, nc))                              # two identical calls
    for i in (0, 1, 37, 64):                                        # alone and inside B = 65
        one = call(m, x[i:i + 1], nc)
        assert all(np.array_equal(one[k][0], full[k][i]) for k in ("x_adv", "r_norm", "iters", "final_class")), i
        assert (one["choices"][:, 0] == full["choices"][:, i]).all()
    atk = attacks.DeepFool(m)
    for bs in (None, 4, 64):                                        # generate's chunkings
        xa, rn, it, fc = atk.generate(x, nb_candidate=nc, batch_size=bs, return_info=True)
        assert _same(full, {"x_adv": xa, "r_norm": rn, "iters": it, "final_class": fc}), bs
    side = torch.cuda.Stream()
    assert _same(full, call(m, x, nc, stream=side))                 # a side stream, synchronised by the caller
    t = torch.from_numpy(x).cuda()
    out = atk.generate(t, nb_candidate=nc)                          # a device tensor in gives a device tensor out
    assert isinstance(out, torch.Tensor) and np.array_equal(out.cpu().numpy(), full["x_adv"])


def test_the_two_gradient_paths_agree_bit_for_bit(runs):
    """The product library replicates the rows (one backward of B nc rows); the measurement build runs nc backwards of B rows."""
    v = runs["F28"]
    a = call(v["model"], v["x"], v["nc"])
    b = call(v["model"], v["x"], v["nc"], lib=_native.load(measure=True))
    assert _same(a, b) and (a["choices"] == b["choices"]).all()


# ---------------------------------------------------------------------- 5. refusals
def test_refusals(runs):
    lib = _native.load()
    v = runs["convlin5"]
    m = v["model"]
    t = torch.from_numpy(v["x"]).cuda()
    o = torch.empty_like(t)
    h, X, O = m._handle, t.data_ptr(), o.data_ptr()

    def rc(handle=h, x=X, B=3, nc=10, ov=0.02, it=5, lo=0.0, hi=1.0, out=O):
        return lib.dg_deepfool(handle, x, B, nc, ov, it, lo, hi, out, None, None, None, None)
    assert rc() == 0                                                # the optional outputs may be NULL
    torch.cuda.synchronize()
    for kw, word in ((dict(x=None), b"null"), (dict(out=None), b"null"), (dict(handle=None), b"null"), (dict(B=0), b"B must be >= 1"),
                     (dict(nc=1), b"nb_candidate"), (dict(nc=11), b"nb_candidate"), (dict(it=-1), b"max_iter"),
                     (dict(lo=1.0, hi=0.0), b"clip_min")):
        assert rc(**kw) == -1 and word in lib.dg_last_error(), kw
    bare = DR.model_of("convlin", (5, 5, 1))
    bare._ensure()
    assert rc(handle=bare._handle) == -2 and b"has no weights" in lib.dg_last_error()          # DG_E_STATE, the other classifier calls' code
    bare.close()
    c = torch.empty(5, 3, dtype=torch.int32, device="cuda")
    assert lib.dg_deepfool_choices(h, 3, 4, c.data_ptr(), None) == -2                           # the last call had max_iter = 5
    atk = attacks.DeepFool(m)
    with pytest.raises(ValueError, match="nb_candidate must not exceed"):
        atk.generate(v["x"], nb_candidate=11)
    with pytest.raises(ValueError, match="x must be"):
        atk.generate(v["x"][:, :4])
    m.rec_layer = object()
    try:
        with pytest.raises(NotImplementedError, match="reconstruction layer"):
            atk.generate(v["x"])
        with pytest.raises(NotImplementedError, match="reconstruction layer"):
            attacks.robustness(m, v["x"])
    finally:
        m.rec_layer = None


# ---------------------------------------------------------------------- 6. it finds the boundary
def test_it_finds_the_boundary_and_robustness_reports_it(runs):
    """Model F at synthetic weights: every decidable image the reference fools is fooled.  CarliniWagnerL2 at its defaults on the same
    images gives the yardstick: the device's ratio mean r_norm / mean CW l2 must not exceed the ratio the float64 reference's r_norm
    gives over the same CW distances by more than NORM_TOL -- no constant is asserted.  Measured on one MI355X: DESIGN.md section 7."""
    v = runs["F28"]
    ref = DR.case_run("F28")
    dec = DR.decidable(ref)
    got = call(v["model"], v["x"], v["nc"])
    fooled_ref = ref["final_class"] != ref["orig"]
    assert fooled_ref[dec].any() and (got["final_class"][dec & fooled_ref] != ref["orig"][dec & fooled_ref]).all()
    _, l2, cls = attacks.CarliniWagnerL2(v["model"]).generate(v["x"], return_info=True)
    ok = dec & fooled_ref & (cls != -1)
    assert ok.any()
    cw = np.sqrt(l2[ok].astype(np.float64)).mean()
    ratio, ratio_ref = got["r_norm"][ok].mean() / cw, ref["r_norm"][ok].mean() / cw
    print("DeepFool mean r_norm %.5f, CarliniWagnerL2 mean l2 %.5f on %d images: ratio %.4f (reference %.4f)" %
          (got["r_norm"][ok].mean(), cw, ok.sum(), ratio, ratio_ref))
    assert ratio <= ratio_ref * (1 + NORM_TOL)
    r = attacks.robustness(v["model"], v["x"], nb_candidate=v["nc"])
    xn = np.sqrt(np.square(v["x"].astype(np.float64)).reshape(len(dec), -1).sum(axis=1))
    assert abs(r["rho"] - (got["r_norm"] / xn).mean()) <= 1e-6 * r["rho"] and abs(r["mean_l2"] - got["r_norm"].mean()) <= 1e-6 * r["mean_l2"]
    assert r["mean_iters"] == got["iters"].mean() and 0.0 < r["fooled"] <= 1.0
    assert r["fooled"] >= (dec & fooled_ref).mean()
