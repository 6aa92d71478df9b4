"""-m gpu: the parts of dg_deepfool.hip that tests/test_gpu_deepfool.py does not execute -- the second trips of the image-strided
loops (B past both grid caps), pass 2's candidate stride (nb_candidate >= 258, up to the 2048 that still runs), the scalar path from
an unaligned pointer at P % 4 == 0, x_adv == x, a signed clip range, and the step that a NaN logit takes back.  The inputs are fixed in
tests/support/deepfool_reference.py; tests/test_deepfool_edges_cpu.py shows on the CPU that each has the property it is chosen for and
at least 75 % decidable images.  The bounds are tests/test_gpu_deepfool.py's; every test prints the share of each it used."""
import numpy as np
import pytest
import torch

from defensegan_amd import _native, network_builder as nb
from tests.support import deepfool_reference as DR
from tests.test_gpu_deepfool import GRAD_TOL, HOST_NORM_TOL, NORM_TOL

pytestmark = pytest.mark.gpu

KEYS = ("x_adv", "r_norm", "iters", "final_class")


def call(m, x, nc=10, overshoot=0.02, max_iter=50, lo=0.0, hi=1.0, x_off=0, out_off=0, inplace=False):
    """One dg_deepfool call through the C ABI with the pointers under the test's control: x (x_adv) lies ``x_off`` (``out_off``) floats
    into a buffer of its own, or x_adv is x itself.  A dict of NumPy arrays (x_adv, r_norm, iters, final_class, choices [max_iter, B])."""
    dev = nb._ready(m)
    xs = np.ascontiguousarray(x, np.float32)
    B, N = int(xs.shape[0]), xs.size
    xbuf = torch.zeros(N + x_off, dtype=torch.float32, device=dev)
    xbuf[x_off:] = torch.from_numpy(xs.reshape(-1)).to(dev)
    obuf = xbuf if inplace else torch.zeros(N + out_off, dtype=torch.float32, device=dev)
    if inplace:
        out_off = x_off
    assert xbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    rn = torch.empty(B, dtype=torch.float32, device=dev)
    it, fc = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    ch = torch.empty(max_iter, B, dtype=torch.int32, device=dev)
    lib = _native.load()
    s = torch.cuda.current_stream(dev)
    _native.check(lib.dg_deepfool(m._handle, xbuf.data_ptr() + 4 * x_off, B, nc, overshoot, max_iter, lo, hi, obuf.data_ptr() + 4 * out_off,
                                  rn.data_ptr(), it.data_ptr(), fc.data_ptr(), s.cuda_stream), lib)
    _native.check(lib.dg_deepfool_choices(m._handle, B, max_iter, ch.data_ptr(), s.cuda_stream), lib)
    s.synchronize()
    return {"x_adv": obuf[out_off:].cpu().numpy().reshape(xs.shape), "r_norm": rn.cpu().numpy(), "iters": it.cpu().numpy(),
            "final_class": fc.cpu().numpy(), "choices": ch.cpu().numpy()}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, keys=KEYS + ("choices",)):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _check_step(tag, got, ref, x, lo=0.0, hi=1.0):
    """test_one_step_value_for_value's assertions (max_iter = 1, overshoot = 0)."""
    dec = DR.decidable(ref)
    bound = GRAD_TOL * np.abs(ref["r_tot"]).max()
    d = np.abs((got["x_adv"].astype(np.float64) - x) - (ref["x_adv"] - x))[dec].max()
    print("%s: decidable %d/%d, max |d r| %.3e, bound %.3e, share of the bound used %.4f" % (tag, dec.sum(), dec.size, d, bound, d / bound))
    assert dec.mean() >= 0.75
    assert (got["choices"][0][dec] == ref["choices"][0][dec]).all() and (got["iters"][dec] == ref["iters"][dec]).all()
    assert d <= bound
    assert np.isfinite(got["x_adv"]).all() and got["x_adv"].min() >= lo and got["x_adv"].max() <= hi


def _check_run(tag, got, ref, x, lo=0.0, hi=1.0, finite=None):
    """test_whole_run's assertions; ``finite`` [B] bool leaves the images with a NaN pixel out of the checks that need numbers."""
    dec = DR.decidable(ref)
    fin = np.ones(len(dec), bool) if finite is None else finite
    assert not (dec & ~fin).any()
    rel = np.abs(got["r_norm"][dec] - ref["r_norm"][dec]) / ref["r_norm"][dec]
    host = np.sqrt(np.square(got["x_adv"].astype(np.float64) - x).reshape(len(dec), -1).sum(axis=1))
    hrel = (np.abs(got["r_norm"] - host) / np.maximum(host, 1e-30))[fin]
    print("%s: decidable %d/%d, max rel r_norm error %.3e (%.4f of the bound %.0e), against the host %.3e (%.4f of the bound %.0e), "
          "iters up to %d" % (tag, dec.sum(), dec.size, rel.max(), rel.max() / NORM_TOL, NORM_TOL, hrel.max(), hrel.max() / HOST_NORM_TOL,
                              HOST_NORM_TOL, got["iters"].max()))
    assert dec.mean() >= 0.75
    assert (got["final_class"][dec] == ref["final_class"][dec]).all()
    assert (got["iters"][dec] == ref["iters"][dec]).all()
    assert (got["choices"][:, dec] == ref["choices"][:, dec]).all()
    assert rel.max() <= NORM_TOL
    assert hrel.max() <= HOST_NORM_TOL
    assert np.isfinite(got["x_adv"][fin]).all() and np.isfinite(got["r_norm"][fin]).all()
    assert got["x_adv"][fin].min() >= lo and got["x_adv"][fin].max() <= hi


# ---------------------------------------------------------------------- 1. many images: the second trip of every image-strided loop
@pytest.mark.parametrize("name", sorted(DR.TILE_CASES))
def test_tiled_past_both_grid_caps_every_tile_is_the_base_run(name):
    """67 images, image 0 inactive from the start (a NaN pixel), first against the float64 reference, then tiled to B = 65538: the step
    and the final kernel's workgroup 0 takes base image 0 (inactive: the early continue) and then base image 10 (active, on the LDS the
    first image never touched), workgroup 1 base images 1 and 11 (both active: the LDS is reused behind the trailing barrier), and the
    wave-strided kernels make five trips.  Every image works alone, so every tile must be the base run bit for bit."""
    c = DR.TILE_CASES[name]
    m, p, x = DR.tile_inputs(name)
    ref = DR.edge_run(name, m, p, x, c)
    m.set_weights(p)
    base = call(m, x, c["nc"], 0.02, c["max_iter"])
    fin = np.arange(len(x)) != 0
    _check_run(name, base, ref, x, finite=fin)
    assert base["iters"][0] == 0 and (base["choices"][:, 0] == -1).all() and base["final_class"][0] == 0
    nan = np.isnan(x[0])
    assert np.isnan(base["x_adv"][0][nan]).all() and np.array_equal(base["x_adv"][0][~nan], x[0][~nan])
    B, n = DR.TILE_B, len(x)
    got = call(m, x[np.arange(B) % n], c["nc"], 0.02, c["max_iter"])
    m.close()
    whole, rest = B // n, B % n
    assert whole * n > DR.IMAGE_CAP - n and rest == 12
    for k in KEYS + ("choices",):
        g, b = _bits(got[k]), _bits(base[k])
        if k == "choices":                                          # [max_iter, B]: the images are the second axis
            g, b = np.moveaxis(g, 1, 0), np.moveaxis(b, 1, 0)
        tiles = g[:whole * n].reshape((whole, n) + g.shape[1:])
        bad = np.argwhere((tiles != b[None]).reshape(whole, n, -1).any(axis=2))
        assert bad.size == 0, (k, "first differing (tile, image):", bad[:5].tolist())
        assert np.array_equal(g[whole * n:], b[:rest]), k
    print("%s: %d tiles of %d images and %d more equal the base run bit for bit (x_adv, r_norm, iters, final_class, choices)" %
          (name, whole, n, rest))


# ---------------------------------------------------------------------- 2. many candidates: pass 2's stride, and its limit
@pytest.mark.parametrize("name,shape,B,nc", DR.MANY_STEP_CASES)
def test_one_step_with_hundreds_of_candidates(name, shape, B, nc):
    m, p, x = DR.case_inputs(dict(model=name, shape=shape, B=B, **DR.MANY_SEEDS[name]))
    ref = DR.run(m, p, x, nc, 0.0, 1, 0.0, 1.0, shadow=torch.float32)
    m.set_weights(p)
    got = call(m, x, nc, 0.0, 1)
    _check_step("%s %s B %d nc %d" % (name, shape, B, nc), got, ref, x)
    if nc == 2048:                                                  # one more candidate is refused by name, not run
        lib = _native.load()
        t = torch.from_numpy(x).cuda()
        o = torch.empty_like(t)
        assert lib.dg_deepfool(m._handle, t.data_ptr(), B, 2049, 0.0, 1, 0.0, 1.0, o.data_ptr(), None, None, None, None) == -1
        assert b"not implemented for more than 2048" in lib.dg_last_error()
    m.close()


def test_whole_run_with_300_candidates():
    c = DR.MANY_RUN
    m, p, x = DR.case_inputs(c)
    ref = DR.edge_run("many_run", m, p, x, c)
    m.set_weights(p)
    got = call(m, x, c["nc"], 0.02, c["max_iter"])
    m.close()
    _check_run("lin300 nc 300", got, ref, x)


# ---------------------------------------------------------------------- 3. unaligned pointers, in-place output
def test_unaligned_pointers_take_the_scalar_path_and_x_adv_may_be_x():
    """lin70, P = 784: with x or x_adv 4 bytes off a 16-byte boundary the call runs DfVec<1> at P % 4 == 0.  The two widths sum in
    different orders, so the floats are held to the reference, the decisions to the aligned call.  x_adv == x (aligned): every output
    is the out-of-place call's, bit for bit."""
    c = DR.RUN_CASES["lin70"]
    m, p, x = DR.case_inputs("lin70")
    ref = DR.case_run("lin70")
    m.set_weights(p)
    aligned = call(m, x, c["nc"])
    _check_run("lin70 aligned", aligned, ref, x)
    for tag, kw in (("x 4 bytes off", dict(x_off=1)), ("x_adv 4 bytes off", dict(out_off=1))):
        got = call(m, x, c["nc"], **kw)
        _check_run("lin70 " + tag, got, ref, x)
        assert all(np.array_equal(got[k], aligned[k]) for k in ("choices", "iters", "final_class")), tag
        diff = np.abs(got["x_adv"] - aligned["x_adv"]).max()
        print("lin70 %s: largest |x_adv - aligned x_adv| %.3e" % (tag, diff))
    inplace = call(m, x, c["nc"], inplace=True)
    m.close()
    assert _same(inplace, aligned)


# ---------------------------------------------------------------------- 4. a signed clip range
def test_signed_clip_range():
    c = DR.SIGNED_CASE
    m, p, x = DR.case_inputs(c)
    ref = DR.edge_run("signed", m, p, x, c)
    m.set_weights(p)
    got = call(m, x, c["nc"], 0.02, c["max_iter"], c["lo"], c["hi"])
    m.close()
    _check_run("signed [-1, 1]", got, ref, x, c["lo"], c["hi"])
    dec = DR.decidable(ref)
    for bound in (-1.0, 1.0):                                       # both bounds bind on the device too
        share = float(((got["x_adv"][dec] == bound) == (ref["x_adv"][dec] == bound)).mean())
        print("signed: the pixels at exactly %g agree with the reference on %.5f of the decidable images' pixels" % (bound, share))
        assert (got["x_adv"] == bound).any()


# ---------------------------------------------------------------------- 5. the step a NaN logit takes back
def test_a_step_that_lands_on_a_nan_logit_is_taken_back():
    """Image 1's logits are finite at x; its first step crosses into float32 overflow, where the last layer subtracts two infinities
    (tests/test_deepfool_edges_cpu.py shows both in float32 on the CPU).  df_activity_kernel flips rsel back to the buffer that holds
    r = 0: one counted iteration, one choice, x_adv = clip(x) to the bit, final_class = orig, r_norm = 0.  The neighbours are what they
    are without it."""
    m, p, x = DR.takeback_case()
    m.set_weights(p)
    got = call(m, x, 3, 0.02, 5)
    alone = call(m, x[[0, 2]], 3, 0.02, 5)
    m.close()
    print("take-back: iters %s, choices of image 1 %s, final_class %s, r_norm %s" %
          (got["iters"].tolist(), got["choices"][:, 1].tolist(), got["final_class"].tolist(), got["r_norm"].tolist()))
    assert got["iters"][1] == 1
    assert got["choices"][0, 1] >= 0 and (got["choices"][1:, 1] == -1).all()
    assert np.array_equal(_bits(got["x_adv"][1]), _bits(np.clip(x[1], 0.0, 1.0)))
    assert got["final_class"][1] == 0
    host = np.sqrt(np.square(got["x_adv"][1].astype(np.float64) - x[1]).sum())
    assert got["r_norm"][1] == host == 0.0                          # that of the written image
    for k in KEYS:
        assert np.array_equal(_bits(got[k][[0, 2]]), _bits(alone[k])), k
    assert np.array_equal(got["choices"][:, [0, 2]], alone["choices"])
    assert np.isfinite(got["x_adv"]).all() and np.isfinite(got["r_norm"]).all() and (got["iters"][[0, 2]] >= 1).all()
