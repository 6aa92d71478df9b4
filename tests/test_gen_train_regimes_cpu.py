"""-m "not gpu": the inputs of the large-batch generator tests (tests/test_gpu_gen_train_regimes.py).  generator_reference.draw_rows
selects rows whose ReLU gates float32 cannot flip; for every (latent, net_dim, N) those tests use it must succeed within its pool
cap, and the CPU's own float32 autograd must leave most of the gradient bound unused, so that a device failure at such a case
cannot be put down to rounding."""
import numpy as np
import pytest
import torch

from tests.support import generator_reference as GR

GRAD_TOL = 1e-4                 # the project's gradient bound (tests/test_gpu_gen_train.py)
FLOAT32_SHARE = 0.25            # the most of it the CPU's float32 autograd may use for a case to be usable


def bound_use(got, ref, scales):
    """{name: |got - ref| max / (GRAD_TOL * scale)} over the eight tensors and dz, scale as in test_gpu_gen_train.check_grads."""
    out = {}
    for name in GR.NAMES:
        scale = scales.get(name, float(np.abs(ref["grads"][name]).max()))
        out[name] = float(np.abs(got["grads"][name].astype(np.float64) - ref["grads"][name]).max()) / (GRAD_TOL * scale)
    out["dz"] = float(np.abs(got["dz"].astype(np.float64) - ref["dz"]).max()) / (GRAD_TOL * float(np.abs(ref["dz"]).max()))
    return out


@pytest.mark.parametrize("latent,nd,N", GR.ROW_CASES)
def test_draw_rows_serves_every_large_batch_case(latent, nd, N):
    """draw_rows finds N rows in a pool of at most 16 N; every kept row's float64 pre-activations lie outside the per-layer margins
    (4 x the largest float32 - float64 difference over the pool), ``accepted`` holds on the batch, and float32 autograd on the CPU
    uses at most 0.25 of the 1e-4 bound on every tensor and on dz.  Measured (one CPU; the float32 side
    is the CPU's BLAS, so another machine gives somewhat other margins and rows): kept shares 0.58 ... 0.60 (0.23 at NET_DIM 128),
    margins of 2.2e-6 ... 3.4e-5, float32 use at most 0.033 (Generator.5.Filters at 128 / 64 / 257); every figure is printed."""
    z, dy, info = GR.draw_rows(latent, nd, N)
    print("draw_rows(%d, %d, %d): pool %d (cap %d), kept share %.3f, margins %s"
          % (latent, nd, N, info["pool"], GR.ROW_POOL_CAP * N, info["kept"], " ".join("%.3e" % m for m in info["margins"])))
    assert z.shape == (N, latent) and dy.shape == (N, 28, 28, 1) and z.dtype == dy.dtype == np.float32
    assert info["pool"] <= GR.ROW_POOL_CAP * N and info["pool"] % N == 0
    assert all(m > 0 for m in info["margins"])
    p = GR.weights(latent, nd)
    for a, m in zip(GR.preacts(p, z, torch.float64), info["margins"]):
        assert np.abs(a).min() > m
    assert GR.accepted(p, z)
    # the rows are rows of the recorded stream, in its order, with their own dy
    zp, dyp = GR.draw(0, info["pool"], latent)
    rows = [int(np.flatnonzero((zp == r).all(axis=1))[0]) for r in z]
    assert rows == sorted(rows) and len(set(rows)) == N and np.array_equal(dyp[rows], dy)
    # a second call returns the same values in fresh arrays
    z2, dy2, _ = GR.draw_rows(latent, nd, N)
    assert np.array_equal(z2, z) and np.array_equal(dy2, dy) and z2 is not z
    ref = GR.gradient(p, z, dy)
    f32 = GR.gradient(p, z, dy, dtype=torch.float32)
    use = bound_use(f32, ref, GR.bias_scales(p, z, dy))
    for name, u in use.items():
        print("  float32 CPU %-22s uses %.4f of the bound" % (name, u))
    worst = max(use, key=use.get)
    print("  worst: %s %.4f (cap %.2f)" % (worst, use[worst], FLOAT32_SHARE))
    assert use[worst] <= FLOAT32_SHARE, (worst, use[worst])


def test_draw_rows_refuses_what_its_pool_cannot_give():
    """A margin no row can meet ends at the cap with an error, not with fewer rows."""
    saved = GR.ROW_MARGIN_FACTOR
    GR.ROW_MARGIN_FACTOR = 1e9
    try:
        with pytest.raises(AssertionError, match="do not yield"):
            GR.draw_rows(128, 64, 2, params=GR.weights())
    finally:
        GR.ROW_MARGIN_FACTOR = saved
