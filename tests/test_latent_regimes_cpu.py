"""-m "not gpu": what tests/test_gpu_latent_regimes.py stands on, checked on the reference alone -- the tracker's rules for NaN,
+inf, ties and more than 64 restarts by hand; the row selection of the many-row cases (served within the pool cap, float32 on the
CPU within half of each bound, both states of the hinge present); the R > 64 tracker case in float64."""
import numpy as np
import pytest

from tests.support import generator_reference as GR
from tests.support import latent_reference as LR

nan, inf = np.nan, np.inf


def track(m, d, kappa=0.0):
    """margins, dists [K][R] of ONE image -> (best_dist, best_margin, best_iter, best_row) as Python numbers."""
    out = LR.track(np.asarray(m, np.float64)[:, None, :], np.asarray(d, np.float64)[:, None, :], kappa)
    return tuple(o[0].item() for o in out)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g != g and w != w) or g == w, (got, want)


def test_nan_in_row_0():
    # no success: the smallest margin among the rows that have one (the rule before kept row 0 whatever the others held)
    same(track([[nan, 2, 1]], [[5, 6, 7]]), (7, 1, -1, 2))
    same(track([[nan, 1, 1]], [[nan, 6, 7]]), (6, 1, -1, 1))
    # a NaN margin is no success, even where its distance is the smallest
    same(track([[nan, -1, -2]], [[0, 3, 2]]), (2, -2, 0, 2))
    # the final iterate decides the no-success branch, not an earlier one
    same(track([[0, 1, 2], [nan, 3, 2]], [[1, 2, 3], [4, 5, 6]]), (6, 2, -1, 2))


def test_nan_in_the_middle():
    same(track([[3, nan, 1, 2]], [[1, 2, 3, 4]]), (3, 1, -1, 2))
    same(track([[-1, nan, -1]], [[4, 0, 3]]), (3, -1, 0, 2))
    same(track([[2, nan, nan, 2]], [[1, 2, 3, 4]]), (1, 2, -1, 0))


def test_all_nan():
    same(track([[nan, nan]], [[1, 2]]), (1, nan, -1, 0))
    same(track([[nan, nan], [nan, nan]], [[1, 2], [3, 4]]), (3, nan, -1, 0))            # row 0 of the FINAL iterate
    same(track([[nan, nan, nan]], [[nan, nan, nan]]), (nan, nan, -1, 0))
    # a success in an earlier iterate stays, whatever the final iterate holds
    same(track([[1, -1], [nan, nan]], [[1, 2], [3, 4]]), (2, -1, 0, 1))


def test_a_nan_distance_on_the_only_success():
    # never taken as a success (the rule before took it while the image had none): the image has no success, and the no-success
    # branch takes the smallest margin -- here that very row, with its NaN distance and best_iter = -1
    same(track([[-1, 2, 0.5]], [[nan, 1, 2]]), (nan, -1, -1, 0))
    # ... of the FINAL iterate
    same(track([[-1, 2, 0.5], [3, 2, 0.5]], [[nan, 1, 2], [4, 5, 6]]), (6, 0.5, -1, 2))
    # beside a success of finite distance it just does not count, before or after it
    same(track([[-1, -1]], [[nan, 9]]), (9, -1, 0, 1))
    same(track([[-1, -1]], [[9, nan]]), (9, -1, 0, 0))
    same(track([[-1, 1], [-3, 1]], [[9, 1], [nan, 1]]), (9, -1, 0, 0))


def test_inf_compares_as_a_number():
    same(track([[inf, inf, inf]], [[1, 2, 3]]), (1, inf, -1, 0))                          # equal smallest margins: the smallest r
    same(track([[nan, inf, inf]], [[1, 2, 3]]), (2, inf, -1, 1))
    same(track([[inf, 5]], [[1, 2]]), (2, 5, -1, 1))
    same(track([[-1, 1]], [[inf, 1]]), (inf, -1, 0, 0))                                   # an +inf distance is taken ...
    same(track([[-1, 1], [1, -1]], [[inf, 1], [1, 7]]), (7, -1, 1, 1))                    # ... and beaten by any finite one
    same(track([[-1, -1]], [[inf, inf]]), (inf, -1, 0, 0))
    same(track([[-inf, -1]], [[3, 3]]), (3, -inf, 0, 0))


def test_equal_distances_and_equal_margins():
    same(track([[-1, -2, -3]], [[2, 1, 1]]), (1, -2, 0, 1))                               # equal distances at different r
    same(track([[1, -1], [-2, 1], [-3, -3]], [[9, 4], [4, 9], [4, 4]]), (4, -1, 0, 1))    # ... at different k: the earliest
    same(track([[1, 1], [-2, -3], [-4, -5]], [[9, 9], [4, 4], [4, 4]]), (4, -2, 1, 0))    # earliest k, then smallest r
    same(track([[2, 1, 1]], [[1, 2, 3]]), (2, 1, -1, 1))                                  # equal smallest margins
    same(track([[0, 0]], [[1, 2]]), (1, 0, -1, 0))                                        # m = -kappa is no success
    same(track([[-0.5, -0.5]], [[1, 2]], 0.5), (1, -0.5, -1, 0))


@pytest.mark.parametrize("R", [65, 130])
def test_more_than_64_restarts(R):
    last = R - 1
    m, d = np.full(R, -1.0), np.full(R, 5.0)
    d[last] = 1.0
    same(track([m], [d]), (1, -1, 0, last))                                               # the winner in the last row
    d[64] = 1.0
    same(track([m], [d]), (1, -1, 0, 64))
    d[3] = 1.0
    same(track([m], [d]), (1, -1, 0, 3))                                                  # 3, 64 and the last tie: the smallest r
    m = np.full(R, 2.0)
    m[last] = 1.0
    same(track([m], [d]), (1, 1, -1, last))                                               # no success: the smallest margin
    m[64] = 1.0
    same(track([m], [d]), (1, 1, -1, 64))
    m[:64] = nan
    same(track([m], [d]), (1, 1, -1, 64))
    # the only success sits behind 64 rows of NaN margins and one NaN distance
    m = np.full(R, nan)
    m[64:] = -1.0
    d = np.full(R, 5.0)
    d[64] = nan
    same(track([m], [d]), (5, -1, 0, 65) if R > 65 else (nan, -1, -1, 64))


@pytest.mark.parametrize("name", sorted(LR.REGIME_CASES))
def test_the_row_selection_serves_every_case(name):
    """Within ROW_POOL_CAP blocks every image has its R kept restarts; float32 on the CPU uses at most MAX_SHARE of each bound on
    the selected batch at both teacher-forced steps; the hinge is on in some rows and off in others; the cases hold what they are
    named for."""
    p = LR.REGIME_CASES[name]
    rc = LR.regime_case(name)
    info, N = rc["info"], p["B"] * p["R"]
    print("%s: pool %d of at most %d (kept %.2f), hinge on in %s of %d rows, absolute margin bound on %s rows; float32 on the CPU uses "
          "%.3f / %.3f / %.3f of the dz / margin / dist bounds" % ((name, info["pool"], GR.ROW_POOL_CAP * N, info["kept"], info["hinge_on"], N,
                                                                    info["absolute"]) + rc["shares"]))
    assert info["pool"] <= GR.ROW_POOL_CAP * N and GR.ROW_POOL_CAP == 16 and GR.ROW_MARGIN_FACTOR == 4.0
    assert max(rc["shares"]) <= LR.MAX_SHARE == 0.5
    assert rc["z"][0].shape == (N, p["latent"]) and len(set(map(bytes, rc["z"][0]))) == N            # no row twice
    for k in range(LR.REGIME_STEPS):
        assert 0 < info["hinge_on"][k] < N
        it = rc["its"][k]
        assert np.array_equal(it["margin"] + p["kappa"] > 0, it["dlogits"].any(axis=1))
        # the margin's bound per row: relative up to a cancellation of MAX_CONDITION, absolute beyond, and never narrower there
        mag = np.abs(it["Z"][np.arange(N), rc["lab_rows"]]) + np.abs(it["Z"][np.arange(N), it["other"]])
        assert np.array_equal(rc["absolute"][k], mag / np.abs(it["margin"]) > LR.MAX_CONDITION)
        assert (rc["scale"][k] >= LR.SCALAR_TOL * np.abs(it["margin"]) * (1 - 1e-12)).all()
    n = LR.KINDS[p["kind"]][-1][1]
    assert set(rc["labels"].tolist()) <= set(range(n))
    if name == "conv_4x65":
        # row 256 opens the margin kernel's second workgroup and belongs to image 3, whose label is not image 0's (256 % 4 = 0)
        assert N > 256 and 256 // p["R"] == 3 and {0, 9} <= set(rc["labels"].tolist()) and rc["labels"][3] != rc["labels"][0]
        assert len(set(rc["labels"].tolist())) == 4
    if name == "lin_130x2_l64":
        assert set(rc["labels"].tolist()) == {0, 1, 2} and N > 256
    if name == "lin2_3x3":
        assert n == 2 and set(rc["its"][0]["other"].tolist()) == {0, 1}


def test_a_selection_that_cannot_be_served_raises():
    saved = GR.ROW_MARGIN_FACTOR
    GR.ROW_MARGIN_FACTOR = 1e9
    try:
        with pytest.raises(AssertionError, match="do not yield"):
            LR.regime_case.__wrapped__("lin2_3x3")
    finally:
        GR.ROW_MARGIN_FACTOR = saved


@pytest.mark.parametrize("R", [65, 130])
def test_the_tracker_case_past_64_restarts_in_float64(R):
    """What the GPU test asserts about the device's result holds for the reference: an image with a success, one without, a winner
    at r >= 64 -- and by a distance no rounding can close."""
    ref = LR.tracker_reference(R)
    bi, br = ref["best_iter"], ref["best_row"]
    print("R = %d: best_iter %s best_row %s best_dist %s" % (R, bi, br, ref["best_dist"]))
    assert bi[0] >= 0 and bi[1] == -1 and bi[2] >= 0 and br[2] == R - 1 >= 64
    K = LR.TRACKER["nb_iter"] + 1
    m, d = ref["margin"].reshape(K, 3, R), ref["dist"].reshape(K, 3, R)
    assert d[:, 2, :R - 1].min() > 10 * d[:, 2, R - 1].max()
    assert (m[:, 1] > -LR.TRACKER["kappa"] + 0.1).all()                                   # image 1 stays far from success
    assert (m[:, 2] < -LR.TRACKER["kappa"] - 0.1).all()
    ok0 = m[:, 0] < -LR.TRACKER["kappa"]
    assert ok0.any() and not ok0.all()                                                    # image 0: some (k, r) succeed, not all
