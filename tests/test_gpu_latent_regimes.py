"""-m gpu: the latent-space attack (defensegan_amd/csrc/dg_latent.hip) where tests/test_gpu_latent.py does not go: values at 260
rows (the margin kernel's second workgroup, j / R past 6, two classes), the tracker past 64 restarts, on ties and on NaN, the three
scalar code paths, calls that evaluate nothing, one handle across shapes, classifiers and options, Adam off its defaults.

Bounds are the project's, unchanged: dz within 1e-4 of the reference tensor's largest entry, dist 1e-5 relative, the margin 1e-5
relative where its cancellation (|Z[label]| + |Z[o]|) / |m| is at most 10 and 1e-6 of |Z[label]| + |Z[o]| beyond
(latent_reference.regime_scale), an Adam step from the device's own dz, m, v within rtol 1e-6 / atol 1e-6 max of the float32
restatement.  The 260-row batches are selected rows (latent_reference.regime_case; tests/test_latent_regimes_cpu.py shows each case
is served and what float32 itself costs).  Everything else is bit for bit: against the reference tracker on the device's own traces,
against a fresh pair of handles, against the aligned call."""

import numpy as np
import pytest

from tests.support import generator_reference as GR
from tests.support import latent_reference as LR
from tests.support.latent_device import KEYS, big, build, dev, host, same

pytestmark = pytest.mark.gpu
TRACES = KEYS + ("margin", "dist")


def regime(name):
    p, rc = LR.REGIME_CASES[name], LR.regime_case(name)
    g, model, atk = build(p["latent"], p["kind"], p["clf_seed"], rc["gp"], rc["clf"])
    return g, model, atk, rc


def forced(atk, rc, k, x=None, m=None, v=None, **kw):
    """One teacher-forced iteration from the reference's state k; returns (host dict, the device's m and v after it)."""
    md = dev(rc["m"][k]) if m is None else m
    vd = dev(rc["v"][k]) if v is None else v
    out = atk.call(dev(rc["x"]) if x is None else x, dev(rc["labels"]), rc["R"], 1, LR.LR, rc["c"], rc["kappa"], z0=dev(rc["z"][k]), m=md, v=vd,
                   t_start=k, keep_state=True, traces=True, want_dz=True, **kw)
    return host(out), md.cpu().numpy(), vd.cpu().numpy()


def value_shares(out, rc, k):
    it = rc["its"][k]
    return (float(np.abs(out["dz"] - it["dz"]).max() / np.abs(it["dz"]).max() / LR.DZ_TOL),
            float((np.abs(out["margin"][0] - it["margin"]) / rc["scale"][k]).max()),
            float((np.abs(out["dist"][0] - it["dist"]) / np.abs(it["dist"])).max() / LR.SCALAR_TOL))


def adam_close(got, want):
    return np.allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


def unaligned(t):
    """A copy of ``t`` that starts one float into a larger flat buffer: 4 bytes off a 16-byte boundary."""
    import torch
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ---------------------------------------------------------------------- values at many rows
@pytest.mark.parametrize("name", sorted(LR.REGIME_CASES))
def test_values_at_many_rows(name):
    """Teacher-forced steps k = 0, 1 on the selected batch: margin, dist and dz of every row against the float64 iteration, the
    update against adam_f32 from the device's own dz.  conv_4x65: row 256 opens the margin kernel's second workgroup and belongs to
    image 3; lin_130x2_l64: j / R up to 129; lin2_3x3: two classes.  Measured (one MI355X, one run): see DESIGN.md section 7."""
    g, model, atk, rc = regime(name)
    for k in range(LR.REGIME_STEPS):
        out, m1, v1 = forced(atk, rc, k)
        s = value_shares(out, rc, k)
        print("%s k=%d: dz %.3f, margin %.3f (%d rows on the absolute bound), dist %.3f of the bound" %
              (name, k, s[0], s[1], int(rc["absolute"][k].sum()), s[2]))
        assert max(s) <= 1.0, s
        z2, m2, v2 = GR.adam_f32(rc["z"][k], out["dz"], rc["m"][k], rc["v"][k], k + 1, LR.LR, LR.BETA1, LR.BETA2)
        assert adam_close(out["z"], z2) and adam_close(m1, m2) and adam_close(v1, v2)
    g.close()
    model.close()


# ---------------------------------------------------------------------- the tracker
def tracker(R):
    t = LR.TRACKER
    gp, clf, x, labels, z0 = LR.tracker_inputs(R)
    g, model, atk = build(t["latent"], t["kind"], t["clf_seed"], gp, clf)
    return g, model, atk, x, labels, z0, dict(learning_rate=t["lr"], c=t["c"], confidence=t["kappa"])


def check_track(out, B, R, kappa):
    K = out["margin"].shape[0]
    bd, bm, bi, br = LR.track(out["margin"].reshape(K, B, R), out["dist"].reshape(K, B, R), np.float32(kappa))
    assert np.array_equal(out["best_iter"], bi) and np.array_equal(out["best_row"], br), (out["best_iter"], bi, out["best_row"], br)
    assert np.array_equal(out["best_dist"], bd, equal_nan=True) and np.array_equal(out["best_margin"], bm, equal_nan=True)
    return bi, br


@pytest.mark.parametrize("R", [65, 130])
def test_tracker_past_64_restarts(R):
    """Every lane of the tracker's wave holds two or three rows (R = 130) or lane 0 alone holds two (R = 65).  best_* equal the
    reference tracker on the device's traces; x_adv is dg_generate at the winning z; the case holds an image with a success, one
    without, and a winner at r >= 64 (latent_reference.TRACKER says how)."""
    g, model, atk, x, labels, z0, kw = tracker(R)
    nb = LR.TRACKER["nb_iter"]
    xd, ld, zd = dev(x), dev(labels), dev(z0)
    out = host(atk.call(xd, ld, R, nb, z0=zd, traces=True, **kw))
    bi, br = check_track(out, 3, R, kw["confidence"])
    print("R = %d: best_iter %s best_row %s" % (R, bi, br))
    assert (bi >= 0).any() and (bi < 0).any() and (br[bi >= 0] >= 64).any()
    for k in sorted(set(bi.tolist())):
        zk = out["z"] if k < 0 else host(atk.call(xd, ld, R, k, z0=zd, keep_state=True, **kw))["z"] if k > 0 else z0
        for b in np.flatnonzero(bi == k):
            assert np.array_equal(g.generate(zk[b * R + br[b]][None])[0], out["x_adv"][b]), (k, b)
    g.close()
    model.close()


@pytest.mark.parametrize("branch", ["success", "no success"])
def test_ties_inside_an_iterate(branch):
    """Rows r = 3, 64 and 70 of one image are copies of the row that wins it: lane 3 holds the first and (R = 130) lanes 0 and 6
    the others in their second turn, so the tie is settled in the shuffle reduction.  The winner is r = 3."""
    R, nb = 130, 2
    g, model, atk, x, labels, z0, kw = tracker(R)
    if branch == "no success":
        kw["confidence"] = 1e6
    xd, ld = dev(x), dev(labels)
    first = host(atk.call(xd, ld, R, nb, z0=dev(z0), traces=True, **kw))
    b = 0 if branch == "success" else 1
    assert (first["best_iter"][b] >= 0) == (branch == "success")
    q = int(first["best_row"][b])
    z = z0.copy()
    img = z[b * R:(b + 1) * R]                       # a view
    spare = next(r for r in range(R) if r not in (q, 3, 64, 70))
    for r in (3, 64, 70):
        img[r] = z0[b * R + q]
    if q not in (3, 64, 70):
        img[q] = z0[b * R + spare]                   # the winner's old place holds a row that did not win
    out = host(atk.call(xd, ld, R, nb, z0=dev(z), traces=True, **kw))
    m, d = out["margin"].reshape(nb + 1, 3, R), out["dist"].reshape(nb + 1, 3, R)
    for r in (64, 70):                               # the precondition: copies have identical traces
        assert np.array_equal(m[:, b, 3], m[:, b, r]) and np.array_equal(d[:, b, 3], d[:, b, r])
    assert np.array_equal(m[:, b, 3], first["margin"].reshape(nb + 1, 3, R)[:, b, q])
    check_track(out, 3, R, kw["confidence"])
    assert out["best_row"][b] == 3 and out["best_iter"][b] == first["best_iter"][b]
    assert out["best_dist"][b] == first["best_dist"][b] and out["best_margin"][b] == first["best_margin"][b]
    assert np.array_equal(out["x_adv"][b], first["x_adv"][b])
    g.close()
    model.close()


def test_ties_across_iterates():
    """learning_rate = 0: lr_t = 0, z does not move and every iterate repeats the first one's bits, so a successful image keeps
    best_iter = 0 (strict "<"), in one call of three iterations and in chained calls that carry the state."""
    import torch
    R = 65
    g, model, atk, x, labels, z0, kw = tracker(R)
    kw["learning_rate"] = 0.0
    xd, ld, zd = dev(x), dev(labels), dev(z0)
    out = host(atk.call(xd, ld, R, 3, z0=zd, traces=True, **kw))
    assert np.array_equal(out["z"], z0)
    for k in range(1, 4):
        assert np.array_equal(out["margin"][k], out["margin"][0]) and np.array_equal(out["dist"][k], out["dist"][0])
    ok = out["best_iter"] >= 0
    assert ok.any() and (out["best_iter"][ok] == 0).all()
    check_track(out, 3, R, kw["confidence"])
    m, v, state, z = torch.zeros_like(zd), torch.zeros_like(zd), None, zd
    for t in range(3):
        o = atk.call(xd, ld, R, 1, z0=z, m=m, v=v, t_start=t, keep_state=True, state=state, **kw)
        z, state = o["z"], {k: o[k] for k in KEYS if k != "z"}
    o = atk.call(xd, ld, R, 0, z0=z, m=m, v=v, t_start=3, state=state, **kw)
    same(out, host({k: o[k] for k in KEYS}))
    g.close()
    model.close()


def test_a_nan_pixel():
    """B = 3, R = 10: image 1 has one NaN pixel in x, so every distance of it is NaN while its margins are finite.  On the success
    branch (kappa 0: every row succeeds by its margin, none is taken, the image ends on the no-success branch with a NaN best_dist)
    and on the no-success branch (kappa 1e6) the result is the reference tracker's on the device's traces, and the images that share
    the call have the bits of the call without the NaN.  Ordinary kernels on non-finite data.

    NaN margins: test_a_nan_classifier_bias (whole images) and test_nan_in_z0 (what a NaN row of z0 does on the device)."""
    g, model, atk = build(128, "conv10", 0)
    B, R = 3, 10
    x, _, z0 = LR.draw(128, B, R, 3)
    lab = np.array([1, 6, 9], np.int32)              # none is the class every G(z) of the synthetic generator falls into (4)
    xn = x.copy()
    xn[1, 13, 13, 0] = np.nan
    for kappa in (0.0, 1e6):
        for nb in (0, 2):
            kw = dict(learning_rate=0.1, c=2.0, confidence=kappa, traces=True)
            clean = host(atk.call(dev(x), dev(lab), R, nb, z0=dev(z0), **kw))
            out = host(atk.call(dev(xn), dev(lab), R, nb, z0=dev(z0), **kw))
            m, d = out["margin"].reshape(nb + 1, B, R), out["dist"].reshape(nb + 1, B, R)
            assert np.isfinite(m[0]).all() and np.isnan(d[:, 1]).all() and np.isfinite(np.delete(d, 1, axis=1)).all()
            bi, br = check_track(out, B, R, kappa)
            print("kappa %g, nb_iter %d: best_iter %s best_row %s" % (kappa, nb, bi, br))
            assert bi[1] == -1 and np.isnan(out["best_dist"][1])
            if nb == 0:
                assert ((m[0, 1] < 0).all() or kappa > 0) and br[1] == m[0, 1].argmin() and np.isfinite(out["best_margin"][1])
                assert bi[0] == bi[2] == (0 if kappa == 0.0 else -1)
            cm, cd = clean["margin"].reshape(nb + 1, B, R), clean["dist"].reshape(nb + 1, B, R)
            assert np.array_equal(m[0], cm[0])
            for b_ in (0, 2):
                assert np.array_equal(m[:, b_], cm[:, b_]) and np.array_equal(d[:, b_], cd[:, b_])
                for k in KEYS:
                    a, c = (out[k][b_ * R:(b_ + 1) * R], clean[k][b_ * R:(b_ + 1) * R]) if k == "z" else (out[k][b_], clean[k][b_])
                    assert np.array_equal(a, c), k
    g.close()
    model.close()


def test_nan_in_z0():
    """B = 4, R = 10: a NaN in restart 0 of image 0, in restart 4 of image 1, in every restart of image 2; image 3 is clean.
    What the device does with such a row is NOT a NaN margin: every Linear output of the row is NaN, the engine's ReLU
    (t > 0 ? t : 0) turns each into 0, and the row yields the generator's bias-only image -- finite margins and distances, the same
    for every such row of an image, at every iterate (dz is 0 behind the closed gates, so z stays where it is).  Asserted as such, so
    that a ReLU rewritten to pass a NaN on shows here.  The results are the reference tracker's on the device's traces (image 2: ten
    equal rows, so row 0), and every clean row and the clean image have the bits of the call without the NaN."""
    g, model, atk = build(128, "conv10", 0)
    B, R = 4, 10
    x, _, z0 = LR.draw(128, B, R, 3)
    lab = np.array([1, 6, 0, 9], np.int32)
    zn = z0.copy()
    zn[0, 5] = np.nan
    zn[R + 4, 0] = np.nan
    zn[2 * R:3 * R, 7] = np.nan
    planted = np.isnan(zn).any(axis=1).reshape(B, R)
    for kappa in (0.0, 1e6):
        for nb in (0, 2):
            kw = dict(learning_rate=0.1, c=2.0, confidence=kappa, traces=True)
            clean = host(atk.call(dev(x), dev(lab), R, nb, z0=dev(z0), **kw))
            out = host(atk.call(dev(x), dev(lab), R, nb, z0=dev(zn), **kw))
            m, d = out["margin"].reshape(nb + 1, B, R), out["dist"].reshape(nb + 1, B, R)
            assert np.isfinite(m).all() and np.isfinite(d).all()
            # the bias-only image: one margin and one distance for all ten rows of image 2, unchanged from iterate to iterate
            assert (m[:, 2] == m[0, 2, 0]).all() and (d[:, 2] == d[0, 2, 0]).all()
            assert (m[:, 0, 0] == m[0, 0, 0]).all() and (m[:, 1, 4] == m[0, 1, 4]).all()
            bi, br = check_track(out, B, R, kappa)
            print("kappa %g, nb_iter %d: best_iter %s best_row %s" % (kappa, nb, bi, br))
            assert br[2] == 0 and bi[2] == (0 if m[0, 2, 0] < -kappa else -1)
            cm, cd = clean["margin"].reshape(nb + 1, B, R), clean["dist"].reshape(nb + 1, B, R)
            assert np.array_equal(m[:, ~planted], cm[:, ~planted]) and np.array_equal(d[:, ~planted], cd[:, ~planted])
            assert not np.array_equal(m[0, planted], cm[0, planted])
            for k in KEYS:
                a, c = (out[k][3 * R:], clean[k][3 * R:]) if k == "z" else (out[k][3], clean[k][3])
                assert np.array_equal(a, c), k
    g.close()
    model.close()


def test_a_nan_classifier_bias():
    """The bias of the classifier's LAST class is NaN, so that logit is NaN in every row.  Images labelled with that class (0 and 2
    of B = 4, R = 10) have a NaN margin in every row: never a success, and with every margin NaN the result is row 0 of the final
    iterate with best_iter = -1 and a finite best_dist.  The other images keep finite margins -- a NaN logit is never greater than
    the runner-up so far, and class 9 is not their first other class -- and have the bits of a call that holds them alone.  Equal to
    the reference tracker on the device's traces on both branches."""
    layers, params = LR.classifier("conv10", 0)
    params = [(W.copy(), b.copy()) for W, b in params]
    params[-1][1][9] = np.nan
    g, model, atk = build(128, "conv10", 0, clf=(layers, params))
    B, R = 4, 10
    x, _, z0 = LR.draw(128, B, R, 3)
    lab = np.array([9, 1, 9, 6], np.int32)
    keep = np.array([1, 3])
    rows = (keep[:, None] * R + np.arange(R)).ravel()
    for kappa in (0.0, 1e6):
        for nb in (0, 2):
            kw = dict(learning_rate=0.1, c=2.0, confidence=kappa, traces=True)
            out = host(atk.call(dev(x), dev(lab), R, nb, z0=dev(z0), **kw))
            m, d = out["margin"].reshape(nb + 1, B, R), out["dist"].reshape(nb + 1, B, R)
            assert np.isnan(m[:, [0, 2]]).all() and np.isfinite(m[:, keep]).all() and np.isfinite(d).all()
            bi, br = check_track(out, B, R, kappa)
            print("kappa %g, nb_iter %d: best_iter %s best_row %s" % (kappa, nb, bi, br))
            for b in (0, 2):
                assert bi[b] == -1 and br[b] == 0 and np.isnan(out["best_margin"][b]) and out["best_dist"][b] == d[nb, b, 0]
                assert np.array_equal(out["x_adv"][b], g.generate(out["z"][b * R][None])[0])
            if nb == 0:
                assert (bi[keep] == (0 if kappa == 0.0 else -1)).all()
            alone = host(atk.call(dev(x[keep]), dev(lab[keep]), R, nb, z0=dev(z0[rows]), **kw))
            assert np.array_equal(alone["margin"], out["margin"][:, rows]) and np.array_equal(alone["dist"], out["dist"][:, rows])
            for k in KEYS:
                assert np.array_equal(alone[k], out[k][rows] if k == "z" else out[k][keep]), k
    g.close()
    model.close()


# ---------------------------------------------------------------------- the scalar paths
def test_scalar_distance_kernel():
    """x four bytes off alignment: latent_dist_seed_kernel<1>.  dy is the same fmaf per element, so dz keeps the aligned call's
    bits; the distance is another order of summation and is held to the float64 reference, like the aligned one."""
    g, model, atk, rc = regime("conv_4x65")
    aligned, _, _ = forced(atk, rc, 0)
    out, _, _ = forced(atk, rc, 0, x=unaligned(dev(rc["x"])))
    assert np.array_equal(out["dz"], aligned["dz"]) and np.array_equal(out["z"], aligned["z"])
    assert np.array_equal(out["margin"][0], aligned["margin"][0])            # (with keep_state row 1 of a trace is not written)
    for what, o in (("aligned", aligned), ("scalar", out)):
        s = value_shares(o, rc, 0)
        print("%s distance kernel: dist uses %.3f of the bound" % (what, s[2]))
        assert s[2] <= 1.0
    print("scalar against aligned distance: %d of %d rows differ in bits, at most %.3e relative" %
          ((out["dist"][0] != aligned["dist"][0]).sum(), out["dist"][0].size, np.abs(out["dist"][0] / aligned["dist"][0] - 1).max()))
    g.close()
    model.close()


def test_scalar_tracker_copy():
    """x_adv four bytes off alignment: the tracker copies the winning row float by float.  Every output has the aligned call's bits."""
    import torch
    g, model, atk, x, lab = big()
    aligned = host(atk.call(x, lab, 10, 3, seed=5, learning_rate=0.1, c=2.0))
    state = {"x_adv": unaligned(torch.full_like(x, -1.0)), "best_dist": torch.empty(7, device="cuda"), "best_margin": torch.empty(7, device="cuda"),
             "best_iter": torch.empty(7, dtype=torch.int32, device="cuda"), "best_row": torch.empty(7, dtype=torch.int32, device="cuda")}
    out = atk.call(x, lab, 10, 3, seed=5, learning_rate=0.1, c=2.0, state=state)
    assert out["x_adv"].data_ptr() == state["x_adv"].data_ptr()
    same(aligned, host(out))
    g.close()
    model.close()


def test_scalar_adam_kernel():
    """m and v four bytes off alignment: latent_adam_kernel<1>.  z, m, v against adam_f32 from the device's own dz, at the existing
    Adam test's tolerances.  The aligned call's bits are NOT the scalar call's: the compiler contracts b m + (1 - b) g into fused
    multiply-adds differently in the two instantiations (measured on one MI355X: 4821 / 8674 / 6355 of 33280 elements of z / m / v
    differ, by an ulp), so the difference is printed and both are held to adam_f32."""
    g, model, atk, rc = regime("conv_4x65")
    k = 1
    aligned, ma, va = forced(atk, rc, k)
    mu, vu = unaligned(dev(rc["m"][k])), unaligned(dev(rc["v"][k]))
    out, m1, v1 = forced(atk, rc, k, m=mu, v=vu)
    assert np.array_equal(out["dz"], aligned["dz"])
    z2, m2, v2 = GR.adam_f32(rc["z"][k], out["dz"], rc["m"][k], rc["v"][k], k + 1, LR.LR, LR.BETA1, LR.BETA2)
    assert adam_close(out["z"], z2) and adam_close(m1, m2) and adam_close(v1, v2)
    diff = [int((a != b).sum()) for a, b in ((out["z"], aligned["z"]), (m1, ma), (v1, va))]
    ulp = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in ((out["z"], aligned["z"]), (m1, ma), (v1, va))]
    print("scalar against vector Adam: elements that differ in z, m, v: %s, at most %s of the largest entry" % (diff, ulp))
    assert adam_close(aligned["z"], z2) and adam_close(ma, m2) and adam_close(va, v2)
    g.close()
    model.close()


# ---------------------------------------------------------------------- calls that evaluate nothing, counters that do not fit
def test_nothing_to_evaluate_and_counters():
    import torch
    from defensegan_amd import _native
    lib = _native.load()
    g, model, atk = build(128, "lin3", 0)
    B, R = 2, 3
    x, lab, z0 = LR.draw(128, B, R, 1)
    xd, ld, zd = dev(x), dev((lab % 3).astype(np.int32)), dev(z0)
    xa = torch.full_like(xd, -7.0)
    mv = [torch.zeros_like(zd), torch.zeros_like(zd)]
    best = [torch.full((B,), -7.0, device="cuda"), torch.full((B,), -7.0, device="cuda"),
            torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")]

    def call(nb_iter, t_start, keep_state):
        return lib.dg_latent_attack(g._handle, model._handle, xd.data_ptr(), ld.data_ptr(), B, R, zd.data_ptr(), 0, 0, nb_iter, 0.05, 0.9, 0.999,
                                    1.0, 0.0, mv[0].data_ptr(), mv[1].data_ptr(), t_start, keep_state, xa.data_ptr(), best[0].data_ptr(),
                                    best[1].data_ptr(), best[2].data_ptr(), best[3].data_ptr(), None, None, None, None, None)
    assert call(0, 0, 1) == -1 and b"evaluates nothing" in lib.dg_last_error()
    assert call(1, 2 ** 31 - 1, 1) == -1 and b"does not fit best_iter" in lib.dg_last_error()
    assert call(2 ** 31 - 1, 1, 1) == -1 and b"does not fit best_iter" in lib.dg_last_error()
    assert call(0, 2 ** 40, 0) == -1 and b"does not fit best_iter" in lib.dg_last_error()
    assert call(1, 2 ** 63 - 1, 1) == -1 and b"does not fit best_iter" in lib.dg_last_error()      # (the check itself does not overflow)
    torch.cuda.synchronize()
    assert (xa == -7.0).all() and all((b == -7).all() for b in best)              # a refused call wrote nothing
    assert call(0, 0, 0) == 0                                                       # nb_iter = 0 alone judges z0
    torch.cuda.synchronize()
    assert (best[3] >= 0).all() and not (xa == -7.0).any()
    # nb_iter = 0 with keep_state and t_start > 0 is legal: the state and x_adv keep their bits, z = z0
    first = atk.call(xd, ld, R, 2, z0=zd, m=mv[0], v=mv[1], keep_state=True)
    state = {k: first[k] for k in KEYS if k != "z"}
    before = host(state)
    m0, v0 = mv[0].clone(), mv[1].clone()
    out = atk.call(xd, ld, R, 0, z0=first["z"], m=mv[0], v=mv[1], t_start=2, keep_state=True, state=state)
    same(before, host(out), [k for k in KEYS if k != "z"])
    assert torch.equal(out["z"], first["z"]) and torch.equal(mv[0], m0) and torch.equal(mv[1], v0)
    g.close()
    model.close()


# ---------------------------------------------------------------------- one handle, many shapes and options
def attack_inputs(B, R, n, latent=128):
    x, lab, z0 = LR.draw(latent, B, R, 20 + B)
    return dev(x), dev((lab % n).astype(np.int32)), dev(z0)


def attacked(atk, B, R, n):
    x, lab, z0 = attack_inputs(B, R, n)
    return host(atk.call(x, lab, R, 2, z0=z0, learning_rate=0.1, c=2.0, traces=True, want_dz=True))


ALL = TRACES + ("dz",)


def test_one_handle_called_with_many_shapes():
    """B x R = 1x3, 4x65, 1x3, 7x10, 1x1 on one pair of handles: the per-row buffers and the tracker state grow, then serve smaller
    calls.  Every result has the bits of a fresh pair at that shape."""
    g, model, atk = build(128, "conv10", 0)
    for B, R in ((1, 3), (4, 65), (1, 3), (7, 10), (1, 1)):
        got = attacked(atk, B, R, 10)
        g2, model2, atk2 = build(128, "conv10", 0)
        same(attacked(atk2, B, R, 10), got, ALL)
        g2.close()
        model2.close()
    g.close()
    model.close()


def test_one_generator_two_classifiers():
    """lin3 at 20 rows, conv10 at 10 rows (the seed buffer grows from 60 to 100 floats while the row buffers stay), lin3 again."""
    from defensegan_amd import network_builder as nb
    g, lin, atk_lin = build(128, "lin3", 0)
    conv = nb.MLP(LR.mlp_layers("conv10"), device=g._device)
    conv.set_weights(LR.classifier("conv10", 0)[1])
    atk_conv = nb.LatentAttack(conv, g)
    for atk, kind, n, B, R in ((atk_lin, "lin3", 3, 2, 10), (atk_conv, "conv10", 10, 1, 10), (atk_lin, "lin3", 3, 2, 10)):
        got = attacked(atk, B, R, n)
        g2, model2, atk2 = build(128, kind, 0)
        same(attacked(atk2, B, R, n), got, ALL)
        g2.close()
        model2.close()
    for h in (g, lin, conv):
        h.close()


def test_reconstruct_around_an_attack():
    """reconstruct, an attack, reconstruct (and the same with generator_gradient in between): the reconstructions have the same
    bits -- the attack's scope puts the handle's path back and leaves its workspace usable."""
    g, model, atk = build(128, "conv10", 0)
    zs = GR.draw(7, 6, 128)[0]
    x = g.generate(zs[:3])
    a = g.reconstruct(x, seed=5, return_details=True)
    attacked(atk, 7, 10, 10)
    b = g.reconstruct(x, seed=5, return_details=True)
    z, dy = GR.draw(200, 4, 128)
    g.generator_gradient(z, dy)
    attacked(atk, 1, 3, 10)
    c = g.reconstruct(x, seed=5, return_details=True)
    for k in ("rec", "loss", "z", "idx"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    g.close()
    model.close()


@pytest.mark.parametrize("option", [("frag_path", 1), ("latent_turn", 0)], ids=["frag_path", "latent_turn0"])
def test_options_that_do_not_reach_the_attack(option):
    """The attack runs on the NHWC path whatever frag_path says (NhwcScope) and launches the Linear backward, the slice sum and the
    Linear forward on their own, never the latent turn: bit for bit a default handle's, before and after a reconstruction on the
    handle's own path."""
    g, model, atk = build(128, "conv10", 0)
    want = attacked(atk, 7, 10, 10)
    g2, model2, atk2 = build(128, "conv10", 0)
    g2.set_option(*option)
    same(want, attacked(atk2, 7, 10, 10), ALL)
    zs = GR.draw(7, 3, 128)[0]
    g2.reconstruct(g.generate(zs), seed=5)
    same(want, attacked(atk2, 7, 10, 10), ALL)
    for h in (g, model, g2, model2):
        h.close()


def test_nsplit_changed():
    """nsplit = 8: dz is another slice sum, within the gradient bound of float64 on a teacher-forced case; nothing before the
    backward depends on it, so margin and dist of the first iterate keep the default handle's bits."""
    g, model, atk, rc = regime("conv_4x65")
    base, _, _ = forced(atk, rc, 0)
    g.set_option("nsplit", 8)
    out, _, _ = forced(atk, rc, 0)
    s = value_shares(out, rc, 0)
    print("nsplit 8: dz uses %.3f of the bound (nsplit 16: %.3f); %d of %d dz elements differ in bits" %
          (s[0], value_shares(base, rc, 0)[0], (out["dz"] != base["dz"]).sum(), out["dz"].size))
    assert s[0] <= 1.0
    assert np.array_equal(out["margin"], base["margin"]) and np.array_equal(out["dist"], base["dist"])
    g.close()
    model.close()


# ---------------------------------------------------------------------- Adam's edges
@pytest.mark.parametrize("b1,b2,t_start", [(0.0, 0.999, 1), (0.9, 0.0, 1), (0.0, 0.0, 1), (0.9, 0.999, 100000)],
                         ids=["beta1=0", "beta2=0", "both=0", "t=100000"])
def test_adam_edges(b1, b2, t_start):
    """One default step gives non-zero moments; then one step with the edge's betas or counter against adam_f32 from the device's
    own dz, m, v (t = t_start + 1; lr_t is formed on the host from pow(beta, t))."""
    import torch
    g, model, atk = build(128, "conv10", 0)
    x, lab, z0 = attack_inputs(3, 2, 10)
    m, v = torch.zeros_like(z0), torch.zeros_like(z0)
    first = atk.call(x, lab, 2, 1, z0=z0, m=m, v=v, keep_state=True)
    state = {k: first[k] for k in KEYS if k != "z"}
    zb, mb, vb = first["z"].cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
    assert mb.any() and vb.any()
    out = atk.call(x, lab, 2, 1, z0=first["z"], m=m, v=v, t_start=t_start, keep_state=True, state=state, beta1=b1, beta2=b2, want_dz=True)
    dz = out["dz"].cpu().numpy()
    z2, m2, v2 = GR.adam_f32(zb, dz, mb, vb, t_start + 1, 0.05, b1, b2)
    assert np.isfinite(z2).all() and not np.array_equal(z2, zb)
    for got, want in ((out["z"], z2), (m, m2), (v, v2)):
        assert adam_close(got.cpu().numpy(), want)
    if b1 == 0.0:
        assert np.array_equal(m.cpu().numpy(), dz)
    if b2 == 0.0:
        assert np.array_equal(v.cpu().numpy(), dz * dz)
    g.close()
    model.close()
