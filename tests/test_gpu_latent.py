"""-m gpu: the latent-space attack (dg_latent_attack, defensegan_amd/csrc/dg_latent.hip) against the float64 reference of
tests/support/latent_reference.py.

dz is taken from the entry's optional debug output ``out_dz`` (the dz of the call's last backward), margin and dist from the traces.
Bounds are the project's: dz within 1e-4 of the reference tensor's largest entry (tests/test_gpu_gen_train.py's bound for dz), margin
and dist 1e-5 relative (the one-image, ten-restart case: the margin within 1e-6 of |Z[label]| + |Z[o]|, latent_reference.MARGIN_ABS), an Adam step from the device's own dz, m, v within rtol 1e-6 / atol 1e-6 max of the float32 restatement.
Inputs are the recorded draws of latent_reference.SEEDS (found on the CPU; tests/test_latent_cpu.py re-checks them).  Everything
else is bit for bit against the device's own outputs."""
import ctypes as C

import numpy as np
import pytest

from tests.support import generator_reference as GR
from tests.support import latent_reference as LR

from tests.support.latent_device import KEYS, big, build, dev, host, same

pytestmark = pytest.mark.gpu


def case(name):
    latent, kind, B, R, c, kappa = LR.CASES[name]
    cs, ds = LR.SEEDS[name]
    gp, clf, x, labels, z0 = LR.case_inputs(name, cs, ds)
    g, model, atk = build(latent, kind, cs, gp, clf)
    return g, model, atk, gp, clf, x, labels, z0, R, c, kappa


@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_one_iteration_teacher_forced(name):
    """From the reference's z_k, m_k, v_k (rounded to float32), k = 0, 1, 2: one iteration with the state passed in; margin, dist and
    dz against the float64 iteration at that rounded z, and the update against the float32 Adam from the device's own dz."""
    import torch
    g, model, atk, gp, clf, x, labels, z0, R, c, kappa = case(name)
    ref = LR.run(gp, clf, x, labels, R, z0, 3, c=c, kappa=kappa)
    xd, ld = dev(x), dev(labels)
    m = v = np.zeros_like(z0, dtype=np.float64)
    for k in range(3):
        zk = ref["z"][k].astype(np.float32)
        it = LR.iteration(gp, clf, x, labels, R, zk.astype(np.float64), c, kappa)
        md, vd = dev(m.astype(np.float32)), dev(v.astype(np.float32))
        m32, v32 = md.cpu().numpy(), vd.cpu().numpy()
        out = host(atk.call(xd, ld, R, 1, LR.LR, c, kappa, z0=dev(zk), m=md, v=vd, t_start=k, keep_state=True, traces=True, want_dz=True))
        e_dz = np.abs(out["dz"] - it["dz"]).max() / np.abs(it["dz"]).max()
        # the margin's bound is relative, or for the cases of latent_reference.MARGIN_ABS 1e-6 of |Z[label]| + |Z[o]| (see there)
        e_m = (np.abs(out["margin"][0] - it["margin"]) / LR.margin_scale(it, labels, R, name in LR.MARGIN_ABS)).max() * LR.SCALAR_TOL
        e_d = (np.abs(out["dist"][0] - it["dist"]) / np.abs(it["dist"])).max()
        print("%s k=%d: dz %.3e (%.3f of the bound), margin %.3e (%.3f), dist %.3e (%.3f)" %
              (name, k, e_dz, e_dz / LR.DZ_TOL, e_m, e_m / LR.SCALAR_TOL, e_d, e_d / LR.SCALAR_TOL))
        assert e_dz <= LR.DZ_TOL and e_m <= LR.SCALAR_TOL and e_d <= LR.SCALAR_TOL
        z2, m2, v2 = GR.adam_f32(zk, out["dz"], m32, v32, k + 1, LR.LR, LR.BETA1, LR.BETA2)
        for got, want in ((out["z"], z2), (md.cpu().numpy(), m2), (vd.cpu().numpy(), v2)):
            assert np.allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
        # the next step's state is the reference's own
        _, m, v = LR.CR.adam_update(ref["z"][k], ref["steps"][k]["dz"], m, v, k + 1, LR.LR, LR.BETA1, LR.BETA2)
    g.close()
    model.close()


def test_adam_on_z_from_the_devices_own_state():
    """Steps 1-6 chained through m, v and t_start: each update equals the float32 restatement (generator_reference.adam_f32's form)
    from the device's own dz, m, v.  beta1 = 0 and zero gradients leave finite values."""
    import torch
    g, model, atk, gp, clf, x, labels, z0, R, c, kappa = case("conv_3x2")
    xd, ld = dev(x), dev(labels)
    z = dev(z0)
    md, vd = torch.zeros_like(z), torch.zeros_like(z)
    for t in range(6):
        zb, mb, vb = z.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy()
        out = atk.call(xd, ld, R, 1, LR.LR, c, kappa, z0=z, m=md, v=vd, t_start=t, keep_state=True, want_dz=True)
        z2, m2, v2 = GR.adam_f32(zb, out["dz"].cpu().numpy(), mb, vb, t + 1, LR.LR, LR.BETA1, LR.BETA2)
        for got, want in ((out["z"], z2), (md, m2), (vd, v2)):
            assert np.allclose(got.cpu().numpy(), want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
        z = out["z"]
    out = host(atk.call(xd, ld, R, 2, LR.LR, c, kappa, z0=dev(z0), beta1=0.0))
    assert np.isfinite(out["z"]).all() and not np.array_equal(out["z"], z0)
    # zero gradients: c = 0 and x = G(z0) exactly, one restart
    y0 = g.generate(dev(z0))
    out = host(atk.call(y0, dev(np.zeros(len(z0), np.int32)), 1, 2, LR.LR, 0.0, 0.0, z0=dev(z0), traces=True))
    assert np.array_equal(out["z"], z0) and not out["dist"].any()
    g.close()
    model.close()


def test_composition_bit_for_bit():
    import torch
    g, model, atk, x, lab = big()
    R, seed = 10, 77
    full = host(atk.call(x, lab, R, 3, seed=seed, traces=True))
    same(full, host(atk.call(x, lab, R, 3, seed=seed, traces=True)), KEYS + ("margin", "dist"))            # a call repeated
    # three chained one-iteration calls with state, then the closing forward
    z = g.init_latents(70, seed=seed, first_row=0)
    same(full, host(atk.call(x, lab, R, 3, z0=z, traces=True)), KEYS + ("margin", "dist"))                 # z0 = NULL is that draw
    m, v, state = torch.zeros_like(z), torch.zeros_like(z), None
    for t in range(3):
        out = atk.call(x, lab, R, 1, z0=z, m=m, v=v, t_start=t, keep_state=True, state=state, traces=True)
        assert np.array_equal(out["margin"][0].cpu().numpy(), full["margin"][t])
        assert np.array_equal(out["dist"][0].cpu().numpy(), full["dist"][t])
        z, state = out["z"], {k: out[k] for k in KEYS if k != "z"}
    out = atk.call(x, lab, R, 0, z0=z, m=m, v=v, t_start=3, state=state, traces=True)
    assert np.array_equal(out["margin"][0].cpu().numpy(), full["margin"][3])
    same(full, host({k: out[k] for k in KEYS}))
    # the same images in calls of 2, 2 and 3 with the matching first_row
    parts = [host(atk.call(x[a:b], lab[a:b], R, 3, seed=seed, first_row=a * R)) for a, b in ((0, 2), (2, 4), (4, 7))]
    same(full, {k: np.concatenate([p[k] for p in parts]) for k in KEYS})
    # one image alone (B = 1: one tracker workgroup) is that image of the full call
    for b in (0, 6):
        one = host(atk.call(x[b:b + 1], lab[b:b + 1], R, 3, seed=seed, first_row=b * R))
        same({k: full[k][b * R:(b + 1) * R] if k == "z" else full[k][b:b + 1] for k in KEYS}, one)
    # LatentAttack.generate: its own keying of the rows by the global image index -- batch_size does not show, with a drawn and
    # with a given z_init
    xa, info = atk.generate(x, lab, rec_rr=R, nb_iter=3, seed=seed, return_info=True)
    same(full, dict(host(info), x_adv=xa.cpu().numpy()))
    for kw in (dict(seed=seed), dict(z_init=g.init_latents(70, seed=seed + 1))):
        whole = atk.generate(x, lab, rec_rr=R, nb_iter=3, return_info=True, **kw)
        for bs in (1, 3):
            cut = atk.generate(x, lab, rec_rr=R, nb_iter=3, batch_size=bs, return_info=True, **kw)
            assert np.array_equal(whole[0].cpu().numpy(), cut[0].cpu().numpy())
            for k in whole[1]:
                assert np.array_equal(whole[1][k].cpu().numpy(), cut[1][k].cpu().numpy(), equal_nan=True), (bs, k)
    g.close()
    model.close()


def test_tracker_from_the_devices_own_traces():
    g, model, atk, x, lab = big()
    R, seed, nb = 10, 5, 6
    for kappa in (0.0, 0.5):
        out = host(atk.call(x, lab, R, nb, learning_rate=0.1, c=2.0, confidence=kappa, seed=seed, traces=True))
        bd, bm, bi, br = LR.track(out["margin"].reshape(nb + 1, 7, R), out["dist"].reshape(nb + 1, 7, R), np.float32(kappa))
        print("kappa %g best_iter %s best_row %s" % (kappa, bi, br))
        assert np.array_equal(out["best_dist"], bd) and np.array_equal(out["best_margin"], bm)
        assert np.array_equal(out["best_iter"], bi) and np.array_equal(out["best_row"], br)
        # x_adv = dg_generate at the winning z, recovered by re-running with nb_iter = best_iter and keep_state
        for k in sorted(set(bi.tolist())):
            zk = out["z"] if k < 0 else host(atk.call(x, lab, R, k, learning_rate=0.1, c=2.0, confidence=kappa, seed=seed, keep_state=True))["z"]
            for b in np.flatnonzero(bi == k):
                row = zk[b * R + br[b]][None]
                assert np.array_equal(g.generate(row)[0], out["x_adv"][b]), (k, b)
    g.close()
    model.close()


def test_regions():
    """A kappa no row can meet: best_iter = -1 everywhere and the smallest margin of the final iterate.  c = 0: Adam on the
    projection loss, dz = dg_loss_grad's within the gradient bound."""
    g, model, atk, x, lab = big()
    R = 10
    out = host(atk.call(x, lab, R, 2, confidence=1e6, seed=9, traces=True))
    assert (out["best_iter"] == -1).all()
    last = out["margin"][2].reshape(7, R)
    assert np.array_equal(out["best_row"], last.argmin(axis=1)) and np.array_equal(out["best_margin"], last.min(axis=1))
    z0 = g.init_latents(70, seed=9)
    out = host(atk.call(x, lab, R, 1, c=0.0, z0=z0, want_dz=True, traces=True))
    _, loss, dz = g.loss_grad(x, z0)
    err = np.abs(out["dz"] - dz.cpu().numpy()).max() / np.abs(dz.cpu().numpy()).max()
    print("c = 0: dz vs dg_loss_grad %.3e of the largest entry" % err)
    assert err <= LR.DZ_TOL
    assert np.allclose(out["dist"][0], loss.cpu().numpy(), rtol=LR.SCALAR_TOL, atol=0)
    g.close()
    model.close()


def test_it_attacks():
    """Labels = the classifier's own predictions on G(z_true); 30 iterations from a fresh draw, R = 2, B = 8.  The float64 reference
    (found on the CPU: seed ATTACK_SEED ends with at least 6 of 8 successful) and the device: success counts within 1, best_dist
    of the images successful in both within 1e-2 relative."""
    a = LR.ATTACK
    gp, clf, x, labels, z0 = LR.attack_inputs(LR.ATTACK_SEED)
    ref = LR.attack_reference(LR.ATTACK_SEED)
    assert int((ref["best_iter"] >= 0).sum()) >= 6
    g, model, atk = build(a["latent"], a["kind"], LR.ATTACK_SEED, gp, clf)
    x_adv, info = atk.generate(x, labels, rec_rr=a["R"], nb_iter=a["nb_iter"], learning_rate=a["lr"], c=a["c"], confidence=a["kappa"],
                               z_init=z0, return_info=True)
    ok_d, ok_r = info["best_iter"] >= 0, ref["best_iter"] >= 0
    print("successes: device %d, reference %d" % (ok_d.sum(), ok_r.sum()))
    assert abs(int(ok_d.sum()) - int(ok_r.sum())) <= 1
    both = ok_d & ok_r
    rel = np.abs(info["best_dist"][both] - ref["best_dist"][both]) / ref["best_dist"][both]
    print("best_dist: worst relative difference %.3e" % rel.max())
    assert (rel <= 1e-2).all()
    # and the images do fool the bare classifier
    assert (model.get_logits(x_adv).argmax(axis=1)[ok_d] != labels[ok_d]).all()
    g.close()
    model.close()


def test_refusals():
    """Valid pointers only; the documented codes and words."""
    import torch
    from defensegan_amd import _native, network_builder as nb
    lib = _native.load()
    g, model, atk = build(128, "lin3", 0)
    x, lab = torch.zeros(2, 28, 28, 1, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    xa = torch.empty_like(x)

    def call(gh, ch, B=2, R=1, b1=0.9):
        return lib.dg_latent_attack(gh, ch, x.data_ptr(), lab.data_ptr(), B, R, None, 0, 0, 1, 0.05, b1, 0.999, 1.0, 0.0, None, None, 0, 0,
                                    xa.data_ptr(), None, None, None, None, None, None, None, None, None)
    for arch, bn in ((1, 0), (0, 1)):
        h = C.c_void_p()
        assert lib.dg_create(arch, 128, 64, bn, 0, C.byref(h)) == 0
        assert call(h, model._handle) == -1 and b"not implemented for" in lib.dg_last_error()
        lib.dg_destroy(h)
    other = nb.MLP([nb.Flatten(), nb.Linear(3)], input_shape=(None, 14, 14, 1), device=g._device)
    other.init_like_reference()
    assert call(g._handle, other._handle) == -1 and b"is not the generator's image" in lib.dg_last_error()
    drop = nb.MLP([nb.Flatten(), nb.Dropout(0.5), nb.Linear(3)], device=g._device)
    drop.init_like_reference()
    assert call(g._handle, drop._handle) == -1 and b"Dropout before the logits" in lib.dg_last_error()
    h = C.c_void_p()
    assert lib.dg_create(0, 128, 64, 0, 0, C.byref(h)) == 0
    assert call(h, model._handle) == -2 and b"weights" in lib.dg_last_error()                     # the generator's are incomplete
    lib.dg_destroy(h)
    bare = nb.MLP([nb.Flatten(), nb.Linear(3)], device=g._device)
    bare._ensure()
    assert call(g._handle, bare._handle) == -2 and b"has no weights" in lib.dg_last_error()       # the classifier's
    assert call(g._handle, model._handle, B=0) == -1 and call(g._handle, model._handle, R=0) == -1
    assert call(g._handle, model._handle, B=1 << 20, R=2) == -1 and b"rows per call" in lib.dg_last_error()
    assert call(g._handle, model._handle, b1=1.0) == -1 and b"betas" in lib.dg_last_error()
    mv = torch.zeros(2, 128, device="cuda")
    assert lib.dg_latent_attack(g._handle, model._handle, x.data_ptr(), lab.data_ptr(), 2, 1, None, 0, 0, 1, 0.05, 0.9, 0.999, 1.0, 0.0,
                                mv.data_ptr(), mv.data_ptr(), 1, 0, xa.data_ptr(), None, None, None, None, None, None, None, None, None) == -1
    assert b"needs its best_dist" in lib.dg_last_error()                  # a continued attack without the tracker's state
    assert call(g._handle, model._handle) == 0
    # the Python class: the library's words for a CelebA or Batchnorm gan, a label outside the classes
    from defensegan_amd.gan import CelebADefenseGAN, MnistDefenseGAN
    for bad in (CelebADefenseGAN(cfg={"USE_BN": False}, test_mode=True), MnistDefenseGAN(cfg={"USE_BN": True}, test_mode=True)):
        with pytest.raises(NotImplementedError, match="not implemented for"):
            nb.LatentAttack(model, bad).generate(np.zeros((1, 28, 28, 1), np.float32), [0])
    with pytest.raises(ValueError, match="outside"):
        atk.generate(np.zeros((1, 28, 28, 1), np.float32), [3])
    for m in (other, drop, bare, model):
        m.close()
    g.close()
