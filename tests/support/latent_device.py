"""What the latent-space attack's GPU tests share (tests/test_gpu_latent.py, tests/test_gpu_latent_regimes.py): the handles for the
synthetic generator and the reference's classifier, host / device copies, the 70-row batch, the bit-for-bit comparison."""
import numpy as np

from tests.support import generator_reference as GR
from tests.support import latent_reference as LR


def build(latent, kind, clf_seed, gen_params=None, clf=None):
    """(gan, model, attack) on the device for the synthetic generator and the reference's classifier."""
    from defensegan_amd import network_builder as nb
    from defensegan_amd.gan import MnistDefenseGAN
    g = MnistDefenseGAN(cfg={"USE_BN": False, "LATENT_DIM": latent, "NET_DIM": 64}, test_mode=True, rec_rr=2, rec_iters=3)
    assert g.set_weights(gen_params if gen_params is not None else GR.weights(latent, 64)) == []
    g._ensure_handle()
    model = nb.MLP(LR.mlp_layers(kind), device=g._device)
    model.set_weights((clf or LR.classifier(kind, clf_seed))[1])
    return g, model, nb.LatentAttack(model, g)


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def big():
    """70 rows: B = 7, R = 10, the 10-class classifier, latents drawn on the device."""
    g, model, atk = build(128, "conv10", 0)
    x, lab, _ = LR.draw(128, 7, 10, 3)
    return g, model, atk, dev(x), dev((lab % 10).astype(np.int32))


KEYS = ("x_adv", "best_dist", "best_margin", "best_iter", "best_row", "z")


def same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
