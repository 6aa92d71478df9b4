"""-m gpu: ``python -m defensegan_amd.whitebox --attack_type latent`` end to end on a data_dir of idx files, by the recipe of
tests/test_gpu_whitebox.py (a separable 10-class set drawn from the generator's own range, model F): whitebox -> LatentAttack.generate
-> dg_latent_attack -> model_eval_gan, nothing replaced -- the two calls the test looks into are wrapped, and still run.  The stubbed
flow is tests/test_latent_cpu.py's."""
import os
import pickle

import numpy as np
import pytest

from defensegan_amd import datasets, network_builder as nb, synth, whitebox as wb

pytestmark = pytest.mark.gpu

N_FILE, N_TEST, BATCH, RR = 1200, 24, 16, 2          # load_mnist_split takes the first 5/6 of the train file: 1 000 images


def _write_idx(path, header_bytes, payload):
    with open(path, "wb") as f:
        f.write(b"\0" * header_bytes)
        f.write(np.ascontiguousarray(payload, np.uint8).tobytes())


def test_main_with_attack_type_latent_on_idx_files(tmp_path, monkeypatch):
    from tests.helpers import make_gan
    weights = synth.make_weights("mnist", seed=1234, gain=2.0, bias_range=0.1)
    gan, _ = make_gan("mnist", wseed=1234, gain=2.0, bias_range=0.1, rec_rr=RR, rec_iters=20)
    rs = np.random.RandomState(3)
    protos = rs.standard_normal((10, 128))
    y = rs.randint(0, 10, N_FILE + N_TEST).astype(np.int64)
    z = ((protos[y] + 0.3 * rs.standard_normal((len(y), 128))) * np.sqrt(1.0 / 128)).astype(np.float32)
    x = np.asarray(gan.generate(z)).reshape(-1, 28, 28, 1)
    gan.close()
    d, init = tmp_path / "idx", tmp_path / "gan"
    d.mkdir()
    init.mkdir()
    np.savez(str(init / "generator.npz"), **weights)
    q = lambda a: np.round(a * 255.0)
    _write_idx(str(d / datasets.IDX_FILES["train_images"]), 16, q(x[:N_FILE]))
    _write_idx(str(d / datasets.IDX_FILES["train_labels"]), 8, y[:N_FILE])
    _write_idx(str(d / datasets.IDX_FILES["test_images"]), 16, q(x[N_FILE:]))
    _write_idx(str(d / datasets.IDX_FILES["test_labels"]), 8, y[N_FILE:])
    monkeypatch.chdir(tmp_path)

    seen = {}
    real_generate, real_eval = nb.LatentAttack.generate, wb.gan_defense.model_eval_gan

    def generate(self, x_, y_, **kw):
        out = real_generate(self, x_, y_, **kw)
        seen["attack"] = dict(x=np.asarray(x_), y=np.asarray(y_), kw=kw, x_adv=np.asarray(out), defended=self.model.rec_layer is not None)
        return out

    def model_eval_gan(reconstruct, model, X, Y, batch_size, **kw):
        out = real_eval(reconstruct, model, X, Y, batch_size, **kw)
        seen["eval"] = dict(X=np.asarray(X), Y=np.asarray(Y), batch_size=batch_size, kw=kw, out=out, projected=reconstruct is not None)
        return out

    monkeypatch.setattr(nb.LatentAttack, "generate", generate)
    monkeypatch.setattr(wb.gan_defense, "model_eval_gan", model_eval_gan)
    out = str(tmp_path / "out")
    argv = ["--cfg", "mnist", "--data_dir", str(d), "--init_path", str(init), "--defense_type", "defense_gan", "--attack_type", "latent",
            "--nb_epochs", "2", "--batch_size", str(BATCH), "--rec_rr", str(RR), "--rec_iters", "20", "--latent_iters", "8", "--latent_c", "2.0",
            "--results_dir", out]
    assert wb.main(argv) == 0
    path = os.path.join(out, "0_model=F_nodefense_attack=latent.txt")          # the naming rule's last branch: defense_gan without rec_path
    assert os.path.exists(path), os.listdir(out)
    acc, zero = open(path).read().split()
    # the attack: the original 8-bit test images in generator range, the true labels, the flags
    a = seen["attack"]
    assert a["defended"] and a["x"].shape == (N_TEST, 28, 28, 1) and 0.0 <= a["x"].min() and a["x"].max() <= 1.0
    np.testing.assert_allclose(a["x"], q(x[N_FILE:]) / 255.0, atol=1e-6)
    np.testing.assert_array_equal(a["y"], y[N_FILE:])
    assert a["kw"] == dict(rec_rr=RR, nb_iter=8, learning_rate=0.05, c=2.0, seed=wb.SEED, batch_size=BATCH)
    assert a["x_adv"].shape == a["x"].shape and 0.0 <= a["x_adv"].min() and a["x_adv"].max() <= 1.0 and not np.array_equal(a["x_adv"], a["x"])
    # the evaluation: x_adv through model_eval_gan's projection, and its result is what the file holds
    e = seen["eval"]
    assert e["projected"] and e["batch_size"] == BATCH and e["kw"]["rec_rr"] == RR
    np.testing.assert_array_equal(e["X"], a["x_adv"])
    correct, n, roc = e["out"]
    assert n == N_TEST and zero == "0" and float(acc) == correct / float(n)
    back = pickle.load(open(path.replace(".txt", "_roc.pkl"), "rb"))
    np.testing.assert_array_equal(back[0], y[N_FILE:])
    assert float(acc) == float((back[1] == back[0]).mean())
    print("main: defended accuracy under the latent attack (8 iterations, R = 2) %.4f" % float(acc))
