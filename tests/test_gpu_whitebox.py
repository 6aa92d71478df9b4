"""-m gpu: the white-box driver end to end on the device (defensegan_amd/whitebox.py), by the recipe of tests/test_gpu_bpda.py's and
tests/test_gpu_blackbox.py's end-to-end tests: a separable 10-class set drawn from the generator's own range (x = G(z), z a class
prototype plus noise), model F for 3 epochs on 2 000 images, 64 test images, the projection at R = 2, L = 20.  Only orderings are
asserted; each run prints its accuracy (pytest -s shows them).  The stubbed flow is tests/test_whitebox_cpu.py's."""
import argparse
import os
import pickle
import warnings

import numpy as np
import pytest

from defensegan_amd import datasets, network_builder as nb, whitebox as wb
from tests.helpers import make_gan

pytestmark = pytest.mark.gpu

N_TRAIN, N_TEST, BATCH = 2000, 64, 128
KW = dict(batch_size=BATCH, learning_rate=0.001, nb_epochs=3, eps=0.3)


@pytest.fixture(scope="module")
def world():
    """The generator, the data, and a cache of whitebox() runs keyed by (defense, attack): each runs once and is never modified."""
    import torch
    gan, _ = make_gan("mnist", wseed=1234, gain=2.0, bias_range=0.1, rec_rr=2, rec_iters=20, rec_lr=10.0)
    rs = np.random.RandomState(3)
    protos = rs.standard_normal((10, 128))
    y = rs.randint(0, 10, N_TRAIN + N_TEST).astype(np.int64)
    z = ((protos[y] + 0.3 * rs.standard_normal((len(y), 128))) * np.sqrt(1.0 / 128)).astype(np.float32)
    x = gan.generate(z)
    x = (x if isinstance(x, np.ndarray) else x.cpu().numpy()).reshape(-1, 28, 28, 1).astype(np.float32)
    data = (x[:N_TRAIN], y[:N_TRAIN], x[N_TRAIN:], y[N_TRAIN:])
    runs = {}

    def run(defense, attack, tmp_path, **kw):
        if (defense, attack) not in runs:
            model = nb.model_f()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                         # the zero-gradient FGSM's note
                out = wb.whitebox(gan if defense == "defense_gan" else None, model, data, attack_type=attack, defense_type=defense,
                                  **dict(KW, **kw))
            flags = argparse.Namespace(defense_type=defense, attack_type=attack, dataset_name="mnist", rec_path=None, train_on_recs=False,
                                       num_tests=-1, num_train=-1, model="F", fgsm_eps_tr=0.15)
            results_dir, name = wb.get_results_dir_filename(flags, gan)
            path = wb.result_path(os.path.join(str(tmp_path), results_dir), name, "run")
            wb.write_results(path, out)
            clean, _, _ = model.eval_batch(data[2], labels=data[3])
            runs[(defense, attack)] = dict(out=out, path=path, clean=clean / float(N_TEST))
            print("%s + %s: clean accuracy %.4f, accuracy under attack %.4f" % (defense, attack, clean / float(N_TEST), out[0]))
            model.close()
        return runs[(defense, attack)]
    yield dict(gan=gan, data=data, run=run)
    torch.cuda.synchronize()
    gan.close()


def _check_file(r, defense, attack):
    assert os.path.basename(r["path"]) == "0_model=F_%sattack=%s.txt" % ("advTrEps=0.15" if defense == "adv_tr" else "nodefense_", attack)
    assert open(r["path"]).read() == str(r["out"][0]) + " 0 \n"
    assert os.path.exists(r["path"].replace(".txt", "_roc.pkl")) == (defense == "defense_gan")


@pytest.mark.parametrize("defense,attack,kw", [
    ("none", "fgsm", {}), ("none", "rand_fgsm", {}), ("none", "pgd", {}), ("adv_tr", "pgd", {}),
    ("none", "cw", {"attack_params": {"max_iterations": 10}})])
def test_bare_flows_return_and_write_their_file(world, tmp_path, defense, attack, kw):
    r = world["run"](defense, attack, tmp_path, **kw)
    acc, zero, roc = r["out"]
    assert 0.0 <= acc <= 1.0 and zero == 0 and roc is None
    _check_file(r, defense, attack)
    assert r["clean"] >= 0.95


def test_pgd_is_at_least_as_strong_as_fgsm_on_the_bare_model(world, tmp_path):
    fgsm, pgd = world["run"]("none", "fgsm", tmp_path), world["run"]("none", "pgd", tmp_path)
    print("bare model F: accuracy under FGSM %.4f, under PGD %.4f" % (fgsm["out"][0], pgd["out"][0]))
    assert fgsm["clean"] >= 0.95 and pgd["clean"] >= 0.95
    assert pgd["out"][0] <= fgsm["out"][0]


def test_defended_flows_return_the_roc_triple_and_bpda_beats_the_zero_gradient_fgsm(world, tmp_path):
    gan, (_, _, xte, yte) = world["gan"], world["data"]
    fgsm = world["run"]("defense_gan", "fgsm", tmp_path, batch_size=32)
    bpda = world["run"]("defense_gan", "bpda", tmp_path, batch_size=32, attack_params={"nb_iter": 5})
    for r, attack in ((fgsm, "fgsm"), (bpda, "bpda")):
        acc, zero, (labels, preds, diffs) = r["out"]
        assert zero == 0 and labels.shape == preds.shape == diffs.shape == (N_TEST,) and diffs.dtype == np.float32
        np.testing.assert_array_equal(labels, yte)
        assert acc == float((preds == labels).mean())
        _check_file(r, "defense_gan", attack)
        back = pickle.load(open(r["path"].replace(".txt", "_roc.pkl"), "rb"))
        for a, b in zip(back, r["out"][2]):
            np.testing.assert_array_equal(a, b)
        assert r["clean"] >= 0.95
    # the zero-gradient FGSM returned clip(x) = x: its diffs are mean((x - rec)^2) of the evaluation's own projection
    rec = gan.reconstruct(xte[:16], seed=wb.SEED, first_row=0)
    rec = rec if isinstance(rec, np.ndarray) else rec.cpu().numpy()
    np.testing.assert_allclose(fgsm["out"][2][2][:16], ((xte[:16] - rec) ** 2).mean(axis=(1, 2, 3)), rtol=1e-5)
    print("defended accuracy under the zero-gradient FGSM %.4f, under BPDA(eps 0.3, nb_iter 5) %.4f" % (fgsm["out"][0], bpda["out"][0]))
    assert bpda["out"][0] < fgsm["out"][0]


def _write_idx(path, header_bytes, payload):
    with open(path, "wb") as f:
        f.write(b"\0" * header_bytes)
        f.write(np.ascontiguousarray(payload, np.uint8).tobytes())


def test_main_on_a_data_dir_of_idx_files(world, tmp_path, monkeypatch):
    xtr, ytr, xte, yte = world["data"]
    d = tmp_path / "idx"
    d.mkdir()
    # load_mnist_split takes the first 5/6 of the train file as the train split: 2 400 images give the 2 000 of the other tests
    q = lambda a: np.round(a * 255.0)
    xall, yall = np.concatenate([xtr, xtr[:400]]), np.concatenate([ytr, ytr[:400]])
    _write_idx(str(d / datasets.IDX_FILES["train_images"]), 16, q(xall))
    _write_idx(str(d / datasets.IDX_FILES["train_labels"]), 8, yall)
    _write_idx(str(d / datasets.IDX_FILES["test_images"]), 16, q(xte))
    _write_idx(str(d / datasets.IDX_FILES["test_labels"]), 8, yte)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "out")
    argv = ["--cfg", "mnist", "--data_dir", str(d), "--defense_type", "none", "--attack_type", "pgd", "--nb_epochs", "3", "--batch_size",
            str(BATCH), "--nb_iter", "5", "--results_dir", out]
    assert wb.main(argv) == 0
    path = os.path.join(out, "0_model=F_nodefense_attack=pgd.txt")
    acc, zero = open(path).read().split()
    assert zero == "0" and 0.0 <= float(acc) <= 1.0
    print("main: accuracy under PGD(nb_iter 5) on the 8-bit images %.4f" % float(acc))
    assert wb.main(argv) == 0 and os.path.exists(os.path.join(out, "1_model=F_nodefense_attack=pgd.txt"))          # the counter
