"""``python -m defensegan_amd.train_classifier``: train one of the reference's classifiers on MNIST as whitebox.py:120-170 does
(cleverhans model_train, Adam, 10 epochs of batch 128 at lr 0.001 by default; ``--adv_tr`` for ``--defense_type adv_tr`` with
FGSM at ``--fgsm_eps_tr``), printing the test accuracy after every epoch, and save the parameters for ``MLP.load_weights``.

    python -m defensegan_amd.train_classifier --data_dir data/mnist --model F --out clf.npz [--adv_tr --fgsm_eps_tr 0.15]

``--data_dir`` holds the four idx-ubyte files (datasets.load_mnist_split: the first 50 000 training images train, the test
split evaluates).  Initial weights: the reference's initialisers drawn with ``--init_seed`` (MLP.init_like_reference)."""
import argparse
import sys

import numpy as np

from . import datasets, network_builder, utils_tf


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m defensegan_amd.train_classifier", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data_dir", required=True, help="directory of the MNIST idx-ubyte files")
    ap.add_argument("--model", default="F", choices=sorted(network_builder.MODELS), help="the reference's model letter")
    ap.add_argument("--nb_epochs", type=int, default=10)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--learning_rate", type=float, default=0.001)
    ap.add_argument("--adv_tr", action="store_true", help="adversarial training (whitebox.py --defense_type adv_tr)")
    ap.add_argument("--fgsm_eps_tr", type=float, default=0.15, help="FGSM eps of adversarial training (blackbox.py:733)")
    ap.add_argument("--init_seed", type=int, default=0, help="seed of the initial weights")
    ap.add_argument("--seed", type=int, default=11241990, help="seed of the Dropout masks")
    ap.add_argument("--eval_batch", type=int, default=1000, help="images per evaluation batch")
    ap.add_argument("--out", default="clf.npz", help=".npz to write the trained parameters to")
    return ap


def accuracy(model, x, y, batch: int) -> float:
    correct = 0
    for s in range(0, len(x), batch):
        c, _, _ = model.eval_batch(x[s:s + batch], labels=y[s:s + batch])
        correct += c
    return correct / float(len(x))


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    x_tr, y_tr = datasets.load_mnist_split(args.data_dir, "train")
    x_te, y_te = datasets.load_mnist_split(args.data_dir, "test")
    x_tr, x_te = datasets.to_generator_range(x_tr, "mnist"), datasets.to_generator_range(x_te, "mnist")
    y_tr, y_te = np.asarray(y_tr, np.int32), np.asarray(y_te, np.int32)
    model = network_builder.MODELS[args.model](input_shape=(None,) + tuple(x_tr.shape[1:]))
    model.init_like_reference(seed=args.init_seed)

    def evaluate():
        print("Test accuracy on legitimate examples: %0.4f" % accuracy(model, x_te, y_te, args.eval_batch), flush=True)

    utils_tf.model_train(model, x_tr, y_tr, args={"nb_epochs": args.nb_epochs, "batch_size": args.batch_size,
                                                  "learning_rate": args.learning_rate},
                         rng=np.random.RandomState(utils_tf.WHITEBOX_RNG_SEED), adv_eps=args.fgsm_eps_tr if args.adv_tr else None,
                         adv_clip=(0.0, 1.0), evaluate=evaluate, seed=args.seed)
    model.save_weights(args.out)
    print("saved %s (model %s, %d parameter tensors)" % (args.out, args.model, 2 * len(model.param_shapes())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
