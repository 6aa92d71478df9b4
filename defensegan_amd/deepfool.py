"""``python -m defensegan_amd.deepfool``: the DeepFool robustness of a classifier of the zoo (Moosavi-Dezfooli et al. 2016): how far,
in L2 and without choosing a budget, its test images lie from the decision boundary.  Not in the reference.

    deepfool    trains the classifier as ``whitebox`` does (``--adv_tr``: with FGSM inputs), or loads it (``--clf``), runs
                ``attacks.robustness`` on the ORIGINAL test images and returns its dict: rho = mean ||r||_2 / ||x||_2, mean_l2, fooled,
                mean_iters.  With a generator and ``defense_type`` 'defense_gan' it adds ``defended_accuracy``: the accuracy of the
                DEFENDED model (``gan_defense.model_eval_gan``) on the DeepFool images crafted against the BARE classifier --
                DeepFool through the projection would need BPDA and is not implemented.
    main        the flags, the printed dict and its JSON file

    python -m defensegan_amd.deepfool --cfg mnist --data_dir data/mnist --model F --num_tests 1000
    python -m defensegan_amd.deepfool --cfg mnist --data_dir data/mnist --model F --adv_tr --clf clf_f_advtr.npz
    python -m defensegan_amd.deepfool --cfg mnist --data_dir data/mnist --model F --init_path output/gans/mnist --defense_type defense_gan

``whitebox --attack_type`` does NOT take 'deepfool': DeepFool has no budget and reports distances, not an accuracy under ``eps``, so it
has this command of its own (and 'deepfool' stays whitebox's example of an unknown attack type)."""
import argparse
import json
import os
import sys

import numpy as np

from . import attacks, config, datasets, gan_defense, network_builder
from .blackbox import SEED, _labels, result_path


def deepfool(model, data, gan=None, defense_type="none", clf_path=None, batch_size=128, learning_rate=0.001, nb_epochs=10, num_tests=-1,
             num_train=-1, fgsm_eps_tr=0.15, seed=SEED, init_seed=0, deepfool_params=None):
    """``data`` = (train_images, train_labels, test_images, test_labels) in generator range.  ``defense_type``: 'none', 'adv_tr' (how the
    classifier is trained) or 'defense_gan' (trained as 'none'; ``gan`` then judges the DeepFool images).  ``clf_path``: an ``.npz`` of
    ``MLP.save_weights`` to load instead of training.  Returns ``robustness``'s dict, plus ``clean_accuracy`` and, with
    'defense_gan', ``defended_accuracy``."""
    if defense_type not in ("none", "adv_tr", "defense_gan"):
        raise ValueError("defense_type must be none, adv_tr or defense_gan, got %r" % (defense_type,))
    if defense_type == "defense_gan" and gan is None:
        raise ValueError("defense_type defense_gan needs a gan")
    params = dict(deepfool_params or {})
    attacks.DeepFool.parse_params(params)                          # refusals before anything is trained
    x_tr, y_tr, x_te, y_te = data
    y_te = _labels(y_te)
    if num_tests > 0:
        x_te, y_te = x_te[:num_tests], y_te[:num_tests]
    model._ensure()
    if clf_path:
        model.load_weights(clf_path)
    else:
        from .whitebox import whitebox
        whitebox(None, model, (x_tr, y_tr, x_te, y_te), batch_size=batch_size, learning_rate=learning_rate, nb_epochs=nb_epochs,
                 attack_type=None, defense_type="adv_tr" if defense_type == "adv_tr" else "none", num_train=num_train,
                 fgsm_eps_tr=fgsm_eps_tr, seed=seed, init_seed=init_seed)
    correct, n, _ = gan_defense.model_eval_gan(None, model, x_te, y_te, batch_size, compute_diffs=False)
    out = attacks.robustness(model, x_te, **params)
    out["clean_accuracy"] = correct / float(max(n, 1))
    if defense_type == "defense_gan":
        x_adv = attacks.DeepFool(model).generate(np.asarray(x_te, np.float32), **params)
        correct, n, _ = gan_defense.model_eval_gan(gan.reconstruct, model, x_adv, y_te, batch_size, rec_rr=int(gan.rec_rr), seed=seed)
        out["defended_accuracy"] = correct / float(max(n, 1))
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = config.add_rec_flags(argparse.ArgumentParser(prog="python -m defensegan_amd.deepfool", description=__doc__.split("\n\n")[0]))
    ap.add_argument("--data_dir", required=True, help="directory of the dataset's idx-ubyte files (mnist, f-mnist)")
    ap.add_argument("--model", default="F", choices=sorted(network_builder.MODELS), help="The classifier model.")
    ap.add_argument("--clf", default=None, help="classifier weights (.npz of MLP.save_weights); without it the classifier is trained as whitebox does")
    ap.add_argument("--adv_tr", action="store_true", help="train with FGSM inputs (defense_type adv_tr)")
    ap.add_argument("--defense_type", default="none", choices=["none", "defense_gan", "adv_tr"], help="Type of defense")
    ap.add_argument("--init_path", default=None, help="generator weights, for --defense_type defense_gan")
    ap.add_argument("--num_tests", type=int, default=-1, help="Number of test samples.")
    ap.add_argument("--num_train", type=int, default=-1, help="Number of training data to load.")
    ap.add_argument("--nb_classes", type=int, default=10, help="Number of classes.")
    ap.add_argument("--learning_rate", type=float, default=0.001, help="Learning rate for training.")
    ap.add_argument("--nb_epochs", type=int, default=10, help="Number of epochs to train model.")
    ap.add_argument("--fgsm_eps_tr", type=float, default=0.15, help="FGSM epsilon for adversarial training.")
    ap.add_argument("--nb_candidate", type=int, default=10, help="DeepFool: classes considered per image")
    ap.add_argument("--overshoot", type=float, default=0.02, help="DeepFool: the final perturbation is (1 + overshoot) r")
    ap.add_argument("--max_iter", type=int, default=50, help="DeepFool: iterations at most")
    ap.add_argument("--results_dir", default=None, help="The final subdirectory of the results.")
    ap.add_argument("--seed", type=int, default=SEED, help="seed of the Dropout masks and the latent draws")
    ap.add_argument("--init_seed", type=int, default=0, help="seed of the classifier's initial weights")
    return ap


def resolve_defense(args):
    """``--adv_tr`` is ``--defense_type adv_tr``; together with defense_gan it is refused."""
    if args.adv_tr and args.defense_type == "defense_gan":
        raise SystemExit("--adv_tr and --defense_type defense_gan exclude each other")
    return "adv_tr" if args.adv_tr else args.defense_type


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    defense_type = resolve_defense(args)
    from .__main__ import resolve_cfg
    from .gan import gan_from_config
    cfg_path = resolve_cfg(args.cfg)
    cfg = config.load_config(cfg_path)
    dataset_name = str(cfg.get("DATASET_NAME", "mnist")).lower()
    if dataset_name not in ("mnist", "f-mnist"):
        raise SystemExit("python -m defensegan_amd.deepfool loads mnist and f-mnist; call deepfool() with your own arrays for %s" % dataset_name)
    rp = config.resolve_rec_params(cfg, args)
    gan = None
    if defense_type == "defense_gan":
        if not args.init_path:
            raise SystemExit("--defense_type defense_gan needs the generator (--init_path)")
        gan = gan_from_config(cfg_path, rec_rr=rp["rec_rr"], rec_iters=rp["rec_iters"], rec_lr=rp["rec_lr"])
        gan.load_generator(args.init_path)
    x_tr, y_tr = datasets.load_mnist_split(args.data_dir, "train")
    x_te, y_te = datasets.load_mnist_split(args.data_dir, "test")
    x_tr, x_te = datasets.to_generator_range(x_tr, dataset_name), datasets.to_generator_range(x_te, dataset_name)
    model = network_builder.MODELS[args.model](input_shape=(None,) + tuple(x_tr.shape[1:]), nb_classes=args.nb_classes)
    out = deepfool(model, (x_tr, y_tr, x_te, y_te), gan=gan, defense_type=defense_type, clf_path=args.clf, batch_size=rp["batch_size"],
                   learning_rate=args.learning_rate, nb_epochs=args.nb_epochs, num_tests=args.num_tests, num_train=args.num_train,
                   fgsm_eps_tr=args.fgsm_eps_tr, seed=args.seed, init_seed=args.init_seed,
                   deepfool_params={"nb_candidate": args.nb_candidate, "overshoot": args.overshoot, "max_iter": args.max_iter})
    print(json.dumps(out, sort_keys=True))
    name = "model={}_{}{}deepfool.json".format(args.model, "numtest={}_".format(args.num_tests) if args.num_tests > -1 else "",
                                               {"none": "nodefense_", "adv_tr": "advTrEps={:.2f}_".format(args.fgsm_eps_tr),
                                                "defense_gan": "defense=gan_"}[defense_type])
    path = result_path(os.path.join("results", "deepfool_{}_{}".format(defense_type, dataset_name)), name, args.results_dir)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, sort_keys=True)
        f.write("\n")
    print("[*] saved the robustness in {}".format(path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
