"""``python -m defensegan_amd.train_gan``: train the Defense-GAN (WGAN-GP, the MNIST / F-MNIST generator and critic, USE_BN False) on
the device as the reference's ``train.py`` does through ``train(phase=None)`` (models/gan.py:253-329) -- ``DefenseGANBase.train_gan``.

    python -m defensegan_amd.train_gan --cfg mnist --data_dir data/mnist --out_dir out/gan [--train_iters N] [--resume]

``--cfg``: ``mnist`` / ``f-mnist`` (the reference's shipped settings: latent 128, net_dim 64, batch 50, 5 critic steps, lambda 10,
30 000 iterations) or the path of a configuration file.  ``--data_dir`` holds the four idx-ubyte files.  ``generator.npz`` and
``discriminator.npz`` (parameters under their tflib names plus each optimiser's state) are written to ``--out_dir`` every
``--save_every`` (500) iterations and at the end, as the reference saves; ``--resume`` continues from them.  ``generator.npz`` loads
through ``--init_path`` / ``load_generator``.  Initial weights: tflib's initialisers drawn with ``--init_seed``."""
import argparse
import json
import os
import sys

import numpy as np

from . import config as _config, datasets, synth
from .gan import dataset_gan_dict

DEFAULTS = {"mnist": {"DATASET_NAME": "mnist"}, "f-mnist": {"DATASET_NAME": "f-mnist"}}
SHIPPED = {"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": 64, "BATCH_SIZE": 50, "CRITIC_ITERS": 5, "GRADIENT_PENALTY_LAMBDA": 10.0,
           "MODE": "wgan-gp", "TRAIN_ITERS": 30000}


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m defensegan_amd.train_gan", description=__doc__.split("\n\n")[0])
    ap.add_argument("--cfg", default="mnist", help="mnist, f-mnist or a configuration file")
    ap.add_argument("--data_dir", required=True, help="directory of the idx-ubyte files")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--train_iters", type=int, default=None)
    ap.add_argument("--save_every", type=int, default=500)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--seed", type=int, default=11241990)
    ap.add_argument("--init_seed", type=int, default=0)
    return ap


def chunks(done: int, total: int, every: int):
    """[(start, count)] of the train_gan calls between saves: saves fall on multiples of ``every`` and at the end."""
    out, it = [], int(done)
    while it < total:
        nxt = min(total, (it // every + 1) * every)
        out.append((it, nxt - it))
        it = nxt
    return out


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    gp, dp, sp = (os.path.join(args.out_dir, f) for f in ("generator.npz", "discriminator.npz", "train_state.json"))
    # --resume continues a run that exists; it never starts one over the files of another
    if args.resume and not all(os.path.exists(f) for f in (gp, dp, sp)):
        ap.error("--resume: %s holds no run to continue (generator.npz, discriminator.npz and train_state.json are needed)" % args.out_dir)
    cfg = dict(SHIPPED)
    cfg.update(DEFAULTS[args.cfg] if args.cfg in DEFAULTS else _config.load_config(args.cfg))
    name = str(cfg.get("DATASET_NAME", "mnist")).lower()
    gan = dataset_gan_dict[name](cfg=cfg, test_mode=False)
    gan._check_trainable()
    total = int(gan.train_iters if args.train_iters is None else args.train_iters)
    x, _ = datasets.load_mnist_split(args.data_dir, "train")
    x = datasets.to_generator_range(x, "mnist")
    os.makedirs(args.out_dir, exist_ok=True)
    done = 0
    if args.resume:
        with open(sp) as fh:
            done = int(json.load(fh)["iterations"])
        gan.load_generator_state(gp)
        gan.load_discriminator(dp)
    else:
        gan.set_weights(synth.make_weights(name, seed=args.init_seed, gain=1.0, latent_dim=int(gan.latent_dim), net_dim=int(gan.net_dim)))
        gan.critic.init_like_tflib(seed=args.init_seed)
    for start, count in chunks(done, total, max(1, args.save_every)):
        costs = gan.train_gan(x, train_iters=count, seed=args.seed, start_iter=start)
        gan.save_generator(gp)
        gan.save_discriminator(dp)
        with open(sp, "w") as fh:
            json.dump({"iterations": start + count}, fh)
        print("iter %d  critic cost %.6g  w %.6g  P %.6g  generator cost %.6g" % ((start + count,) + tuple(float(c) for c in costs[-1])),
              flush=True)
    gan.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
