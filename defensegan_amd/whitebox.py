"""``python -m defensegan_amd.whitebox``: the reference's white-box flow (whitebox.py:56-306) with every tensor operation on the
device:

    whitebox    trains the classifier (cleverhans model_train; ``adv_tr`` adds FGSM inputs; ``train_on_recs`` trains on cached
                reconstructions), attacks the ORIGINAL test images (fgsm, rand_fgsm, cw -- and pgd and jsma on a bare model, bpda and
                latent on a defended one, spsa on either, which the reference has not) and measures the accuracy on the adversarial images, through the
                Defense-GAN projection for ``defense_gan`` (with the ROC triple)                       whitebox.py:56-233
    main        the flags and the result files of whitebox.py:236-392

    python -m defensegan_amd.whitebox --cfg mnist --data_dir data/mnist --defense_type none --attack_type pgd
    python -m defensegan_amd.whitebox --cfg mnist --data_dir data/mnist --init_path output/gans/mnist \\
        --defense_type defense_gan --attack_type bpda --results_dir run0
    python -m defensegan_amd.whitebox --cfg mnist --data_dir data/mnist --init_path output/gans/mnist \\
        --defense_type defense_gan --attack_type latent --latent_iters 100 --rec_rr 10
    python -m defensegan_amd.whitebox --cfg mnist --data_dir data/mnist --init_path output/gans/mnist \\
        --defense_type defense_gan --attack_type spsa --spsa_samples 32 --spsa_delta 0.01 --num_tests 100
    python -m defensegan_amd.whitebox --cfg mnist --data_dir data/mnist --defense_type none --attack_type ead --ead_beta 1e-2 --ead_rule L1
    python -m defensegan_amd.whitebox --cfg mnist --data_dir data/mnist --defense_type none --attack_type jsma --jsma_theta 1.0 --jsma_gamma 0.1

Kept from the reference: ``RandomState([11, 24, 1990])`` for the training schedule; the clean accuracy on the (reconstructed) test
split printed after every epoch; with ``defense_gan`` the reconstruction layer is attached AFTER training and BEFORE the attack
is built, so FGSM differentiates through it, sees a zero gradient and returns ``clip(x)`` (network_builder._REC_GRADIENT_NOTE);
``rand`` in the attack type takes one random sign step of ``alpha`` first and ``alpha`` off the budget.  Not reproduced:
``online_training`` (NotImplementedError)."""
import argparse
import os
import sys

import numpy as np

from . import config, datasets, gan_defense, network_builder, py2pickle, utils_tf
from .blackbox import SEED, _Phase, _accuracy, _labels, load_recs, result_path

ATTACKS = ("fgsm", "cw", "pgd", "bpda", "latent", "spsa", "ead", "jsma")
# whitebox.py:203-209; 'feed' is TensorFlow's business
CW_PARAMS = {"binary_search_steps": 1, "max_iterations": 100, "learning_rate": 10.0, "initial_const": 100}
# the elastic-net attack (network_builder.ElasticNetMethod): this setting is chosen here, not taken from the reference, which has no ead
EAD_PARAMS = {"binary_search_steps": 5, "max_iterations": 100, "learning_rate": 1e-2, "initial_const": 1.0}
EAD_DEFAULTS = {"ead_beta": 1e-3, "ead_rule": "EN"}
ITERATIVE_DEFAULTS = {"eps_iter": 0.05, "nb_iter": 10, "eot_samples": 1}
# the latent-space attack (network_builder.LatentAttack): Adam steps on z, their learning rate, the weight of the classification term
LATENT_DEFAULTS = {"latent_iters": 100, "latent_lr": 0.05, "latent_c": 1.0}
# the score-based black-box attack (network_builder.SPSA): direction pairs per iteration and the probe size; eps_iter and nb_iter as pgd's
SPSA_DEFAULTS = {"spsa_samples": 32, "spsa_delta": 0.01}
# the saliency-map attack (network_builder.SaliencyMapMethod): the step per feature and the share of the features it may move; chosen
# here, the reference has no jsma (cleverhans' own default is gamma 1.0: every feature)
JSMA_DEFAULTS = {"jsma_theta": 1.0, "jsma_gamma": 0.1}
PGD_CALL_IMAGES = 10000                       # images per dg_pgd call: bounds the kept activations, not the result


def attack_kind(attack_type):
    """None for no attack (None / 'none'), else (kind in ATTACKS, rand): ``rand`` when the type contains 'rand'
    (whitebox.py:192), the kind by the reference's tests ('fgsm' in the type, whitebox.py:198; 'cw' exactly, :201)."""
    if attack_type is None or str(attack_type).lower() == "none":
        return None
    t = str(attack_type).lower()
    rand = "rand" in t
    if "fgsm" in t:
        return "fgsm", rand
    base = t.replace("rand", "").strip("_+")
    if base in ATTACKS and not (rand and base in ("cw", "latent", "spsa", "ead", "jsma")):
        return base, rand
    raise ValueError("unknown attack_type %r: fgsm, rand_fgsm, cw, ead, pgd or jsma (defense_type none / adv_tr), bpda or latent (defense_gan), spsa" % (attack_type,))


def attack_ord_value(attack_ord, kind=None):
    """``attack_ord`` (np.inf, 1, 2 or their names 'inf', '1', '2') as np.inf or an int, checked against the attack ``kind``: fgsm
    takes 1 and 2 (``FastGradientMethod``'s ord), pgd and bpda take 2 (1 is NotImplementedError: the L1 projection needs a sort), cw
    is an L2 attack already and takes none, as do latent and spsa; ead is the L1 attack and jsma the L0 attack, and they take none either."""
    who = "attack_ord" if kind is None else "attack_ord with attack_type %s" % kind
    allowed = {"fgsm": (np.inf, 1, 2), "pgd": (np.inf, 2), "bpda": (np.inf, 2), "cw": (np.inf,), "ead": (np.inf,), "latent": (np.inf,), "spsa": (np.inf,), "jsma": (np.inf,)}.get(kind, (np.inf, 1, 2))
    return network_builder._attack_ord(attack_ord, allowed, who)


def _attack_params(kind, attack_params):
    """The overrides ``attack_params`` holds for this attack: eps_iter / nb_iter (pgd, bpda), eot_samples (bpda), any
    CarliniWagnerL2 parameter (cw), latent_iters / latent_lr / latent_c (latent), eps_iter / nb_iter / spsa_samples / spsa_delta (spsa), ead_beta / ead_rule and any ElasticNetMethod parameter (ead), jsma_theta / jsma_gamma (jsma).  Values of None and the iterative attacks' keys given to another attack are left out."""
    given = {k: v for k, v in (attack_params or {}).items() if v is not None}
    known = (set(ITERATIVE_DEFAULTS) | set(network_builder.CarliniWagnerL2.DEFAULTS) | set(LATENT_DEFAULTS) | set(SPSA_DEFAULTS)
             | set(EAD_DEFAULTS) | set(network_builder.ElasticNetMethod.DEFAULTS) | set(JSMA_DEFAULTS))
    if set(given) - known:
        raise ValueError("unknown attack_params: %s" % sorted(set(given) - known))
    if kind == "cw":
        return {k: v for k, v in given.items() if k in network_builder.CarliniWagnerL2.DEFAULTS}
    if kind == "ead":
        out = {k: v for k, v in given.items() if k in network_builder.ElasticNetMethod.DEFAULTS}
        out.setdefault("beta", given.get("ead_beta", EAD_DEFAULTS["ead_beta"]))
        out.setdefault("decision_rule", given.get("ead_rule", EAD_DEFAULTS["ead_rule"]))
        return out
    if kind == "latent":
        return {k: given.get(k, d) for k, d in LATENT_DEFAULTS.items()}
    if kind == "jsma":
        return {k: given.get(k, d) for k, d in JSMA_DEFAULTS.items()}
    keys = {"pgd": ("eps_iter", "nb_iter"), "bpda": ("eps_iter", "nb_iter", "eot_samples"), "spsa": ("eps_iter", "nb_iter")}.get(kind, ())
    out = {k: given.get(k, ITERATIVE_DEFAULTS[k]) for k in keys}
    if kind == "spsa":
        out.update({k: given.get(k, d) for k, d in SPSA_DEFAULTS.items()})
    return out


def whitebox(gan, model, data, rec_data_path=None, batch_size=128, learning_rate=0.001, nb_epochs=10, eps=0.3, alpha=0.05,
             online_training=False, train_on_recs=False, test_on_dev=True, attack_type="fgsm", defense_type="none", num_tests=-1,
             num_train=-1, fgsm_eps_tr=0.15, same_init=False, recs=None, attack_params=None, seed=SEED, init_seed=0, phases=None,
             attack_ord=np.inf, norms=None):
    """whitebox.py:56-233.  ``gan``: a DefenseGANBase with its generator loaded, or None (``defense_type`` 'none' and 'adv_tr' need
    none); ``model``: the classifier's MLP (initialised with the reference's initialisers from ``init_seed`` when its weights are not
    set); ``data`` = (train_images, train_labels, test_images, test_labels), the ORIGINAL images in generator range, labels one-hot
    or class indices.  ``num_tests`` / ``num_train`` > 0 truncate the splits.

    Training: on the originals, or -- ``defense_gan`` with ``train_on_recs`` -- on ``recs`` = (train, train_labels, test, test_labels),
    the cached reconstructions ``rec_data_path`` points to in the reference (``train_on_recs`` without them is refused,
    whitebox.py:90-91); after every epoch the clean accuracy on the test split of what was trained on is printed
    (whitebox.py:126-135).  ``adv_tr`` adds FGSM(``fgsm_eps_tr``) inputs clipped to [0, 1] ([-1, 1] for CelebA).  With
    ``attack_type`` None (or 'none') the function returns ``(training accuracy, 0, None)`` here (whitebox.py:172-173).

    Attacks, always from the original test images (``eps`` the budget, ``rand``: whitebox.py:192-196 with ``alpha``, the signs drawn
    from the training ``RandomState``):
      fgsm, rand_fgsm   FastGradientMethod, the label the model's own prediction (whitebox.py:198-200)
      cw                CarliniWagnerL2 with binary_search_steps 1, max_iterations 100, learning_rate 10, initial_const 100
      ead               ElasticNetMethod (the L1 attack) with EAD_PARAMS: binary_search_steps 5, max_iterations 100, learning_rate
                        0.01, initial_const 1 -- chosen here, the reference has no ead; ``attack_params`` ead_beta (1e-3), ead_rule
                        ('EN') and any ElasticNetMethod parameter.  ``norms``: a dict that receives 'l1' and 'l2', the means of
                        ||x_adv - x||_1 and ||x_adv - x||_2 over the images the attack succeeded on (NaN when on none), and 'successes'
      pgd               ProjectedGradientDescent on the true labels: 'none' and 'adv_tr' only
      jsma              SaliencyMapMethod (the L0 attack), 'none' and 'adv_tr' only; the target of image i is (y_i + 1 + r_i) % nb_classes,
                        r_i drawn from the training ``RandomState`` (``jsma_targets``): never the true class.  ``attack_params``
                        jsma_theta (1.0) and jsma_gamma (0.1) -- chosen here, the reference has no jsma.  ``norms``: a dict that
                        receives 'success_rate' (the share of images whose class at x_adv is the target) and 'l0' (the mean of
                        n_changed / F over those images, NaN when there is none)
      bpda              BPDA on the true labels: 'defense_gan' only
      latent            LatentAttack on the true labels, ``gan.rec_rr`` restarts per image: 'defense_gan' only.  x_adv = G(z) lies in
                        the generator's range, not in the ``eps`` ball; ``attack_params`` latent_iters (100), latent_lr (0.05), latent_c (1)
      spsa              SPSA on the true labels, from the model's logits alone: any defense type (with 'defense_gan' every query goes
                        through the projection: nb_iter (2 spsa_samples + 1) + 1 projections per image); ``attack_params`` eps_iter,
                        nb_iter, spsa_samples (32), spsa_delta (0.01)
    ``attack_params`` overrides ``eps_iter`` (0.05), ``nb_iter`` (10), ``eot_samples`` (1) of pgd / bpda and any CarliniWagnerL2
    parameter.  pgd with 'defense_gan' or bpda without it is a ValueError.  ``attack_ord`` (default np.inf): 2 runs pgd / bpda in an
    L2 ball of radius ``eps`` (their ``ord``), 1 or 2 runs fgsm / rand_fgsm as FGM with that norm; 1 with pgd / bpda is
    NotImplementedError, any value but np.inf with cw or ead a ValueError.

    ``defense_gan``: the reconstruction layer is attached after training (``same_init``: with one sigma = 1 draw of
    [batch_size * rec_rr, latent_dim] as every batch's z0), the attack is built on that model, and the accuracy comes from
    ``gan_defense.model_eval_gan`` with ``roc_info = [labels, preds, diffs]``, diffs = mean((x_adv - rec)^2).  FGSM then sees the
    zero gradient and returns clip(x), as in the reference.  DEVIATION for cw: the reference builds CarliniWagnerL2 on the defended
    model as well, where the zero gradient reduces it to the tanh round trip of x at a hundred defended evaluations per batch;
    ``CarliniWagnerL2`` refuses such a model here, so the attack is built BEFORE ``add_rec_model``, sees the bare classifier, and its
    images are then evaluated through the projection (one printed line says so).  ead behaves as cw does: ``ElasticNetMethod`` refuses a
    defended model for the same reason, is built before ``add_rec_model``, and the same notice is printed.

    Returns ``(accuracy on the adversarial images, 0, roc_info or None)``.  ``test_on_dev`` and ``rec_data_path`` are the data
    loader's business and are accepted for signature compatibility.  ``phases``: a dict that receives the seconds spent in
    'training', 'attack' and 'evaluation' (tools/whitebox_time.py)."""
    defense_type = defense_type or "none"
    if defense_type not in ("none", "adv_tr", "defense_gan"):
        raise ValueError("defense_type must be none, adv_tr or defense_gan, got %r" % (defense_type,))
    defended = defense_type == "defense_gan"
    if defended and gan is None:
        raise ValueError("defense_type defense_gan needs a gan")
    kind = attack_kind(attack_type)
    if kind is not None:
        if kind[0] == "pgd" and defended:
            raise ValueError("attack_type pgd differentiates a bare classifier (defense_type none or adv_tr); with defense_gan the "
                             "iterative attack is bpda")
        if kind[0] == "jsma" and defended:
            raise ValueError("attack_type jsma differentiates a bare classifier (defense_type none or adv_tr): the gradient through the "
                             "projection is zero and no pair of features is admissible")
        if kind[0] == "bpda" and not defended:
            raise ValueError("attack_type bpda needs the projection (defense_type defense_gan); on a bare classifier (%s) the "
                             "iterative attack is pgd" % defense_type)
        if kind[0] == "latent" and not defended:
            raise ValueError("attack_type latent searches the generator's range and needs the projection (defense_type defense_gan), "
                             "not %s" % defense_type)
        if kind[0] in ("bpda", "spsa") and same_init:
            raise ValueError("attack_type %s draws fresh latents for every projection: not with same_init" % kind[0])
        extra = _attack_params(kind[0], attack_params)
        attack_ord = attack_ord_value(attack_ord, kind[0])
        if attack_ord != np.inf and kind[0] in ("pgd", "bpda"):
            extra["ord"] = attack_ord
    if online_training:
        raise NotImplementedError("online_training (training through the Defense-GAN projection) is not implemented; the reference's "
                                  "whitebox() takes the flag and never trains through the projection either (it only enters the "
                                  "assert of whitebox.py:90-91): train on cached reconstructions (recs=..., train_on_recs)")
    if defended and train_on_recs and recs is None:
        raise ValueError("train_on_recs needs the cached reconstructions (recs=...), as whitebox.py:90-91 asserts")

    train_images, train_labels, test_images, test_labels = data
    train_labels, test_labels = _labels(train_labels), _labels(test_labels)
    rec_test_images, rec_test_labels = test_images, test_labels
    if defended and train_on_recs:
        train_images, train_labels, rec_test_images, rec_test_labels = recs[0], _labels(recs[1]), recs[2], _labels(recs[3])
    if num_tests > 0:
        test_images, test_labels = test_images[:num_tests], test_labels[:num_tests]
        rec_test_images, rec_test_labels = rec_test_images[:num_tests], rec_test_labels[:num_tests]
    if num_train > 0:
        train_images, train_labels = train_images[:num_train], train_labels[:num_train]
    is_celeba = gan is not None and "celeba" in str(gan.dataset_name or gan.arch_name)
    min_val = -1.0 if is_celeba else 0.0

    model._ensure()
    if not model._weights_set:
        model.init_like_reference(seed=int(init_seed))
    dev = model._device

    def evaluate():
        print("Test accuracy on legitimate examples: %0.4f" % _accuracy(model, rec_test_images, rec_test_labels, batch_size))

    rng = np.random.RandomState(utils_tf.WHITEBOX_RNG_SEED)
    with _Phase(phases, "training", dev):
        utils_tf.model_train(model, train_images, train_labels,
                             args={"nb_epochs": nb_epochs, "batch_size": batch_size, "learning_rate": learning_rate}, rng=rng,
                             adv_eps=fgsm_eps_tr if defense_type == "adv_tr" else None, adv_clip=(min_val, 1.0), evaluate=evaluate,
                             seed=seed)
        acc = _accuracy(model, train_images, train_labels, batch_size)
    print("[#] Accuracy on clean examples {}".format(acc))
    if kind is None:
        return acc, 0, None
    kind, rand = kind

    attack = None
    if kind in ("cw", "ead") and defended:
        attack = (network_builder.CarliniWagnerL2 if kind == "cw" else network_builder.ElasticNetMethod)(model)
        print("[*] " + kind + " with defense_gan: the attack is built before the reconstruction layer is attached and sees the BARE classifier "
              "(the reference's sees a zero gradient); its images are evaluated through the projection")
    z_init = None
    if defended:
        if same_init:
            z_init = np.random.RandomState(seed).randn(int(batch_size) * int(gan.rec_rr), int(gan.latent_dim)).astype(np.float32)
        model.add_rec_model(gan, z_init, batch_size)

    if rand:
        test_adv_from, eps = network_builder.rand_fgsm_prestep(test_images, eps, alpha, min_val, 1.0, rng=rng)
    else:
        test_adv_from = test_images
    with _Phase(phases, "attack", dev):
        if kind == "fgsm":
            attack = network_builder.FastGradientMethod(model)
            par = {"eps": eps, "ord": attack_ord, "clip_min": min_val, "clip_max": 1.0}
            x_adv = utils_tf.batch_eval(lambda xb: attack.generate(xb, **par), test_adv_from, batch_size)
        elif kind == "cw":
            attack = attack or network_builder.CarliniWagnerL2(model)
            x_adv = attack.generate(test_adv_from, **dict(CW_PARAMS, batch_size=batch_size, **extra))
        elif kind == "ead":
            attack = attack or network_builder.ElasticNetMethod(model)
            x_adv, _, ead_class = attack.generate(test_adv_from, return_info=True, **dict(EAD_PARAMS, batch_size=batch_size, **extra))
            if norms is not None:
                norms.update(ead_norms(x_adv, test_adv_from, ead_class, dev))
        elif kind == "pgd":
            attack = network_builder.ProjectedGradientDescent(model)
            x_adv = attack.generate(test_adv_from, test_labels, eps=eps, clip_min=min_val, clip_max=1.0, seed=seed,
                                    batch_size=PGD_CALL_IMAGES, **extra)
        elif kind == "jsma":
            attack = network_builder.SaliencyMapMethod(model)
            y_target = jsma_targets(test_labels, int(model.nb_classes), rng)
            x_adv, _, jsma_class, jsma_changed = attack.generate(test_adv_from, y_target=y_target, theta=float(extra["jsma_theta"]),
                                                                 gamma=float(extra["jsma_gamma"]), clip_min=min_val, clip_max=1.0,
                                                                 return_info=True)
            summary = jsma_summary(jsma_class, y_target, jsma_changed, int(np.prod(np.asarray(test_adv_from).shape[1:])))
            if norms is not None:
                norms.update(summary)
            print("[*] jsma: success rate %0.4f, mean share of features changed on the successful images %0.4f" %
                  (summary["success_rate"], summary["l0"]))
        elif kind == "latent":
            attack = network_builder.LatentAttack(model, gan)
            x_adv = attack.generate(test_adv_from, test_labels, rec_rr=int(gan.rec_rr), nb_iter=int(extra["latent_iters"]),
                                    learning_rate=float(extra["latent_lr"]), c=float(extra["latent_c"]), seed=seed, batch_size=batch_size)
        elif kind == "spsa":
            attack = network_builder.SPSA(model)
            x_adv = attack.generate(test_adv_from, test_labels, eps=eps, eps_iter=extra["eps_iter"], nb_iter=extra["nb_iter"],
                                    spsa_samples=int(extra["spsa_samples"]), delta=float(extra["spsa_delta"]), clip_min=min_val, clip_max=1.0,
                                    seed=seed, batch_size=batch_size)
        else:
            attack = network_builder.BPDA(model)
            x_adv = attack.generate(test_adv_from, test_labels, eps=eps, clip_min=min_val, clip_max=1.0, seed=seed, batch_size=batch_size,
                                    **extra)
    with _Phase(phases, "evaluation", dev):
        if defended:
            correct, n, roc_info = gan_defense.model_eval_gan(gan.reconstruct, model, x_adv, test_labels, batch_size,
                                                              rec_rr=int(gan.rec_rr), seed=seed, same_init_z=z_init)
        else:
            correct, n, _ = gan_defense.model_eval_gan(None, model, x_adv, test_labels, batch_size, compute_diffs=False)
            roc_info = None
    acc_adv = correct / float(max(n, 1))
    print("Test accuracy on adversarial examples: %0.4f\n" % acc_adv)
    return acc_adv, 0, roc_info


def ead_norms(x_adv, x, best_class, dev):
    """{'l1', 'l2', 'successes'}: the means of the per-image ||x_adv - x||_1 and ||x_adv - x||_2 (``dg_row_norms``; ord = 1 there is a
    plain sum, not a projection) over the images with ``best_class != -1``, float64 means on the host; NaN when none succeeded."""
    a, b = network_builder._to_device(np.asarray(x_adv, np.float32), dev), network_builder._to_device(np.asarray(x, np.float32), dev)
    ok = np.asarray(best_class) != -1
    out = {"successes": int(ok.sum())}
    for name, o in (("l1", 1), ("l2", 2)):
        v = network_builder._row_norms(a, b, o).cpu().numpy().astype(np.float64)
        out[name] = float(v[ok].mean()) if ok.any() else float("nan")
    return out


def jsma_targets(labels, nb_classes, rng):
    """The target class per image of ``--attack_type jsma``: ``(y + 1 + r) % nb_classes`` with ``r = rng.randint(0, nb_classes - 1, n)``,
    one draw for all images: uniform over the classes that are not the true one."""
    y = np.asarray(labels).astype(np.int64)
    if int(nb_classes) < 2:
        raise ValueError("jsma needs at least 2 classes to draw a target from")
    r = rng.randint(0, int(nb_classes) - 1, len(y))
    return ((y + 1 + r) % int(nb_classes)).astype(np.int32)


def jsma_summary(final_class, y_target, n_changed, features):
    """{'success_rate', 'l0'}: the share of images with ``final_class == y_target`` and the mean of ``n_changed / features`` over them
    (float64 on the host; NaN when none succeeded)."""
    ok = np.asarray(final_class) == np.asarray(y_target)
    l0 = np.asarray(n_changed, np.float64)[ok] / float(features)
    return {"success_rate": float(ok.mean()) if ok.size else float("nan"), "l0": float(l0.mean()) if ok.any() else float("nan")}


# ---------------------------------------------------------------------------------------------------- result files, CLI
def get_results_dir_filename(flags, gan):
    """whitebox.py:309-341 ``_get_results_dir_filename``: (results directory, file name without the counter prefix).

    DEVIATION in the ``defense_gan``-with-``rec_path`` branch: the reference formats 'Iter={}_RR={:d}_LR={:.4f}' with
    (rec_rr, rec_lr, rec_iters) -- the values in another order than the names, and ``rec_lr``, a float since main's
    ``float(tr_lr)``, under '{:d}', which raises ValueError in Python: the reference cannot name this file.  The name it meant is
    written instead: Iter = rec_iters, RR = rec_rr, LR = rec_lr."""
    results_dir = os.path.join("results", "whitebox_{}_{}".format(flags.defense_type, flags.dataset_name))
    if flags.rec_path and flags.defense_type == "defense_gan":
        results_dir = gan.checkpoint_dir.replace("output", "results")
        result_file_name = "Iter={}_RR={:d}_LR={:.4f}_defense=gan".format(int(gan.rec_iters), int(gan.rec_rr), float(gan.rec_lr))
        if not flags.train_on_recs:
            result_file_name = "orig_" + result_file_name
    elif flags.defense_type == "adv_tr":
        result_file_name = "advTrEps={:.2f}".format(flags.fgsm_eps_tr)
    else:
        result_file_name = "nodefense_"
    if flags.num_tests > -1:
        result_file_name = "numtest={}_".format(flags.num_tests) + result_file_name
    if flags.num_train > -1:
        result_file_name = "numtrain={}_".format(flags.num_train) + result_file_name
    result_file_name = "model={}_".format(flags.model) + result_file_name
    attack_ord = attack_ord_value(getattr(flags, "attack_ord", np.inf))
    result_file_name += "attack={}{}.txt".format(flags.attack_type, "" if attack_ord == np.inf else "_ord={}".format(attack_ord))
    return results_dir, result_file_name


def write_results(path, accuracies, norms=None):
    """whitebox.py:295-306: the line ``str(acc) + ' ' + '0 '`` (appended) and, with roc_info, ``*_roc.pkl`` in a pickle the
    Python-2 reference reads.  ``norms`` (whitebox()'s dict) adds two entries to the line: ``l1=<mean> l2=<mean>`` for ead,
    ``success=<rate> l0=<mean share of features changed on the successful images>`` for jsma."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        f.writelines([str(accuracies[i]) + " " for i in range(2)])
        if norms and "l1" in norms:
            f.write("l1=%s l2=%s " % (norms["l1"], norms["l2"]))
        if norms and "success_rate" in norms:
            f.write("success=%s l0=%s " % (norms["success_rate"], norms["l0"]))
        f.write("\n")
    print("[*] saved accuracy in {}".format(path))
    if accuracies[2]:
        pkl = path.replace(".txt", "_roc.pkl")
        with open(pkl, "wb") as f:
            py2pickle.dump(accuracies[2], f)
        print("[*] saved roc_info in {}".format(pkl))


def build_parser() -> argparse.ArgumentParser:
    """The flags and defaults of whitebox.py:344-392 on top of the reconstruction flags (config.add_rec_flags), plus the
    iterative attacks' parameters."""
    ap = config.add_rec_flags(argparse.ArgumentParser(prog="python -m defensegan_amd.whitebox", description=__doc__.split("\n\n")[0]))
    ap.add_argument("--data_dir", required=True, help="directory of the dataset's idx-ubyte files (mnist, f-mnist)")
    ap.add_argument("--init_path", default=None, help="generator weights: TensorFlow checkpoint dir/prefix or .npz pack")
    ap.add_argument("--alpha", type=float, default=0.05, help="RAND+FGSM random perturbation scale")
    ap.add_argument("--nb_classes", type=int, default=10, help="Number of classes.")
    ap.add_argument("--learning_rate", type=float, default=0.001, help="Learning rate for training.")
    ap.add_argument("--nb_epochs", type=int, default=10, help="Number of epochs to train model.")
    ap.add_argument("--lmbda", type=float, default=0.1, help="accepted and ignored, as in the reference")
    ap.add_argument("--fgsm_eps", type=float, default=0.3, help="FGSM epsilon: the budget of every L-infinity attack.")
    ap.add_argument("--fgsm_eps_tr", type=float, default=0.15, help="FGSM epsilon for adversarial training (a config key in the reference).")
    ap.add_argument("--num_tests", type=int, default=-1, help="Number of test samples.")
    ap.add_argument("--random_test_iter", type=int, default=-1, help="accepted and ignored, as in the reference")
    ap.add_argument("--online_training", action="store_true", help="not implemented (NotImplementedError)")
    ap.add_argument("--defense_type", default="none", choices=["none", "defense_gan", "adv_tr"], help="Type of defense")
    ap.add_argument("--attack_type", default="none", help="Type of attack [fgsm|cw|ead|rand_fgsm|pgd|jsma|bpda|latent|spsa]; none: train and stop")
    ap.add_argument("--results_dir", default=None, help="The final subdirectory of the results.")
    ap.add_argument("--model", default="F", choices=sorted(network_builder.MODELS), help="The classifier model.")
    ap.add_argument("--debug_dir", default="temp", help="accepted and ignored (the reference's qualitative debug output)")
    ap.add_argument("--num_train", type=int, default=-1, help="Number of training data to load.")
    ap.add_argument("--debug", action="store_true", help="accepted and ignored (saving reconstructions)")
    ap.add_argument("--train_on_recs", action="store_true", help="Train the classifier on the reconstructed samples using Defense-GAN.")
    ap.add_argument("--eps_iter", type=float, default=None, help="pgd / bpda step size (default 0.05)")
    ap.add_argument("--nb_iter", type=int, default=None, help="pgd / bpda iterations (default 10)")
    ap.add_argument("--eot_samples", type=int, default=None, help="bpda: projections the gradient is summed over per iteration (default 1)")
    ap.add_argument("--spsa_samples", type=int, default=None, help="spsa: direction pairs per iteration (default 32): 2 of them + 1 queries per image")
    ap.add_argument("--spsa_delta", type=float, default=None, help="spsa: probe size of the finite difference (default 0.01)")
    ap.add_argument("--latent_iters", type=int, default=None, help="latent: Adam steps on z (default 100); --rec_rr is its restarts per image")
    ap.add_argument("--latent_lr", type=float, default=None, help="latent: Adam's learning rate (default 0.05)")
    ap.add_argument("--latent_c", type=float, default=None, help="latent: weight of the classification term (default 1)")
    ap.add_argument("--ead_beta", type=float, default=EAD_DEFAULTS["ead_beta"], help="ead: weight of the L1 term (default 1e-3)")
    ap.add_argument("--ead_rule", default=EAD_DEFAULTS["ead_rule"], choices=["EN", "L1"],
                    help="ead: the best iterate is the successful one of the smallest elastic-net (EN) or L1 distance (default EN)")
    ap.add_argument("--jsma_theta", type=float, default=JSMA_DEFAULTS["jsma_theta"], help="jsma: what a chosen feature moves by (default 1.0; negative: downwards)")
    ap.add_argument("--jsma_gamma", type=float, default=JSMA_DEFAULTS["jsma_gamma"], help="jsma: the share of the features the attack may move (default 0.1)")
    ap.add_argument("--attack_ord", default="inf", choices=["inf", "1", "2"],
                    help="norm of the attack's ball: pgd / bpda take inf or 2, fgsm / rand_fgsm inf, 1 or 2 (default inf)")
    ap.add_argument("--seed", type=int, default=SEED, help="seed of the Dropout masks and the latent draws")
    ap.add_argument("--init_seed", type=int, default=0, help="seed of the classifier's initial weights")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .__main__ import resolve_cfg
    from .gan import gan_from_config
    cfg_path = resolve_cfg(args.cfg)
    cfg = config.load_config(cfg_path)
    args.dataset_name = str(cfg.get("DATASET_NAME", "mnist")).lower()
    if args.dataset_name not in ("mnist", "f-mnist"):
        raise SystemExit("python -m defensegan_amd.whitebox loads mnist and f-mnist; call whitebox() with your own arrays for %s"
                         % args.dataset_name)
    rp = config.resolve_rec_params(cfg, args)
    gan = None
    if args.init_path:
        gan = gan_from_config(cfg_path, rec_rr=rp["rec_rr"], rec_iters=rp["rec_iters"], rec_lr=rp["rec_lr"])
        gan.load_generator(args.init_path)
        gan.checkpoint_dir = args.init_path
    elif args.defense_type == "defense_gan":
        raise SystemExit("--defense_type defense_gan needs the generator (--init_path)")
    if args.defense_type == "defense_gan" and not args.rec_path and args.train_on_recs:
        raise SystemExit("--train_on_recs needs --rec_path (whitebox.py:259)")
    batch_size = rp["batch_size"]                                          # FLAGS.batch_size: --batch_size, else the cfg's BATCH_SIZE
    x_tr, y_tr = datasets.load_mnist_split(args.data_dir, "train")
    x_te, y_te = datasets.load_mnist_split(args.data_dir, "test")          # test_on_dev=True selects the TEST split
    x_tr, x_te = datasets.to_generator_range(x_tr, args.dataset_name), datasets.to_generator_range(x_te, args.dataset_name)
    if args.num_train > 0:
        x_tr, y_tr = x_tr[:args.num_train], y_tr[:args.num_train]
    if args.num_tests > 0:
        x_te, y_te = x_te[:args.num_tests], y_te[:args.num_tests]
    # the reconstructions of the arrays as truncated above, and only where they are trained on: whitebox() reads them nowhere else
    recs = None
    if args.rec_path and args.defense_type == "defense_gan" and args.train_on_recs:
        recs = load_recs(gan, args.rec_path, {"train": (x_tr, y_tr), "test": (x_te, y_te)}, batch_size=batch_size)
    model = network_builder.MODELS[args.model](input_shape=(None,) + tuple(x_tr.shape[1:]), nb_classes=args.nb_classes)
    results_dir, name = get_results_dir_filename(args, gan)
    path = result_path(results_dir, name, args.results_dir)
    norms = {}
    accuracies = whitebox(gan, model, (x_tr, y_tr, x_te, y_te), rec_data_path=args.rec_path, batch_size=batch_size,
                          learning_rate=args.learning_rate, nb_epochs=args.nb_epochs, eps=args.fgsm_eps, alpha=args.alpha,
                          online_training=args.online_training, train_on_recs=args.train_on_recs, attack_type=args.attack_type,
                          defense_type=args.defense_type, num_tests=args.num_tests, num_train=args.num_train,
                          fgsm_eps_tr=args.fgsm_eps_tr, same_init=args.same_init, recs=recs,
                          attack_params={"eps_iter": args.eps_iter, "nb_iter": args.nb_iter, "eot_samples": args.eot_samples,
                                         "latent_iters": args.latent_iters, "latent_lr": args.latent_lr, "latent_c": args.latent_c,
                                         "spsa_samples": args.spsa_samples, "spsa_delta": args.spsa_delta,
                                         "ead_beta": args.ead_beta, "ead_rule": args.ead_rule,
                                         "jsma_theta": args.jsma_theta, "jsma_gamma": args.jsma_gamma},
                          seed=args.seed, init_seed=args.init_seed, attack_ord=args.attack_ord, norms=norms)
    write_results(path, accuracies, norms)
    return 0


if __name__ == "__main__":
    sys.exit(main())
