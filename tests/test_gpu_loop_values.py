"""-m gpu: the projection loop (dg_reconstruct) step by step against tests/support/loop_reference.py: the momentum update from the
device's own partials, the gradient it consumed against float64, the forward and the selection a call ends on, the state at call
boundaries, the lr staircase, the loop variants and small row groups.  tests/test_loop_reference_cpu.py shows without a GPU that
these checks reject a dropped K slice, the previous step's partials, m not advanced / advanced twice, an update skipped on the
last partial 32-row block or on the second row group, lr undecayed / decayed a step early, m carried over and the dead L-th update.

The loop is deterministic and a call with rec_iters = L is the prefix of the call with L + 1, so per case ONE handle runs
L = 1 .. 6 on the same inputs and after every call z, m, part, y, loss and every act<d> are read (dg_debug_read): run L - 1 and
run L hold everything that goes into and comes out of update k = L - 2 (loop_reference's docstring: what a call leaves behind).
Inputs (loop_reference.make_case): synth.make_weights(seed 1234, gain 2, bias 0.1); targets G(0.09 N(0, 1)) pushed by
synth.adversarial(0.3); z0 = synth.make_z; lr 10 (MNIST), 2 (CelebA); momentum 0.7.

Routes (read off enqueue_steps / run_backward / run_latent_turn of dg_engine.cpp), each at the smallest rows that reach it:

  route                                                       how it is reached                         cases (rows = B x R)
  momentum_update_kernel behind lin_stationary_kernel<8, 0>   defaults, NET_DIM 64, LATENT_DIM 128      MNIST 1, 33, 47, 5 x 10, 5 x 7; CelebA 9, 33, 5 x 7
    (one / two 32-row blocks, the last one partial)
  loop forward + backward (tail_backward = 1, want_y = 0),    every step but the last of every call     all cases
    B1 writing part at the group's row offset
  momentum_update_kernel at qrow = 16, B1 on the generic      LATENT_DIM 64                             MNIST 33
    GEMM (the weight-stationary backward needs latent 128)
  two passes of 8 -> one pass of 4 slices, B1 on the generic  nsplit = 4                                MNIST 33
    GEMM (K slices of 1024 features)
  lin_stationary_kernel<8, 0, true> (folded update)           update_fold = 1                           MNIST 33, 5 x 10; CelebA 33
  latent_turn_kernel                                          turn_fused = 1                            MNIST 33, 5 x 10; CelebA 33
  B1 / F1 on gemm_batched_kernel                              latent_turn = 0                           MNIST 33; CelebA 33
  two row groups, r0 = 21 (no multiple of 32)                 two_streams 2, two_stream_min_rows 1      MNIST 5 x 7; CelebA 5 x 7
  two unequal row groups (4 + 1 images), r0 = 28              ... two_stream_split 80                   MNIST 5 x 7; CelebA 5 x 7
  three row groups (2 + 2 + 1 images), r0 = 14, 28            two_streams 3, two_stream_min_rows 1      MNIST 5 x 7; CelebA 5 x 7
  lr staircase, host side of enqueue_steps                    rec_lr_schedule "intended", L = 10, 15    MNIST 33, z0 = 0.3 N(0, 1)
The kernel of each update variant is confirmed from the per-launch profile of one further call (profile_read names the launches).

Not reached here: the captured loop graph (graph_max_rows, off by default); the fragment-order forward path (frag_path, off by
default; tests/test_gpu_frag.py); Batchnorm (tests/test_gpu_bn_values.py); row groups combined with update_fold / turn_fused
(bit-identity at >= 640 rows in tests/test_gpu_variants.py); NET_DIM 128; more than two 32-row blocks per group and job lists
of several rounds (tests/test_gpu_variants.py at 700 .. 2560 rows, end results only); the timed one-or-two-groups choice
(two_streams = "auto": below 1024 rows always one group).

The checks ((1) .. (7), tests/support/loop_reference.py):
 (1) update, teacher-forced from the device's partials: g32 = float32 slice sum of part in slice order from 0; in float64 on the
     float32 values M[k + 1] within 1 ulp of mu M[k] + g32 and Z[k + 1] within 1 ulp of Z[k] - lr_k M[k + 1] (ulp at the larger
     of the product and the result); every element of every row.  The kernels run the FUSED multiply-add (update_fold and
     turn_fused spell it __builtin_fmaf and are bit-identical to momentum_update_kernel), which alone is within 0.5 ulp.
 (2) g32 against the float64 backward from the device's Z[k] with the device's gates at Z[k] (acts of run L - 1): 1e-5 of max|dz|
     over the case, every row -- the only value check of the backward as the loop runs it.
 (3) y against the float64 tail fed the device's last activation (2e-6 per tap class, yardstick rule of path_reference); loss
     against the float64 loss at the device's Z[L - 1], rtol 1e-5; rec[b] the bits of y[b R + idx[b]]; idx[b] the first argmin
     of the device's own loss row.
 (4) after L = 1, M is exactly 0 and Z the bits of z0; the same call again returns the same Z, M, loss; a call of 9 rows behind
     the 33-row calls equals a fresh handle's on Z, M, part, loss, rec, idx.
 (5) lr_schedule "intended": (1) with lr_k = lr 0.1^(k // ceil(0.8 L)) at L = 10 (update 8, from the run of 9) and L = 15
     (update 12 from the CONSTANT run of 13, update 13 from the intended run of 14); the same steps under "constant" with lr.
     Asserted on the device: intended 9 == constant 9 bit for bit; part of intended 14 == part of constant 14 (the gradient at the
     shared Z[12]).  Condition: at each decayed step |0.9 lr M[k + 1]| > 8 ulp(Z[k + 1]) on at least half of the elements.
 (6) update_fold = 1 and turn_fused = 1: Z, M, part, loss, rec, idx bit-identical to the default after every L = 1 .. 6 (both
     variants leave their partials in part: write-through stores of the same tiles, dg_linear.hip / dg_turn.hip phase B -- no
     read had to be skipped); latent_turn = 0: (1) - (3), to rounding (bit identity is not asked of it here).
 (7) row groups: dg_call_row_groups confirms the group count; Z, M, part, loss, rec, idx bit for bit the one-group call's after
     every L, and (1) - (3) hold.

Measured on MI355X in one run, worst case of each check group over all 25 cases (device error | float32 yardstick error |
bound | bound / error; the yardstick is the same teacher-forced step in numpy float32, for (1) with the UNFUSED multiply-add):
  (1) update m              0.5 ulp  | 0.99 ulp | 1 ulp    | x2.0   every case: the one rounding of the fused multiply-add
  (1) update z              0.5 ulp  | 0.5 ulp  | 1 ulp    | x2.0   every case, decayed steps included
  (2) g32 end to end        1.86e-06 | 7.73e-07 | 1e-05    | x5.4   schedule case, update 13 of L = 15, row 2 (of max|dz| = 0.00215)
  (3) y                     1.06e-06 | 4.62e-07 | 2e-06    | x1.9   CelebA 5 x 7, L = 6, class 0 (tanh near 1; MNIST: 1.9e-07, x10.5)
  (3) loss                  2.16e-07 | 1.20e-07 | 1e-05    | x46.3  CelebA 33 rows, L = 4
  (3) idx, rec              first argmin and the bits of y in every call of every case
  (4), (6), (7)             601 bit comparisons, none differs
  (5) condition             |0.9 lr M| > 8 ulp(Z) on 1.000 of the elements at updates 8 (L = 10), 12 and 13 (L = 15)
No bound came from the yardstick rule; no check failed on the device, so no kernel was changed."""

import numpy as np
import pytest

from tests.support import loop_reference as LR
from tests.support import path_reference as PR

pytestmark = pytest.mark.gpu

LMAX = 6
_MEMO, _DEFAULT = {}, {}


def _gan(case, opts):
    from defensegan_amd.gan import dataset_gan_dict
    gan = dataset_gan_dict[case["arch"]](cfg={"USE_BN": False, "LATENT_DIM": case["latent"], "NET_DIM": case["net_dim"]}, test_mode=True,
                                         rec_rr=case["R"], rec_iters=1, rec_lr=case["lr"])
    assert gan.rec_momentum == case["momentum"]
    assert gan.set_weights(case["p"]) == []
    if case["nsplit"] != 16:
        gan.set_option("nsplit", case["nsplit"])
    for k, v in opts.items():
        gan.set_option(k, v)
    return gan


def _read(gan, what, shape):
    n = int(np.prod(shape))
    t = gan.debug_read(what, n)
    assert t.numel() == n, (what, t.numel(), n)
    return t.cpu().numpy().reshape(shape)


def _run(gan, case, L, schedule="constant", B=None):
    """One call and everything it leaves behind, as a run record of loop_reference."""
    arch, p, R = case["arch"], case["p"], case["R"]
    B = case["B"] if B is None else B
    n = B * R
    gan.rec_iters, gan.rec_lr_schedule = L, schedule
    out = gan.reconstruct(case["x"][:B], z_init_val=case["z0"][:n], return_details=True)
    run = {"L": L, "z": out["z"], "loss": out["loss"], "rec": out["rec"], "idx": out["idx"]}
    assert np.array_equal(_read(gan, "z", (n, case["latent"])).view(np.uint32), run["z"].view(np.uint32))
    assert np.array_equal(_read(gan, "loss", (n,)).view(np.uint32), run["loss"].view(np.uint32))
    run["m"] = _read(gan, "m", (n, case["latent"]))
    run["part"] = _read(gan, "part", (n, case["nsplit"], case["latent"])) if L >= 2 else None
    run["y"] = _read(gan, "y", (n,) + tuple(case["x"].shape[1:]))
    acts = []
    for d in range(PR.n_act(arch)):
        if d == 0:
            shape = (n, 4, 4, p["Generator.Input.W"].shape[1] // 16)
        else:
            name, _, e, _, _ = PR.O._arch_layers(arch)[d - 1]
            shape = (n, e, e, p[name + ".Filters"].shape[2])
        acts.append(_read(gan, "act%d" % d, shape))
    run["acts"] = acts
    return run


def _launches(gan, case):
    """Names of the launches of one more call of three steps (the per-launch profile)."""
    gan.profile_reset()
    gan.profile_enable(1)
    _run(gan, case, 3)
    gan.profile_enable(0)
    return [q["name"] for q in gan.profile_read() if q["launches"] > 0]


ROUTE = {
    "default": lambda names: any("momentum_update_kernel" in n for n in names) and not any("latent_turn_kernel" in n for n in names),
    "update_fold": lambda names: any(n.startswith("B1@lin_stationary_kernel") and n.endswith(", true>") for n in names)
                                 and not any("momentum_update_kernel" in n for n in names),
    "turn_fused": lambda names: any("latent_turn_kernel" in n for n in names) and not any("momentum_update_kernel" in n for n in names),
    "latent_turn": lambda names: any(n.startswith("B1@gemm_batched_kernel") for n in names) and any(n.startswith("F1@gemm_batched_kernel") for n in names),
}


def _memo(key):
    """The reference evaluations of ONE input set (by the bytes of their inputs: variants that leave z and the gates bit for bit
    the same share them); dropped, with the default engine's runs on it, when the next input set begins."""
    if key not in _MEMO:
        _MEMO.clear(); _DEFAULT.clear()
        _MEMO[key] = PR.Memo()
    return _MEMO[key]


def _default_runs(key, case):
    """Runs L = 1 .. LMAX of the default engine on an input set, computed once."""
    _memo(key)
    if key not in _DEFAULT:
        gan = _gan(case, {})
        assert gan.row_groups(case["B"]) == 1
        _DEFAULT[key] = ({L: _run(gan, case, L) for L in range(1, LMAX + 1)}, gan)
    return _DEFAULT[key]


# (kind, arch, B, R, latent, nsplit, options).  kinds: steps = (1) - (4) on the handle's own runs; bits = (6) against the default;
# groups = (7); schedule = (5)
def _cases():
    c = []
    for B, R in ((1, 1), (33, 1), (47, 1), (5, 10), (5, 7)):
        c.append(("steps", "mnist", B, R, 128, 16, {}))
    for B, R in ((9, 1), (33, 1), (5, 7)):
        c.append(("steps", "celeba", B, R, 128, 16, {}))
    c.append(("steps", "mnist", 33, 1, 64, 16, {}))
    c.append(("steps", "mnist", 33, 1, 128, 4, {}))
    for arch, B, R in (("mnist", 33, 1), ("mnist", 5, 10), ("celeba", 33, 1)):
        c.append(("bits", arch, B, R, 128, 16, {"update_fold": 1}))
        c.append(("bits", arch, B, R, 128, 16, {"turn_fused": 1}))
    for arch in ("mnist", "celeba"):
        c.append(("steps", arch, 33, 1, 128, 16, {"latent_turn": 0}))
        c.append(("groups", arch, 5, 7, 128, 16, {"two_streams": 2, "two_stream_min_rows": 1}))
        c.append(("groups", arch, 5, 7, 128, 16, {"two_streams": 2, "two_stream_min_rows": 1, "two_stream_split": 80}))
        c.append(("groups", arch, 5, 7, 128, 16, {"two_streams": 3, "two_stream_min_rows": 1}))
    c.append(("schedule", "mnist", 33, 1, 128, 16, {}))
    c.sort(key=lambda v: (v[0] == "schedule", v[1], v[4], v[2], v[3], v[5], v[0] != "steps" or bool(v[6])))   # an input set's cases next to each other
    return c


def _id(c):
    kind, arch, B, R, latent, nsplit, opts = c
    return "%s-%s-%dx%d-latent%d-nsplit%d-%s" % (kind, arch, B, R, latent, nsplit, ",".join("%s=%s" % kv for kv in sorted(opts.items())) or "defaults")


def _check_boundaries(res, case, gan, runs):
    """(4) beyond the first call: the same call again; then a call of fewer rows on the same handle against a fresh handle's."""
    again = _run(gan, case, LMAX)
    LR.same_bits(res, 4, "second call", again, runs[LMAX], keys=("z", "m", "loss", "part", "rec", "idx"))
    small = _run(gan, case, 3, B=9)
    fresh = _run(_gan(case, {}), case, 3, B=9)
    LR.same_bits(res, 4, "9 rows behind %d" % case["n"], small, fresh)


@pytest.mark.parametrize("c", _cases(), ids=_id)
def test_loop_step_by_step(c):
    """(1) - (7) of the module docstring on one route of its table."""
    kind, arch, B, R, latent, nsplit, opts = c
    lines = []
    try:
        if kind == "schedule":
            case = LR.schedule_case()
            memo = _memo(("schedule",))
            gan = _gan(case, opts)
            runs = {(s, L): _run(gan, case, L, s) for s, L in LR.SCHEDULE_RUNS}
            res = LR.run_schedule_checks(case, runs, memo)
        else:
            case = LR.make_case(arch, B, R, latent_dim=latent, nsplit=nsplit)
            key = (arch, B, R, latent)
            memo = _memo(key)
            if kind == "steps" and not opts and nsplit == 16:
                runs, gan = _default_runs(key, case)
            else:
                gan = _gan(case, opts)
                runs = {L: _run(gan, case, L) for L in range(1, LMAX + 1)}
            if kind == "groups":
                want = min(int(opts["two_streams"]), B)
                assert gan.row_groups(B) == want, (gan.row_groups(B), want)
            res = LR.run_step_checks(case, runs, memo)
            if kind in ("bits", "groups"):           # (bit identity is not required of latent_turn = 0: it runs as "steps")
                ref, _ = _default_runs(key, case)
                for L in range(1, LMAX + 1):
                    LR.same_bits(res, 6 if kind == "bits" else 7, "L=%d against the default" % L, runs[L], ref[L])
            if kind == "steps" and not opts and nsplit == 16 and (B, R) == (33, 1) and latent == 128:
                _check_boundaries(res, case, gan, runs)
            if kind != "groups":
                route = next((k for k in ("update_fold", "turn_fused", "latent_turn") if k in opts), "default")
                names = _launches(gan, case)
                res.note(6, "route " + route, bool(ROUTE[route](names)), "launches: " + ", ".join(sorted(set(n.partition("<")[0] for n in names))))
            assert all(np.isfinite(r["loss"]).all() for r in runs.values())
        lines = res.lines + ["--"] + res.summary()
        assert res.fails == [], "\n".join(l for _, _, l in res.fails)
    finally:
        print("\n[%s]\n  " % _id(c) + "\n  ".join(lines))
