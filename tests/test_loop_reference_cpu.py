"""tests/support/loop_reference.py (the step-by-step checks of tests/test_gpu_loop_values.py) without a GPU: the checks accept a
float32 numpy emulation of the loop (path_reference's float32 layers, split-K partials, the momentum update) and reject it with
one seeded defect at a time -- a dropped K slice, the previous step's partials, m not advanced / advanced twice, the update
skipped on the last partial 32-row block or on the second row group, lr undecayed at a decayed step / decayed a step early, m
carried over from the previous call, the reference's dead L-th update applied.  The lr condition of check (5) is asserted on the
float64 trajectory of the very inputs the GPU case uses (loop_reference.schedule_case)."""
import numpy as np
import pytest

from tests.support import loop_reference as LR
from tests.support import path_reference as PR

_STATE = {}


def _setup(name):
    """One case, its memo of reference evaluations and its clean runs, shared by the defect cases on it."""
    if name not in _STATE:
        if name == "mnist":                  # 35 rows as 5 images x 7 restarts: rows 32 .. 34 are the partial block, row 21 begins group 2
            case, Lmax = LR.make_case("mnist", 5, 7), 5
        elif name == "celeba":
            case, Lmax = LR.make_case("celeba", 9, 1), 3
        else:
            case, Lmax = LR.schedule_case(), 0
        s = dict(case=case, Lmax=Lmax, memo=PR.Memo(), emu=PR.Memo())
        s["clean"] = {L: LR.emulate_call(case, L, memo=s["emu"]) for L in range(1, Lmax + 1)}
        _STATE[name] = s
    return _STATE[name]


def _ran(res):
    return {c for c in range(1, 8) if any(l.startswith("(%d)" % c) for l in res.lines)}


def test_lr_at_is_the_engines_staircase():
    f = np.float32
    assert [LR.decay_iter(L) for L in (9, 10, 13, 14, 15, 200)] == [8, 8, 11, 12, 12, 160]
    assert LR.lr_at(10.0, 7, 10, "intended") == f(10.0) and LR.lr_at(10.0, 8, 10, "intended") == f(10.0) * f(0.1)
    assert LR.lr_at(10.0, 8, 10, "constant") == f(10.0)
    assert LR.lr_at(2.0, 13, 15, "intended") == f(2.0) * f(0.1) and LR.lr_at(2.0, 11, 15, "intended") == f(2.0)
    # the slices are added in slice order in float32: another order gives other bits
    rs = np.random.RandomState(0)
    part = (rs.standard_normal((64, 16, 128)) * 10.0 ** rs.randint(-3, 3, (64, 16, 1))).astype(f)
    g = LR.slice_sum(part)
    assert g.dtype == f and not np.array_equal(g, LR.slice_sum(part[:, ::-1])) and not np.array_equal(g, part.sum(axis=1, dtype=np.float64).astype(f))


@pytest.mark.parametrize("name", ["mnist", "celeba"])
def test_checks_accept_the_clean_emulation(name):
    s = _setup(name)
    case = s["case"]
    res = LR.run_step_checks(case, s["clean"], s["memo"])
    print("\n  " + "\n  ".join(res.lines + ["--"] + res.summary()))
    assert res.fails == [], res.fails
    assert _ran(res) == {1, 2, 3, 4}
    assert all(np.isfinite(r["loss"]).all() for r in s["clean"].values())


def _schedule_runs(s, defect=()):
    return {(sch, L): LR.emulate_call(s["case"], L, sch, defect, memo=s["emu"]) for sch, L in LR.SCHEDULE_RUNS}


def test_schedule_checks_accept_the_clean_emulation():
    s = _setup("schedule")
    runs = _schedule_runs(s)
    res = LR.run_schedule_checks(s["case"], runs, s["memo"])
    print("\n  " + "\n  ".join(res.lines + ["--"] + res.summary()))
    assert res.fails == [], res.fails
    assert _ran(res) == {1, 2, 3, 5}
    # the two schedules do differ where the staircase has set in, and only there
    assert not np.array_equal(runs[("intended", 10)]["z"], runs[("constant", 10)]["z"])
    assert np.array_equal(runs[("intended", 10)]["m"], runs[("constant", 10)]["m"])


def test_lr_condition_holds_on_the_float64_trajectory_of_the_gpu_case():
    """Condition, not a measurement: at every decayed step of the float64 trajectory at least half of the elements move by more
    than 8 ulp(Z) further under lr than under 0.1 lr -- otherwise check (1) could not tell the two."""
    case = LR.schedule_case()
    for L, ks in ((10, (8,)), (15, (12, 13))):
        Z, M = LR.trajectory64(case, L, "intended")
        assert all(np.isfinite(z).all() for z in Z)
        for k in ks:
            assert LR.is_decayed(k, L)
            share = LR.lr_condition(M[k + 1], Z[k + 1], case["lr"])
            print("L=%d update %d: |0.9 lr M| > 8 ulp(Z) on %.3f of the elements; median |lr M| / ulp(Z) = %.3g"
                  % (L, k, share, np.median(np.abs(case["lr"] * M[k + 1]) / np.spacing(np.abs(Z[k + 1]).astype(np.float32)))))
            assert share >= LR.LR_COND_SHARE, (L, k, share)
    # the contractive regime the condition is there to refuse: a momentum of a few ulp of z is rejected
    res = PR.Result()
    z = np.full((4, 8), 0.1, np.float32)
    LR.check_lr_condition(res, np.full((4, 8), 1e-9, np.float32), z, 10.0, "tiny m")
    assert res.labels(5) == ["condition tiny m"]


UPDATE_DEFECTS = [
    (("drop_slice", 5), "update m"),
    (("prev_part",), "update m"),
    (("m_not_updated",), "update m"),
    (("m_twice",), "update m"),
    (("skip_rows", 32, 35), "rows [32, 33, 34]"),            # the last partial 32-row block of 35 rows
    (("skip_rows", 21, 35), "rows [21, 22, 23, 24, 25, 26]"),  # the second row group of 5 x 7 (B = 5, R = 7: images 3 and 4)
]


@pytest.mark.parametrize("defect,expect", UPDATE_DEFECTS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_checks_reject_a_defect_of_the_update(defect, expect):
    s = _setup("mnist")
    case = s["case"]
    runs = {L: LR.emulate_call(case, L, defect=defect, memo=s["emu"]) for L in range(1, s["Lmax"] + 1)}
    res = LR.run_step_checks(case, runs, s["memo"])
    print("\n  " + "\n  ".join(l for _, _, l in res.fails))
    got = res.labels(1)
    assert got, "defect %s was not rejected by check (1)" % (defect,)
    assert any(expect in l or expect in line for _, l, line in res.fails), (expect, got)
    # every update of every call is affected, from the first one on
    assert any(l.startswith("update m k=0") for l in got) and any(l.startswith("update m k=%d" % (s["Lmax"] - 2)) for l in got)
    # teacher forcing localises: the partials, the forward and the selection are what they should be at the (wrong) latents
    assert not res.labels(2) and not res.labels(3) and not res.labels(4)
    if defect[0] == "skip_rows":
        # exactly the skipped rows, in m and in z
        lines = [line for c, l, line in res.fails if c == 1 and l.endswith("elements")]
        n_el = (defect[2] - defect[1]) * case["latent"]
        assert lines and all(" rows %s" % expect[5:-1] in line for line in lines)
        assert all(0 < int(line.split(" of ")[0].split()[-1]) <= n_el for line in lines)


def test_checks_reject_m_carried_over_from_the_previous_call():
    s = _setup("mnist")
    case, L = s["case"], s["Lmax"]
    carried = s["clean"][L]["m"]
    runs = {k: LR.emulate_call(case, k, m_init=carried, memo=s["emu"]) for k in range(1, L + 1)}
    res = LR.run_step_checks(case, runs, s["memo"])
    assert res.labels(4) == ["m after L=1"], res.fails
    # the update itself is self-consistent from the state the call started in: only the boundary checks see this defect
    assert not res.labels(1) and not res.labels(2) and not res.labels(3)
    res = PR.Result()
    LR.same_bits(res, 4, "second call", runs[L], s["clean"][L], keys=("z", "m", "loss"))
    assert res.labels(4) == ["second call: loss", "second call: m", "second call: z"]


def test_checks_reject_the_dead_last_update():
    s = _setup("mnist")
    case = s["case"]
    runs = {L: LR.emulate_call(case, L, defect=("dead_update",), memo=s["emu"]) for L in range(1, s["Lmax"] + 1)}
    res = LR.run_step_checks(case, runs, s["memo"])
    print("\n  " + "\n  ".join(l for _, _, l in res.fails))
    # the loss the call returns is not the loss at the z it returns; z, m have moved once more than the partials in front of them say
    assert any(l.startswith("loss L=") for l in res.labels(3)) and res.labels(1)


@pytest.mark.parametrize("defect", [("lr_undecayed",), ("lr_early",)], ids=lambda d: d[0])
def test_checks_reject_a_defect_of_the_schedule(defect):
    s = _setup("schedule")
    res = LR.run_schedule_checks(s["case"], _schedule_runs(s, defect), s["memo"])
    print("\n  " + "\n  ".join(l for _, _, l in res.fails))
    bad_z = [l for l in res.labels(1) if l.startswith("update z") and not l.endswith("elements")]
    assert not [l for l in res.labels(1) if l.startswith("update m")]           # m does not depend on lr within one step
    assert not res.labels(3)
    if defect[0] == "lr_undecayed":
        # exactly the three decayed updates, under the intended schedule only
        assert bad_z == sorted("update z k=%d intended L=%d [ulp]" % kl for kl in ((8, 10), (12, 14), (13, 15))), bad_z
        assert not res.labels(2) and not res.labels(5)
    else:
        # update 7 of the intended run of 9 is decayed: that run is no longer the constant run of 9; the intended run of 14 decays
        # its update 11 and so does not pass through the constant run of 13's state: its partials are not the gradient there
        assert "intended 9 = constant 9: z" in res.labels(5) and "update z k=12 intended L=14 [ulp]" in bad_z
        assert "intended 14 = constant 14 in front of update 12: part" in res.labels(5)
        assert res.labels(2) == ["dz k=12 intended L=14 every row", "g32 k=12 intended L=14 end to end"]
