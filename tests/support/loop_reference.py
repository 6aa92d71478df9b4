"""The projection loop (dg_reconstruct: L forwards, L - 1 backward + momentum updates, the selection) step by step: the checks
shared by tests/test_gpu_loop_values.py, which feeds them the device, and tests/test_loop_reference_cpu.py, which feeds them a
float32 emulation with and without seeded defects.  Built on tests/support/path_reference.py (the float64 layers, the float32
yardstick, Result, Memo); nothing of it is restated here.

The loop is deterministic, and a call with rec_iters = L is the prefix of the call with rec_iters = L + 1 (constant schedule).
A RUN is what one call leaves behind (read off enqueue_steps / dg_reconstruct of dg_engine.cpp): for L >= 2

  z     Z[L - 1]                               return_details["z"] == debug_read("z")
  m     M[L - 1]                               debug_read("m")
  part  PART[L - 2] [rows][nsplit][latent]     debug_read("part"): the split-K partials of the last backward = the gradient at Z[L - 2]
  acts  ACT[L - 1]                             every act<d>: the last launch of a call is a forward, the gates at Z[L - 1]
  y, loss at Z[L - 1]; rec, idx                the selection

and for L in (0, 1): Z[0] = z0, M[0] = 0, no valid part.  The pair of runs (L - 1, L) holds everything that goes into and comes
out of update k = L - 2, so every step is checked teacher-forced: from the device's own previous state.

Checks (numbered as in the module docstring of tests/test_gpu_loop_values.py):
 (1) the update from the device's partials: g32 = the float32 sum of PART[k] over the slices in slice order from 0 (exactly what
     momentum_update_kernel adds); in float64 on the float32 values, M[k + 1] within 1 float32 ulp of mu * M[k] + g32 (ulp at the
     larger of |mu * M[k]| and the result), Z[k + 1] within 1 ulp of Z[k] - lr_k * M[k + 1] with the device's M[k + 1] (ulp at the
     larger of |lr_k * M[k + 1]| and the result).  Every element of every row.  One ulp admits the fused and the unfused
     multiply-add; the kernels run the fused one (dg_linear.hip / dg_turn.hip spell it __builtin_fmaf and are bit-identical to
     momentum_update_kernel, whose a * b + c hipcc contracts), which alone is within half an ulp.
 (2) g32 against path_reference's end-to-end float64 backward from the device's Z[k] with the device's gates at Z[k] (the acts
     of run L - 1): path_reference's check (4), 1e-5 of max|dz| over the case, every row.
 (3) the forward the call ends on: y against the float64 tail fed the device's last activation (path_reference's check (1), its
     figure and yardstick rule); loss against the float64 loss at the device's Z[L - 1], rtol 1e-5; rec[b] the bits of
     y[b R + idx[b]]; idx[b] the first argmin of the device's own loss row.
 (4) call boundaries: after L = 1 M is exactly 0 and Z the bits of z0; bit comparisons of repeated / smaller calls (same_bits).
 (5) the lr schedule: lr_at() below in (1); the CONDITION that makes (1) tell lr from 0.1 lr: at a decayed step at least half of
     the elements have |0.9 lr M[k + 1]| > 8 ulp(Z[k + 1]).
 (6), (7) variants and row groups: same_bits on z, m, part, loss, rec, idx, and (1) - (3) again."""
from __future__ import annotations

import math

import numpy as np

from defensegan_amd import archs, synth
from tests.support import path_reference as PR

F32 = np.float32
UPDATE_ULPS = 1.0       # (1)
LR_COND_ULPS = 8.0      # (5)
LR_COND_SHARE = 0.5


# ---- inputs (the same arrays on the device and in the CPU test) ---------------------------------------------------------------
_W = {}


def weights(arch, net_dim=64, latent_dim=128):
    """One weight dict per (arch, width, latent): Memo keys on its identity."""
    k = (arch, net_dim, latent_dim)
    if k not in _W:
        _W[k] = synth.make_weights(arch, seed=1234, gain=2.0, bias_range=0.1, latent_dim=latent_dim, net_dim=net_dim)
    return _W[k]


def make_case(arch, B, R, net_dim=64, latent_dim=128, z0_scale=None, lr=None, nsplit=16, momentum=0.7):
    """Targets: G(z_t), z_t = 0.09 N(0, 1), pushed by synth.adversarial(0.3) (the inputs of tests/test_gpu_variants.py, G in
    float64 here); z0 = synth.make_z (N(0, 1 / latent)) or z0_scale * N(0, 1).  lr: 10 (MNIST), 2 (CelebA: where its loop
    contracts with these weights, tests/test_gpu_frag.py)."""
    p = weights(arch, net_dim, latent_dim)
    a = archs.make_arch(arch, latent_dim, net_dim)
    rs = np.random.RandomState(1000 + 37 * B + R)
    zt = rs.standard_normal((B, latent_dim)) * 0.09
    x = PR.forward_from_z(p, arch, zt)["y"].astype(F32)
    x = synth.adversarial(x, 0.3, a.in_lo, a.in_hi, seed=2000 + B)
    n = B * R
    if z0_scale is None:
        z0 = synth.make_z(n, latent_dim, seed=3000 + n)
    else:
        z0 = (np.random.RandomState(3000 + n).standard_normal((n, latent_dim)) * z0_scale).astype(F32)
    if lr is None:
        lr = 2.0 if arch == "celeba" else 10.0
    return dict(arch=arch, p=p, x=x, z0=np.ascontiguousarray(z0, F32), B=B, R=R, n=n, latent=latent_dim, net_dim=net_dim,
                lr=float(lr), momentum=float(momentum), nsplit=int(nsplit))


def schedule_case():
    """The one shape of the schedule checks (5): MNIST, 33 rows (one whole 32-row block and a partial one), adversarial targets
    and z0 = 0.3 N(0, 1) -- far from the targets, so that the momentum is still large where the staircase sets in."""
    return make_case("mnist", 33, 1, z0_scale=0.3)


# ---- the schedule -------------------------------------------------------------------------------------------------------------
def decay_iter(L):
    return int(math.ceil(0.8 * float(L))) if L > 0 else 1


def lr_at(lr, k, L, schedule):
    """float32 lr of update k of a call with rec_iters = L (enqueue_steps: lr * powf(0.1f, k / ceil(0.8 L)); powf(0.1f, 0) = 1 and
    powf(0.1f, 1) = 0.1f exactly, and k <= L - 2 < 2 ceil(0.8 L) leaves no other exponent)."""
    if schedule == "constant":
        return F32(lr)
    assert schedule == "intended", schedule
    e = k // decay_iter(L)
    assert e in (0, 1), (k, L)
    return F32(lr) * F32(0.1) if e else F32(lr)


def is_decayed(k, L):
    return k // decay_iter(L) >= 1


# ---- the checks ---------------------------------------------------------------------------------------------------------------
def slice_sum(part):
    """g32: the slices added in float32 from 0 in slice order, as momentum_update_kernel (and the folded / fused updates) do."""
    part = np.asarray(part, F32)
    g = np.zeros((part.shape[0], part.shape[2]), F32)
    for s in range(part.shape[1]):
        g = g + part[:, s]
    assert g.dtype == F32
    return g


def _ulp_at(*vals):
    big = np.maximum.reduce([np.abs(np.asarray(v, np.float64)) for v in vals])
    return np.spacing(big.astype(F32)).astype(np.float64)


def _gates(acts):
    return [np.asarray(a) > 0 for a in acts]


def _e2e32(p, arch, z, x, R, gates):
    """The float32 yardstick of (2) and of the loss of (3): path_reference's layers in float32 from z."""
    fwd = PR.forward_from_z(p, arch, z, F32)
    loss, _ = PR.loss_and_dy(fwd["y"], x, R, F32)
    return loss, PR.backward_with_gates(p, arch, fwd["y"], x, R, gates, F32)[0]


def check_update(res, case, prev, cur, lr_k, tag=""):
    """(1) for the update between two runs; lr_k as float32.  Lines are in float32 ulps (bound 1); the yardstick is the same step
    in numpy float32 with the unfused multiply-add."""
    k = cur["L"] - 2
    mu, lrk = np.float64(F32(case["momentum"])), np.float64(F32(lr_k))
    g32 = slice_sum(cur["part"])
    Mk, Zk = np.asarray(prev["m"], np.float64), np.asarray(prev["z"], np.float64)
    M1, Z1 = np.asarray(cur["m"], np.float64), np.asarray(cur["z"], np.float64)
    t = mu * Mk
    want_m = t + g32
    ulp_m = _ulp_at(t, want_m)
    yard_m = (F32(case["momentum"]) * np.asarray(prev["m"], F32) + g32).astype(np.float64)
    u = lrk * M1
    want_z = Zk - u
    ulp_z = _ulp_at(u, want_z)
    yard_z = (np.asarray(prev["z"], F32) - F32(lr_k) * np.asarray(cur["m"], F32)).astype(np.float64)
    for name, got, want, ulp, yard in (("m", M1, want_m, ulp_m, yard_m), ("z", Z1, want_z, ulp_z, yard_z)):
        e = np.abs(got - want) / ulp
        bad = ~(e <= UPDATE_ULPS)
        label = "update %s k=%d%s [ulp]" % (name, k, tag)
        res.add(1, "update " + name, label, float(e.max()) if np.isfinite(e).all() else float("nan"), float((np.abs(yard - want) / ulp).max()),
                UPDATE_ULPS, 1.0, False)
        if bad.any():
            r, c = np.unravel_index(int(np.argmax(np.where(np.isfinite(e), e, np.inf))), e.shape)
            res.note(1, label + " elements", False, "%d of %d elements beyond %g ulp, rows %s..; worst at row %d col %d: got %.9g want %.9g"
                     % (int(bad.sum()), bad.size, UPDATE_ULPS, sorted(set(np.nonzero(bad)[0].tolist()))[:6], r, c, got[r, c], want[r, c]))
    return g32


def check_gradient(res, case, prev, cur, memo, g32=None, tag=""):
    """(2): path_reference.check_end_to_end on g32 with the record of run L - 1 (z, gates); plus a figure line with the float32
    yardstick for the report (same bound)."""
    k = cur["L"] - 2
    g32 = slice_sum(cur["part"]) if g32 is None else g32
    rec = {"z": prev["z"], "x": case["x"], "R": case["R"], "acts": prev["acts"]}
    PR.check_end_to_end(res, rec, case["p"], case["arch"], memo, g32, None, check=2, tag=" k=%d%s" % (k, tag))
    gates = _gates(prev["acts"])
    _, dz64 = memo(PR.end_to_end, case["p"], case["arch"], prev["z"], case["x"], case["R"], gates)
    _, dz32 = memo(_e2e32, case["p"], case["arch"], prev["z"], case["x"], case["R"], gates)
    s = float(np.abs(dz64).max())
    e = np.abs(np.asarray(g32, np.float64) - dz64).max()
    res.add(2, "gradient", "g32 k=%d%s end to end" % (k, tag), float(e), float(np.abs(dz32 - dz64).max()), PR.GRAD_TOL * s, s, False)


def check_final(res, case, cur, memo, tag=""):
    """(3) on one run."""
    p, arch, x, R, L = case["p"], case["arch"], case["x"], case["R"], cur["L"]
    y64 = memo(PR.tail_forward, p, arch, cur["acts"][-1], dtype=np.float64)
    y32 = memo(PR.tail_forward, p, arch, cur["acts"][-1], dtype=F32)
    PR.class_check(res, 3, "y", "y L=%d%s" % (L, tag), cur["y"], y64, y32, PR.tap_class_masks(arch, PR.n_act(arch), "fwd")[0], PR.FWD_TOL)
    gates = _gates(cur["acts"])
    loss64, _ = memo(PR.end_to_end, p, arch, cur["z"], x, R, gates)
    loss32, _ = memo(_e2e32, p, arch, cur["z"], x, R, gates)
    loss = np.asarray(cur["loss"], np.float64)
    rel = np.abs(loss - loss64) / loss64
    res.add(3, "loss", "loss L=%d%s [rel]" % (L, tag), float(rel.max()) if np.isfinite(loss).all() else float("nan"),
            float((np.abs(loss32 - loss64) / loss64).max()), PR.LOSS_RTOL, 1.0, False)
    B = case["B"]
    lrow = np.asarray(cur["loss"]).reshape(B, R)
    first = np.array([int(np.argmin(lrow[b])) for b in range(B)])
    idx = np.asarray(cur["idx"]).astype(np.int64)
    res.note(3, "idx L=%d%s" % (L, tag), bool(np.array_equal(idx, first)), "first argmin of the loss rows: %d of %d images differ" % (int((idx != first).sum()) if idx.shape == first.shape else B, B))
    ok = idx.shape == (B,) and bool(((idx >= 0) & (idx < R)).all())
    if ok:
        ysel = np.asarray(cur["y"]).reshape(B, R, -1)[np.arange(B), idx]
        ok = bool(np.array_equal(ysel.view(np.uint32), np.ascontiguousarray(np.asarray(cur["rec"], F32).reshape(B, -1)).view(np.uint32)))
    res.note(3, "rec L=%d%s" % (L, tag), ok, "rec[b] is y[b R + idx[b]] bit for bit: %s" % ok)


def check_first_call(res, case, run1):
    """(4): a call without an update leaves M exactly 0 and Z the bits of z0."""
    m, z = np.ascontiguousarray(run1["m"], F32), np.ascontiguousarray(run1["z"], F32)
    res.note(4, "m after L=%d" % run1["L"], bool((m.view(np.uint32) << 1 == 0).all()), "%d of %d elements not 0" % (int((m != 0).sum() + np.isnan(m).sum()), m.size))
    same = np.array_equal(z.view(np.uint32), case["z0"].view(np.uint32))
    res.note(4, "z after L=%d" % run1["L"], bool(same), "the bits of z0: %s" % same)


def same_bits(res, check, label, a, b, keys=("z", "m", "part", "loss", "rec", "idx"), rows=None):
    """Bit equality of two runs on `keys` (a part that either run lacks is left out); rows: only the first `rows` latent rows
    (of a, for a run b of fewer rows; rec / idx then per image are not compared)."""
    for key in keys:
        u, v = a.get(key), b.get(key)
        if u is None or v is None:
            continue
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        if rows is not None:
            u = np.ascontiguousarray(u[:rows])
        ok = u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()
        n = int((u != v).sum()) if u.shape == v.shape else -1
        res.note(check, "%s: %s" % (label, key), bool(ok), "bit for bit: %s (%d elements differ)" % (ok, n))


def lr_condition(m_next, z_next, lr):
    """Share of the elements at which a step of lr M differs from a step of 0.1 lr M by more than 8 ulp of the result."""
    d = np.abs(0.9 * np.float64(F32(lr)) * np.asarray(m_next, np.float64))
    return float((d > LR_COND_ULPS * _ulp_at(z_next)).mean())


def check_lr_condition(res, m_next, z_next, lr, label):
    share = lr_condition(m_next, z_next, lr)
    res.note(5, "condition " + label, share >= LR_COND_SHARE, "|0.9 lr M| > %g ulp(Z) on %.3f of the elements (need %.2f)" % (LR_COND_ULPS, share, LR_COND_SHARE))


def run_step_checks(case, runs, memo=None, tag=""):
    """(1) - (4) on runs = {L: run} (constant schedule): (4) on the run of L = 1, (3) on every run, (1) and (2) on every pair
    (L - 1, L) present."""
    memo = memo or PR.Memo()
    res = PR.Result()
    if 1 in runs:
        check_first_call(res, case, runs[1])
    for L in sorted(runs):
        check_final(res, case, runs[L], memo, tag)
        if L >= 2 and L - 1 in runs:
            g32 = check_update(res, case, runs[L - 1], runs[L], lr_at(case["lr"], L - 2, L, "constant"), tag)
            check_gradient(res, case, runs[L - 1], runs[L], memo, g32, tag)
    return res


# Runs the schedule checks need, as (schedule, L): with L = 10 the staircase ceil(0.8 L) = 8 first applies at update 8, the last one
# of the call; its input is the run of L = 9 (ceil(7.2) = 8: updates 0 .. 7, none decayed under either schedule).  With L = 15
# (ceil(12) = 12) updates 12 and 13 are decayed; L = 14 has ceil(11.2) = 12 as well, so the intended run of 14 is the prefix of the
# intended run of 15 through update 12, and the input of update 12 -- 13 steps, none decayed -- is the CONSTANT run of 13 (the
# intended run of 13 decays its update 11: ceil(10.4) = 11).
SCHEDULE_RUNS = [("constant", L) for L in (9, 10, 13, 14, 15)] + [("intended", L) for L in (9, 10, 14, 15)]
# (previous run, run, schedule of the update, decayed?)
SCHEDULE_PAIRS = [(("intended", 9), ("intended", 10), "intended", True), (("constant", 9), ("constant", 10), "constant", False),
                  (("constant", 13), ("intended", 14), "intended", True), (("intended", 14), ("intended", 15), "intended", True),
                  (("constant", 13), ("constant", 14), "constant", False), (("constant", 14), ("constant", 15), "constant", False)]


def run_schedule_checks(case, runs, memo=None):
    """(5) on runs = {(schedule, L): run} for SCHEDULE_RUNS: the prefixes the pairs rely on are asserted, not assumed -- the
    intended run of 9 is the constant run of 9 bit for bit; the partials of the intended run of 14 (the gradient at Z[12], the
    state in front of its first decayed update) are the constant run of 14's bit for bit; and through (2) the gradient every
    update consumed is the float64 gradient at the previous run's Z."""
    memo = memo or PR.Memo()
    res = PR.Result()
    assert is_decayed(8, 10) and not is_decayed(7, 10) and not is_decayed(7, 9)
    assert is_decayed(12, 14) and is_decayed(12, 15) and is_decayed(13, 15) and not is_decayed(11, 14) and not is_decayed(11, 15) and is_decayed(11, 13)
    same_bits(res, 5, "intended 9 = constant 9", runs[("intended", 9)], runs[("constant", 9)])
    same_bits(res, 5, "intended 14 = constant 14 in front of update 12", runs[("intended", 14)], runs[("constant", 14)], keys=("part",))
    for kp, kc, schedule, decayed in SCHEDULE_PAIRS:
        prev, cur = runs[kp], runs[kc]
        L, k = cur["L"], cur["L"] - 2
        assert prev["L"] == L - 1 and kc[1] == L and (schedule == "intended" and is_decayed(k, L)) == decayed
        tag = " %s L=%d" % (schedule, L)
        lr_k = lr_at(case["lr"], k, L, schedule)
        assert (lr_k == F32(case["lr"]) * F32(0.1)) if decayed else (lr_k == F32(case["lr"]))
        g32 = check_update(res, case, prev, cur, lr_k, tag)
        check_gradient(res, case, prev, cur, memo, g32, tag)
        if decayed:
            check_lr_condition(res, cur["m"], cur["z"], case["lr"], "update %d%s" % (k, tag))
    for key in SCHEDULE_RUNS:
        if key[1] in (10, 14, 15):
            check_final(res, case, runs[key], memo, " %s" % key[0])
    return res


# ---- the float64 trajectory (the lr condition without a device) and the float32 emulation ---------------------------------------
def trajectory64(case, L, schedule="constant"):
    """Float64 loop from z0: lists Z[0 .. L - 1], M[0 .. L - 1]."""
    p, arch = case["p"], case["arch"]
    z, m = case["z0"].astype(np.float64), np.zeros(case["z0"].shape, np.float64)
    Z, M = [z], [m]
    for k in range(L - 1):
        fwd = PR.forward_from_z(p, arch, z)
        g = PR.backward_with_gates(p, arch, fwd["y"], case["x"], case["R"], _gates(fwd["act"]))[0]
        m = np.float64(F32(case["momentum"])) * m + g
        z = z - np.float64(lr_at(case["lr"], k, L, schedule)) * m
        Z.append(z); M.append(m)
    return Z, M


def _emul_state(p, arch, z, x, R, nsplit):
    """Float32 forward and backward at z (path_reference's float32 layers): acts, y, loss, and the split-K partials of dz
    [rows][nsplit][latent] (slice s = features [s ks, (s + 1) ks) of the Linear layer's output, f = (oh * 4 + ow) * C + c)."""
    fwd = PR.forward_from_z(p, arch, z, F32)
    loss, _ = PR.loss_and_dy(fwd["y"], x, R, F32)
    _, grads = PR.backward_with_gates(p, arch, fwd["y"], x, R, _gates(fwd["act"]), F32)
    da0 = grads[0].reshape(len(z), -1)
    W = np.asarray(p["Generator.Input.W"], F32)
    ks = da0.shape[1] // nsplit
    part = np.stack([da0[:, s * ks:(s + 1) * ks] @ W[:, s * ks:(s + 1) * ks].T for s in range(nsplit)], axis=1)
    return {"acts": fwd["act"], "y": fwd["y"], "loss": loss, "part": np.ascontiguousarray(part, F32)}


def emulate_call(case, L, schedule="constant", defect=(), m_init=None, memo=None, rows=None):
    """One call of the loop in numpy float32 (the update with the device's fused multiply-adds) as a run record.  rows: only the first `rows` latent rows (whole images).  defect,
    one of
      ("drop_slice", s)       slice s is left out of g
      ("prev_part",)          the slices are summed, but from the previous step's part (zeros at step 0)
      ("m_not_updated",)      z is stepped with the old m, m stays
      ("m_twice",)            m is advanced twice per step
      ("skip_rows", lo, hi)   rows [lo, hi) are not updated
      ("lr_undecayed",)       a decayed step uses lr
      ("lr_early",)           the step in front of the first decayed one is decayed too
      ("dead_update",)        the reference's L-th update is applied behind the last forward
    m_init: the momentum buffer the call starts from (None = zeros; the previous call's m = "m carried over")."""
    memo = memo or PR.Memo()
    p, arch, R, ns = case["p"], case["arch"], case["R"], case["nsplit"]
    n = case["n"] if rows is None else rows
    x, z = case["x"][:n // R], case["z0"][:n].copy()
    m = np.zeros_like(z) if m_init is None else np.asarray(m_init, F32)[:n].copy()
    kind = defect[0] if defect else None
    mu = F32(case["momentum"])
    steps = max(L, 1)
    part = prev_part = None
    for k in range(steps):
        st = memo(_emul_state, p, arch, z, x, R, ns)
        if k == steps - 1 and kind != "dead_update":
            break
        if k == steps - 1 and steps < 2:
            break
        prev_part, part = part, st["part"]
        src = part
        if kind == "prev_part":
            src = prev_part if prev_part is not None else np.zeros_like(part)
        g = np.zeros_like(z)
        for s in range(ns):
            if kind == "drop_slice" and s == defect[1]:
                continue
            g = g + src[:, s]
        kk = k
        if kind == "lr_undecayed":
            lr_k = F32(case["lr"])
        else:
            if kind == "lr_early" and schedule == "intended" and k + 1 < steps and is_decayed(k + 1, L):
                kk = k + 1
            lr_k = lr_at(case["lr"], kk, L, schedule)
        # the device's fused multiply-adds: one rounding each (formed in float64, where the product is exact)
        fma = lambda a, b, c: (np.float64(a) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)
        if kind == "m_not_updated":
            m1, z1 = m, fma(-lr_k, m, z)
        elif kind == "m_twice":
            m1 = fma(mu, fma(mu, m, g), g)
            z1 = fma(-lr_k, m1, z)
        else:
            m1 = fma(mu, m, g)
            z1 = fma(-lr_k, m1, z)
        if kind == "skip_rows":
            m1[defect[1]:defect[2]] = m[defect[1]:defect[2]]
            z1[defect[1]:defect[2]] = z[defect[1]:defect[2]]
        m, z = m1.astype(F32), z1.astype(F32)
    B = n // R
    idx = np.argmin(np.asarray(st["loss"]).reshape(B, R), axis=1).astype(np.int32)
    rec = st["y"].reshape(B, R, *st["y"].shape[1:])[np.arange(B), idx]
    return {"L": L, "z": z, "m": m, "part": part, "acts": st["acts"], "y": st["y"], "loss": st["loss"], "rec": rec, "idx": idx}
