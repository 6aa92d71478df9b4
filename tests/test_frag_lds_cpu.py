"""Without a GPU: the LDS layout of the fragment-order GEMM (defensegan_amd/csrc/dg_frag_lds.h, used by dg_fgemm.hip) against the
kernel's barriers, and the case table of tests/test_gpu_frag_values.py against the planner.

tests/support/frag_lds_epochs.cpp lists, for every wave of a workgroup, K splits 1, 2 and 4 and both output forms, the byte
intervals the wave reads and writes, grouped by barrier epoch.  THE EPOCH TABLE IS A HAND TRANSCRIPTION of the barriers of
frag_body (dg_fgemm.hip lines 206-224 for the reduction, 245-296 for the epilogue; the lines are cited one by one in that file);
the offsets and sizes are the header's.  Two accesses of different waves are ORDERED only when a barrier both waves pass lies
between them: same epoch = unordered, and whatever a wave does after its last barrier is unordered against everything another
wave does from that epoch on.  Asserted: unordered accesses of different waves, at least one a write, never share a byte; every
interval lies inside the launch's dynamic LDS.

The same walk with the rule the kernel had before (epilogue slice = wave * 32 * pitch) reports exactly what that rule did wrong:
at K split 2 with NHWC output wave 2 writes its slice [17408, 26112) while wave 0 may still be reading tile 0's image
[0, 32768) -- wave 0 then adds wave 2's outputs to its accumulators.  Derived from the code, never reproduced on demand."""
import ctypes as C
import os
import subprocess

import pytest

from tests.support import frag_cases as FC
from tests.support import path_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "defensegan_amd", "csrc")
SUP = os.path.join(ROOT, "tests", "support")
SO = os.path.join(SUP, "_build", "libdgfrag_test.so")
TW, TN = 2, 4                                 # dg_fgemm.hip launch_mo


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    srcs = [os.path.join(SUP, "frag_lds_epochs.cpp"), os.path.join(SUP, "plan_host_exec.cpp"), os.path.join(CSRC, "dg_plan.cpp")]
    deps = srcs + [os.path.join(CSRC, f) for f in ("dg_frag_lds.h", "dg_plan.h", "dg_types.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SO] + srcs)
    l = C.CDLL(SO)
    l.dgf_intervals.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int), C.c_int]
    l.dgp_build.restype = C.c_void_p
    l.dgp_build.argtypes = [C.c_char_p] + [C.c_int] * 7
    l.dgp_free.argtypes = [C.c_void_p]
    l.dgp2_build.restype = C.c_void_p
    l.dgp2_build.argtypes = [C.c_void_p]
    l.dgp2_free.argtypes = [C.c_void_p]
    l.dgp2_classes.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    l.dgp2_info.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    l.dgp2_frag_jobs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    return l


# ---- the LDS layout ---------------------------------------------------------------------------------------------------------
def _intervals(lib, ks, out_frag, rule):
    buf = (C.c_int * (6 * 64))()
    n = lib.dgf_intervals(ks, out_frag, rule, TW, TN, buf, 64)
    assert n >= 0
    keys = ("wave", "epoch", "last", "write", "begin", "end")
    return [dict(zip(keys, buf[6 * i:6 * i + 6])) for i in range(n)]


def _unordered(a, b):
    if a["wave"] == b["wave"]:
        return False                          # a wave's own LDS accesses execute in program order
    if a["epoch"] == b["epoch"]:
        return True
    lo, hi = (a, b) if a["epoch"] < b["epoch"] else (b, a)
    return lo["epoch"] == lo["last"]          # the earlier wave never arrives at the barrier the later one has passed


def _conflicts(recs):
    out = []
    for i, a in enumerate(recs):
        for b in recs[i + 1:]:
            if _unordered(a, b) and (a["write"] or b["write"]) and a["begin"] < b["end"] and b["begin"] < a["end"]:
                out.append((a, b))
    return out


@pytest.mark.parametrize("out_frag", [0, 1])
@pytest.mark.parametrize("ks", [1, 2, 4])
def test_no_two_waves_share_a_byte_that_no_barrier_orders(lib, ks, out_frag):
    recs = _intervals(lib, ks, out_frag, 0)
    size = lib.dgf_launch_bytes(TW, TN)
    assert size == 65536 and lib.dgf_fits(TW, TN) == 1
    assert all(0 <= r["begin"] < r["end"] <= size for r in recs), recs
    assert _conflicts(recs) == []
    # the table is not empty where the kernel uses LDS: one image hand-off per odd K part, an epilogue slice per NHWC tile
    waves_with_slice = {r["wave"] for r in recs if r["epoch"] == r["last"] and r["write"]}
    assert waves_with_slice == (set() if out_frag else {1: {0, 1, 2, 3}, 2: {0, 2}, 4: {0}}[ks])
    assert sum(r["write"] and r["end"] - r["begin"] == 32768 for r in recs) == {1: 0, 2: 2, 4: 3}[ks]


def test_the_former_slice_rule_is_reported_as_the_wave0_read_wave2_write_overlap(lib):
    found = {}
    for ks in (1, 2, 4):
        for out_frag in (0, 1):
            c = _conflicts(_intervals(lib, ks, out_frag, 1))
            if c:
                found[(ks, out_frag)] = c
    assert list(found) == [(2, 0)], sorted(found)
    (a, b), = found[(2, 0)]
    rd, wr = (a, b) if b["write"] else (b, a)
    assert (rd["wave"], rd["write"], rd["begin"], rd["end"]) == (0, 0, 0, 32768)                # wave 0 adding tile 0's image
    assert (wr["wave"], wr["write"], wr["begin"], wr["end"]) == (2, 1, 17408, 26112)            # wave 2 transposing its outputs
    assert rd["epoch"] == wr["epoch"] == 1 == rd["last"] == wr["last"]                          # both behind the only barrier


def test_the_walk_sees_an_unordered_access_of_a_wave_that_has_left():
    """The rule itself: a wave in its final epoch is unordered against a later epoch of another wave."""
    a = dict(wave=1, epoch=1, last=1, write=1, begin=0, end=16)
    b = dict(wave=0, epoch=2, last=3, write=0, begin=8, end=24)
    assert _conflicts([a, b]) and not _conflicts([dict(a, last=2), b]) and not _conflicts([dict(a, wave=0), b])


# ---- the GPU case table against the planner ---------------------------------------------------------------------------------
def _planner_jobs(lib, h_in, h_used, cin, cout, rows):
    """(supported, [(ksplit, n_mblk, n_taps)], [(positions, chunks)] per class) of the engine's plan of one forward layer without Batchnorm."""
    h1 = lib.dgp_build(b"deconv_fwd", h_in, h_in, h_used, h_used, cin, cout, cout)
    h2 = lib.dgp2_build(h1)
    try:
        buf = (C.c_int * (3 * 65536))()
        n = lib.dgp2_frag_jobs(h2, rows, buf, 65536)
        assert n >= 0
        i2 = (C.c_longlong * 4)()
        lib.dgp2_info(h2, i2)
        cls = (C.c_int * (2 * i2[0]))()
        lib.dgp2_classes(h2, cls)
        return n > 0, [tuple(buf[3 * i:3 * i + 3]) for i in range(n)], [(cls[2 * i], cls[2 * i + 1]) for i in range(i2[0])]
    finally:
        lib.dgp2_free(h2); lib.dgp_free(h1)


def test_layer_shapes_are_the_generators():
    from defensegan_amd import synth
    for arch in ("mnist", "celeba"):
        for net_dim in (64, 128):
            p = synth.make_weights(arch, seed=1, gain=1.0, bias_range=0.1, net_dim=net_dim)
            for d, (h_in, h_used, cin, cout) in enumerate(FC.gemm_layers(arch, net_dim), start=1):
                name = PR.O._arch_layers(arch)[d - 1][0]
                assert p[name + ".Filters"].shape == (5, 5, cout, cin), (arch, net_dim, d)
            assert p["Generator.Input.W"].shape[1] == 16 * FC.gemm_layers(arch, net_dim)[0][2]


def test_python_restatement_of_the_k_split_is_the_planners(lib):
    for arch in ("mnist", "celeba"):
        for net_dim in FC.NET_DIMS:
            nd = PR.n_act(arch)
            ok_all = True
            for d, (h_in, h_used, cin, cout) in enumerate(FC.gemm_layers(arch, net_dim), start=1):
                sup, jobs, classes = _planner_jobs(lib, h_in, h_used, cin, cout, 33)
                assert sup == FC.layer_supported(cin, cout), (arch, net_dim, d)
                ok_all = ok_all and sup
                if not sup:
                    continue
                # per class (positions, taps) -> K split: the planner's classes and the reference's are the same multiset
                mine = sorted((c["positions"], c["taps"], ks) for c, ks in zip(PR.tap_class_masks(arch, d, "fwd")[1], FC.class_ksplits(arch, net_dim, d)))
                theirs = sorted({(pos, ch * 32 // cin) for pos, ch in classes})
                assert sorted({(a, b) for a, b, _ in mine}) == theirs
                assert {(t, ks) for _, t, ks in mine} == {(t, ks) for ks, _, t in jobs}, (arch, net_dim, d)
            assert ok_all == FC.generator_supported(arch, net_dim), (arch, net_dim)


def test_case_table_reaches_every_reachable_pair(lib):
    """Reachable = what build_frag_jobs hands to a generator the engine accepts, at any of the widths looked at.  Named here: the
    pair no supported generator reaches (FC.UNREACHED: K split 4 with NHWC output)."""
    reachable = set()
    for arch in ("mnist", "celeba"):
        for net_dim in FC.NET_DIMS:
            layers = FC.gemm_layers(arch, net_dim)
            runs = [_planner_jobs(lib, h_in, h_used, cin, cout, 33) for h_in, h_used, cin, cout in layers]
            if not all(r[0] for r in runs):
                assert FC.pairs(arch, net_dim) == set()
                continue
            got = {(ks, "nhwc" if d == len(layers) else "frag") for d, r in enumerate(runs, start=1) for ks, _, _ in r[1]}
            assert got == FC.pairs(arch, net_dim), (arch, net_dim)
            reachable |= got
    covered = set().union(*(FC.pairs(a, n) for a, n, _ in FC.CASES))
    assert covered == reachable == FC.ALL_PAIRS - FC.UNREACHED, (sorted(covered), sorted(reachable))
    assert FC.pairs(*FC.FALLBACK[:2]) == set()                      # the fall-back case really is one
    assert FC.UNREACHED == {(4, "nhwc")}


def test_case_table_holds_partial_tiles_and_short_last_jobs(lib):
    """33 / 47 rows: a class's M blocks (2 row blocks x positions) are no multiple of the 4 of a wave tile somewhere (nvalid < TN);
    129 rows on MNIST: 5 row blocks, jobs with fewer M blocks than the TN * (4 / ksplit) of a full job, at every K split."""
    short = set()
    for rows in (33, 47, 129):
        partial = False
        for h_in, h_used, cin, cout in FC.gemm_layers("mnist", 64):
            _, jobs, _ = _planner_jobs(lib, h_in, h_used, cin, cout, rows)
            partial = partial or any(n % FC.TN for _, n, _ in jobs)
            if rows == 129:
                short |= {ks for ks, n, _ in jobs if n < FC.TN * (4 // ks)}
        assert partial, rows
    assert short == {1, 2, 4}
