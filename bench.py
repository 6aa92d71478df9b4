#!/usr/bin/env python
"""Benchmark of the Defense-GAN latent-projection hot path on MI355X.

metric : projected images/sec at L=200, R=10 (MNIST 28x28)      (BASELINE.json)
step   : one pass of the hot path (dg_reconstruct) over one batch of B synthetic images per GPU,
         inputs already resident in HBM; weak scaling (every rank projects its own batch).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...        (no launcher: re-executes itself as the line above; exits non-zero when the node
                                         has fewer than N GPUs -- it never prints an n_gpus it did not run on)

--strong: BASELINE configs[4] shape instead -- a step is ONE defended evaluation of a fixed list of 10 000 synthetic
images (FGSM eps = 0.3 inputs from the bare classifier, model A; built untimed), sharded contiguously over the ranks (gan_defense.shard_range), projected
in batches, with the single all_gather of (labels, preds, diffs) at the end; images/s = 10 000 / wall ("scaling": "strong").

A plain run does only what the headline figure needs: set-up, the W warm-up steps, the K timed steps, the outputs
(--dump-outputs) and the JSON line; its `roofline` holds the whole-path figures only.  --full adds the measurements that take
runs of their own, after the timed steps: the per-kernel event pass below (`kernels`, the dominant kernel's roofline) and the
torch-CPU baseline (`cpu_baseline`).

The timed region carries NO instrumentation.  Per-kernel durations for the roofline leg (--full) come from ONE extra, untimed
step after it, in which every kernel of every GD iteration sits between two hipEvent markers on the launch stream
(consecutive launches share the marker between them, so the durations add up to that step's wall time,
`roofline.profiled_step_ms`; the markers themselves make that step ~2 % longer than a timed one).

--dump-outputs DIR: what the last timed step returned to its caller (rec, idx, loss, z; --strong: accuracy, labels, preds,
diffs), written after the timed steps as DIR/<name>.npy (dump_outputs).  The inputs are drawn from fixed seeds, so two builds
run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from defensegan_amd import archs, synth
from defensegan_amd.gan import dataset_gan_dict

PEAK_FP32_TFLOPS = 157.3        # MI355X fp32 MFMA == fp32 vector peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0

WORKLOADS = {
    # name: (arch, weight seed, gain, B, R, L)
    "mnist": ("mnist", 1234, 2.0, 256, 10, 200),       # BASELINE configs[1]
    "fmnist": ("f-mnist", 4321, 2.0, 256, 10, 200),    # configs[2]
    "celeba": ("celeba", 1234, 2.0, 128, 10, 200),     # configs[3]
}


def build_id():
    """First 12 hex digits of the SHA-256 over the HIP/C++ sources the loaded library was built from (comments and layout
    excluded: defensegan_amd.build.code_digest)."""
    from defensegan_amd import build as _b
    return _b.code_digest()[:12]


def traffic_for(workload, layers, B, R, tuning_id=None):
    """HBM-side bytes per launch of the LAYERS that ran as the dominant kernel symbol, from the committed rocprofv3 PMC passes
    (tools/pmc_traffic.py: FETCH_SIZE doubled per the gfx950 correction + WRITE_SIZE, separate --pmc runs, rows keyed by layer
    through the fixed launch order of a GD iteration).  PMC counters cannot be read from inside this process, so the figure
    comes from a file -- and is quoted ONLY when that file was collected on exactly this build of the kernels (its "build"
    equals build_id()), on this row count, and -- the job list of a layer being a timed choice -- with the SAME job lists
    (its "tuning_id" equals this process's, tools/collect_profiles.sh shares them through DG_TUNING_CACHE); otherwise null.
    The value is the mean over the named layers (what `achieved` averages over)."""
    path = os.path.join(ROOT, "profiles", TRAFFIC_FILE)
    key = "mnist" if workload in ("mnist", "fmnist") else workload
    if not layers or not os.path.exists(path) or B * R != {"mnist": 2560, "celeba": 1280}.get(key, -1):
        return None, None
    with open(path) as fh:
        doc = json.load(fh)
    if doc.get("builds", {}).get(key) != build_id():
        return None, None
    if tuning_id is not None and doc.get("tuning_ids", {}).get(key) != tuning_id:
        return None, None
    rows = doc.get(key, {}).get("by_layer", {})
    vals = [rows[l]["bytes_per_launch"] for l in layers if l in rows]
    if len(vals) != len(layers):
        return None, None
    return int(sum(vals) / len(vals)), "profiles/" + TRAFFIC_FILE


PROFILE_ROUND = "r06"                  # profiles/<round>_*: the evidence collected on this build (tools/final_validation.sh)
TRAFFIC_FILE = PROFILE_ROUND + "_pmc_traffic.json"
TUNING_FILE = PROFILE_ROUND + "_tuning_%s.txt"       # profiles/: the job-list choice of the profiling run, per architecture
COLL_BACKEND = os.environ.get("DG_BENCH_BACKEND", "nccl")     # "gloo": the shared-GPU test mode of the N > 1 flow (see main)
DUMP_LIMIT_BYTES = 64 << 20            # --dump-outputs: the most a run writes


def dump_outputs(arrays, out_dir, suffix="", limit=DUMP_LIMIT_BYTES):
    """Writes every named array (torch tensor, NumPy array or scalar) as <out_dir>/<name><suffix>.npy: float64 stays float64,
    integers and booleans become float64 (exact below 2**53), every other type float32.  When the files would add up to more
    than `limit` bytes, each array keeps the same fraction of its leading-axis rows, a fixed sample (RandomState(0), rows in order)."""
    conv = {}
    for name, v in arrays.items():
        v = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
        conv[name] = v.astype(np.float64 if v.dtype == np.float64 or v.dtype.kind in "biu" else np.float32)
    total = sum(v.nbytes for v in conv.values())
    budget = limit - 4096 * len(conv)                               # room for the .npy headers
    if total > budget:
        frac = budget / float(total)
        for name, v in conv.items():
            if v.ndim and v.shape[0] > 1:
                n = max(1, int(v.shape[0] * frac))
                conv[name] = v[np.sort(np.random.RandomState(0).choice(v.shape[0], n, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    for name, v in conv.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), v)


def make_inputs(gan, a, B, rank=0, first_image=0):
    """The bench's synthetic inputs, resident in HBM: x = clip(G(z_true) + 0.3*sign(noise)), an FGSM-eps-0.3-like
    perturbation of in-range images (whitebox.py:199).  Both draws are counter-based and keyed by the image index, so the
    images do not depend on how they are batched or sharded.  Also used by tests/test_gpu_parity_tiers.py."""
    import torch
    zt = gan.init_latents(B, seed=1000 + rank, first_row=first_image)
    x = gan.generate(zt)
    P = int(np.prod(a.image_dim))
    rows = (P + a.latent_dim - 1) // a.latent_dim
    noise = gan.init_latents(B * rows, seed=7 + rank, first_row=first_image * rows, std=1.0).view(B, -1)[:, :P].reshape(x.shape)
    return torch.clamp(x + 0.3 * torch.sign(noise), a.in_lo, a.in_hi).contiguous()


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores_one_socket():
    """(physical cores of socket 0, logical CPUs) from /proc/cpuinfo; (None, n) when it cannot be read."""
    ncpu = os.cpu_count() or 1
    try:
        cores, phys, core = set(), None, None
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                k, _, v = line.partition(":")
                k = k.strip()
                if k == "physical id":
                    phys = v.strip()
                elif k == "core id":
                    core = v.strip()
                elif not k and phys is not None and core is not None:
                    if phys == "0":
                        cores.add(core)
                    phys = core = None
        if phys == "0" and core is not None:
            cores.add(core)
        return (len(cores) or None), ncpu
    except OSError:
        return None, ncpu


# The ONE thread count of the CPU baseline.  Rounds 4 / 5 probed {8, 16, 32, 64, cores of a socket} and kept the fastest: the probe
# flipped between 16, 32 and 64 from box to box (6.1 ... 8.5 images/s for one CPU model), so the reported figure meant a different
# thing every time.  The rule is now fixed: 16 threads -- where this workload (160 MFLOP per image-step in 5x5 convolutions over
# 16 x R rows) stops scaling on the pool's EPYC 9575F hosts: 8.5 images/s at 16, 4-6 at 32, 2.1 at 64 = the physical cores of a
# socket (profiles/r05_bench_*; more threads lose to the thread pool's synchronisation per small convolution) -- pinned to 16
# distinct physical cores of socket 0, two timed full-L batches, the faster one reported with the spread.
CPU_BASELINE_THREADS = 16


def socket0_core_cpus():
    """Logical CPU ids, one per distinct physical core of socket 0, in /proc/cpuinfo order ([] when it cannot be read)."""
    try:
        out, seen, cur = [], set(), {}
        with open("/proc/cpuinfo") as fh:
            for line in list(fh) + ["\n"]:
                k, _, v = line.partition(":")
                k = k.strip()
                if k in ("processor", "physical id", "core id"):
                    cur[k] = v.strip()
                elif not k and cur:
                    if cur.get("physical id", "0") == "0" and cur.get("core id") not in seen and "processor" in cur:
                        seen.add(cur.get("core id"))
                        out.append(int(cur["processor"]))
                    cur = {}
        return out
    except (OSError, ValueError):
        return []


def cpu_baseline(arch, params, x_np, R, L, budget_s=16.0):
    """The oracle's torch-CPU formulation (a PORT of the reference graph: TF 1.7 cannot be installed here) on this box's host
    cores, by a FIXED rule (CPU_BASELINE_THREADS): 16 threads pinned to 16 distinct physical cores of socket 0, one warm-up of two
    steps, then TWO batches over the FULL L steps -- measured, not a short sample scaled by (2L-1); `value` is the faster one,
    `spread` = (slower - faster) / faster, both times are in `sample`.  A batch is 64 images, halved (32 / 16 / 8 / 4) while a warm
    two-step run predicts more than `budget_s` seconds for it (MNIST: 64 images, ~10 s; CelebA: 16 images, ~16 s), and only then
    are the steps cut: 20-30 s of CPU work in all."""
    from oracle import torch_ref as T          # checker / baseline only -- never on the product path
    phys, ncpu = physical_cores_one_socket()
    threads = max(1, min(CPU_BASELINE_THREADS, phys or ncpu, ncpu))
    cpus = socket0_core_cpus()[:threads]
    old_aff = None
    try:
        if len(cpus) == threads and hasattr(os, "sched_setaffinity"):
            old_aff = os.sched_getaffinity(0)
            allowed = [c for c in cpus if c in old_aff]
            if len(allowed) == threads:
                os.sched_setaffinity(0, allowed)
            else:
                old_aff = None
    except OSError:
        old_aff = None
    pinned = old_aff is not None
    torch.set_num_threads(threads)
    gen = T.TorchGenerator(params, arch)
    a = archs.make_arch(arch)
    nimg = min(64, len(x_np))
    z0 = synth.make_z(nimg * R, a.latent_dim, seed=3)
    try:
        T.reconstruct(params, x_np[:nimg], z0, R, 2, arch=arch, gen=gen)      # warm-up (thread pool, allocator)
        t0 = time.perf_counter()
        T.reconstruct(params, x_np[:nimg], z0, R, 2, arch=arch, gen=gen)
        per_pass = (time.perf_counter() - t0) / 3.0                            # L steps = 2L - 1 passes over nimg images
        Ls, n_run = L, nimg
        while n_run > 4 and per_pass * (n_run / float(nimg)) * (2 * L - 1) > budget_s:
            n_run //= 2
        if per_pass * (n_run / float(nimg)) * (2 * L - 1) > budget_s:
            Ls = int(max(3, (budget_s / (per_pass * n_run / float(nimg)) + 1) // 2))
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            T.reconstruct(params, x_np[:n_run], z0[:n_run * R], R, Ls, arch=arch, gen=gen)
            times.append(time.perf_counter() - t0)
    finally:
        if old_aff is not None:
            try:
                os.sched_setaffinity(0, old_aff)
            except OSError:
                pass
    dt = min(times)
    t_full = dt * (2 * L - 1) / (2 * Ls - 1)                                  # == dt when the full L ran
    sample = "%d images x R=%d x L=%d, torch-CPU autograd restatement, %d threads (fixed rule)%s of %d host CPUs (%s physical cores on socket 0), two batches %.1f s and %.1f s, the faster one reported%s" % (
        n_run, R, Ls, threads, " pinned to %d cores of socket 0" % threads if pinned else "", ncpu, phys if phys else "?", times[0], times[1],
        "" if Ls == L else ", scaled by (2L-1) to L=%d" % L)
    return {"value": n_run / t_full, "unit": "images/s", "cores": threads, "threads": threads, "host_cores": ncpu,
            "physical_cores_socket0": phys, "pinned": pinned, "spread": round((max(times) - dt) / dt, 4),
            "cpu_model": _cpu_model(), "kind": "port", "sample": sample}


def roofline_from_profile(prof, workload, B, R, path_tflops, tuning_id=None):
    """Per-layer rows + the roofline object of the dominant kernel symbol from the engine's event profile.  Profile
    entries are "<layer>@<kernel symbol>": per-layer rows for the breakdown, per-symbol groups (what rocprofv3 --stats
    aggregates) for the roofline."""
    kernels, groups = [], {}
    for p in prof:
        if p["launches"] == 0:
            continue
        layer, _, sym = p["name"].partition("@")
        avg_ms = p["ms"] / p["launches"]
        tf = (p["flops"] / p["launches"]) / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
        kernels.append({"name": layer, "kernel": sym, "launches_sampled": p["launches"],
                        "avg_us": round(avg_ms * 1e3, 2), "tflops": round(tf, 2)})
        g = groups.setdefault(sym, {"ms": 0.0, "flops": 0.0, "launches": 0})
        g["ms"] += p["ms"]; g["flops"] += p["flops"]; g["launches"] += p["launches"]
    dom = None
    if groups:
        # dominant kernel symbol = the one that did the most ALGORITHMIC FLOP in the profiled step; ties -> the symbol launched
        # first in a GD iteration (the forward layer).  (Round 4 took the symbol with the most TIME: Generator.3's forward and
        # backward run as two symbols with the same FLOP and durations 0.05 % apart, so the choice flipped from run to run.)
        order = []
        for k in kernels:
            if k["kernel"] not in order:
                order.append(k["kernel"])
        sym = max(order, key=lambda q: (round(groups[q]["flops"] / max(g_["flops"] for g_ in groups.values()), 3), -order.index(q)))
        g = groups[sym]
        dom = {"kernel": sym, "avg_us": round(g["ms"] / g["launches"] * 1e3, 2),
               "flop_per_launch": g["flops"] / g["launches"],
               "tflops": round(g["flops"] / (g["ms"] * 1e-3) / 1e12, 2)}
    dom_layers = [k["name"] for k in kernels if dom and k["kernel"] == dom["kernel"]]
    traffic, traffic_src = traffic_for(workload, dom_layers, B, R, tuning_id)
    roofline = {
        "bound": "mfma",
        "kernel": dom["kernel"] if dom else None,
        "layers": dom_layers,
        "avg_launch_us": dom["avg_us"] if dom else None,
        "flop_per_launch": dom["flop_per_launch"] if dom else None,
        "achieved": dom["tflops"] if dom else round(path_tflops, 2),
        "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s",
        "frac": round((dom["tflops"] if dom else path_tflops) / PEAK_FP32_TFLOPS, 4),
        "traffic": traffic, "traffic_source": traffic_src,
        "path_achieved": round(path_tflops, 2),
        "path_frac": round(path_tflops / PEAK_FP32_TFLOPS, 4),
        "sum_kernel_ms_per_step": round(sum(g["ms"] for g in groups.values()), 3) if groups else None,
        # every MFMA layer of the loop, largest first: the roofline fraction does not hang on which one is called dominant
        "mfma_layers": [{"layer": k["name"], "kernel": k["kernel"], "avg_us": k["avg_us"], "tflops": k["tflops"],
                         "frac": round(k["tflops"] / PEAK_FP32_TFLOPS, 4)}
                        for k in sorted(kernels, key=lambda q: -q["tflops"] * q["avg_us"]) if k["tflops"] > 0][:8],
    }
    return kernels, roofline


def self_launch_command(argv, n_gpus, port):
    """The command `python bench.py --gpus N ...` turns itself into when N > 1 and no launcher set WORLD_SIZE: one rank
    per GPU of this node under torch.distributed.run (backend nccl = RCCL), rendezvous on 127.0.0.1 (the container's
    hostname may not resolve).  `argv` = the bench's own arguments, passed through unchanged."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(n_gpus)),
            "--master-addr", "127.0.0.1", "--master-port", str(int(port)), os.path.abspath(__file__)] + list(argv)


def rank_cpus(local_rank, local_world, cpus):
    """The host CPUs rank `local_rank` of `local_world` ranks on this node enqueues from: a contiguous 1 / local_world slice of
    the CPUs this process may run on (sorted), at most 8 of them -- a rank's ~1600 enqueues per projection call then stay on
    the cores (and the NUMA node) they started on instead of migrating between calls."""
    cpus = sorted(cpus)
    per = max(1, len(cpus) // max(1, local_world))
    mine = cpus[local_rank * per:(local_rank + 1) * per] or cpus
    return mine[:8]


def pin_host_thread(local_rank, local_world):
    """os.sched_setaffinity by LOCAL_RANK (DG_BENCH_PIN=0 switches it off); returns the CPU list, or None when not pinned."""
    if os.environ.get("DG_BENCH_PIN", "1") == "0" or not hasattr(os, "sched_setaffinity"):
        return None
    try:
        mine = rank_cpus(local_rank, local_world, os.sched_getaffinity(0))
        os.sched_setaffinity(0, mine)
        return mine
    except OSError:
        return None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def resolve_ranks(n_gpus, env, device_count):
    """(world, rank, device index, relaunch) for `--gpus n_gpus` under the environment `env` on a node where this process sees
    `device_count` GPUs.  relaunch = True: this process must re-exec itself under torch.distributed.run (N > 1 asked for, no
    launcher present).  Raises SystemExit with a message -- never a silent 1-GPU run -- when the request cannot be honoured."""
    if n_gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1 (got %d)" % n_gpus)
    if "WORLD_SIZE" not in env:
        if device_count < n_gpus:
            raise SystemExit("bench.py: --gpus %d but only %d GPU(s) are visible on this node; refusing to report a %d-GPU "
                             "number from fewer devices" % (n_gpus, device_count, n_gpus))
        return (1, 0, 0, False) if n_gpus == 1 else (n_gpus, 0, 0, True)
    # a launcher started us: it must have started exactly N ranks, and this rank must have a GPU of its own
    world, rank, local_rank = int(env["WORLD_SIZE"]), int(env.get("RANK", "0")), int(env.get("LOCAL_RANK", "0"))
    if world != n_gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (n_gpus, world))
    if device_count < 1:
        raise SystemExit("bench.py: --gpus %d: rank %d sees 0 GPU(s) (no GPU visible)" % (n_gpus, rank))
    if 0 <= local_rank < device_count:
        return world, rank, local_rank, False
    if device_count == 1:
        return world, rank, 0, False            # the launcher narrowed this rank's visibility to its own GPU
    raise SystemExit("bench.py: LOCAL_RANK=%d but %d GPU(s) are visible to this rank" % (local_rank, device_count))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="mnist", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--rec_rr", type=int, default=None)
    ap.add_argument("--rec_iters", type=int, default=None)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also the untimed per-kernel event pass (kernels, roofline of the dominant kernel) "
                         "and the torch-CPU baseline; a plain run does neither")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-profile", action="store_true", help="--full without the untimed per-kernel event pass")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB)")
    ap.add_argument("--strong", action="store_true",
                    help="configs[4] shape: one step = a defended evaluation of --images images sharded over the ranks")
    ap.add_argument("--images", type=int, default=10000, help="--strong: images in the evaluated list")
    ap.add_argument("--host-io", action="store_true",
                    help="hand the images over as a pageable host (NumPy) array and take rec / idx / loss / z back on the host every step: "
                         "the PCIe-inclusive rate of the Python mirror (tagged io=host in the line; never the headline value)")
    ap.add_argument("--opt", action="append", default=[], help="engine option key=value (tuning)")
    ap.add_argument("--retune", action="store_true",
                    help="time the job lists on this box instead of installing the committed choice (profiles/r06_tuning_<arch>.txt)")
    ap.add_argument("--use_bn", action="store_true",
                    help="USE_BN: True variant of the generator (batch-statistics Batchnorm after every hidden layer, "
                         "tflib/ops/batchnorm.py:80-93); not a BASELINE config (the shipped cfgs have USE_BN: False)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")

    world, rank, local_rank, relaunch = resolve_ranks(args.gpus, os.environ, torch.cuda.device_count())
    if relaunch:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, RCCL)
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC only on this driver (RCCL needs it)
        env.setdefault("OMP_NUM_THREADS", "8")
        sys.stdout.flush()
        raise SystemExit(subprocess.call(self_launch_command(sys.argv[1:], args.gpus, _free_port()), env=env))
    # DG_BENCH_FORCE_DIST=1 exercises the RCCL code path with a single rank (used to test it on a 1-GPU box)
    distributed = world > 1 or os.environ.get("DG_BENCH_FORCE_DIST") == "1"
    pinned = pin_host_thread(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world))) if world > 1 else None
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        # DG_BENCH_BACKEND=gloo (tests/test_gpu_dist.py only): the N > 1 flow -- rank 0's job lists broadcast, the barriers, the
        # gathers, the max over ranks -- with the control tensors on the CPU, so that two ranks can share the one GPU of a test box
        # (RCCL refuses two ranks on one device).  The line then says so and reports n_gpus = 1: it is never a multi-GPU number.
        if COLL_BACKEND == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    cdev = torch.device("cpu") if COLL_BACKEND == "gloo" else dev      # where the control tensors of the collectives live

    arch, wseed, gain, B, R, L = WORKLOADS[args.workload]
    if args.strong:
        if args.workload != "mnist":
            raise SystemExit("--strong is the MNIST configs[4] workload")
        B = 1250                    # projection batch = the per-GPU shard of 10 000 images at 8 GPUs
    B = args.batch or B
    R = args.rec_rr or R
    L = args.rec_iters or L
    a = archs.make_arch(arch)
    params = synth.make_weights(arch, seed=wseed, gain=gain, bias_range=0.0, use_bn=args.use_bn,
                                bn_jitter=0.2 if args.use_bn else 0.0)
    gan = dataset_gan_dict[arch](cfg={"USE_BN": bool(args.use_bn), "LATENT_DIM": a.latent_dim, "NET_DIM": a.net_dim},
                                 test_mode=True, rec_rr=R, rec_iters=L, rec_lr=10.0, device=local_rank)
    assert gan.set_weights(params) == []
    for kv in args.opt:
        k, v = kv.split("=", 1)
        gan.set_option(k, v)

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(dev)

    st = {}                       # what the setup below leaves for the timed loop: x, step(i), labels / classifier (--strong)
    if args.strong:
        from defensegan_amd import gan_defense, network_builder as nb
        n_total = args.images
        s0, e0 = gan_defense.shard_range(n_total, rank, world)
        # model_eval_gan coalesces the caller's batches of B images into engine calls of up to COALESCE_ROWS latent rows
        # (--batch 50 = the reference's BATCH_SIZE: 25 caller batches per call): the shapes the engine has to be prepared for,
        # + the ragged last call of this rank's shard
        B_call = gan_defense.engine_batch_images(B, R, max(e0 - s0, 1))
        shapes = [B_call] + ([(e0 - s0) % B_call] if (e0 - s0) % B_call else [])
        units_per_step = n_total
    else:
        shapes = [B]
        units_per_step = world * B
    result = {}

    def build_inputs():
        if args.strong:
            # ---- configs[4]: a fixed image list, sharded by image; ONE gather of (labels, preds, diffs) per evaluation
            clf = nb.model_a()
            clf._device = local_rank
            clf.init_like_reference(seed=5)
            # untimed setup, the step BEFORE the path (whitebox.py:198-210): clean images G(z_true) keyed by the global image
            # index, labels = the classifier's predictions on them, x = FastGradientMethod(classifier).generate(eps = 0.3,
            # clip [0, 1]) on the bare classifier (the attack is built before the reconstruction layer is attached)
            fgsm = nb.FastGradientMethod(clf)
            xs, ls = [], []
            for i in range(s0, e0, 2000):
                n_i = min(2000, e0 - i)
                clean = gan.generate(gan.init_latents(n_i, seed=1000, first_row=i))
                lab = clf.fprop(clean)["logits"].argmax(dim=1)
                xs.append(fgsm.generate(clean, eps=0.3, y=lab, clip_min=a.in_lo, clip_max=a.in_hi))
                ls.append(lab.cpu().numpy())
            x = torch.cat(xs).contiguous() if xs else torch.empty((0,) + tuple(a.image_dim), device=dev)
            labels = np.concatenate(ls) if ls else np.zeros(0, np.int64)

            def step(i):
                acc, roc = gan_defense.model_eval_gan_sharded(gan.reconstruct, clf, x, labels, batch_size=B, rec_rr=R,
                                                              n_total=n_total, seed=2024 + i)
                result["acc"], result["roc"] = acc, roc
                return None
        else:
            x = make_inputs(gan, a, B, rank)

            def step(i):
                # a new batch of images every step: global row index advances, so z0 differs
                first_row = ((i * world) + rank) * B * R
                return gan.reconstruct(x, seed=2024, first_row=first_row, return_details=True)
            if args.host_io:
                if distributed:
                    raise SystemExit("--host-io is a single-process measurement")
                x_host = x.cpu().numpy()           # pageable, as a caller of the reference hands its images over

                def step(i):
                    return gan.reconstruct(x_host, seed=2024, first_row=i * B * R, return_details=True)
        st["x"], st["step"] = x, step

    # workspace + timed job lists: outside the hot call (dg_prepare); the steps below only enqueue.  With several ranks, rank 0
    # times the candidates and every other rank installs ITS choices (dg_export_tuning -> broadcast -> dg_import_tuning): all
    # ranks launch the same job lists, and the line below names them (tuning_id).
    # The committed choice of the profiling run (tools/collect_profiles.sh), when there is one for this architecture: the lists the
    # rocprofv3 evidence under profiles/ was collected with -- so roofline.traffic can be quoted and two runs launch the same
    # kernels.  A text for another configuration / CU count is refused by the engine (then, and with --retune, the lists are timed
    # here); row counts it does not hold are timed as usual.  DG_TUNING_CACHE (gan.prepare) overrides.
    committed = os.path.join(ROOT, "profiles", TUNING_FILE % ("mnist" if a.arch_id == 0 else "celeba"))
    tun = {"source": "timed in this process"}

    def install_job_lists():
        if not args.retune and not args.use_bn and not args.opt and "DG_TUNING_CACHE" not in os.environ and os.path.exists(committed):
            try:
                with open(committed) as fh:
                    if gan.import_tuning(fh.read()) > 0:
                        tun["source"] = "profiles/" + os.path.basename(committed)
            except Exception as e:         # another configuration / CU count / planner: said in the JSON line, then timed here
                tun["source"] = "timed in this process (profiles/%s refused: %s)" % (os.path.basename(committed), str(e)[:200])
        if distributed and world > 1:
            if rank == 0:
                for b in shapes:
                    gan.prepare(b)
                payload = torch.tensor(list(gan.export_tuning().encode()), dtype=torch.uint8, device=cdev)
                n_bytes = torch.tensor([payload.numel()], dtype=torch.int64, device=cdev)
            else:
                n_bytes = torch.zeros(1, dtype=torch.int64, device=cdev)
            dist.broadcast(n_bytes, 0)
            if rank != 0:
                payload = torch.empty(int(n_bytes.item()), dtype=torch.uint8, device=cdev)
            dist.broadcast(payload, 0)
            if rank != 0:
                gan.import_tuning(bytes(payload.cpu().tolist()).decode())

    # rank 0 times / installs its lists and sends them off FIRST and builds its inputs afterwards; the other ranks build their
    # inputs first and pick the lists up when they are done: rank 0's dg_prepare overlaps their setup instead of following it
    # (--strong builds its inputs through the engine -- dg_generate times job lists for the shard's row count -- so there rank 0
    # builds FIRST and its export carries those lists too; the other ranks install before they build: equal shards then run the
    # same lists in the setup as well, and the per-rank tuning ids of the line agree)
    if (rank == 0) != bool(args.strong):
        install_job_lists()
        build_inputs()
    else:
        build_inputs()
        install_job_lists()
    x, step, tuning_source = st["x"], st["step"], tun["source"]
    torch.cuda.synchronize()
    t_prep = time.perf_counter()
    for b in shapes:
        gan.prepare(b)
    torch.cuda.synchronize()
    prepare_ms = (time.perf_counter() - t_prep) * 1e3    # workspace + job lists of the call shapes: timing the candidates when no text held them
    tuning_id = gan.tuning_id()
    for i in range(args.warmup):
        step(i)
    barrier()
    t0 = time.perf_counter()
    out = None
    for i in range(args.steps):
        out = step(args.warmup + i)
    if distributed and not args.strong:
        # the path's one exchange: per-image (selected restart, best loss) gathered over RCCL/xGMI
        best = out["loss"].view(B, R).min(dim=1).values
        msg = torch.stack([out["idx"].float(), best], dim=1).contiguous().to(cdev)
        gathered = [torch.empty_like(msg) for _ in range(world)]
        dist.all_gather(gathered, msg)
    barrier()
    dt = time.perf_counter() - t0
    per_rank_ms, rank_tuning = [dt / args.steps * 1e3], [tuning_id]
    if distributed:
        # every rank's own time and job-list id (12 hex digits = 6 bytes), then the MAX over ranks is the reported time
        mine = torch.tensor([dt] + [float(b) for b in bytes.fromhex(tuning_id)], dtype=torch.float64, device=cdev)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_ms = [float(t[0].item()) / args.steps * 1e3 for t in allr]
        rank_tuning = [bytes(int(v) for v in t[1:].tolist()).hex() for t in allr]
        dt = max(float(t[0].item()) for t in allr)

    # ---- what the last timed step returned to its caller (every rank its own batch; --strong: the gathered evaluation, rank 0)
    if args.dump_outputs and not (args.strong and rank != 0):
        if args.strong:
            arrays = {"accuracy": result["acc"], "labels": result["roc"][0], "preds": result["roc"][1], "diffs": result["roc"][2]}
        else:
            arrays = out
        dump_outputs(arrays, args.dump_outputs, suffix="_rank%d" % rank if rank else "",
                     limit=DUMP_LIMIT_BYTES // (1 if args.strong else world))

    # ---- untimed (--full): one more step with every kernel of every GD iteration bracketed by hipEvents (rank 0 reports)
    prof = []
    profiled_step_ms = None
    if args.full and not args.no_profile and not args.strong:
        gan.profile_reset()
        gan.profile_enable(1)
        torch.cuda.synchronize(dev)
        tp0 = time.perf_counter()
        step(args.warmup + args.steps)
        torch.cuda.synchronize(dev)
        profiled_step_ms = (time.perf_counter() - tp0) * 1e3
        gan.profile_enable(0)
        prof = gan.profile_read()
    # every rank's duration of the layer with the most FLOP in that marked step: the same job list does the same number of
    # matrix-pipe cycles on every rank, so the ratio of these durations is the ratio of the GEMM clocks the ranks sustained
    # (the per-rank "GEMM clock" a PMC pass would give as GRBM cycles / duration; counters cannot be read from inside the bench)
    big_layer_us = [None]
    if prof:
        top = max((p_ for p_ in prof if p_["launches"]), key=lambda p_: p_["flops"] / p_["launches"], default=None)
        if top:
            big_layer_us = [round(top["ms"] / top["launches"] * 1e3, 2)]
            if distributed:
                mine = torch.tensor([big_layer_us[0]], dtype=torch.float64, device=cdev)
                allr = [torch.empty_like(mine) for _ in range(world)]
                dist.all_gather(allr, mine)
                big_layer_us = [round(float(t.item()), 2) for t in allr]

    if rank == 0:
        value = units_per_step * args.steps / dt
        flop_img = archs.flop_per_image(a, R, max(L, 1))
        path_tflops = value * flop_img / 1e12 / world           # per GPU
        kernels, roofline = roofline_from_profile(prof, args.workload + ("_bn" if args.use_bn else ""), B, R, path_tflops, tuning_id)
        # wall time of the ONE untimed step that carried the stream markers: its kernels' durations (consecutive launches share
        # a marker) add up to it; it is longer than a timed step by what ~8 markers per GD iteration cost (~3 us each)
        roofline["profiled_step_ms"] = round(profiled_step_ms, 3) if profiled_step_ms is not None else None
        # Row groups (dg_call_row_groups; CelebA's default is 2): the timed region runs them on separate streams, where their
        # kernels OVERLAP -- a launch's duration there is not its rate.  The marked step runs the SAME launches (row counts, job
        # lists) one after the other on one stream: `avg_launch_us`, `flop_per_launch` and `traffic` are per launch of ONE group,
        # `frac` is the kernel alone on the chip; `path_frac` is the timed region's wall clock.
        row_groups = gan.row_groups(B)
        roofline["row_groups"] = row_groups
        roofline["launches"] = ("as in the timed region" if row_groups == 1 else
                                "the timed region's launches (%d row groups of %d rows each), run one at a time in the marked step; "
                                "in the timed region the groups' kernels overlap on %d streams" % (row_groups, B * R // row_groups, row_groups))
        cfgno = 4 if args.strong else {"mnist": 1, "fmnist": 2, "celeba": 3}[args.workload]
        if args.strong:
            wl = ("%s whitebox FGSM eps=0.3 (classifier model A, dg_fgsm) evaluation of %d images, L=%d R=%d, projection batch %d, classifier model A "
                  "(BASELINE configs[4]); images sharded contiguously over %d rank(s), one all_gather of (labels, preds, "
                  "diffs)" % (arch, args.images, L, R, B, world))
        else:
            wl = ("%s L=%d R=%d batch=%d fp32 (BASELINE configs[%d]%s); synthetic tflib-init weights gain %.1f, "
                  "x = clip(G(z)+0.3*sign(n))" % (arch, L, R, B, cfgno, " with USE_BN: True" if args.use_bn else "", gain))
        res = {
            "metric": "projected images/sec at L=%d,R=%d (%s)" % (L, R, "MNIST 28x28" if a.arch_id == 0 else "CelebA 64x64"),
            "value": round(value, 3), "unit": "images/s", "n_gpus": 1 if COLL_BACKEND == "gloo" else world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "strong" if args.strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": wl, "batch_per_gpu": B, "rec_rr": R, "rec_iters": L, "rec_lr": 10.0,
                       "parallelism": "shard%d" % world, "row_groups": row_groups},
            "io": "host (pageable NumPy in, NumPy out: PCIe-inclusive)" if args.host_io else "resident in HBM",
            "build": build_id(),
            # which job lists ran (a timed choice per layer and row count; identical ids = identical lists on every rank)
            "tuning_id": tuning_id, "tuning_id_per_rank": rank_tuning, "tuning_source": tuning_source, "prepare_ms": round(prepare_ms, 1),
            "ranks": dist.get_world_size() if distributed else 1,     # ranks the process group (RCCL) actually holds
            "ms_per_step_per_rank": [round(v, 3) for v in per_rank_ms],
            "biggest_layer_us_per_rank": big_layer_us,     # duration ratio between ranks = ratio of their GEMM clocks
            "host_cpus_rank0": pinned,        # the CPUs rank 0's host thread is pinned to (multi-rank runs; None = not pinned)
            "roofline": roofline,
            "kernels": kernels,
        }
        if args.strong:
            res["accuracy"] = round(float(result["acc"]), 4)
            res["mean_diff"] = round(float(result["roc"][2].mean()), 6)
        else:
            loss = torch.as_tensor(out["loss"]).view(B, R).min(dim=1).values        # NumPy with --host-io
            res["mean_best_loss"] = round(float(loss.mean().item()), 6)
        if args.full and world == 1 and not args.no_cpu_baseline and not args.use_bn:
            res["cpu_baseline"] = cpu_baseline(arch, params, x[:64].cpu().numpy(), R, L)
        print(json.dumps(res), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    gan.close()


if __name__ == "__main__":
    main()
