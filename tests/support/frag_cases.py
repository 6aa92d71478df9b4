"""The case table of tests/test_gpu_frag_values.py and what the planner makes of it, restated in Python so that the GPU test needs
no host build: which forward layers run on dg_fgemm.hip, the K split of every tap class (dg_plan.cpp frag_ksplit) and the output
form of every layer.  tests/test_frag_lds_cpu.py holds these restatements against dg_plan.cpp itself (build_frag_jobs,
frag_supported) and asserts that the table reaches every (K split, output form) pair a supported generator can reach."""
from tests.support import path_reference as PR

# (arch, NET_DIM, rows): the shapes of the value checks, each run with frag_path = 1 and 2.
#   1, 33, 47   a padded last 32-row block; a partial last tile (rows-blocks x positions is no multiple of 4 M blocks); two row blocks
#   129         5 row blocks: per class 5 x positions M blocks, so the last job of a class holds fewer than its 4, 8 or 16
CASES = [("mnist", 64, r) for r in (1, 33, 47, 129)] + [("celeba", 64, r) for r in (1, 33, 47)]
FALLBACK = ("mnist", 128, 33)            # first deconv K = 512: not addressable, the engine keeps dg_gemm.hip
NET_DIMS = (32, 64, 128)                 # the widths looked at for "reachable"

TN = 4                                   # M blocks per wave tile (dg_fgemm.hip launch_mo)


def gemm_layers(arch, net_dim):
    """Per forward layer d = 1 .. n_act - 1 (the Deconv2D that writes act<d>): (h_in, h_used, cin, cout)."""
    chans = {"mnist": [4, 2, 1], "celeba": [4, 2, 1, 1]}[arch]
    layers = PR.O._arch_layers(arch)
    return [(layers[d - 1][1], layers[d - 1][2], chans[d - 1] * net_dim, chans[d] * net_dim) for d in range(1, PR.n_act(arch))]


def ksplit_of(taps, cin):
    """dg_plan.cpp frag_ksplit: the class's K chunks of 32 decide, capped so that a wave's part is whole turns of the 4-deep ring."""
    nchunks = taps * cin // 32
    ks = 4 if nchunks >= 40 else (2 if nchunks >= 20 else 1)
    while ks > 1 and ks > (cin // 8) // 4:
        ks >>= 1
    return ks


def layer_supported(cin, cout):
    """dg_plan.cpp frag_supported for these generators (offsets and row strides are multiples of 32 whenever cout % 64 == 0)."""
    return cin in (64, 128, 256) and cout % 64 == 0


def generator_supported(arch, net_dim):
    """dg_engine.cpp frag_shapes_ok: every forward GEMM layer qualifies (and the Linear output is whole 128-feature tiles)."""
    return all(layer_supported(cin, cout) for _, _, cin, cout in gemm_layers(arch, net_dim)) and (16 * 4 * net_dim) % 128 == 0


def class_ksplits(arch, net_dim, d):
    """K split of every tap class of forward layer d under frag_path = 1, in path_reference.tap_class_masks order."""
    cin = gemm_layers(arch, net_dim)[d - 1][2]
    return [ksplit_of(c["taps"], cin) for c in PR.tap_class_masks(arch, d, "fwd")[1]]


def pairs(arch, net_dim):
    """The (K split, output form) pairs frag_path = 1 runs on this generator; empty when it falls back."""
    if not generator_supported(arch, net_dim):
        return set()
    nd = PR.n_act(arch)
    return {(ks, "nhwc" if d == nd - 1 else "frag") for d in range(1, nd) for ks in class_ksplits(arch, net_dim, d)}


ALL_PAIRS = {(ks, form) for ks in (1, 2, 4) for form in ("frag", "nhwc")}
# No supported generator reaches this one: NHWC output belongs to the last GEMM layer, whose K split is 4 only from 40 chunks up --
# more than 9 taps at K = 128, or K = 256, which the last GEMM layer has only at NET_DIM 128 (MNIST: 256; CelebA: 128), where the
# first deconv has K = 512 and the whole path falls back.
UNREACHED = {(4, "nhwc")}
