// LDS layout of the fragment-order GEMM (dg_fgemm.hip), as constexpr host / device functions: the kernel and its launch use
// them, and tests/support/frag_lds_epochs.cpp lists from them the bytes every wave touches between two barriers
// (tests/test_frag_lds_cpu.py: no two waves that no barrier orders may share a byte unless both only read it).
//
// A workgroup = 4 waves; a job splits the K axis of a wave tile over ks = 1, 2 or 4 of them:
//   ks = 1   wave w owns tile w, K part 0          no image; epilogue slice of wave w
//   ks = 2   wave w owns tile w / 2, K part w % 2  part 1 hands its accumulators to part 0 through the tile's IMAGE
//   ks = 4   one tile, wave w = K part w           round 1: part 1 -> 0 through image 0, part 3 -> 2 through image 1;
//                                                  round 2: part 2 -> 0 through image 0
// The wave holding K part 0 runs the epilogue; with NHWC output it transposes every 32-row block through its SLICE.  The rule
// for the slice: every byte a wave touches after its last barrier belongs to that wave alone.  For ks = 2 the two epilogue
// waves (0 and 2) leave the only barrier at different times, so the slice of each lies inside its tile's own image, which
// that wave alone reads and has finished reading (a wave's LDS accesses execute in program order).
#pragma once

#ifdef __HIPCC__
#define DG_LDS_FN __host__ __device__ constexpr
#else
#define DG_LDS_FN constexpr
#endif

namespace dg {
namespace frag_lds {

constexpr int WAVES = 4;

// accumulator image of one wave tile: [tw][tn][4 quads][64 lanes][4 floats]
DG_LDS_FN int img_bytes(int tw, int tn) { return tw * tn * 16 * 256; }
// epilogue slice: 32 rows of tw * 32 floats, row pitch + 16 B (the 16 lanes of a b128 write pass hit 16 different bank quads)
DG_LDS_FN int slice_pitch(int tw) { return 32 * tw * 4 + 16; }
DG_LDS_FN int slice_bytes(int tw) { return 32 * slice_pitch(tw); }
// dynamic LDS of a launch: two images
DG_LDS_FN int launch_bytes(int tw, int tn) { return 2 * img_bytes(tw, tn); }

DG_LDS_FN int tile_of(int ks, int wave) { return ks == 4 ? 0 : (ks == 2 ? wave >> 1 : wave); }
DG_LDS_FN int kpart_of(int ks, int wave) { return wave & (ks - 1); }

// byte offset of the image through which K part q (odd) of `tile` meets part q - 1 in round 1 (ks = 2, 4)
DG_LDS_FN int image_off(int ks, int q, int tile, int tw, int tn) { return (ks == 4 ? (q >> 1) : tile) * img_bytes(tw, tn); }
// ... and of the image through which part 2 meets part 0 in round 2 (ks = 4)
DG_LDS_FN int image2_off() { return 0; }
// byte offset of the epilogue slice of `wave` (the persistent kernel: ks = 1)
DG_LDS_FN int slice_off(int ks, int wave, int tw, int tn) { return ks == 2 ? tile_of(2, wave) * img_bytes(tw, tn) : wave * slice_bytes(tw); }

// everything inside the launch size, every ks = 2 slice inside its own tile's image
DG_LDS_FN bool fits(int tw, int tn) {
    bool ok = slice_bytes(tw) <= img_bytes(tw, tn) && image2_off() + img_bytes(tw, tn) <= launch_bytes(tw, tn);
    for (int ks = 1; ks <= 4; ks *= 2)
        for (int w = 0; w < WAVES; ++w) {
            ok = ok && slice_off(ks, w, tw, tn) >= 0 && slice_off(ks, w, tw, tn) + slice_bytes(tw) <= launch_bytes(tw, tn);
            if (ks > 1) {
                const int io = image_off(ks, kpart_of(ks, w), tile_of(ks, w), tw, tn);
                ok = ok && io >= 0 && io + img_bytes(tw, tn) <= launch_bytes(tw, tn);
                if (ks == 2) ok = ok && slice_off(2, w, tw, tn) >= io && slice_off(2, w, tw, tn) + slice_bytes(tw) <= io + img_bytes(tw, tn);
            }
        }
    return ok;
}

}  // namespace frag_lds
}  // namespace dg
