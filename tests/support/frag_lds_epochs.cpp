// TEST SUPPORT (never linked into the product library): which LDS bytes every wave of a dg_fgemm.hip workgroup reads and writes,
// grouped by BARRIER EPOCH, with the offsets and sizes taken from dg_frag_lds.h (the header the kernel itself uses).
//
// The epoch table below is a HAND TRANSCRIPTION of the barriers of frag_body (defensegan_amd/csrc/dg_fgemm.hip); a change to
// the kernel's barriers or to what stands between them belongs here too.  Epoch e of a wave = what it does after its e-th
// __syncthreads() and before its next one; what a wave does after its LAST barrier is its final epoch, which nothing orders
// against anything another wave does from that epoch on.  Lines mirrored (all tiles of the job taken as active, the case with
// the most accesses):
//   ks = 1 (also every tile of fgemm_persist_kernel): no barrier (line 75 and the `if (ks > 1)` of line 207); epilogue slice
//          written (275) and read back (292) by every wave -- epoch 0, final.
//   ks = 2: K part 1 (waves 1, 3) puts its tile's image (210) | barrier (211) | part 1 returns (212); part 0 (waves 0, 2) adds its
//          tile's image (213), then writes and reads its slice (275, 292) -- epoch 1, final.
//   ks = 4: parts 1, 3 put images 0, 1 (210) | barrier (211) | parts 1, 3 return; parts 0, 2 add images 0, 1 (213) | barrier
//          (216) | part 2 puts the round-2 image (217) | barrier (218) | part 2 returns (219); part 0 adds the round-2 image
//          (220), then its slice (275, 292) -- epoch 3, final.
// With fragment-order output (OUTFRAG) the epilogue stores from registers and touches no slice (lines 266-272).
#include "dg_frag_lds.h"

namespace {

struct Rec { int wave, epoch, last_epoch, write, begin, end; };

// slice_rule 0: dg_frag_lds.h slice_off; 1: the rule the kernel had before (slice = wave * 32 * pitch), kept here so that the test
// can show it finds that rule's overlap
int slice_of(int rule, int ks, int wave, int tw, int tn) {
    return rule == 1 ? wave * dg::frag_lds::slice_bytes(tw) : dg::frag_lds::slice_off(ks, wave, tw, tn);
}

}  // namespace

extern "C" {

// out: records of 6 ints (wave, epoch, the wave's last epoch, 1 = write / 0 = read, first byte, one past the last byte);
// returns the number of records, or -1 when `cap` records do not hold them / the arguments are not a layout of the kernel.
int dgf_intervals(int ks, int out_frag, int slice_rule, int tw, int tn, int* out, int cap) {
    namespace L = dg::frag_lds;
    if (ks != 1 && ks != 2 && ks != 4) return -1;
    int n = 0;
    bool full = false;
    auto emit = [&](int wave, int epoch, int last, int write, int begin, int bytes) {
        if (n >= cap) { full = true; return; }
        const Rec r = {wave, epoch, last, write, begin, begin + bytes};
        int* o = out + 6 * n++;
        o[0] = r.wave; o[1] = r.epoch; o[2] = r.last_epoch; o[3] = r.write; o[4] = r.begin; o[5] = r.end;
    };
    const int img = L::img_bytes(tw, tn), sl = L::slice_bytes(tw);
    for (int w = 0; w < L::WAVES; ++w) {
        const int q = L::kpart_of(ks, w), tile = L::tile_of(ks, w);
        // barriers this wave passes before it ends
        const int last = ks == 1 ? 0 : (ks == 2 ? 1 : ((q & 1) ? 1 : 3));
        if (ks > 1) {
            const int i1 = L::image_off(ks, q, tile, tw, tn);
            if (q & 1) emit(w, 0, last, 1, i1, img);              // put(img1)
            else emit(w, 1, last, 0, i1, img);                    // add(img1)
            if (ks == 4 && q == 2) emit(w, 2, last, 1, L::image2_off(), img);      // put(img2)
            if (ks == 4 && q == 0) emit(w, 3, last, 0, L::image2_off(), img);      // add(img2)
        }
        if (q == 0 && !out_frag) {                                // the epilogue's transposition, in the wave's final epoch
            emit(w, last, last, 1, slice_of(slice_rule, ks, w, tw, tn), sl);
            emit(w, last, last, 0, slice_of(slice_rule, ks, w, tw, tn), sl);
        }
    }
    return full ? -1 : n;
}

int dgf_launch_bytes(int tw, int tn) { return dg::frag_lds::launch_bytes(tw, tn); }
int dgf_fits(int tw, int tn) { return dg::frag_lds::fits(tw, tn) ? 1 : 0; }

}  // extern "C"
