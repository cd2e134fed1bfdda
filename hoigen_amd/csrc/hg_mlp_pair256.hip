// The MLP of a transformer block as one persistent launch with c_proj on 256 x 256 TILES (gfx950).  hg_mlp_pair.hip describes the launch
// and its hand-off - c_fc tiles publish per 256-row panel of `fc`, c_proj tiles wait for their panel, producers and consumers of a
// panel on one XCD by HW_REG_XCC_ID and the census - and all of that holds here unchanged.  What differs:
//
//   * c_proj runs the 256 x 256 ring body (hg_gemm_ring_body.h, four phases, EPI_RESID_LN_F32 with the residual stream as fp32 or as
//     centre + hi + lo) instead of ring2's 128 x 256 body.  On the global -> LDS path, which bounds both K loops, the bigger tile moves
//     7.6 KB per MFLOP instead of 11.4.  A row leaves with the bits ring2 gives it: same K order, same MFMA, the same epilogue
//     expressions, the same partial statistics per 64 columns; lo is read and written in ring2's tile order - a 256-row tile is ring2's
//     tiles (2 k, n) and (2 k + 1, n) -, so out_proj, which stays on ring2, consumes it as before.
//   * A c_proj tile is a whole panel high, so its wait is simple: wave 0 polls ready[panel] in front of the tile (bounded, *err as in
//     hg_mlp_pair.hip: never a hang), a barrier publishes the answer, then the body runs that ONE tile - prologue, 48 K-tiles,
//     epilogue.  The operand ring therefore never reaches into a panel that is not complete; the price is one refill of the ring per
//     tile (~2 % of a tile).
//   * The slots of an XCD share its tiles by WORK (hg_mlp_pair_deal.h): a c_proj tile weighs `ratio` c_fc tiles (option mlp_pair256_ratio), the slots
//     that own one c_proj tile more own that many c_fc tiles fewer, reach c_proj first and take the XCD's earliest panels.  Every slot
//     runs all of its c_fc tiles before any of its c_proj tiles, so resident workgroups always progress.
//
// The text tower's form (gamma in the activation copy) has no instance here: it stays on hg_mlp_pair.hip.
#include "hg_mlp_pair256_dev.h"

namespace hg {

// (the schedules, the arguments and the kernel's code: hg_mlp_pair256_dev.h, shared with the two-phase form in hg_mlp_pair256p.hip)
template <int HL>
__global__ __launch_bounds__(512, 2) void mlp_pair256_kernel(const Pair256Args P_in) {
    mlp_pair256_run<HL, false>(P_in);
}

// what hg_mlp_pair.hip's launch takes, without the text tower's gamma form and from min_m rows on (hg_tower.hip: option mlp_pair256_min_m)
bool mlp_pair256_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu, int min_m) {
    if (!mlp_pair_shapes_ok(fc, proj, n_cu) || proj.gamma) return false;
    if (fc.M < min_m) return false;
    // c_proj's A and lo through 32-bit offsets of whole 256-row tiles
    if ((size_t)((proj.M + 255) / 256) * 256 * proj.lda * 2 >= (1ull << 31)) return false;
    return proj.hl == 0 || proj.hl == 2 || proj.hl == 3;
}

static hipError_t launch_pair256_hl(const Pair256Args& a, int hl, int grid, int lds, hipStream_t s) {
    switch (hl) {
        case 0: return mlp_launch_instance<mlp_pair256_kernel<0>>(a, grid, lds, s);
        case 2: return mlp_launch_instance<mlp_pair256_kernel<2>>(a, grid, lds, s);
        case 3: return mlp_launch_instance<mlp_pair256_kernel<3>>(a, grid, lds, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_mlp_pair256(const GemmArgs& fc, const GemmArgs& proj, unsigned* ready, int* err, int ch, int ratio, int n_cu,
                              hipStream_t s, int grid_short) {
    return mlp_pair256_launch("pair256", fc, proj, ready, err, ch, ratio, n_cu, s, grid_short, launch_pair256_hl);
}

}  // namespace hg
