// The MLP pair launch with c_proj on 256 x 256 tiles (hg_mlp_pair256.hip describes it) with c_proj's K loop in the two-phase form c_fc
// already runs: 32 MFMAs per segment, two barrier pairs per K-tile instead of four, every K-tile instantiated by its position in the
// tile - first, middle, second to last, last - so that the middle of the loop holds no comparison and no branch but its back edge.  A
// c_proj call of the body is one tile (Pair256ProjSched), so no tile follows inside it and no stores are pending at its start: only the
// last K-tile carries the residual prefetch, and the waits of the last two count exactly what is behind them (hg_gemm_ring_body.h: ONE).
// That loop's fragments are read into fixed register tuples (ds_read_fixed there), so every MFMA operand tuple starts at a multiple of 4.
// Same arguments, dealing, census, bounded wait, hand-off and bits as mlp_pair256_kernel; option mlp_pair256_ph2 chooses between them.
#include "hg_mlp_pair256_dev.h"

namespace hg {

template <int HL>
__global__ __launch_bounds__(512, 2) void mlp_pair256p_kernel(const Pair256Args P_in) {
    mlp_pair256_run<HL, true>(P_in);
}

static hipError_t launch_pair256p_hl(const Pair256Args& a, int hl, int grid, int lds, hipStream_t s) {
    switch (hl) {
        case 0: return mlp_launch_instance<mlp_pair256p_kernel<0>>(a, grid, lds, s);
        case 2: return mlp_launch_instance<mlp_pair256p_kernel<2>>(a, grid, lds, s);
        case 3: return mlp_launch_instance<mlp_pair256p_kernel<3>>(a, grid, lds, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_mlp_pair256p(const GemmArgs& fc, const GemmArgs& proj, unsigned* ready, int* err, int ch, int ratio, int n_cu,
                               hipStream_t s, int grid_short) {
    return mlp_pair256_launch("pair256p", fc, proj, ready, err, ch, ratio, n_cu, s, grid_short, launch_pair256p_hl);
}

}  // namespace hg
