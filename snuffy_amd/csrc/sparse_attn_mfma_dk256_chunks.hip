// K7 (fast form, bf16) at head width 256, second translation unit: the statistics pass (MODE 1) and the main pass (MODE 2) of a
// key-chunked launch at 2 and 4 key blocks, single bag and varlen (see sparse_attn_mfma_dk256_impl.h; the switch is in attn_width.h).
#include "sparse_attn_mfma_dk256_impl.h"

namespace snf {
int attn_dk256_launch_chunk(int mode, const snf_attn::AttnParams& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s) {
    return snf_attn::width_launch_chunk<A256>(mode, P, pl, out, s);
}
}  // namespace snf
