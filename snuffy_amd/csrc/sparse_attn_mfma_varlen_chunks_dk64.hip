// K7 (fast form), translation unit 7: the key-chunked varlen variants (many bags per launch, k above one LDS image), dk = 64
// (see sparse_attn_mfma_impl.h).
#include "sparse_attn_mfma_impl.h"

namespace snf {
int attn_launch_varlen_chunk_dk64(bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    return launch_nkb_varlen_chunk<64>(stats_pass, P, pl, out, s);
}
}  // namespace snf
