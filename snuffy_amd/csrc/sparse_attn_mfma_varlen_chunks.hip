// K7 (fast form), translation unit 6: the key-chunked varlen variants (many bags per launch, k above one LDS image), dk = 128
// (see sparse_attn_mfma_impl.h).
#include "sparse_attn_mfma_impl.h"

namespace snf {
int attn_launch_varlen_chunk_dk128(bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    return launch_nkb_varlen_chunk<128>(stats_pass, P, pl, out, s);
}
}  // namespace snf
