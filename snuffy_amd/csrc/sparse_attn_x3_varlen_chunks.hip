// K7 (fp32-class form), second translation unit: the key-chunked varlen variants (many bags per launch, k above one LDS image; see
// sparse_attn_x3_impl.h).
#include "sparse_attn_x3_impl.h"

namespace snf {
int x3_launch_varlen_chunk(int dk, int mode, const snf_attn::X3Params& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s) {
    return dk == 128 ? x3_dispatch_varlen_chunk<128>(P, pl, out, s, mode) : x3_dispatch_varlen_chunk<64>(P, pl, out, s, mode);
}
}  // namespace snf
