// K7 (fp32-class form) at head width 192, second translation unit: the statistics pass (MODE 1) and the main pass (MODE 2) of a
// key-chunked launch at 2 and 4 key blocks, single bag and varlen (see sparse_attn_x3_dk192_impl.h; the switch is in attn_width.h).
#include "sparse_attn_x3_dk192_impl.h"

namespace snf {
int x3_dk192_launch_chunk(int mode, const snf_attn::X3Params& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s) {
    return snf_attn::width_launch_chunk<X3W>(mode, P, pl, out, s);
}
}  // namespace snf
