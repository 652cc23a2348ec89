// K7 (fast form), translation unit 3: the dk = 192 kernel variants (see sparse_attn_mfma_impl.h).
#include "sparse_attn_mfma_impl.h"

namespace snf {
int attn_launch_dk192(int qv_dtype, bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    if (stats_pass)
        return qv_dtype == SNF_DT_F32 ? launch_stats<192, float>(P, pl, s) : launch_stats<192, unsigned short>(P, pl, s);
    return qv_dtype == SNF_DT_F32 ? launch_nkb<192, float>(P, pl, out, s) : launch_nkb<192, unsigned short>(P, pl, out, s);
}
}  // namespace snf
