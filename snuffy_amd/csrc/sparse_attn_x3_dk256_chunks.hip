// K7 (fp32-class form) at head width 256, second translation unit: the statistics pass (MODE 1) and the main pass (MODE 2) of a
// key-chunked launch at 2 and 4 key blocks, single bag and varlen (see sparse_attn_x3_dk256_impl.h).
#include "sparse_attn_x3_dk256_impl.h"

namespace {
template <int NB, bool VL>
int x3y_chunk_modes(int mode, const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    if (mode == 1) return x3y_launch<NB, false, 1, VL>(P, pl, out, s);
    return aux ? x3y_launch<NB, true, 2, VL>(P, pl, out, s) : x3y_launch<NB, false, 2, VL>(P, pl, out, s);
}
}  // namespace

namespace snf {
int x3_dk256_launch_chunk(int mode, const snf_attn::X3Params& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s) {
    const bool vl = P.vl != nullptr;
    switch (pl.nkb) {
        case 2: return vl ? x3y_chunk_modes<2, true>(mode, P, pl, out, s) : x3y_chunk_modes<2, false>(mode, P, pl, out, s);
        case 4: return vl ? x3y_chunk_modes<4, true>(mode, P, pl, out, s) : x3y_chunk_modes<4, false>(mode, P, pl, out, s);
        default: break;
    }
    set_error("sparse_attn_x3_dk256 (key chunks): key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}
}  // namespace snf
