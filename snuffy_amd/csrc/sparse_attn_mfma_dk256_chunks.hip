// K7 (fast form, bf16) at head width 256, second translation unit: the statistics pass (MODE 1) and the main pass (MODE 2) of a
// key-chunked launch at 2 and 4 key blocks, single bag and varlen (see sparse_attn_mfma_dk256_impl.h).
#include "sparse_attn_mfma_dk256_impl.h"

namespace {
template <int NB, bool VL>
int a256_chunk_modes(int mode, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    if (mode == 1) return a256_launch<NB, false, 1, VL>(P, pl, out, s);
    return aux ? a256_launch<NB, true, 2, VL>(P, pl, out, s) : a256_launch<NB, false, 2, VL>(P, pl, out, s);
}
}  // namespace

namespace snf {
int attn_dk256_launch_chunk(int mode, const snf_attn::AttnParams& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s) {
    const bool vl = P.vl != nullptr;
    switch (pl.nkb) {
        case 2: return vl ? a256_chunk_modes<2, true>(mode, P, pl, out, s) : a256_chunk_modes<2, false>(mode, P, pl, out, s);
        case 4: return vl ? a256_chunk_modes<4, true>(mode, P, pl, out, s) : a256_chunk_modes<4, false>(mode, P, pl, out, s);
        default: break;
    }
    set_error("sparse_attn_mfma_dk256 (key chunks): key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}
}  // namespace snf
