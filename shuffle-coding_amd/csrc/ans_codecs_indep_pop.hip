// Independent<Categorical> resume pops (ans_dev_independent_pop) on the fast decoder (ans_mfast.hpp
// k_mdec<kRes> with IndepModel): the instantiations of ans_codecs_indep_dec.hip again, on the
// message in each slot, in place.
#include "ans_mfast_launch.hpp"

namespace shuffle_coding {
namespace mfast {
namespace {

template <int NR, int kL, bool kLean>
void dec_m(const IndepFast& f, uint8_t* in, uint64_t cap, uint32_t* lens, const uint8_t* tids, uint64_t L,
           uint64_t nfull, void* out, int w, uint32_t* st, hipStream_t s) {
    using M = IndepModel<false, NR, DecLayout<kL>::kTab, kLean>;
    const bool wide = kL == kLanesW;
    const M m{f.md.enc_img, wide ? f.dec_img_w : f.md.dec_img, f.md.nsym, f.md.enc_bytes,
              wide ? f.dec_bytes_w : f.md.dec_bytes, f.md.k_off, f.md.ro, f.md.no, f.md.so};
    const uint32_t lds = wide ? kLdsMax : kDecTab + m.dec_bytes;
    if (w == 1 && f.kmax * 16 <= 60) mdec<M, uint8_t, 16, kL, true>(m, in, cap, nullptr, lens, tids, L, nfull, ANS_GEN_EMPTY, out, st, ChunkInit{}, lds, s);
    else if (w == 1) mdec<M, uint8_t, 8, kL, true>(m, in, cap, nullptr, lens, tids, L, nfull, ANS_GEN_EMPTY, out, st, ChunkInit{}, lds, s);
    else if (w == 2) mdec<M, uint16_t, 8, kL, true>(m, in, cap, nullptr, lens, tids, L, nfull, ANS_GEN_EMPTY, out, st, ChunkInit{}, lds, s);
    else mdec<M, uint32_t, 4, kL, true>(m, in, cap, nullptr, lens, tids, L, nfull, ANS_GEN_EMPTY, out, st, ChunkInit{}, lds, s);
}
template <int NR, int kL>
void dec_l(const IndepFast& f, uint8_t* in, uint64_t cap, uint32_t* lens, const uint8_t* tids, uint64_t L,
           uint64_t nfull, void* out, int w, uint32_t* st, hipStream_t s) {
    if (kL == kLanesW ? f.lean_w : f.lean)
        dec_m<NR, kL, true>(f, in, cap, lens, tids, L, nfull, out, w, st, s);
    else
        dec_m<NR, kL, false>(f, in, cap, lens, tids, L, nfull, out, w, st, s);
}
// the 1,024-lane layout when the set has its image and the call the chains for one such
// workgroup per CU (four waves per SIMD); below that, 256-lane workgroups spread over more CUs
template <int NR>
void dec_w(const IndepFast& f, uint8_t* in, uint64_t cap, uint32_t* lens, const uint8_t* tids, uint64_t L,
           uint64_t nfull, void* out, int w, uint32_t* st, hipStream_t s) {
    if (f.dec_img_w && f.wide(nfull))
        dec_l<NR, kLanesW>(f, in, cap, lens, tids, L, nfull, out, w, st, s);
    else
        dec_l<NR, kLanes>(f, in, cap, lens, tids, L, nfull, out, w, st, s);
}

}  // namespace

void indep_fast_pop(const IndepFast& f, uint8_t* in, uint64_t cap, uint32_t* lens, const uint8_t* tids, uint64_t L,
                    uint64_t nfull, void* out, int w, uint32_t* st, hipStream_t s) {
    if (f.nr == fast::kNormSmall) dec_w<fast::kNormSmall>(f, in, cap, lens, tids, L, nfull, out, w, st, s);
    else if (f.nr == fast::kNormBig) dec_w<fast::kNormBig>(f, in, cap, lens, tids, L, nfull, out, w, st, s);
    else dec_w<fast::kNormStd>(f, in, cap, lens, tids, L, nfull, out, w, st, s);
}

}  // namespace mfast
}  // namespace shuffle_coding
