// ans_codecs_indep_impl.hpp — the dispatch of Independent<Categorical> (src/codec.rs:366-403) onto
// the fast kernels (ans_mfast.hpp k_menc / k_mdec with IndepModel): norm range, renorm screen
// (encoder) or lean model (decoder), lane layout, symbol width.  kRes: the resume forms
// (ans_dev_independent_push / _pop), the same instantiations starting from the message in each
// slot.  Included only by ans_codecs_indep_{enc,push,dec,pop}.hip, one side and one kRes each.
#pragma once

#include "ans_mfast_launch.hpp"

namespace shuffle_coding {
namespace mfast {
namespace {

template <bool kRes, bool R, int NR, int kL>
void enc_l(const IndepFast& f, const EncArgs& a) {
    using M = IndepModel<R, NR, kDecTab, false, EncLayout<kL>::kTab>;
    const M m{f.md.enc_img, f.md.dec_img, f.md.nsym, f.md.enc_bytes, f.md.dec_bytes, f.md.k_off, f.md.ro, f.md.no, f.md.so};
    const uint32_t lds = kL == kLanesW ? kLdsMax : kEncTab + m.enc_bytes;
    auto go = [&](auto sym, auto spp) { menc_of<M, kL, kRes>(m, a, lds, sym, spp); };
    // a point per 16 u8 symbols needs at most 4 bytes each (64 between points), else per 8
    if (a.w == 1 && f.kmax * 16 <= 60) go(uint8_t{}, Spp<16>{});
    else if (a.w == 1) go(uint8_t{}, Spp<8>{});
    else if (a.w == 2) go(uint16_t{}, Spp<8>{});
    else go(uint32_t{}, Spp<4>{});
}
// the 1,024-lane layout (one shared table image, four waves per SIMD) when the set's image fits
// it and the call has the chains for one such workgroup per CU
template <bool kRes, bool R, int NR>
void enc_w(const IndepFast& f, const EncArgs& a) {
    if (f.enc_wide && f.wide(a.nfull)) enc_l<kRes, R, NR, kLanesW>(f, a);
    else enc_l<kRes, R, NR, kLanes>(f, a);
}
template <bool kRes, int NR>
void enc_nr(const IndepFast& f, const EncArgs& a) {
    if (f.rare) enc_w<kRes, true, NR>(f, a);
    else enc_w<kRes, false, NR>(f, a);
}
template <bool kRes>
void indep_enc(const IndepFast& f, const EncArgs& a) {
    if (f.nr == fast::kNormSmall) enc_nr<kRes, fast::kNormSmall>(f, a);
    else if (f.nr == fast::kNormBig) enc_nr<kRes, fast::kNormBig>(f, a);
    else enc_nr<kRes, fast::kNormStd>(f, a);
}

// (The decoder's renorm handles the bidirectional cases whatever the set: no screen variant.)
template <bool kRes, int NR, int kL, bool kLean>
void dec_m(const IndepFast& f, const DecArgs& a) {
    using M = IndepModel<false, NR, DecLayout<kL>::kTab, kLean>;
    const bool wide = kL == kLanesW;
    const M m{f.md.enc_img, wide ? f.dec_img_w : f.md.dec_img, f.md.nsym, f.md.enc_bytes,
              wide ? f.dec_bytes_w : f.md.dec_bytes, f.md.k_off, f.md.ro, f.md.no, f.md.so};
    const uint32_t lds = wide ? kLdsMax : kDecTab + m.dec_bytes;
    auto go = [&](auto sym, auto spp) { mdec_of<M, kL, kRes>(m, a, lds, sym, spp); };
    if (a.w == 1 && f.kmax * 16 <= 60) go(uint8_t{}, Spp<16>{});  // as the encoder's points
    else if (a.w == 1) go(uint8_t{}, Spp<8>{});
    else if (a.w == 2) go(uint16_t{}, Spp<8>{});
    else go(uint32_t{}, Spp<4>{});
}
template <bool kRes, int NR, int kL>
void dec_l(const IndepFast& f, const DecArgs& a) {
    if (kL == kLanesW ? f.lean_w : f.lean) dec_m<kRes, NR, kL, true>(f, a);
    else dec_m<kRes, NR, kL, false>(f, a);
}
// the 1,024-lane layout when the set has its image and the call the chains for one such
// workgroup per CU (four waves per SIMD); below that, 256-lane workgroups spread over more CUs
template <bool kRes, int NR>
void dec_w(const IndepFast& f, const DecArgs& a) {
    if (f.dec_img_w && f.wide(a.nfull)) dec_l<kRes, NR, kLanesW>(f, a);
    else dec_l<kRes, NR, kLanes>(f, a);
}
template <bool kRes>
void indep_dec(const IndepFast& f, const DecArgs& a) {
    if (f.nr == fast::kNormSmall) dec_w<kRes, fast::kNormSmall>(f, a);
    else if (f.nr == fast::kNormBig) dec_w<kRes, fast::kNormBig>(f, a);
    else dec_w<kRes, fast::kNormStd>(f, a);
}

}  // namespace
}  // namespace mfast
}  // namespace shuffle_coding
