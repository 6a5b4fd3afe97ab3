// ans_mfast_launch.hpp — launchers of the ans_mfast.hpp skeletons, shared by ans_codecs.hip
// (Uniform, LogUniform) and the four Independent<Categorical> units
// ans_codecs_indep_{enc,push,dec,pop}.hip.  Those hold that codec's many instantiations (norm
// range x renorm screen x lane layout x symbol width, for new and for resumed messages) so they
// compile in parallel; their one dispatch ladder per side is ans_codecs_indep_impl.hpp.
#pragma once

#include <type_traits>

#include "ans_launchlog.hpp"
#include "ans_mfast.hpp"

namespace shuffle_coding {
namespace mfast {

template <class M, typename Sym, int SPP, int kL = kLanes, bool kRes = false>
void menc(const M& md, const void* syms, const uint8_t* tids, uint64_t L, uint64_t nfull, uint8_t* slots, uint64_t cap,
          uint32_t* lens, uint32_t* st, ChunkInit ini, uint32_t lds, hipStream_t s) {
    k_menc<M, Sym, SPP, kL, kRes><<<static_cast<unsigned>((nfull + kL - 1) / kL), kL, lds, s>>>(
        md, static_cast<const Sym*>(syms), tids, L, nfull, slots, cap, lens, st, ini);
}
template <class M, typename Sym, int SPP, int kL = kLanes, bool kRes = false>
void mdec(const M& md, const uint8_t* in, uint64_t cap, const uint64_t* offs, const uint32_t* lens, const uint8_t* tids,
          uint64_t L, uint64_t nfull, int gen_kind, void* out, uint32_t* st, ChunkInit ini, uint32_t lds, hipStream_t s) {
    k_mdec<M, Sym, SPP, kL, kRes><<<static_cast<unsigned>((nfull + kL - 1) / kL), kL, lds, s>>>(
        md, in, cap, offs, lens, tids, L, nfull, gen_kind, static_cast<Sym*>(out), st, ini);
}

// What a call hands through its dispatch to the launch, where it is unpacked into menc's / mdec's
// parameters: nfull chunks of L symbols of w bytes (tids: a table id per position, Independent only).
struct EncArgs {
    const void* syms;
    int w;
    const uint8_t* tids;
    uint64_t L, nfull;
    uint8_t* slots;
    uint64_t cap;
    uint32_t* lens;
    uint32_t* st;
    ChunkInit ini;
    hipStream_t s;
    LaunchLog* log = nullptr;  // the context's launch record (Independent calls), or NULL
};
struct DecArgs {
    const uint8_t* in;
    uint64_t cap;
    const uint64_t* offs;
    const uint32_t* lens;
    const uint8_t* tids;
    uint64_t L, nfull;
    int gen_kind;
    void* out;
    int w;
    uint32_t* st;
    ChunkInit ini;
    hipStream_t s;
    LaunchLog* log = nullptr;
};
// The launch record's view of a model: IndepModel's template arguments (the codecs whose ladders
// the record covers); the IID models' launches are not recorded.
template <class M>
struct ModelRec {
    static constexpr bool kIndep = false;
};
template <bool kRare, int kNR, uint32_t kTabD, bool kLean, uint32_t kTabEnc>
struct ModelRec<IndepModel<kRare, kNR, kTabD, kLean, kTabEnc>> {
    static constexpr bool kIndep = true;
    static constexpr int rare = kRare, nr = kNR, lean = kLean;
};
// the launch of one instantiation: the tag arguments give Sym as a value and SPP as an Spp<N>
template <int N>
using Spp = std::integral_constant<int, N>;
template <class M, int kL = kLanes, bool kRes = false, typename Sym, class P>
void menc_of(const M& md, const EncArgs& a, uint32_t lds, Sym, P) {
    if constexpr (ModelRec<M>::kIndep)
        if (a.log) a.log->add(kRecMenc, sizeof(Sym), P::value, kL, kRes, ModelRec<M>::rare, ModelRec<M>::nr);
    menc<M, Sym, P::value, kL, kRes>(md, a.syms, a.tids, a.L, a.nfull, a.slots, a.cap, a.lens, a.st, a.ini, lds, a.s);
}
template <class M, int kL = kLanes, bool kRes = false, typename Sym, class P>
void mdec_of(const M& md, const DecArgs& a, uint32_t lds, Sym, P) {
    if constexpr (ModelRec<M>::kIndep)
        if (a.log) a.log->add(kRecMdec, sizeof(Sym), P::value, kL, kRes, ModelRec<M>::lean, ModelRec<M>::nr);
    mdec<M, Sym, P::value, kL, kRes>(md, a.in, a.cap, a.offs, a.lens, a.tids, a.L, a.nfull, a.gen_kind, a.out, a.st, a.ini,
                                     lds, a.s);
}

// An Independent<Categorical> set's fast-kernel images (built by ans_codecs.hip build_indep_fast).
struct IndepFast {
    bool usable = false;
    bool rare = false;  // some row needs the exact renorm screen (IndepModel<true>)
    uint32_t kmax = 0;  // most bytes one push emits
    int nr = 0;         // the tables' norm range (ans_fast.hpp kNormStd / kNormSmall / kNormBig)
    void* d_mem = nullptr;
    IndepModel<false> md;  // device pointers (every IndepModel instantiation has the same fields)
    // the 1,024-lane decoder's image (tables at LDS offset 0, DecLayout<kLanesW>), when the set fits
    // its 28 KiB; decodes of at least ncu * 1,024 chains use it (one such workgroup per CU)
    const uint4* dec_img_w = nullptr;
    uint32_t dec_bytes_w = 0;
    int ncu = 256;
    int lanes = 0;  // 0: by the call's size; 256 / 1,024: that layout where it exists (ans_gpu_tableset_lanes)
    bool lean = false, lean_w = false;  // IndepModel kLean for the 256- / 1,024-lane decoder image
    bool enc_wide = false;              // the encoder image fits the 1,024-lane layout (kEncTabW)
    // the 1,024-lane layouts when the call has the chains for one such workgroup per CU
    bool wide(uint64_t nfull) const { return lanes ? lanes == kLanesW : nfull >= static_cast<uint64_t>(ncu) * kLanesW; }
};

// the full chunks of a fixed-chunk Independent call (ans_codecs_indep_enc.hip / _dec.hip)
void indep_fast_encode(const IndepFast& f, const EncArgs& a);
void indep_fast_decode(const IndepFast& f, const DecArgs& a);
// resume (ans_codecs_indep_push.hip, k_menc<kRes>): pushes onto the messages in the slots; a lane
// whose message is too short for the prologue leaves kResumeExact in lens[c] for the exact kernel;
// a.ini is ChunkInit{}
void indep_fast_push(const IndepFast& f, const EncArgs& a);
// (ans_codecs_indep_pop.hip, k_mdec<kRes>): pops from the messages in the slots a.in, in place;
// a.lens in/out, a.offs NULL, a.gen_kind ANS_GEN_EMPTY, a.ini ChunkInit{}
void indep_fast_pop(const IndepFast& f, const DecArgs& a);

}  // namespace mfast
}  // namespace shuffle_coding
