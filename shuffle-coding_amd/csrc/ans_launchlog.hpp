// ans_launchlog.hpp — the launch record of a GPU context (ans_ctx.hpp ans_gpu::last), written by
// the launchers of the bulk coders and read by ans_gpu_last_launch (include/ans_capi.h).
#pragma once

#include <cstddef>
#include <cstdint>

// The coder kernels a context's last launcher call started, in launch order, with the template
// arguments its ladder chose (ans_gpu_last_launch formats them).  A launcher clears the record on
// entry and each launch site adds its entry from the same arguments that instantiate the kernel
// (the LAUNCH_* macros of ans_launch_impl.hpp, menc_of / mdec_of, the exact kernels' dev_*), so
// the record names what ran.  Plain data, no heap, nothing formatted on the launch path.
enum LaunchKind : uint8_t {
    kRecEncode,         // fast::k_encode      a = {KMAX, kK32, kGlobalRows, kVar, kNR, kM24}
    kRecEncodeW,        // fast::k_encode_w    a = {kK32, kPack, kSa, kVar, kNR}
    kRecDecode,         // fast::k_decode      a = {SPP, kMode, kP24, kJ4, kVar, kNR}
    kRecDecodeW,        // fast::k_decode_w    a = {kCompact, kPrefix, kVar, kP24, kNR}
    kRecDecodeG,        // fast::k_decode_g    a = {kNR}
    kRecEncodeGeneric,  // k_encode (one lane per chunk)  a = {kLds, kFast}
    kRecDecodeGeneric,  // k_decode (one lane per chunk)  a = {kLds, kFast}
    kRecMenc,           // mfast::k_menc<IndepModel>  a = {SPP, kL, kRes, R (renorm screen), NR}
    kRecMdec,           // mfast::k_mdec<IndepModel>  a = {SPP, kL, kRes, kLean, NR}
    kRecEncode64,       // the exact kernels over a table set (ans_codecs.hip)
    kRecDecode64,
    kRecPush64,
    kRecPop64,
    kRecMsetPush,       // k_mset_push / k_mset_pop (ans_mset.hip)  a = {counts in LDS (1) or global memory (0), workgroups}
    kRecMsetPop,
    kRecPolyaPush,      // k_polya_push / k_polya_pop (ans_polya.hip)  a = {kRedraws, workgroups}
    kRecPolyaPop,
    kRecArerPush,       // k_arer_push / k_arer_pop (ans_arer.hip)  a = {orbits, workgroups}
    kRecArerPop,
    kRecArpuPush,       // k_arpu_push / k_arpu_pop (ans_arpu.hip)  a = {orbits, workgroups}
    kRecArpuPop,
    kRecArerWlPush,     // k_arer_wl_push / _pop, k_arpu_wl_push / _pop (ans_wl.hip)  a = {wl_iter, workgroups, half_iter}
    kRecArerWlPop,
    kRecArpuWlPush,
    kRecArpuWlPop,
    kRecArerWllPush,    // k_arer_wll_push / _pop, k_arpu_wll_push / _pop (ans_wl_labelled.hip)
    kRecArerWllPop,     //   a = {wl_iter, workgroups, half_iter, node labels, edge labels}
    kRecArpuWllPush,
    kRecArpuWllPop,
    kRecJointErPush,    // k_joint_er_push / _pop, k_joint_pu_push / _pop (ans_joint.hip)
    kRecJointErPop,     //   a = {wl_iter, workgroups, half_iter, redraws (the urn's)}
    kRecJointPuPush,
    kRecJointPuPop,
};
struct LaunchRec {
    uint8_t kind;
    uint8_t sym_bytes;
    int16_t a[6];
};
// The slot of a[] in which a record kind keeps its launch's workgroup count (ans_gpu_last_launch_grid
// reads it; the text of ans_gpu_last_launch does not show it), or -1 for a kind that keeps none.
constexpr int rec_grid_slot(uint8_t kind) {
    return kind >= kRecMsetPush && kind <= kRecJointPuPop ? 1 : -1;
}
// ... and the count as the slot holds it: the workspace forms launch at most 8 workgroups per CU;
// the LDS form of the multiset kernels, one lane per chunk, can pass an int16_t and saturates.
constexpr int rec_grid(uint64_t workgroups) { return workgroups > 32767 ? 32767 : static_cast<int>(workgroups); }
struct LaunchLog {
    static constexpr uint32_t kCap = 8;  // (a call starts at most three coder kernels)
    uint32_t n = 0;                      // launches since the clear (entries past kCap are counted only)
    LaunchRec r[kCap] = {};
    void clear() { n = 0; }
    void add(LaunchKind kind, size_t sym_bytes, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0, int a5 = 0) {
        if (n < kCap)
            r[n] = LaunchRec{kind, static_cast<uint8_t>(sym_bytes),
                             {static_cast<int16_t>(a0), static_cast<int16_t>(a1), static_cast<int16_t>(a2),
                              static_cast<int16_t>(a3), static_cast<int16_t>(a4), static_cast<int16_t>(a5)}};
        ++n;
    }
};
