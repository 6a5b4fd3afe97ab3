"""A census of the bulk coders' kernel instantiations: every instantiation a launch ladder can
reach runs here once, named by the context's launch record (ans_gpu_last_launch /
Gpu.last_launch()) and checked byte for byte against the oracle.

The bulk coders are ladders of template instantiations chosen by host-side selectors
(ans_launch_impl.hpp launch_encode / launch_decode / launch_staged_* / launch_lds_decode, and
ans_codecs_indep_impl.hpp for Independent<Categorical>).  ROWS below holds one row per reachable
instantiation, written down from reading those ladders: the record strings the encode and the
decode call must leave, and the smallest table (or table set), symbol width and chunk layout that
select them.  A row is kept only if it names an encoder or a decoder no earlier row names, and no
two rows name the same pair.  UNREACHABLE lists the instantiations the ladders spell out but no
table can select, each with its arithmetic; they stay compiled for now.
NOT_INSTANTIATED lists the combinations the ladders already leave out.

A NEW LADDER BRANCH NEEDS A NEW ROW: whoever adds an instantiation (or a selector) adds the table
that reaches it here, with the record string it must leave.  A change to a kernel is tested by
the rows that name it.

Each GPU case builds the table, codes 1,025 chunks (one more than the widest workgroup has lanes,
so a partly filled workgroup runs) of one or two 128-B symbol groups plus a ragged last chunk
through the device API, asserts the record after the encode and after the decode, compares every
chunk's bytes and length (and the offsets they imply) with oracle.encode_chunks /
codec_encode_chunks, and checks the decode returns the symbols; once from Message::zeros() and
once from Message::random(seed + c) initial messages.  The CPU tests check each row's declared
preconditions (norm range, kmax, K vs 2^32, pmax vs 2^24 ...) from the reference's rules alone;
whether a table decodes far / rows / u, packs or compacts is the library's decision, which the
record assertion checks.
"""
import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

U = {1: "u8", 2: "u16", 4: "u32", 8: "u64"}
NCHUNKS = 1025  # the widest workgroup (k_decode, k_menc / k_mdec with 1,024 lanes) plus one
RAGGED_TAIL = 37


# ====================================================================== the table API's ladders
def _kmax_rows(masses):
    """Per symbol, the most bytes one push can emit: the largest j <= 4 with p K 2^(8j) < 2^64
    (src/ans.rs:246-253 with heads below 2^64); 0 for a zero mass."""
    m = [int(x) for x in masses]
    K = (1 << 56) // sum(m)
    return [max([j for j in range(1, 5) if p * K << (8 * j) < 1 << 64], default=1) if p else 0 for p in m]


def _nr(norm):
    return "std" if (1 << 16) <= norm <= (1 << 31) else ("small" if norm < (1 << 16) else "big")


def _facts(masses):
    """What the ladders' selectors are functions of, from the reference's rules alone."""
    m = [int(x) for x in masses]
    norm = sum(m)
    return dict(nr=_nr(norm), kmax=max(_kmax_rows(m)), k32=int((1 << 56) // norm < 1 << 32),
                m24=int(max(m) < 1 << 24), norm_gt_256=int(norm > 256), pmax_le_4096=int(max(m) <= 4096),
                below_2_16=int(max(m) < 1 << 16), nsym_gt_256=int(len(m) > 256))


def enc_lds(w, t, var):
    """fast::k_encode with LDS rows (launch_encode ENC_KMAX(false), launch_staged_encode ENCL):
    KMAX is max(kmax, 2); kNormSmall has one form, kNormBig always K < 2^32; kM24 (the mass word's
    top byte free) only in the fixed-chunk standard-range form."""
    km, k32 = max(t["kmax"], 2), t["k32"]
    if t["nr"] == "small":
        km, k32 = 2, 0
    if t["nr"] == "big":
        k32 = 1
    m24 = int(not var and t["nr"] == "std" and t["m24"])
    return f"k_encode<{U[w]},kmax={km},k32={k32},grows=0,var={int(var)},nr={t['nr']},m24={m24}>"


def dec_lds(w, t, var):
    """fast::k_decode (launch_lds_decode): u8 symbols take half-unit points (spp 8, kJ4) exactly
    when kmax = 4 outside kNormSmall, wider symbols keep their unit and set kJ4 there; the u-domain
    tables serve u8 symbols' kernels only and never kNormBig; kP24 is off for kNormBig."""
    unit = 16 // w
    k4 = t["kmax"] == 4 and t["nr"] != "small"
    spp = unit // 2 if (w == 1 and k4) else unit
    mode = t["mode"]
    if mode == "u" and (w > 1 or t["nr"] == "big"):
        mode = "rows"
    p24 = int(t["nr"] != "big" and t["m24"] and t["norm_gt_256"])
    return f"k_decode<{U[w]},spp={spp},mode={mode},p24={p24},j4={int(k4)},var={int(var)},nr={t['nr']}>"


def generic(kind, w, t):
    """the one-lane-per-chunk kernels (a fixed call's ragged last chunk): the table staged in LDS
    when its rows and buckets fit 64 KiB, the f64 quotient estimate in the standard range"""
    lds = int(16 * (t["nsym"] + 1) + 2 * 4096 <= 65536)
    return f"k_{kind}_generic<{U[w]},lds={lds},fast={int(t['nr'] == 'std')}>"


M18, M17 = 1 << 18, 1 << 17
MB = (1 << 23) + (1 << 19)  # 256 of these pass 2^31


def _t(masses, mode, **declared):
    masses = np.asarray(masses, dtype=np.uint64)
    return dict(masses=masses, mode=mode, nsym=len(masses), **declared)


# <= 256 symbols.  mode: what the u8 decoder takes (the library's decision: far when an LDS bucket
# holds three or more cdf boundaries, else u when the u-domain image resolves every bucket among
# three candidates, else rows).  The declared facts are checked on the CPU from the masses.
LDS_TABLES = {
    # ---- standard range, K < 2^32
    "std_k4_u": _t([1] + [M18] * 255, "u", nr="std", kmax=4, k32=1, m24=1),
    "std_k4_rows": _t([1, 1] + [M18] * 254, "rows", nr="std", kmax=4, k32=1, m24=1),
    "std_k4_far": _t([1, 1, 1] + [M18] * 253, "far", nr="std", kmax=4, k32=1, m24=1),
    "std_k4_big_mass_u": _t([1 << 25, 1] + [M17] * 254, "u", nr="std", kmax=4, k32=1, m24=0),
    "std_k4_big_mass_rows": _t([1 << 25, 1] + [M17] * 200, "rows", nr="std", kmax=4, k32=1, m24=0),
    "std_k4_big_mass_far": _t([1 << 25, 1, 1, 1] + [M17] * 252, "far", nr="std", kmax=4, k32=1, m24=0),
    "std_k2_big_mass_u": _t([1 << 25] + [M17] * 255, "u", nr="std", kmax=2, k32=1, m24=0),
    "std_k1_big_mass_rows": _t([1 << 30, 1 << 30], "rows", nr="std", kmax=1, k32=1, m24=0),
    "std_k2_big_mass_far": _t([1 << 25] + [1 << 12] * 8 + [M17] * 247, "far", nr="std", kmax=2, k32=1, m24=0),
    "std_k1_u": _t([M18] * 256, "u", nr="std", kmax=1, k32=1, m24=1),
    "std_k1_rows": _t([M18] * 200 + [M18 + 1], "rows", nr="std", kmax=1, k32=1, m24=1),
    "std_k2_far": _t([1 << 12] * 8 + [M18] * 248, "far", nr="std", kmax=2, k32=1, m24=1),
    "std_k3_u": _t([256] + [M18] * 255, "u", nr="std", kmax=3, k32=1, m24=1),
    "std_k3_big_mass": _t([1 << 25, 256] + [M17] * 254, "u", nr="std", kmax=3, k32=1, m24=0),
    # ---- standard range, K >= 2^32 (norm <= 2^24: every mass below 2^24, and kmax <= 3)
    "std_k1_K_u": _t([1 << 15, 1 << 15], "u", nr="std", kmax=1, k32=0, m24=1),
    "std_k3_K": _t([8] + [1 << 12] * 255, "u", nr="std", kmax=3, k32=0, m24=1),
    # ---- norm < 2^16
    "small_2_u": _t([1, 1], "u", nr="small", kmax=1, k32=0, m24=1, norm_gt_256=0),
    "small_3_rows": _t([1, 2], "rows", nr="small", kmax=1, k32=0, m24=1, norm_gt_256=0),
    "small_u": _t([1 << 7] * 256, "u", nr="small", kmax=1, k32=0, m24=1, norm_gt_256=1),
    "small_rows": _t([100] * 100 + [101], "rows", nr="small", kmax=1, k32=0, m24=1, norm_gt_256=1),
    "small_far": _t([1, 1, 1, 1] + [100] * 100, "far", nr="small", kmax=2, k32=0, m24=1, norm_gt_256=1),
    # ---- 2^31 < norm < 2^32
    "big_k1_rows": _t([1 << 31, 1 << 30], "rows", nr="big", kmax=1, k32=1, m24=0),
    "big_k2_far": _t([M17] * 8 + [MB] * 248, "far", nr="big", kmax=2, k32=1, m24=1),
    "big_k3_rows": _t([256] + [MB] * 255, "rows", nr="big", kmax=3, k32=1, m24=1),
    "big_k4_rows": _t([1] + [MB] * 255, "rows", nr="big", kmax=4, k32=1, m24=1),
    "big_k4_far": _t([1, 1, 1] + [MB] * 253, "far", nr="big", kmax=4, k32=1, m24=1),
}


# > 256 symbols (u16 / u32 symbols; ans_wide.hpp k_encode_w / k_decode_w, ans_fast.hpp k_encode
# with global rows and k_decode_g).  enc / dec: the instantiation's arguments, the library's
# decision where they depend on the images it could build (packed prefix, shift bytes, compact
# buckets, the LDS prefix); var is filled in per layout.
def enc_w(w, t, var):
    if t["enc"][0] == "g":  # k_encode with global rows: norm < 2^22, so K >= 2^34 and kmax <= 3
        km = 2 if t["nr"] == "small" else max(t["kmax"], 2)
        return f"k_encode<{U[w]},kmax={km},k32=0,grows=1,var=0,nr={t['nr']},m24=0>"
    _, pack, sa = t["enc"]
    k32 = 1 if t["nr"] == "big" else t["k32"]
    return f"k_encode_w<{U[w]},k32={k32},pack={pack},sa={sa},var={int(var)},nr={t['nr']}>"


def dec_w(w, t, var):
    if t["dec"] == "g":
        return f"k_decode_g<{U[w]},nr={t['nr']}>"
    compact = int(t["dec"] == "compact")
    # (the fixed-chunk compact decoder alone has a kP24 form, standard range)
    p24 = int(compact and not var and t["nr"] == "std" and t["m24"])
    return f"k_decode_w<{U[w]},compact={compact},prefix={1 - compact},var={int(var)},p24={p24},nr={t['nr']}>"


def _zeros_then(nzero, masses):
    return [0] * nzero + list(masses)


WIDE_TABLES = {
    # norm >= 2^22: k_encode_w.  Plain cdf rows below 24,576 symbols; a mass above 2^16 - 1 keeps
    # the decode buckets from compacting (the LDS-prefix decoder)
    "wide_plain_prefix": _t([M17] * 300, None, enc=("w", 0, 0), dec="prefix", nr="std", kmax=2, k32=1, m24=1,
                            nsym_gt_256=1),
    "wide_plain_K_compact": _t([4097] * 1024, None, enc=("w", 0, 0), dec="compact", nr="std", kmax=2, k32=0, m24=1,
                               nsym_gt_256=1, pmax_le_4096=0),
    # the packed prefix (more than 24,576 symbols, masses below 2^16), without shift bytes (a mass
    # above 4,096) and with them
    "wide_pack_K": _t([5000] + [200] * 32767, None, enc=("w", 1, 0), dec="compact", nr="std", kmax=2, k32=0, m24=1,
                      nsym_gt_256=1, below_2_16=1, pmax_le_4096=0),
    "wide_pack": _t([5000] + [300] * 65535, None, enc=("w", 1, 0), dec="compact", nr="std", kmax=3, k32=1, m24=1,
                    nsym_gt_256=1, below_2_16=1, pmax_le_4096=0),
    "wide_sa_K": _t([200] * 32768, None, enc=("w", 1, 1), dec="compact", nr="std", kmax=2, k32=0, m24=1,
                    nsym_gt_256=1, below_2_16=1, pmax_le_4096=1),
    "wide_sa_c4": _t(A.c4_masses(), None, enc=("w", 1, 1), dec="compact", nr="std", kmax=4, k32=1, m24=1,
                     nsym_gt_256=1, below_2_16=1, pmax_le_4096=1),
    "wide_big_plain": _t([MB] * 300, None, enc=("w", 0, 0), dec="prefix", nr="big", kmax=2, k32=1, m24=1,
                         nsym_gt_256=1),
    # (a packed prefix needs blocks of 16 masses below 2^16 together: 24,592 light symbols, then heavy ones)
    "wide_big_pack": _t([4000] * 24592 + [60000] * 40944, None, enc=("w", 1, 0), dec="prefix", nr="big", kmax=3, k32=1, m24=1,
                        nsym_gt_256=1, below_2_16=1, pmax_le_4096=0),
    # norm < 2^22: k_encode with global rows (kmax <= 3 there, K >= 2^34)
    "grows_std_k2": _t([1 << 10] * 300, None, enc=("g",), dec="compact", nr="std", kmax=2, k32=0, m24=1, nsym_gt_256=1),
    "grows_std_k3": _t([2] + [1 << 10] * 300, None, enc=("g",), dec="compact", nr="std", kmax=3, k32=0, m24=1,
                       nsym_gt_256=1),
    "grows_small": _t([3] * 300, None, enc=("g",), dec="compact", nr="small", kmax=2, k32=0, m24=1, nsym_gt_256=1),
    # 24,100 leading zero-mass symbols (more cdf entries than k_decode_w's LDS holds) leave it no
    # prefix with any probability: k_decode_g
    "noprefix_std": _t(_zeros_then(24100, [M17] * 300), None, enc=("w", 0, 0), dec="g", nr="std", kmax=2, k32=1, m24=1,
                       nsym_gt_256=1),
    "noprefix_small": _t(_zeros_then(24100, [3] * 300), None, enc=("g",), dec="g", nr="small", kmax=2, k32=0, m24=1,
                         nsym_gt_256=1),
    "noprefix_big": _t(_zeros_then(24100, [MB] * 300), None, enc=("w", 0, 0), dec="g", nr="big", kmax=2, k32=1, m24=1,
                       nsym_gt_256=1),
}


for _t_ in list(LDS_TABLES.values()) + list(WIDE_TABLES.values()):
    _t_.setdefault("norm_gt_256", 1)  # (declared only below 2^16, where it can fail)


def _table_rows():
    rows, seen_enc, seen_dec = [], set(), set()

    def add(rid, **row):
        if row["enc"] in seen_enc and row["dec"] in seen_dec:
            return
        seen_enc.add(row["enc"])
        seen_dec.add(row["dec"])
        rows.append(dict(id=rid, api="table", **row))

    for name, t in LDS_TABLES.items():
        for w in (1, 2, 4):
            # fixed chunks: two 128-B symbol groups, then a ragged last chunk on the generic kernels
            add(f"{name}-{U[w]}-fixed", table=name, w=w, layout="fixed", chunk_len=256 // w,
                enc=enc_lds(w, t, False) + ";" + generic("encode", w, t),
                dec=dec_lds(w, t, False) + ";" + generic("decode", w, t))
            # ragged chunks of 100 symbols and variable chunks: the staged kVar forms, every chunk
            layout = "var" if w == 2 else "ragged"
            add(f"{name}-{U[w]}-{layout}", table=name, w=w, layout=layout, chunk_len=100,
                enc=enc_lds(w, t, True), dec=dec_lds(w, t, True))
    for name, t in WIDE_TABLES.items():
        for w in (2, 4):
            add(f"{name}-{U[w]}-fixed", table=name, w=w, layout="fixed", chunk_len=256 // w,
                enc=enc_w(w, t, False) + ";" + generic("encode", w, t),
                dec=dec_w(w, t, False) + ";" + generic("decode", w, t))
            if t["enc"][0] == "w" and t["dec"] != "g":  # both sides staged: every chunk on the kVar forms
                layout = "var" if w == 4 else "ragged"
                add(f"{name}-{U[w]}-{layout}", table=name, w=w, layout=layout, chunk_len=100,
                    enc=enc_w(w, t, True), dec=dec_w(w, t, True))
            elif t["dec"] != "g":  # global rows are never staged (the generic encoder), the decoder is
                add(f"{name}-{U[w]}-ragged", table=name, w=w, layout="ragged", chunk_len=100,
                    enc=generic("encode", w, t), dec=dec_w(w, t, True))
    return rows


# ====================================================================== Independent<Categorical>
def _indep_kmax(tables):
    """Most bytes one push emits over every head below 2^64 (the points' spacing)."""
    km = 0
    for m in tables:
        K = (1 << 56) // int(sum(int(x) for x in m))
        for p in m:
            if int(p):
                km = max(km, sum(1 for j in range(1, 8) if ((1 << 64) - 1) >> (8 * j) >= int(p) * K))
    return km


def _indep_facts(tables):
    norms = [sum(int(x) for x in m) for m in tables]
    nrs = {_nr(n) for n in norms}
    kmax = _indep_kmax(tables)
    lean = int(kmax <= 3 and all(n > 256 for n in norms) and all(int(x) < 1 << 24 for m in tables for x in m) and
               (nrs != {"std"} or all(n >= 1 << 20 for n in norms)))
    return dict(nr=nrs.pop() if len(nrs) == 1 else "mixed", kmax4=int(kmax >= 4), lean=lean)


def _perm(m):
    m = np.asarray(m, dtype=np.uint64)
    return [m, m[::-1].copy()]  # two tables of one norm and one multiset of masses


_RB = (1 << 32) - 257  # a kNormBig norm with (2^24 - 1) * 256 = norm + 1 just inside 2^56 / K: a screened row
INDEP_SETS = {
    # rare: some row needs the exact renorm screen (the library's decision; power-of-two norms with
    # a mass norm / 256^j have one).  kmax4 / lean / nr are checked on the CPU
    "std": dict(tables=_perm(np.arange(1, 257) * 257), rare=0, nr="std", kmax4=0, lean=1),
    "std_k4": dict(tables=_perm([1] + [M18] * 255), rare=0, nr="std", kmax4=1, lean=0),
    "std_rare": dict(tables=_perm([1 << 8] * 256), rare=1, nr="std", kmax4=0, lean=0),
    "std_rare_k4": dict(tables=_perm([1, M18 - 1] + [M18] * 253 + [2 * M18]), rare=1, nr="std", kmax4=1, lean=0),  # norm 2^26
    "small": dict(tables=_perm([31000, 3400, 7, 1]), rare=0, nr="small", kmax4=0, lean=1),
    "small_rare": dict(tables=_perm([1] * 256), rare=1, nr="small", kmax4=0, lean=0),
    "big": dict(tables=_perm([(1 << 24) - 1] * 200), rare=0, nr="big", kmax4=0, lean=1),
    "big_rare": dict(tables=_perm([(1 << 24) - 1, _RB - (1 << 24) + 1]), rare=1, nr="big", kmax4=0, lean=0),
    "big_k4": dict(tables=_perm([1] + [MB] * 255), rare=0, nr="big", kmax4=1, lean=0),
    "big_rare_k4": dict(tables=_perm([1, (1 << 24) - 1, _RB - (1 << 24)]), rare=1, nr="big", kmax4=1, lean=0),
    # norms of two ranges: the fast path declines, the exact kernels code every chunk
    "mixed": dict(tables=[np.arange(1, 257, dtype=np.uint64) * 257, np.asarray([3, 5], np.uint64)], rare=None,
                  nr="mixed", kmax4=0, lean=0),
}


def _indep_rows():
    rows, seen_enc, seen_dec = [], set(), set()
    for name, s in INDEP_SETS.items():
        for w in (1, 2, 4):
            for lanes in (256, 1024):
                for res in (0, 1):
                    u = U[w]
                    spp = {1: 8 if s["kmax4"] else 16, 2: 8, 4: 4}[w]
                    # (the 1,024-lane decoder reads lean_w, the 256-lane one lean: build_indep_fast sets
                    # both from one predicate, so no set tells them apart and s["lean"] serves both)
                    if s["nr"] == "mixed":
                        if lanes == 1024:
                            continue
                        enc = f"k_push64<{u}>" if res else f"k_encode64<catset,{u}>"
                        dec = f"k_pop64<{u}>" if res else f"k_decode64<catset,{u}>"
                    else:
                        enc = f"k_menc<indep,{u},spp={spp},lanes={lanes},res={res},rare={s['rare']},nr={s['nr']}>"
                        dec = f"k_mdec<indep,{u},spp={spp},lanes={lanes},res={res},lean={s['lean']},nr={s['nr']}>"
                        # new messages: the ragged last chunk on the exact kernels; resume: the exact
                        # kernels' pass over the chunks the fast ones handed over
                        enc += f";k_push64<{u}>" if res else f";k_encode64<catset,{u}>"
                        dec += f";k_pop64<{u}>" if res else f";k_decode64<catset,{u}>"
                    if enc in seen_enc and dec in seen_dec:
                        continue
                    seen_enc.add(enc)
                    seen_dec.add(dec)
                    rows.append(dict(id=f"{name}-{u}-{lanes}-{'resume' if res else 'new'}", api="indep", set=name, w=w,
                                     lanes=lanes, res=res, chunk_len=256 // w, enc=enc, dec=dec))
    return rows


ROWS = _table_rows() + _indep_rows()

# Instantiations the ladders spell out, and the units compile, that no table or set can select.
UNREACHABLE = [
    ("k_encode<*,kmax=4,k32=0,*>",
     "kmax = 4 needs p K 2^32 < 2^64 for some p >= 1, hence K < 2^32: ENC / ENCL(4, false, ...) for every width, LDS "
     "and global rows, fixed and staged"),
    ("k_encode<*,k32=0,grows=0,var=0,nr=std,m24=0>",
     "m24 = 0 needs a mass >= 2^24, so norm >= 2^24 and K = floor(2^56 / norm) <= 2^32; K = 2^32 only for norm = 2^24, "
     "one symbol holding all of it, and build_fast_table declines a symbol that holds all of a power-of-two norm (no "
     "fast kernel runs): every table the ladder sees has norm > 2^24 and K < 2^32"),
    ("k_encode<*,kmax=4,*,grows=1,*> and k_encode<*,k32=1,grows=1,*>",
     "global rows serve norm < 2^22 (k_encode_w takes 2^22 on, staged when the chunk is off 128 B): K > 2^34, so "
     "k32 = 0 and kmax <= 3; only a failed staging allocation reaches the others"),
    ("k_encode_w<*,sa=1,*,nr=big>", "shift bytes need every mass <= 4096: norm <= 65536 * 4096 = 2^28 < 2^31"),
    ("k_decode<u8,*,mode=far,p24=0,*,nr=small>",
     "p24 = 0 below 2^16 means norm <= 256 <= the 1,624 LDS buckets: width 1, no bucket holds three boundaries"),
    ("k_decode_w<*,compact=1,prefix=0,var=0,p24=0,nr=std>",
     "a compact bucket's first offset is its first symbol's mass, at most 2^16 - 1 < 2^24, and norm >= 2^16 > 256: "
     "p24 = 1 whenever the standard-range buckets compact"),
    ("k_decode_w<*,compact=1,*,nr=big>",
     "norm > 2^31 over at most 65,536 symbols: some five consecutive masses pass 2^16 - 1, no compact image"),
    ("k_decode_w<*,compact=0,prefix=1,*,nr=small>", "norm < 2^16: every candidate offset fits u16, the buckets compact"),
    ("k_menc<indep,u8,spp=8,*,nr=small> and k_mdec<indep,u8,spp=8,*,nr=small>",
     "norm < 2^16 gives p K >= 2^40: at most two bytes a push, 16 symbols between points"),
    ("k_mdec<indep,u8,spp=8,*,lean=1,*>", "lean needs every p K >= 2^32 (kmax <= 3), half-unit points kmax >= 4"),
]

# Combinations of the same arguments that the ladders already leave out (an if constexpr, or no
# branch at all): nothing is compiled for them and no record can name them.  Kept apart from
# UNREACHABLE so that a later removal works from the list of what is there to remove.
NOT_INSTANTIATED = [
    ("k_encode<*,grows=1,*,nr=big,*>", "norm > 2^31 >= 2^22: k_encode_w.  ENC_KMAX(true) has no kNormBig branch (such a "
     "table would fall to its standard-range switch, which no call reaches: fast_chunks declines it)"),
    ("k_encode_w<*,nr=small>", "k_encode_w needs norm >= 2^22; ENCW / ENCV name kNormBig and kNormStd only"),
    ("k_decode<*,j4=1,*,nr=small>", "norm < 2^16 gives K >= 2^40: p K 2^24 >= 2^64, kmax <= 2 (launch_lds_decode's points)"),
    ("k_decode<*,mode=u,*,nr=big>", "the u-domain image needs 2 norm <= 2^32 (launch_lds_decode's modes)"),
]


# ---------------------------------------------------------------------- CPU checks (no GPU)
def test_rows_name_distinct_instantiations():
    pairs = [r["enc"] + " | " + r["dec"] for r in ROWS]
    assert len(set(pairs)) == len(pairs)
    assert len({r["id"] for r in ROWS}) == len(ROWS)
    # every row contributes an encoder or a decoder of its own
    seen_e, seen_d = set(), set()
    for r in ROWS:
        assert r["enc"] not in seen_e or r["dec"] not in seen_d, r["id"]
        seen_e.add(r["enc"])
        seen_d.add(r["dec"])
    assert len(ROWS) > 150


def _matches(pattern, record):
    """UNREACHABLE's patterns: 'name<a,*,b=1,*>' matches a record whose arguments include a and b=1."""
    name, args = pattern.split("<", 1)
    args = [a for a in args.rstrip(">").split(",") if a != "*"]
    for one in record.split(";"):
        rname, rargs = one.split("<", 1)
        rargs = rargs.rstrip(">").split(",")
        if rname == name and all(a in rargs for a in args):
            return True
    return False


def test_no_row_names_an_unreachable_instantiation():
    for pats, why in UNREACHABLE + NOT_INSTANTIATED:
        assert why
        for pat in pats.split(" and "):
            for r in ROWS:
                assert not _matches(pat, r["enc"]) and not _matches(pat, r["dec"]), (pat, r["id"])


@pytest.mark.parametrize("name", sorted(LDS_TABLES) + sorted(WIDE_TABLES))
def test_declared_table_preconditions(name):
    t = (LDS_TABLES.get(name) or WIDE_TABLES[name])
    got = _facts(t["masses"])
    for key in ("nr", "kmax", "k32", "m24", "norm_gt_256", "pmax_le_4096", "below_2_16", "nsym_gt_256"):
        if key in t:
            assert got[key] == t[key], (name, key, got[key])
    assert (len(t["masses"]) > 256) == (name in WIDE_TABLES)


@pytest.mark.parametrize("name", sorted(INDEP_SETS))
def test_declared_set_preconditions(name):
    s = INDEP_SETS[name]
    got = _indep_facts(s["tables"])
    assert all(len(m) <= 256 for m in s["tables"])
    for key in ("nr", "kmax4", "lean"):
        if s["nr"] != "mixed" or key == "nr":
            assert got[key] == s[key], (name, key, got[key])


# ---------------------------------------------------------------------- GPU cases
@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _draw(masses, n, seed):
    """As test_gpu_norm_ranges._symbols: half iid from the table, half uniform over its non-zero
    symbols, so the rare rows that make kmax what it is are coded."""
    rng = np.random.default_rng(seed)
    nz = np.flatnonzero(masses)
    syms = orc.gen_iid(masses, seed, 0, n)
    mask = rng.random(n) < 0.5
    syms[mask] = rng.choice(nz, size=int(mask.sum()))
    return syms.astype(np.uint32)


# The LDS decoder's bucket count (ans_fast.hpp kDecNbMax).  Buckets are the library's, the reference
# has none: this only sizes the input check below; that the library called the table far is the
# record's mode=far.
_DEC_BUCKETS = 1624
_kmax_rows_of = {}


def _chunk_cfs(masses, chunk, okind, seed_c):
    """The cdf values a decoder of this chunk sees, one per symbol, from the oracle itself: its
    stream for the chunk (initial message of the case's kind, seed + c) popped one symbol at a
    time, head mod norm read before each pop (src/ans.rs:96-105)."""
    od, _, _ = orc.encode_chunks(masses, chunk, len(chunk), kind=okind, seed=seed_c)
    m = orc.Message.unflatten(od.tobytes(), okind, seed_c)
    cat = orc.Categorical(masses)
    norm, cfs = int(cat.norm), []
    for x in chunk:
        cfs.append(int(m.head) % norm)
        assert cat.pop(m) == int(x)
    return cfs


def _assert_inputs_reach_the_rows(name, t, syms, chunks, okind, seed):
    """chunks: (c, first, end) of every chunk the fast kernels code."""
    masses = t["masses"]
    if name not in _kmax_rows_of:
        _kmax_rows_of[name] = np.asarray(_kmax_rows(masses))
    kr = _kmax_rows_of[name]
    fast = np.concatenate([syms[a:b] for _, a, b in chunks]).astype(np.int64)
    assert (kr[fast] == kr.max()).any(), "a coded symbol whose push emits kmax bytes"
    if t["mode"] != "far":
        return
    cum = np.concatenate([[0], np.cumsum(masses)]).astype(np.int64)
    norm, shift = int(cum[-1]), 0
    while ((norm - 1) >> shift) + 1 > _DEC_BUCKETS:
        shift += 1
    for c, a, b in chunks:  # (stops at the first chunk that holds one)
        for cf in _chunk_cfs(masses, syms[a:b], okind, seed + c):
            s0 = int(np.searchsorted(cum, (cf >> shift) << shift, side="right")) - 1  # the bucket's first symbol
            if cf >= int(cum[min(s0 + 3, len(masses))]):
                return
    raise AssertionError("no coded cf past its bucket's third boundary")


def _dev(torch, a, w):
    dt = {1: np.uint8, 2: np.int16, 4: np.int32}[w]
    return torch.from_numpy(np.ascontiguousarray(a.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[w]).view(dt))).cuda()


def _slot_bytes(slots, lens, cap):
    """The streams in the slots, concatenated in chunk order (the dense container)."""
    s = slots.cpu().numpy().reshape(len(lens), cap)
    return s[np.arange(cap)[None, :] < lens[:, None]]


def _check_container(slots, d_lens, cap, want):
    odata, ooffs, olens = want
    lens = d_lens.cpu().numpy().astype(np.int64)
    assert np.array_equal(lens, olens.astype(np.int64)), "every chunk's stream length"
    assert np.array_equal(np.cumsum(lens) - lens, ooffs.astype(np.int64)), "the offsets the lengths imply"
    assert _slot_bytes(slots, lens, cap).tobytes() == odata.tobytes(), "every chunk's bytes"


GENS = [("zeros", A.GEN_ZEROS, orc.ZEROS, 0), ("random", A.GEN_RANDOM, orc.RANDOM, 77)]
TABLE_ROWS = [r for r in ROWS if r["api"] == "table"]
INDEP_ROWS = [r for r in ROWS if r["api"] == "indep"]
_tables_on_gpu = {}


def _gpu_table(gpu, name):
    if name not in _tables_on_gpu:
        t = LDS_TABLES.get(name) or WIDE_TABLES[name]
        _tables_on_gpu.clear()  # one table resident at a time
        _tables_on_gpu[name] = (t, A.GpuTable(gpu, A.Categorical(t["masses"])))
    return _tables_on_gpu[name]


@pytest.mark.gpu
@pytest.mark.parametrize("gen", GENS, ids=[g[0] for g in GENS])
@pytest.mark.parametrize("row", TABLE_ROWS, ids=[r["id"] for r in TABLE_ROWS])
def test_table_ladder_row(gpu, row, gen):
    torch = pytest.importorskip("torch")
    _, gkind, okind, seed = gen
    t, gt = _gpu_table(gpu, row["table"])
    w, L = row["w"], row["chunk_len"]
    masses = t["masses"]
    if row["layout"] == "var":
        rng = np.random.default_rng(5)
        sizes = np.concatenate([[0, 1, L], rng.integers(0, 2 * L, NCHUNKS - 3)]).astype(np.uint64)
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        syms = _draw(masses, int(starts[-1]), 3)
        _assert_inputs_reach_the_rows(row["table"], t, syms, [(c, int(starts[c]), int(starts[c + 1])) for c in range(NCHUNKS)
                                                              if starts[c + 1] > starts[c]], okind, seed)
        s = syms.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[w])
        data, offs, lens = gt.encode_var_chunks(s, starts, gen_kind=gkind, seed=seed)
        assert gpu.last_launch() == row["enc"]
        for c in range(0, NCHUNKS, 1):
            a, b = int(starts[c]), int(starts[c + 1])
            if b > a:
                od, _, _ = orc.encode_chunks(masses, syms[a:b], b - a, kind=okind, seed=seed + c)
                want = od.tobytes()
            else:
                m0 = orc.Message.zeros() if okind == orc.ZEROS else orc.Message.random(seed + c)
                want = bytes(m0.flatten())
            assert data[int(offs[c]):int(offs[c] + lens[c])].tobytes() == want, c
        assert np.array_equal(offs, np.cumsum(lens) - lens)
        back = gt.decode_var_chunks(data, offs, lens, starts, s.dtype, gen_kind=gkind, seed=seed)
        assert gpu.last_launch() == row["dec"]
        assert np.array_equal(back, s)
        return
    n = NCHUNKS * L + RAGGED_TAIL
    syms = _draw(masses, n, 3)
    # (the ragged last chunk goes to the generic kernels)
    _assert_inputs_reach_the_rows(row["table"], t, syms, [(c, c * L, (c + 1) * L) for c in range(NCHUNKS)], okind, seed)
    nchunks = NCHUNKS + 1
    cap = gt.slot_capacity(L)
    stream = torch.cuda.Stream()
    d_syms = _dev(torch, syms, w)
    slots = torch.zeros(nchunks * cap, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nchunks, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    gt.dev_encode(d_syms, w, n, L, slots, cap, d_lens, status, stream, gen_kind=gkind, seed=seed)
    assert gpu.last_launch() == row["enc"]
    assert gpu.status(status, stream) == 0
    _check_container(slots, d_lens, cap, orc.encode_chunks(masses, syms, L, kind=okind, seed=seed))
    out = torch.zeros_like(d_syms)
    gt.dev_decode(slots, None, cap, d_lens, n, L, out, w, status, stream, gen_kind=gkind, seed=seed)
    assert gpu.last_launch() == row["dec"]
    assert gpu.status(status, stream) == 0
    assert torch.equal(out, d_syms), "decode returns the symbols"


def _indep_inputs(tables, n, seed):
    rng = np.random.default_rng(seed)
    tids = rng.integers(0, len(tables), size=n).astype(np.uint32)
    syms = np.zeros(n, np.uint64)
    for ti, m in enumerate(tables):
        sel = tids == ti
        syms[sel] = _draw(np.asarray(m, np.uint64), int(sel.sum()), seed + 1 + ti)
    return tids, syms


def _assert_set_inputs_reach_kmax(tables, tids, syms):
    """Some coded (table, symbol) row's push emits as many bytes as any row of the set can."""
    km = [np.asarray([sum(1 for j in range(1, 8) if ((1 << 64) - 1) >> (8 * j) >= int(p) * ((1 << 56) // int(m.sum())))
                      if p else 0 for p in m]) for m in tables]
    coded = np.concatenate([km[ti][syms[tids == ti].astype(np.int64)] for ti in range(len(tables))])
    assert (coded == max(k.max() for k in km)).any(), "a coded row whose push emits the set's kmax bytes"


def _halves(a, nchunks, L):
    """(first halves, second halves) of every chunk of L, each as one array of chunks of L / 2."""
    a = a[:nchunks * L].reshape(nchunks, L)
    return a[:, :L // 2].ravel().copy(), a[:, L // 2:].ravel().copy()


@pytest.mark.gpu
@pytest.mark.parametrize("gen", GENS, ids=[g[0] for g in GENS])
@pytest.mark.parametrize("row", INDEP_ROWS, ids=[r["id"] for r in INDEP_ROWS])
def test_independent_ladder_row(gpu, row, gen):
    torch = pytest.importorskip("torch")
    _, gkind, okind, seed = gen
    s = INDEP_SETS[row["set"]]
    tables = [np.asarray(m, np.uint64) for m in s["tables"]]
    w, L = row["w"], row["chunk_len"]
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    assert (ts.fast() != 0) == (s["nr"] != "mixed")
    ts.lanes(row["lanes"])
    cap = -(-ts.slot_capacity(L) // 128) * 128
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ind = dict(tables=tables, kind=okind, seed=seed)
    if not row["res"]:
        n = NCHUNKS * L + RAGGED_TAIL
        nchunks = NCHUNKS + 1
        tids, syms = _indep_inputs(tables, n, 11)
        _assert_set_inputs_reach_kmax(tables, tids[:NCHUNKS * L], syms[:NCHUNKS * L])
        d_tids = torch.from_numpy(tids.astype(np.uint8)).cuda()
        d_syms = _dev(torch, syms, w)
        slots = torch.zeros(nchunks * cap, dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(nchunks, dtype=torch.int32, device="cuda")
        ts.dev_encode(d_tids, d_syms, w, n, L, slots, cap, d_lens, status, stream, gen_kind=gkind, seed=seed)
        assert gpu.last_launch() == row["enc"]
        assert gpu.status(status, stream) == 0
        _check_container(slots, d_lens, cap, orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, syms, L, tids=tids, **ind))
        out = torch.zeros_like(d_syms)
        ts.dev_decode(d_tids, slots, None, cap, d_lens, n, L, out, w, status, stream, gen_kind=gkind, seed=seed)
        assert gpu.last_launch() == row["dec"]
        assert gpu.status(status, stream) == 0
        assert torch.equal(out, d_syms), "decode returns the symbols"
        return
    # resume: chunk c's second half coded as a new message, its first half pushed on top (the
    # whole chunk's message), then popped again (the second half's message)
    n = NCHUNKS * L
    tids, syms = _indep_inputs(tables, n, 13)
    (ta, tb), (sa, sb) = _halves(tids, NCHUNKS, L), _halves(syms, NCHUNKS, L)
    h = L // 2
    _assert_set_inputs_reach_kmax(tables, tb, sb)  # the new messages' half, then the pushed (and popped) half
    _assert_set_inputs_reach_kmax(tables, ta, sa)
    slots = torch.zeros(NCHUNKS * cap, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(NCHUNKS, dtype=torch.int32, device="cuda")
    d_tb, d_sb = torch.from_numpy(tb.astype(np.uint8)).cuda(), _dev(torch, sb, w)
    d_ta, d_sa = torch.from_numpy(ta.astype(np.uint8)).cuda(), _dev(torch, sa, w)
    ts.dev_encode(d_tb, d_sb, w, NCHUNKS * h, h, slots, cap, d_lens, status, stream, gen_kind=gkind, seed=seed)
    second = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, sb, h, tids=tb, **ind)
    _check_container(slots, d_lens, cap, second)
    ts.dev_push(d_ta, d_sa, w, NCHUNKS * h, h, slots, cap, d_lens, status, stream)
    assert gpu.last_launch() == row["enc"]
    assert gpu.status(status, stream) == 0
    _check_container(slots, d_lens, cap, orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, syms, L, tids=tids, **ind))
    out = torch.zeros_like(d_sa)
    ts.dev_pop(d_ta, slots, cap, d_lens, NCHUNKS * h, h, out, w, status, stream)
    assert gpu.last_launch() == row["dec"]
    assert gpu.status(status, stream) == 0
    assert torch.equal(out, d_sa), "pop returns the pushed symbols"
    _check_container(slots, d_lens, cap, second)


@pytest.mark.gpu
def test_last_launch_buffer_contract():
    """ans_gpu_last_launch: empty before any coder call; a short buffer is ANS_E_LEN with the
    needed length, a buffer of length + 1 receives the NUL-terminated text."""
    import ctypes
    g = A.Gpu(0)
    assert g.last_launch() == ""
    gt = A.GpuTable(g, A.Categorical(LDS_TABLES["std_k1_u"]["masses"]))
    gt.encode_chunks(np.zeros(256 * 3 + 5, np.uint8), 256)
    want = "k_encode<u8,kmax=2,k32=1,grows=0,var=0,nr=std,m24=1>;k_encode_generic<u8,lds=1,fast=1>"
    assert g.last_launch() == want
    n = ctypes.c_size_t(0)
    fn = A.lib().ans_gpu_last_launch
    assert fn(g.h, None, 0, ctypes.byref(n)) == A.ANS_E_LEN and n.value == len(want)
    buf = ctypes.create_string_buffer(len(want) + 1)
    ctypes.memset(buf, 0xFF, len(want) + 1)
    assert fn(g.h, buf, len(want), ctypes.byref(n)) == A.ANS_E_LEN and n.value == len(want)
    assert buf.raw == b"\xff" * (len(want) + 1), "a short buffer is left alone"
    assert fn(g.h, buf, len(want) + 1, ctypes.byref(n)) == A.ANS_OK and buf.value.decode() == want
