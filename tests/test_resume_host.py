"""Resume without a GPU: the C ABI exports and declares the push / pop entries (include/ans_capi.h
section 4b), they refuse a NULL handle, the Python wrappers check their arguments' lengths before
any pointer reaches the library, GpuGraphs.encode refuses label arrays of the wrong length, and the
fast encoder's resume arithmetic (csrc/ans_resume.hpp, compiled with g++) agrees with the oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ans_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ans_dev_independent_push", "ans_dev_independent_pop", "ans_dev_independent_push_var",
           "ans_dev_independent_pop_var", "ans_gpu_independent_push_chunks", "ans_gpu_independent_pop_chunks",
           "ans_gpu_independent_push_var_chunks", "ans_gpu_independent_pop_var_chunks"]


def test_resume_entries_exported_and_declared():
    with open(os.path.join(ROOT, "include", "ans_capi.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert name in A.SIGNATURES, name
        assert getattr(A.lib(), name) is not None
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, re.M)
        assert decl, f"{name} is not declared in ans_capi.h"
        assert len(decl.group(1).split(",")) == len(A.SIGNATURES[name][1]), f"{name}: argument count"


def test_resume_entries_refuse_null_handle():
    total = ctypes.c_uint64(7)
    for name in ENTRIES:
        args = [0 if t in (A.u64, A.ci) else None for t in A.SIGNATURES[name][1]]
        if name.startswith("ans_gpu_"):
            args[-1] = ctypes.byref(total)
        assert getattr(A.lib(), name)(*args) == A.ANS_E_ARG, name


def _bare_tableset():
    """A GpuTableSet without a device: every check under test raises before the handle is used
    (a call that got through would meet the library's NULL-handle check, not a device)."""
    ts = A.GpuTableSet.__new__(A.GpuTableSet)
    ts.h = None
    return ts


def _arg_error(fn, *args, code=A.ANS_E_ARG):
    with pytest.raises(A.AnsError) as e:
        fn(*args)
    assert e.value.code == code


def test_resume_wrappers_check_argument_lengths():
    ts = _bare_tableset()
    data = np.zeros(40, np.uint8)
    offs, lens = np.array([0, 20], np.uint64), np.array([20, 20], np.uint64)
    syms, tids = np.zeros(32, np.uint8), np.zeros(32, np.uint32)
    _arg_error(ts.push_chunks, tids[:31], syms, 16, data, offs, lens)        # a table id per symbol
    _arg_error(ts.push_chunks, tids, syms, 0, data, offs, lens)              # chunk_len
    _arg_error(ts.push_chunks, tids, syms, 8, data, offs, lens)              # 4 chunks, 2 messages
    _arg_error(ts.push_chunks, tids, syms, 16, data, offs, lens[:1])         # offsets and lens differ
    _arg_error(ts.push_chunks, tids, syms, 16, data, offs, np.array([20, 21], np.uint64), code=A.ANS_E_LEN)
    _arg_error(ts.pop_chunks, tids, data, offs, lens, 0)
    _arg_error(ts.pop_chunks, tids, data, offs[:1], lens[:1], 16)
    _arg_error(ts.pop_chunks, tids, data[:39], offs, lens, 16, code=A.ANS_E_LEN)
    starts = np.array([0, 10, 32], np.uint64)
    _arg_error(ts.push_var_chunks, tids, syms, starts[:2], data, offs[:1], lens[:1])   # starts end at 10, not 32
    _arg_error(ts.push_var_chunks, tids, syms, np.array([0, 33, 32]), data, offs, lens)  # not rising
    _arg_error(ts.push_var_chunks, tids, syms, np.array([1, 10, 32]), data, offs, lens)  # not from 0
    _arg_error(ts.push_var_chunks, tids, syms, starts, data, offs[:1], lens[:1])       # 2 chunks, 1 message
    _arg_error(ts.pop_var_chunks, tids, data, offs, lens, starts[:2])
    _arg_error(ts.pop_var_chunks, tids, data, offs, lens, np.zeros(0, np.uint64))
    _arg_error(ts.pop_var_chunks, tids, data, offs[:1], lens[:1], starts)


def test_gpu_graphs_encode_checks_label_lengths():
    """With a node codec every graph needs num_nodes node labels, with an edge-label codec one
    label per edge (ans_capi.h section 5b: the library reads that many)."""
    gg = A.GpuGraphs.__new__(A.GpuGraphs)
    gg.node_cat, gg.edge_cat = object(), object()
    edges = np.array([[0, 1], [1, 2]])
    for graph in [(3, [0, 1], edges, [0, 1]), (3, None, edges, [0, 1]), (3, [0, 1, 2, 0], edges, [0, 1]),
                  (3, [0, 1, 2], edges, [0]), (3, [0, 1, 2], edges, None), (3, [0, 1, 2], edges, [0, 1, 1])]:
        _arg_error(gg.encode, [(3, [0, 1, 2], edges, [0, 1]), graph])


# ---- the fast encoder's resume arithmetic (csrc/ans_resume.hpp) against the oracle, with g++
CSRC = os.path.join(ROOT, "shuffle-coding_amd", "csrc")
ORC_DIR = os.path.join(ROOT, "oracle", "build")

CHECKER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "ans_resume.hpp"
using namespace shuffle_coding::resume;
extern "C" {
void* orc_msg_unflatten(const uint8_t*, uint64_t, int, uint64_t);
void orc_msg_free(void*);
uint64_t orc_msg_flatten(void*, uint8_t*, uint64_t);
void* orc_cat_new(const uint64_t*, uint32_t);
int orc_cat_push(void*, void*, uint64_t);
}

int main(int argc, char** argv) {
    std::mt19937_64 R(2024);
    // tables: norm 2^16, the file's (C3's), norm 2^31, and one below 2^16
    std::vector<std::vector<uint64_t>> tables;
    tables.push_back(std::vector<uint64_t>(256, 256));
    std::vector<uint64_t> c3;
    FILE* f = fopen(argv[1], "r");
    for (unsigned long long v; f && fscanf(f, "%llu", &v) == 1;) c3.push_back(v);
    if (c3.size() != 256) return 2;
    tables.push_back(c3);
    tables.push_back(std::vector<uint64_t>(128, 1ull << 24));
    tables.push_back({3, 5});
    tables.push_back({1, (1ull << 31) - 2});  // p = 1: the smallest bound, four bytes re-emitted
    const int per = atoi(argv[2]);
    long n = 0, shorts = 0, bad = 0;
    for (const auto& masses : tables) {
        uint64_t norm = 0;
        std::vector<uint64_t> cdf;
        for (uint64_t m : masses) { cdf.push_back(norm); norm += m; }
        const uint64_t K = kFull / norm;
        void* cat = orc_cat_new(masses.data(), (uint32_t)masses.size());
        for (int it = 0; it < per; ++it) {
            const uint32_t len = 8 + R() % 13, zeros = (R() % 4 == 0) ? R() % 4 : 0;
            std::vector<uint8_t> b(len + 16);
            for (uint32_t i = 0; i < len; ++i) b[i] = (uint8_t)R();
            for (uint32_t i = 0; i < zeros; ++i) b[len - 1 - i] = 0;
            if (R() % 8 == 0) b[len - 1 - zeros] = 1;  // a small top byte: the eighth byte is needed
            const uint64_t x = R() % masses.size(), p = masses[x], pK = p * K;
            // the reference: unflatten (Empty tail), push, flatten
            void* m = orc_msg_unflatten(b.data(), len, 1, 0);
            const int rc = orc_cat_push(m, cat, x);
            uint8_t want[64];
            const uint64_t wl = orc_msg_flatten(m, want, sizeof want);
            orc_msg_free(m);
            // the fast encoder: prologue to 2^56, the push's renorm_down, the update, flatten
            uint32_t pos = len;
            uint64_t head = pull_to_full(b.data(), pos);
            ++n;
            if (head < kFull) {  // left to the exact kernel: fewer than eight significant bytes
                uint32_t sig = len;
                while (sig && b[sig - 1] == 0) --sig;
                if (pos != 0 || sig >= 8) { ++bad; printf("short lane with %u significant bytes\n", sig); }
                ++shorts;
                continue;
            }
            const uint32_t fp = first_open_page(pos);
            if (rc != 0 || head < pK || (pos && (64 * fp + 1 > pos || pos > 64 * fp + 64)) || (!pos && fp)) {
                ++bad;
                printf("precondition: rc %d head %llx pK %llx pos %u fp %u\n", rc, (unsigned long long)head,
                       (unsigned long long)pK, pos, fp);
                continue;
            }
            while ((head >> 8) >= pK) { b[pos++] = (uint8_t)head; head >>= 8; }  // src/ans.rs:246-253
            head = norm * (head / p) + cdf[x] + head % p;                        // src/ans.rs:101-104
            while (head >> 8) { b[pos++] = (uint8_t)head; head >>= 8; }          // flatten
            b[pos++] = (uint8_t)head;
            bool same = pos == wl;
            for (uint32_t i = 0; same && i < pos; ++i) same = b[i] == want[i];
            if (!same) {
                if (bad < 5) printf("bytes differ: norm %llu p %llu len %u\n", (unsigned long long)norm, (unsigned long long)p, len);
                ++bad;
            }
        }
    }
    printf("checked %ld short %ld bad %ld\n", n, shorts, bad);
    return bad != 0;
}
"""


def test_resume_prologue_matches_oracle_push(tmp_path):
    """ans_resume.hpp with g++: pulling to 2^56 and then the first push (renorm_down, update,
    flatten) gives the oracle's unflatten + push + flatten, over 10^5 messages of 8-20 bytes (random,
    zero bytes on top) and tables of norm 2^16, C3's, 2^31 and below 2^16; a head short of 2^56
    only for messages of fewer than eight significant bytes (the exact kernel's)."""
    src, exe, masses = tmp_path / "resume_check.cpp", tmp_path / "resume_check", tmp_path / "c3.txt"
    src.write_text(CHECKER)
    masses.write_text(" ".join(str(int(m)) for m in A.c3_masses()))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", CSRC, str(src), "-o", str(exe), "-L", ORC_DIR,
                           "-lans_oracle", "-Wl,-rpath," + ORC_DIR])
    out = subprocess.run([str(exe), str(masses), "20000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    line = out.stdout.strip().splitlines()[-1].split()
    assert line[0] == "checked" and int(line[1]) == 100000 and line[-1] == "0", out.stdout
    assert 0 < int(line[3]) < 5000, out.stdout
