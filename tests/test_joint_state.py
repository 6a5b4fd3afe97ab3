"""The per-graph states of joint shuffle coding of graphs behind a checked accessor
(tests/native/joint_state_check.cpp): the templates the kernels of ans_joint.hip run, for both ordered
codecs, wl_iter 0 .. 3, both settings of the half iteration and of the urn's redraws, on one workspace of
fixed bounds (40 nodes, 200 pairs) reused for every graph and full of junk before every push and every
pop, as a lane's entries of the device workspace are.  The ordered urn's arrays lie over the orbit
stage's; a read of an entry the current call has not written is what a wrong overlap shows as.  Built
with ASan + UBSan and run as its own process.  No access may fall outside its region, and no entry may be
read that the current call has not written; run again with every region declared one entry short, the
same program has to report the overruns, or its zero would prove nothing.  CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, E, K = 40, 200, 4  # max_nodes, max_edges, the levels at wl_iter = 3 (the sizes the summary shows)
ORBIT = dict(ids=2 * K * N, ord=N, inv=N, dirty=N, stamp=N, sort=2 * N)
CSR = dict(pos_of=N, node_at=N, off=N + 1, nbr=2 * E)
ADJ = dict(head=N, next=2 * E, deg=N)


def _urn(push):
    return dict(u_urn=N + 1, u_orb=E + 1, u_ord=E, u_rop=E, u_por=E if push else 11, u_head=N, u_next=2 * E)


SIZES = {}
for state, parts in (("er_push", (CSR, ORBIT, dict(scr=N))), ("er_pop", (ADJ, ORBIT)),
                     ("pu_push", (CSR, ORBIT, dict(scr=N), _urn(True))), ("pu_pop", (ADJ, ORBIT, _urn(False)))):
    for part in parts:
        SIZES.update({f"{state}.{name}": size for name, size in part.items()})
OVER = (".scr", ".u_")  # the regions that lie over others: they add nothing to a state's dwords


def _own(state):
    return sum(v for k, v in SIZES.items() if k.startswith(state + ".") and not any(o in k for o in OVER))


def _urn_dwords(state):
    return sum(v for k, v in SIZES.items() if k.startswith(state + ".u_"))


# the dword counts include/ans_capi.h section 5h states, at wl_iter = 3
O = (2 * K + 6) * N
U_PUSH, U_POP = 2 * N + 6 * E + 2, 2 * N + 5 * E + 2 + min(E, 11)
assert _own("er_push") == 3 * N + 2 * E + 1 + O
assert _own("er_pop") == 2 * N + 2 * E + O
assert _own("pu_push") == 3 * N + 2 * E + 1 + O and _urn_dwords("pu_push") == U_PUSH
assert _own("pu_pop") == 2 * N + 2 * E + O and _urn_dwords("pu_pop") == U_POP
SETTINGS = 8   # wl_iter 0 .. 3 x the half iteration, per codec
NAMED = 34     # the 17 named shapes of a setting, each under both settings of redraws


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("joint_state") / "joint_state_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "shuffle-coding_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "joint_state_check.cpp"), "-o", str(exe)])

    def run(*args):
        # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
                   UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-4000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("joint_state_check:")]
        assert len(lines) == 1, out.stdout[-2000:]
        print(lines[0])
        return _parse(lines[0])

    return run


def _parse(line):
    totals = {k: int(v) for k, v in re.findall(r" (\w+)=(\d+)", line.split(" er_push.pos_of:")[0])}
    regions = {}
    for name, fields in re.findall(r" ([\w.]+):(\S+)", line):
        regions[name] = {k: int(v) for k, v in (f.split("=") for f in fields.split(","))}
    assert set(regions) == set(SIZES), line
    return totals, regions


def test_the_published_dword_counts_are_the_headers():
    """ans_joint.hpp's *_entries (which the checker holds against what make() takes, or exits with 2) as
    include/ans_capi.h section 5h states them, at every wl_iter."""
    src = r"""
#include <cstdio>
#include "ans_joint.hpp"
namespace jt = shuffle_coding::joint;
int main() {
    for (unsigned w = 0; w < 4; ++w)
        std::printf("%llu %llu %llu %llu\n", (unsigned long long)jt::er_push_entries(40, 200, w),
                    (unsigned long long)jt::er_pop_entries(40, 200, w), (unsigned long long)jt::pu_push_entries(40, 200, w),
                    (unsigned long long)jt::pu_pop_entries(40, 200, w));
    std::printf("%llu %llu\n", (unsigned long long)jt::pu_push_entries(300, 10, 3), (unsigned long long)jt::pu_pop_entries(300, 10, 3));
}
"""
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        with open(os.path.join(t, "entries.cpp"), "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "shuffle-coding_amd", "csrc"),
                               os.path.join(t, "entries.cpp"), "-o", os.path.join(t, "entries")])
        rows = [[int(v) for v in ln.split()] for ln in subprocess.check_output([os.path.join(t, "entries")], text=True).splitlines()]

    def counts(n, e, w):
        o = (2 * (w + 1) + 6) * n if w else 5 * n + 1
        u_push, u_pop = 2 * n + 6 * e + 2, 2 * n + 5 * e + 2 + min(e, 11)
        return [3 * n + 2 * e + 1 + o, 2 * n + 2 * e + o, 3 * n + 2 * e + 1 + max(o, u_push), max(2 * n + 2 * e + o, u_pop)]

    assert rows[:4] == [counts(N, E, w) for w in range(4)]
    assert rows[4] == counts(300, 10, 3)[2:]  # (few pairs: the orbit stage is the larger of the two)


def test_no_access_out_of_range_and_no_stale_read(checker):
    totals, regions = checker()
    # the inputs: 3,000 random graphs and the named shapes under each codec and setting, each followed
    # by a pop of foreign bytes
    assert totals["graphs"] == 3000 and totals["named"] == 2 * SETTINGS * NAMED
    hostile = totals["hostile"]
    assert hostile == totals["graphs"] + totals["named"]
    assert totals["hostile_ok"] + totals["exhausted"] + totals["len"] + totals["symbol"] == hostile
    assert totals["hostile_bad"] == 0
    assert totals["hostile_ok"] > 0 and totals["exhausted"] > 0 and totals["len"] > 0
    # what is checked
    assert totals["roundtrip_fail"] == 0
    assert totals["oob"] == 0 and totals["stale"] == 0, regions
    assert totals["unfilled"] == 0, regions  # every region's last entry was used under every setting: the bounds are tight
    for name, size in SIZES.items():
        r = regions[name]
        assert r["size"] == size, name
        assert r["oob"] == 0 and r["stale"] == 0 and r["unfilled"] == 0, name
        assert r["states"] == (SETTINGS - 2 if name.endswith(".sort") else SETTINGS), name  # (no scratch at wl_iter = 0)


def test_a_region_one_entry_short_is_reported(checker):
    totals, regions = checker("--short")
    spare = (".u_urn", ".u_orb")  # (one entry more than they use, as the ordered urn's own state: never overrun)
    for name, size in SIZES.items():
        assert regions[name]["size"] == size - 1, name
        if not name.endswith(spare):
            assert regions[name]["oob"] > 0, name
    assert totals["oob"] == sum(r["oob"] for r in regions.values())
    assert totals["stale"] == 0 and totals["roundtrip_fail"] == 0  # (the entries exist: the codec still works)
