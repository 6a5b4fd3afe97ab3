"""The per-graph states of graph shuffle coding with Weisfeiler-Lehman orbits behind a checked accessor
(tests/native/wl_state_check.cpp): the templates the kernels of ans_wl.hip run, for both slice
models, wl_iter 0 .. 3 and both settings of the half iteration, on one workspace of fixed bounds (40
nodes, 200 pairs) reused for every graph and full of junk before every push and every pop, as a
lane's entries of the device workspace are.  Built with ASan + UBSan and run as its own process.  No
access may fall outside its region, and no entry may be read that the current call has not written;
run again with every region declared one entry short, the same program has to report the overruns,
or its zero would prove nothing.  CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, E, K = 40, 200, 4  # max_nodes, max_edges, the levels at wl_iter = 3 (the sizes the summary shows)
ORBIT = dict(ids=2 * K * N, ord=N, inv=N, dirty=N, stamp=N, sort=2 * N)
SLICE = dict(urn=N, sl=N, s_ord=N, rop=N, por=N, s_ids=2 * N, s_orb=N)
CSR = dict(pos_of=N, node_at=N, off=N + 1, nbr=2 * E)
ADJ = dict(head=N, next=2 * E, deg=N)
SIZES = {}
for state, parts in (("er_push", (CSR, dict(mark=N), ORBIT)), ("er_pop", (ADJ, ORBIT)),
                     ("pu_push", (CSR, SLICE, ORBIT)), ("pu_pop", (ADJ, dict(SLICE, por=11), ORBIT))):
    for part in parts:
        SIZES.update({f"{state}.{name}": size for name, size in part.items()})
# the dword counts include/ans_capi.h section 5f states, at wl_iter = 3
O = (2 * K + 4 + 2) * N
assert sum(v for k, v in SIZES.items() if k.startswith("er_push.")) == 4 * N + 2 * E + 1 + O
assert sum(v for k, v in SIZES.items() if k.startswith("er_pop.")) == 2 * N + 2 * E + O
assert sum(v for k, v in SIZES.items() if k.startswith("pu_push.")) == 11 * N + 2 * E + 1 + O
assert sum(v for k, v in SIZES.items() if k.startswith("pu_pop.")) == 9 * N + 11 + 2 * E + O
SETTINGS = 8   # wl_iter 0 .. 3 x the half iteration, per model
NAMED = 14     # the named shapes of a setting


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wl_state") / "wl_state_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "shuffle-coding_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "wl_state_check.cpp"), "-o", str(exe)])

    def run(*args):
        # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
                   UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-4000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("wl_state_check:")]
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


def test_no_access_out_of_range_and_no_stale_read(checker):
    totals, regions = checker()
    # the inputs: 3,000 random graphs and the named shapes under each model and setting, each followed
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
    for name, size in SIZES.items():
        assert regions[name]["size"] == size - 1, name
        assert regions[name]["oob"] > 0, name
    assert totals["oob"] == sum(r["oob"] for r in regions.values())
    assert totals["stale"] == 0 and totals["roundtrip_fail"] == 0  # (the entries exist: the codec still works)
