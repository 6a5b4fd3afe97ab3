"""The per-graph states of the autoregressive Pólya urn codecs behind a checked accessor
(tests/native/arpu_state_check.cpp): the templates the kernels of ans_arpu.hip run, on one workspace
of fixed bounds (40 nodes, 200 pairs) reused for every graph and full of junk before every push and
every pop, as a lane's entries of the device workspace are.  Built with ASan + UBSan and run as its
own process.  No access may fall outside its region, and no entry may be read that the current call
has not written; run again with every region declared one entry short, the same program has to
report the overruns, or its zero would prove nothing.  CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = dict(sl=40, ord=40, rop=40, por=40, ids=80, orb=40)  # the slice scratch: 7 * 40
# max_nodes 40, max_edges 200: push 13 * 40 + 2 * 200 + 2 entries, pop 9 * 40 + 11 + 1 over the first of
# them (the joint layer's pop does not read por: a plain slice's 11 entries)
SIZES = dict(pos_of=40, node_at=40, off=41, nbr=400, urn=40, **SLICE, rk=40, cnt=41,
             pop_urn=40, **{"pop_" + k: v for k, v in SLICE.items()}, deg=40, pop_cnt=41)
SIZES["pop_por"] = 11
REGIONS = tuple(SIZES)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("arpu_state") / "arpu_state_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "shuffle-coding_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "arpu_state_check.cpp"), "-o", str(exe)])

    def run(*args):
        # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
                   UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-4000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("arpu_state_check:")]
        assert len(lines) == 1, out.stdout[-2000:]
        print(lines[0])
        return _parse(lines[0])

    return run


def _parse(line):
    totals = {k: int(v) for k, v in re.findall(r" (\w+)=(\d+)", line.split(" pos_of:")[0])}
    regions = {}
    for name, fields in re.findall(r" (\w+):(\S+)", line):
        regions[name] = {k: int(v) for k, v in (f.split("=") for f in fields.split(","))}
    assert tuple(regions) == REGIONS, line
    return totals, regions


def test_no_access_out_of_range_and_no_stale_read(checker):
    totals, regions = checker()
    # the inputs: a few thousand random graphs and the named shapes under each orbits value
    assert totals["graphs"] == 3000 and totals["named"] == 3 * 19
    hostile = totals["hostile"]
    assert hostile == totals["graphs"] + totals["named"]  # one pop of foreign bytes after each graph
    assert totals["hostile_ok"] + totals["exhausted"] + totals["len"] + totals["symbol"] == hostile
    assert totals["hostile_bad"] == 0
    assert totals["hostile_ok"] > 0 and totals["exhausted"] > 0 and totals["len"] > 0 and totals["symbol"] > 0
    # what is checked
    assert totals["roundtrip_fail"] == 0
    assert totals["oob"] == 0 and totals["stale"] == 0 and totals["rank_oob"] == 0, regions
    for name in REGIONS:
        assert regions[name]["size"] == SIZES[name], name
        assert regions[name]["oob"] == 0 and regions[name]["stale"] == 0, name
        assert regions[name]["highest"] == SIZES[name] - 1, name  # the bounds are tight


def test_a_region_one_entry_short_is_reported(checker):
    totals, regions = checker("--short")
    for name in REGIONS:
        assert regions[name]["size"] == SIZES[name] - 1, name
        assert regions[name]["oob"] > 0, name
    assert totals["oob"] == sum(r["oob"] for r in regions.values())
    assert totals["stale"] == 0 and totals["roundtrip_fail"] == 0  # (the entries exist: the codec still works)
