"""The per-graph states of graph shuffle coding with node and edge labels behind a checked accessor
(tests/native/labelled_state_check.cpp): the templates the kernels of ans_wl_labelled.hip run, for the
four label policies, both slice models, wl_iter 0 .. 3 and both settings of the half iteration, on one
workspace of fixed bounds (40 nodes, 200 pairs) reused for every graph and full of junk before every
push and every pop, as a lane's entries of the device workspace are.  Built with ASan + UBSan and run
as its own process.  No access may fall outside its region, no entry may be read that the current call
has not written, every region's last entry is used (the declared dword counts are tight), and a
node's popped pairs come ascending; run again with every region declared one entry short, the same
program has to report the overruns, or its zero would prove nothing.  CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, E, K = 40, 200, 4  # max_nodes, max_edges, the levels at wl_iter = 3 (the sizes the summary shows)
SLICE = dict(urn=N, sl=N, s_ord=N, rop=N, por=N, s_ids=2 * N, s_orb=N)
CSR = dict(pos_of=N, node_at=N, off=N + 1, nbr=2 * E)
ADJ = dict(head=N, next=2 * E, deg=N)
POLICIES = {"ne": (True, True), "n": (True, False), "e": (False, True), "none": (False, False)}
SIZES, STATES = {}, {}
for tag, (node, edge) in POLICIES.items():
    orbit = dict(ids=2 * K * N, ord=N, inv=N, dirty=N, stamp=N, sort=(3 if edge else 2) * N)
    labels = dict(elab=2 * E if edge else 0, spos=N if edge else 0, slab=N if edge else 0) if node or edge else {}
    for state, parts in (("er_push", (CSR, dict(mark=N), orbit, labels)), ("er_pop", (ADJ, orbit)),
                         ("pu_push", (CSR, SLICE, orbit, labels)), ("pu_pop", (ADJ, dict(SLICE, por=11), orbit))):
        for part in parts:
            SIZES.update({f"{tag}.{state}.{name}": size for name, size in part.items()})
    # the dword counts include/ans_capi.h sections 5f and 5g state, at wl_iter = 3
    o = (2 * K + 4 + 2 + (1 if edge else 0)) * N
    more = 2 * E + 2 * N if edge else 0

    def total(state):
        return sum(v for k, v in SIZES.items() if k.startswith(f"{tag}.{state}."))
    assert total("er_push") == 4 * N + 2 * E + 1 + o + more
    assert total("er_pop") == 2 * N + 2 * E + o
    assert total("pu_push") == 11 * N + 2 * E + 1 + o + more
    assert total("pu_pop") == 9 * N + 11 + 2 * E + o
SETTINGS = 8   # wl_iter 0 .. 3 x the half iteration, per model
NAMED = 10     # the named shapes of a setting
RANDOM = 1500  # 600 graphs under both labels, 300 under each other policy


def _states(name):
    """The settings under which a region exists and is used: the sort scratch is absent at wl_iter = 0
    without edge labels, and with them serves the half iteration alone there."""
    tag, _, region = name.split(".")
    edge = POLICIES[tag][1]
    if SIZES[name] == 0:
        return 0
    if region == "sort":
        return SETTINGS - (1 if edge else 2)
    return SETTINGS


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("labelled_state") / "labelled_state_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "shuffle-coding_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "labelled_state_check.cpp"), "-o", str(exe)])

    def run(*args):
        # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
                   UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, out.stderr[-4000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("labelled_state_check:")]
        assert len(lines) == 1, out.stdout[-2000:]
        print(lines[0][:2000])
        return _parse(lines[0])

    return run


def _parse(line):
    totals = {k: int(v) for k, v in re.findall(r" (\w+)=(\d+)", line.split(" ne.er_push.pos_of:")[0])}
    regions = {}
    for name, fields in re.findall(r" ([\w.]+):(\S+)", line):
        regions[name] = {k: int(v) for k, v in (f.split("=") for f in fields.split(","))}
    assert set(regions) == set(SIZES), line
    return totals, regions


def test_no_access_out_of_range_no_stale_read_and_tight_bounds(checker):
    totals, regions = checker()
    # the inputs: random graphs and the named shapes under each policy, model and setting, each
    # followed by a pop of foreign bytes
    assert totals["graphs"] == RANDOM and totals["named"] == len(POLICIES) * 2 * SETTINGS * NAMED
    hostile = totals["hostile"]
    assert hostile == totals["graphs"] + totals["named"]
    assert totals["hostile_ok"] + totals["exhausted"] + totals["len"] + totals["symbol"] == hostile
    assert totals["hostile_bad"] == 0
    assert totals["hostile_ok"] > 0 and totals["exhausted"] > 0 and totals["len"] > 0
    # what is checked
    assert totals["roundtrip_fail"] == 0
    assert totals["order_bad"] == 0  # v ascending, within v w ascending, as the pop gave them
    assert totals["oob"] == 0 and totals["stale"] == 0, regions
    assert totals["unfilled"] == 0, regions  # every region's last entry was used under every setting
    for name, size in SIZES.items():
        r = regions[name]
        assert r["size"] == size, name
        assert r["oob"] == 0 and r["stale"] == 0 and r["unfilled"] == 0, name
        assert r["states"] == _states(name), name


def test_a_region_one_entry_short_is_reported(checker):
    totals, regions = checker("--short")
    for name, size in SIZES.items():
        assert regions[name]["size"] == max(size - 1, 0), name
        assert (regions[name]["oob"] > 0) == (size > 0), name
    assert totals["oob"] == sum(r["oob"] for r in regions.values())
    assert totals["stale"] == 0 and totals["roundtrip_fail"] == 0  # (the entries exist: the codec still works)
