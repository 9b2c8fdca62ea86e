"""-m gpu: the one-wave-per-lattice determinizer (asr-decoder_amd/csrc/wfst_determinize_wave.h) AT ITS EDGES -- the constructed
lattices of tests/det_edge_util.py (one per named branch: window pricing, the commit rules, the closure's capacities, the state-id
packing, pairs and subsets, normalize, subset matching within delta, the trie's claims and its first-table retry, refusals), through
the development harness tools/det_bench.hip built twice at the product's sizes: plain, and with -DDETW_COUNT, where every lattice's
line ends in the wave's branch counters.  Each build runs ONCE over all the files.

  (a) every lattice is the host build's in both builds -- state count, arc multiset bit for bit (the host build is held against the
      reference's determinizer on these very lattices by tests/test_det_edge_lattices.py);
  (b) from the counted build, every case's named counters moved and the counters it must keep away from stayed 0: a case that no
      longer reaches its branch fails loudly;
  (c) the two builds print the same states, arcs, error code and trie count per lattice: the counters change nothing.

Refusals: with a workspace so small that the host build refuses, the device must refuse with the host's code (3: output states,
5: output arcs).  No such parity is asserted for the trie (code 1): the wave prices queue entries ahead of their turn, and an entry
that turns out stale leaves trie nodes behind that the sequential build never makes -- its node count may legitimately exceed the
host's, so the lattice that outgrows the first table must come back equal to the host's, or with code 1, nothing else.

Seconds on an MI355X: the two compiles and the two runs 16 (each run 5, four of them the host build and the workspace of the two
lattices of 2^21 states; no lattice takes the device more than 15 ms), the three decoder-driven tests 1.9 (the first loads the
library), 0.01 and 0.12."""
import os
import re
import subprocess
import time

import pytest

import det_edge_util as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = [c.name for c in E.cases()]
LINE = re.compile(r"^\s+(\S+)\s+S\s+(\d+) A\s+(\d+) -> (?:REFUSED host_err (\d+) )?states\s+(-?\d+) arcs\s+(-?\d+) err (\d+) trie\s+(-?\d+)\s+alone ([\d.]+) ms\s+(OK|MISMATCH)?")


def parse(stdout):
    """{case name: dict(host_err, states, arcs, err, trie, ms, verdict, cnt {name: value})}"""
    out = {}
    for line in stdout.splitlines():
        m = LINE.match(line)
        if not m:
            continue
        name = os.path.basename(m.group(1))[:-4]
        cnt = {}
        if " | cnt:" in line:
            cnt = {k: int(v) for k, v in (kv.split("=") for kv in line.split(" | cnt:")[1].split())}
        out[name] = dict(host_err=int(m.group(4) or 0), states=int(m.group(5)), arcs=int(m.group(6)), err=int(m.group(7)), trie=int(m.group(8)),
                         ms=float(m.group(9)), verdict=m.group(10), cnt=cnt)
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("detw_edges")
    argv = []
    for c in E.cases():
        p = str(tmp / (c.name + ".bin"))
        E.write_bin(p, c.lat)
        argv += c.args + [p] + (["--cap-states", "0", "--cap-arcs", "0"] if c.args else [])
    src = os.path.join(ROOT, "tools", "det_bench.hip")
    inc = os.path.join(ROOT, "asr-decoder_amd", "csrc")
    exes = {}
    for tag, defs in (("plain", []), ("counted", ["-DDETW_COUNT"])):
        exes[tag] = str(tmp / ("det_bench_" + tag))
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", inc, "-o", exes[tag], src] + defs, timeout=600)
    res = {}
    for tag in ("plain", "counted"):   # each build once, over all files in one process; a run that did not end normally is the last
        t0 = time.time()
        p = subprocess.run([exes[tag], "--variant", "1", "--reps", "0", "--expect-err"] + argv, capture_output=True, text=True, timeout=120)
        print("%s build: %.1f s" % (tag, time.time() - t0))
        print(p.stdout)
        assert p.returncode in (0, 1), (tag, p.returncode, p.stdout[-1500:], p.stderr[-1500:])
        res[tag] = parse(p.stdout)
        assert sorted(res[tag]) == sorted(NAMES), (tag, sorted(set(NAMES) ^ set(res[tag])), p.stderr[-1500:])
    return res


@pytest.mark.parametrize("name", NAMES)
def test_lattice_is_the_host_builds_and_its_branch_ran(runs, name):
    c = next(x for x in E.cases() if x.name == name)
    plain, counted = runs["plain"][name], runs["counted"][name]
    # (c) the counters change nothing
    for k in ("host_err", "states", "arcs", "err", "trie", "verdict"):
        assert plain[k] == counted[k], (name, k, plain[k], counted[k])
    assert plain["ms"] < 1000.0 and counted["ms"] < 1000.0, (name, plain["ms"], counted["ms"])   # well under a second each
    if c.refuse is not None:
        # the host build refused with this code: so must the device (codes 3 and 5 -- see the module's docstring for code 1)
        for r in (plain, counted):
            assert r["host_err"] == c.refuse and r["err"] == c.refuse, (name, r)
        return
    if name == "trie_outgrows_the_first_table":
        for r in (plain, counted):
            assert r["host_err"] == 0 and (r["verdict"] == "OK" or r["err"] == 1), (name, r)
    else:
        # (a) the host build's lattice
        for r in (plain, counted):
            assert r["host_err"] == 0 and r["err"] == 0 and r["verdict"] == "OK", (name, r)
    # (b) the branch the lattice was built for ran; the branch it must keep away from did not
    cnt = counted["cnt"]
    for k, (op, v) in sorted(c.want.items()):
        assert k in cnt, (name, k)
        assert (cnt[k] == v) if op == "==" else (cnt[k] >= v), (name, k, op, v, cnt[k], cnt)
    assert not plain["cnt"]


def test_the_retry_gave_the_hosts_lattice(runs):
    """the harness's copy of the first-table retry (16 slots per raw state, then the whole table): the second attempt ran, once, and
    the lattice is the host's -- on this machine's run, not merely "or err 1" """
    r = runs["counted"]["trie_outgrows_the_first_table"]
    assert r["cnt"]["trie_retry"] == 1 and r["trie"] > E.TRIE_FIRST // 2
    assert r["err"] in (0, 1)
    assert r["err"] == 1 or r["verdict"] == "OK"


@pytest.mark.parametrize("shape", E.DECODER_SHAPES)
def test_the_products_own_csr_build_and_retry(shape, synth, tmp_path):
    """determinize_kernel has its own CSR build (Invert, ArcSort by (word, target, transition-id, cost)) and its own copy of the
    first-table retry; the harness above runs neither.  Three hand-built graphs through a real BatchDecoder with a beam that prunes
    nothing (tests/test_det_edge_lattices.py proves their lattices' shapes from the oracle): a lattice state with 70 word-less
    out-arcs, two strings that keep more than kDwLabs labels behind a shared one, and a chain whose trie outgrows the first table
    of a lattice of at most 256 states -- a broken retry would come back "workspace exceeded", or with a wrong lattice.  Against the
    host build on the device's raw lattice, and the reference where built."""
    import gpu_util as G
    import pyoracle
    from test_gpu_determinize import _check_against, _ref_or_none

    t0 = time.time()
    g, ll, facts = E.decoder_shape(synth, shape)
    gp = str(tmp_path / "g.bin")
    g.write(gp)
    graph = G.wfstdec.Graph.load(gp)
    T = int(ll.shape[0])
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(E.DECODER_CFG), 1, max_frames=T + 8, max_tokens_per_frame=4096, arena_tokens=1 << 16, lattice_links=1 << 15)
    try:
        dev = G.upload([ll])
        dec.init()
        dec.advance([dev[0].data_ptr()], [T], int(ll.shape[1]))
        dec.finalize()
        raw = dec.raw_lattice(0)
        assert raw is not None
        from test_gpu_lattice import as_raw

        for what, got, claimed in facts(as_raw(raw)):
            assert got == claimed, (what, got, claimed)
        D = _check_against(G, dec, 0, raw, pyoracle.build_det_host(), _ref_or_none(), tmp_path, shape)   # (a refusal raises: status 0 or no lattice)
        assert D is not None and D.n_states > 0
    finally:
        dec.free()
        graph.free()
    print("%s: %.2f s" % (shape, time.time() - t0))
