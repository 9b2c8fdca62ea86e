"""-m gpu: wfst-decode --graph-post=DIR [--graph-post-class=..] [--graph-post-scales=..] [--graph-post-out=FILE] (the host mirror's
GraphPosteriors over wfst_decoder_graph_posteriors) in the batch shape and --single-stream, against the Python binding on the same
utterances and graphs to the printed digits, and the tool's other output with and without the flags, byte for byte."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import graph_post_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
N_TID = 600
FRAMES = [50, 21, 3, 33]
LINE = re.compile(r"^(\S+) graph-post found=([01]) loglike=(\S+) frames=(\d+) entries=(\d+)$")
SCALES = (0.8, 1.25)


@pytest.fixture(scope="module")
def setup(synth, tmp_path_factory):
    import gpu_util as G

    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    tmp = tmp_path_factory.mktemp("gpost_cli")
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    gpath = str(tmp / "g.bin")
    g.write(gpath)
    m = np.asarray(synth.default_tid2pdf(N_TID), np.int32)
    m.astype("<i4").tofile(str(tmp / "tid2pdf.bin"))
    (tmp / "decoder.conf").write_text("--beam=12\n--max-active=1000000\n--min-active=0\n--lattice-beam=5\n--prune-interval=10\n")
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=900 + i, mu=-2.2)[0] for i, T in enumerate(FRAMES)]
    # every utterance's own graph: transcripts, and a chain that does not fit its three frames
    graphs = [U.transcript_graph(range(1, 6), seed=60, n_tid=N_TID), U.transcript_graph(range(1, 4), seed=61, n_tid=N_TID),
              U.chain_graph([(7, 1, 0.5)] * 5), U.transcript_graph(range(1, 9), seed=63, n_tid=N_TID, bypass=True)]
    os.mkdir(tmp / "graphs")
    with open(tmp / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = "utt%03d" % i
            f.write(struct.pack("<i", len(key)) + key.encode() + struct.pack("<ii", x.shape[0], x.shape[1]) + x.tobytes())
            graphs[i].write(str(tmp / "graphs" / (key + ".fst")))
    W = G.wfstdec
    graph = W.Graph.load(gpath)
    graph.set_tid2pdf(m)
    dec = W.BatchDecoder(graph, G.gpu_config(dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=5.0, prune_interval=10)), len(mats),
                         max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20)
    ag = W.AlignGraphs.load([str(tmp / "graphs" / ("utt%03d.fst" % i)) for i in range(len(mats))])
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], FRAMES, N_TID // 2)
        dec.finalize()
        want = {"tid": dec.graph_posteriors(ag), "pdf": dec.graph_posteriors(ag, label_map=m, graph_scale=SCALES[0], acoustic_scale=SCALES[1])}
        for i in range(len(mats)):
            U.compare(want["tid"][i], U.graph_posteriors(graphs[i], mats[i], None, m), "binding utt%03d" % i)
    finally:
        ag.free()
        dec.free()
        graph.free()
    return dict(tmp=tmp, gpath=gpath, want=want)


def run(setup, *flags):
    tmp = setup["tmp"]
    p = subprocess.run([CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin")] + list(flags) + [str(tmp / "decoder.conf"), setup["gpath"], str(tmp / "ll.bin")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p


@pytest.mark.parametrize("shape,flags,cls", [("batch", [], "tid"), ("single", ["--single-stream"], "pdf")])
def test_the_tool_against_the_binding(shape, flags, cls, setup):
    plain = run(setup, *flags).stdout
    lists = str(setup["tmp"] / ("lists_%s.txt" % shape))
    extra = ["--graph-post-class=pdf", "--graph-post-scales=%g,%g" % SCALES] if cls == "pdf" else []
    p = run(setup, "--graph-post=" + str(setup["tmp"] / "graphs"), "--graph-post-out=" + lists, *extra, *flags)
    lines = p.stdout.splitlines(keepends=True)
    mine = [l for l in lines if LINE.match(l.rstrip("\n"))]
    # the other output is what it is without the flags, byte for byte
    assert "".join(l for l in lines if l not in mine) == plain and len(plain.splitlines()) == len(FRAMES) and "graph-post" not in plain
    assert len(mine) == len(FRAMES)
    rows = open(lists).read().splitlines()
    assert len(rows) == len(FRAMES)
    n_found = n_entries = 0
    for i in range(len(FRAMES)):
        w = setup["want"][cls][i]
        key, found, ll, frames, entries = LINE.match(mine[i].rstrip("\n")).groups()
        assert key == "utt%03d" % i and int(found) == int(w.found) and w.status == 0
        assert ll == "%.9g" % w.log_like and int(frames) == w.n_frames and int(entries) == w.n_entries
        # the lists, in --frame-post's format
        assert rows[i].split()[0] == key
        per_frame = re.findall(r"\[([^\]]*)\]", rows[i])
        assert len(per_frame) == w.n_frames
        for f, body in enumerate(per_frame):
            tok = body.split()
            lo, hi = int(w.frame_off[f]), int(w.frame_off[f + 1])
            assert [int(x) for x in tok[0::2]] == w.classes[lo:hi].tolist()
            assert tok[1::2] == ["%.9g" % x for x in w.posts[lo:hi]]
        n_found += int(found)
        n_entries += int(entries)
    assert n_found == len(FRAMES) - 1 and n_entries > 100
    print("%s: %d utterances found, %d entries compared" % (shape, n_found, n_entries))


def test_usage_errors(setup):
    for flags in (["--graph-post-class=pdf"], ["--graph-post=/nowhere", "--graph-post-class=word"], ["--graph-post=/nowhere", "--graph-post-class=pdf"],
                  ["--graph-post=/nowhere", "--threads=2"], ["--graph-post=/nowhere", "--graph-post-scales=-1,1"], ["--graph-post-out=x"]):
        p = subprocess.run([CLI] + flags + ["a", "b", "c"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "graph-post" in p.stderr, flags
