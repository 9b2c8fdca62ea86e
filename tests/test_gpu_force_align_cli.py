"""-m gpu: wfst-decode --force-align=DIR [--force-align-class=..] (the host mirror's ForceAlign over wfst_decoder_force_align) in its
three shapes -- the batch decoder over all utterances at once, --batch=4 and --single-stream -- against the Python binding on the
same utterances and graphs, and the tool's other output with and without the flag, byte for byte."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import force_align_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
N_TID = 600
FRAMES = [50, 21, 3, 33, 40]
LINE = re.compile(r"^(\S+) forced found=([01]) cost=(\S+) ali=(.*)$")
WORDS = re.compile(r"^(\S+) forced-words(.*)$")


@pytest.fixture(scope="module")
def setup(synth, tmp_path_factory):
    import gpu_util as G

    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    tmp = tmp_path_factory.mktemp("falign_cli")
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    gpath = str(tmp / "g.bin")
    g.write(gpath)
    m = np.asarray(synth.default_tid2pdf(N_TID), np.int32)
    m.astype("<i4").tofile(str(tmp / "tid2pdf.bin"))
    (tmp / "decoder.conf").write_text("--beam=12\n--max-active=1000000\n--min-active=0\n--lattice-beam=5\n--prune-interval=10\n")
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=900 + i, mu=-2.2)[0] for i, T in enumerate(FRAMES)]
    # every utterance's own graph: transcripts, one in OpenFst's format, one that does not fit its three frames
    graphs = [U.transcript_graph(range(1, 6), seed=60, n_tid=N_TID), U.transcript_graph(range(1, 4), seed=61, n_tid=N_TID),
              U.chain_graph([(7, 1, 0.5)] * 5), U.transcript_graph(range(1, 9), seed=63, n_tid=N_TID, bypass=True),
              U.transcript_graph(range(1, 7), seed=64, n_tid=N_TID)]
    os.mkdir(tmp / "graphs")
    with open(tmp / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = "utt%03d" % i
            f.write(struct.pack("<i", len(key)) + key.encode() + struct.pack("<ii", x.shape[0], x.shape[1]) + x.tobytes())
            if i == 1:
                with open(tmp / "graphs" / (key + ".fst"), "wb") as gf:
                    gf.write(synth.to_openfst_bytes(graphs[i]))
            else:
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
        want = {"tid": dec.force_align(ag), "pdf": dec.force_align(ag, label_map=m)}
        for i in range(len(mats)):
            if i != 1:   # (the OpenFst file's arcs are numbered as the reader lays them out)
                U.compare(want["tid"][i], U.force_align(graphs[i], mats[i], None, m), "binding utt%03d" % i)
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


@pytest.mark.parametrize("shape,flags,cls", [("batch", [], "tid"), ("batch4", ["--batch=4"], "pdf"), ("single", ["--single-stream"], "tid")])
def test_the_tool_against_the_binding(shape, flags, cls, setup):
    plain = run(setup, *flags).stdout
    p = run(setup, "--force-align=" + str(setup["tmp"] / "graphs"), *(["--force-align-class=pdf"] if cls == "pdf" else []), *flags)
    lines = p.stdout.splitlines(keepends=True)
    mine = [l for l in lines if LINE.match(l.rstrip("\n")) or WORDS.match(l.rstrip("\n"))]
    # the other output is what it is without the flag, byte for byte
    assert "".join(l for l in lines if l not in mine) == plain and len(plain.splitlines()) == len(FRAMES) and " forced" not in plain
    assert len(mine) == 2 * len(FRAMES)
    n_found = n_words = 0
    for i in range(len(FRAMES)):
        w = setup["want"][cls][i]
        key, found, cost, ali = LINE.match(mine[2 * i].rstrip("\n")).groups()
        key2, rest = WORDS.match(mine[2 * i + 1].rstrip("\n")).groups()
        assert key == key2 == "utt%03d" % i and int(found) == int(w.found) and w.status == 0
        assert np.float32(float(cost)) == w.path_cost, "nine digits: the float32 itself"
        assert [int(x) for x in ali.split()] == w.alignment.tolist()
        words = [(int(a), int(b)) for a, b in re.findall(r"(\d+)@(\d+)", rest)]
        assert len(words) == len(rest.split()) == w.n_words
        assert [x[0] for x in words] == w.words.tolist() and [x[1] for x in words] == w.word_frame.tolist()
        n_found += int(found)
        n_words += len(words)
    assert n_found == len(FRAMES) - 1 and n_words > 10
    print("%s: %d utterances found, %d words compared" % (shape, n_found, n_words))


def test_usage_errors(setup):
    for flags in (["--force-align-class=pdf"], ["--force-align=/nowhere", "--force-align-class=word"], ["--force-align=/nowhere", "--force-align-class=pdf"],
                  ["--force-align=/nowhere", "--threads=2"]):
        p = subprocess.run([CLI] + flags + ["a", "b", "c"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "force-align" in p.stderr, flags
