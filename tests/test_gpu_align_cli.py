"""-m gpu: word times for n-best paths and given transcripts through the C++ mirror -- wfst-decode --nbest=3 --nbest-word-times and
--align-words=FILE, in the batch shape (GpuBatchDecoder::AlignWords) and with --single-stream (GpuLatticeDecoder::GetNbestWordTimes on
a private decoder): the lines equal what the Python binding's align_words says for the same words on the same utterances."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_compose_lattice import _setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
CD = dict(beam=11.0, max_active=7000, min_active=0, lattice_beam=6.0, prune_interval=10)
SOURCES = [(0, 22), (1, 20), (11, 17), (9, 22), (6, 12), (4, 21)]   # (utterance, frames): short enough for the determinizer (tests/test_gpu_nbest_words.py)
N = 3


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    tmp = tmp_path_factory.mktemp("aligncli")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    g, m, gp, p1, p2, lls = _setup(synth, tmp, 0)
    lls = lls + [synth.make_loglikes(g, 40, 300, m, seed=2950 + u, mu=-2.2)[0] for u in range(9)]
    mats = [np.ascontiguousarray(lls[u][:t]) for u, t in SOURCES]
    m.astype("<i4").tofile(str(tmp / "tid2pdf.bin"))
    (tmp / "decoder.conf").write_text("--beam=11\n--max-active=7000\n--min-active=0\n--lattice-beam=6\n--prune-interval=10\n")
    with open(tmp / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = ("utt%03d" % i).encode()
            f.write(struct.pack("<i", len(key)) + key + struct.pack("<ii", x.shape[0], x.shape[1]) + x.tobytes())
    W = G.wfstdec
    graph = W.Graph.load(gp)
    graph.set_tid2pdf(m)
    dec = W.BatchDecoder(graph, G.gpu_config(CD), len(mats), max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
    dev = G.upload(mats)
    dec.init()
    dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], 300)
    dec.finalize()
    best = [w[0] for w in dec.words()]
    # --align-words: per utterance its best path's words, those words without the first, and a sequence the lattice cannot hold
    asked = [[list(map(int, w)), list(map(int, w[1:])), [100000]] for w in best]
    with open(tmp / "align.txt", "w") as f:
        for i, seqs in enumerate(asked):
            for s in seqs:
                f.write("utt%03d%s\n" % (i, "".join(" %d" % x for x in s)))
    head = [CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin")]
    tail = [str(tmp / "decoder.conf"), gp, str(tmp / "ll.bin")]
    yield dict(dec=dec, head=head, tail=tail, asked=asked, align_file=str(tmp / "align.txt"), n=len(mats))
    dec.free()
    graph.free()


def word_lines(head, words, a):
    if not a["found"]:
        return [head + " notfound"]
    return ["%s#%d %d %d %d" % (head, j + 1, w, b, e) for j, (w, b, e) in enumerate(zip(words, a["begin"], a["end"]))]


def run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.splitlines()


@pytest.mark.parametrize("shape", [[], ["--batch=4"], ["--single-stream"]])
def test_nbest_word_times_equal_the_binding(world, shape):
    plain = run(world["head"] + shape + ["--nbest=%d" % N] + world["tail"])
    lines = run(world["head"] + shape + ["--nbest=%d" % N, "--nbest-word-times"] + world["tail"])
    assert [l for l in lines if "#" not in l.split()[0] and "notfound" not in l] == plain   # the other lines are unchanged
    n_words = 0
    for i in range(world["n"]):
        key = "utt%03d" % i
        paths = [(l.split()[0], [int(x) for x in l.split()[1:]]) for l in plain if l.split()[0].startswith(key + "-")]
        assert paths, key
        al = world["dec"].align_words([[w for _, w in paths]], [i])[0]
        for (head, w), a in zip(paths, al):
            assert a["found"], "an n-best path's words are in the raw lattice"
            got = [l for l in lines if l.split()[0].startswith(head + "#")]
            assert got == word_lines(head, w, a), head
            n_words += len(w)
    assert n_words >= 6


@pytest.mark.parametrize("shape", [[], ["--batch=4"], ["--single-stream"]])
def test_align_words_file_equals_the_binding(world, shape):
    plain = run(world["head"] + shape + world["tail"])
    lines = run(world["head"] + shape + ["--align-words=" + world["align_file"]] + world["tail"])
    assert [l for l in lines if " align " not in l] == plain
    al = world["dec"].align_words(world["asked"])
    want = []
    for i, (seqs, res) in enumerate(zip(world["asked"], al)):
        for q, (s, a) in enumerate(zip(seqs, res)):
            head = "utt%03d align %d" % (i, q + 1)
            want.append("%s found=%d arcs=%d tot=%.9g lm=%.9g" % (head, a["found"], a["n_arcs"], a["tot"], a["lm"]))
            if a["found"]:
                want += word_lines(head, s, a)
    got = [l for l in lines if " align " in l]
    assert sorted(got) == sorted(want)
    assert sum("found=1" in l for l in got) >= world["n"] and sum("found=0" in l for l in got) >= world["n"]
