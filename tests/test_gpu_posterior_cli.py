"""-m gpu: word confidences through the C++ mirror -- wfst-decode --nbest=3 --nbest-word-times --word-confidence=1,0.1 and
--align-words=FILE --word-confidence, in the batch shape, with --batch=4 (GpuBatchDecoder::WordConfidences) and with --single-stream
(GpuLatticeDecoder::WordConfidences on a private decoder): the lines equal what the Python binding's word_confidences says for the same
words on the same utterances, and without the flag every line is what it is without this feature.

The tool prints the doubles with 9 significant digits (%.9g).  A value d.dddddddd x 10^e is rounded by at most half a unit of its
ninth digit, 5e-9 x 10^e, which is at most 5e-9 of the value itself (the worst case is a mantissa just above 1).  Beside that the
sums' free order leaves a rounding of the order of 1e-13 (the derived tolerance of tests/test_gpu_posterior.py on lattices of this
size); 1e-12 covers it."""
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
SOURCES = [(0, 22), (1, 20), (11, 17), (9, 22), (6, 12), (4, 21)]   # (utterance, frames): tests/test_gpu_align_cli.py's
N = 3


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    tmp = tmp_path_factory.mktemp("postcli")
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


def run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.splitlines()


def near(text, value):
    return abs(float(text) - float(value)) <= 5e-9 * abs(float(value)) + 1e-12


def strip(line):
    """a line without what --word-confidence adds to it: the conf column of a word line, logpost= of a path line"""
    f = line.split()
    if "#" in line and "notfound" not in line:
        f = f[:-1]
    return " ".join(x for x in f if not x.startswith("logpost="))


def check_words(lines, head, words, a):
    got = [l for l in lines if l.startswith(head + "#")]
    assert len(got) == len(words), head
    for j, (l, w, b, e, c) in enumerate(zip(got, words, a["begin"], a["end"], a["conf"])):
        f = l[len(head):].split()
        assert f[:4] == ["#%d" % (j + 1), str(w), str(b), str(e)] and len(f) == 5 and near(f[4], c) and 0.0 <= float(f[4]) <= 1.0, l


@pytest.mark.parametrize("shape", [[], ["--batch=4"], ["--single-stream"]])
def test_nbest_word_confidences_equal_the_binding(world, shape):
    plain = run(world["head"] + shape + ["--nbest=%d" % N, "--nbest-word-times"] + world["tail"])
    lines = run(world["head"] + shape + ["--nbest=%d" % N, "--nbest-word-times", "--word-confidence=1,0.1"] + world["tail"])
    assert [strip(l) for l in lines] == plain    # without the flag: byte for byte today's lines
    n_words = 0
    for i in range(world["n"]):
        key = "utt%03d" % i
        paths = [(l.split()[0], [int(x) for x in l.split()[1:]]) for l in plain if l.split()[0].startswith(key + "-") and "#" not in l.split()[0]]
        assert paths, key
        res = world["dec"].word_confidences([[w for _, w in paths]], [i], graph_scale=1.0, acoustic_scale=0.1)[0]
        for (head, w), a in zip(paths, res):
            assert a["found"], "an n-best path's words are in the raw lattice"
            line = [l for l in lines if l.split()[0] == head]
            assert len(line) == 1 and line[0].split()[-1].startswith("logpost=") and near(line[0].split()[-1][8:], a["path_logpost"]), head
            check_words(lines, head, w, a)
            n_words += len(w)
    assert n_words >= 6


@pytest.mark.parametrize("shape", [[], ["--batch=4"], ["--single-stream"]])
def test_align_words_file_with_confidences_equals_the_binding(world, shape):
    plain = run(world["head"] + shape + ["--align-words=" + world["align_file"]] + world["tail"])
    lines = run(world["head"] + shape + ["--align-words=" + world["align_file"], "--word-confidence"] + world["tail"])
    assert [strip(l) if " align " in l else l for l in lines] == plain
    res = world["dec"].word_confidences(world["asked"])
    n_found = n_absent = 0
    for i, (seqs, answers) in enumerate(zip(world["asked"], res)):
        for q, (s, a) in enumerate(zip(seqs, answers)):
            head = "utt%03d align %d" % (i, q + 1)
            line = [l for l in lines if l.startswith(head + " ")]
            assert len(line) == 1 and line[0].startswith("%s found=%d arcs=%d tot=%.9g lm=%.9g" % (head, a["found"], a["n_arcs"], a["tot"], a["lm"])), head
            if a["found"]:
                assert near(line[0].split()[-1][8:], a["path_logpost"]) and line[0].split()[-1].startswith("logpost="), head
                check_words(lines, head, s, a)
                n_found += 1
            else:
                assert "logpost" not in line[0] and not [l for l in lines if l.startswith(head + "#")]
                n_absent += 1
    assert n_found >= world["n"] and n_absent >= world["n"]
