"""-m gpu: sentence and phrase posteriors through the C++ mirror -- wfst-decode --sentence-posterior beside --nbest-word-times and
--align-words=FILE, and --phrase-posterior=FILE, in the batch shape, with --batch=4 (GpuBatchDecoder::SequencePosteriors) and with
--single-stream (GpuLatticeDecoder::SequencePosteriors on a private decoder): the lines equal what the Python binding's
sentence_posteriors / phrase_posteriors say for the same words on the same utterances, and without the new flags every line is what
it is without this feature.

The tool prints the doubles with 9 significant digits (%.9g): at most 5e-9 of the value itself; beside that the sums' free order
leaves a rounding of the order of 1e-13 on lattices of this size (tests/test_gpu_seqpost.py's derived tolerance); 1e-12 covers it."""
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

    tmp = tmp_path_factory.mktemp("seqpostcli")
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
    best = [list(map(int, w[0])) for w in dec.words()]
    asked = [[w, w[1:], [100000]] for w in best]
    # per utterance: every run of two words of its best path, its first word, and a word the graph does not have
    phrases = [[p for p in [w[j:j + 2] for j in range(len(w) - 1)] + [w[:1], [100000]] if p][:64] for w in best]
    for name, lists in (("align.txt", asked), ("phrases.txt", phrases)):
        with open(tmp / name, "w") as f:
            for i, seqs in enumerate(lists):
                for s in seqs:
                    f.write("utt%03d%s\n" % (i, "".join(" %d" % x for x in s)))
    head = [CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin")]
    tail = [str(tmp / "decoder.conf"), gp, str(tmp / "ll.bin")]
    yield dict(dec=dec, head=head, tail=tail, asked=asked, phrases=phrases, align_file=str(tmp / "align.txt"),
               phrase_file=str(tmp / "phrases.txt"), n=len(mats))
    dec.free()
    graph.free()


def run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.splitlines()


def near(text, value):
    return abs(float(text) - float(value)) <= 5e-9 * abs(float(value)) + 1e-12


def field(line, name):
    got = [x[len(name) + 1:] for x in line.split() if x.startswith(name + "=")]
    assert len(got) == 1, (name, line)
    return got[0]


def strip(lines):
    """the lines without what the new flags add: sentpost= of a path line, the phrase lines"""
    return [" ".join(x for x in l.split(" ") if not x.startswith("sentpost=")) for l in lines if " phrase " not in l]


@pytest.mark.parametrize("shape,scales", [([], (1.0, 0.1)), (["--batch=4"], (1.0, 0.1)), (["--single-stream"], (1.0, 0.1)), ([], None)])
def test_the_tool_equals_the_binding(world, shape, scales):
    dec = world["dec"]
    old = ["--nbest=%d" % N, "--nbest-word-times", "--align-words=" + world["align_file"]] + (["--word-confidence=%g,%g" % scales] if scales else [])
    gs, as_ = scales or (1.0, 1.0)
    plain = run(world["head"] + shape + old + world["tail"])
    lines = run(world["head"] + shape + old + ["--sentence-posterior", "--phrase-posterior=" + world["phrase_file"]] + world["tail"])
    assert strip(lines) == plain    # without the new flags: byte for byte today's lines
    assert not [l for l in plain if "sentpost=" in l or " phrase " in l]
    n_paths = n_found = n_absent = n_phrases = n_said = 0
    # the n-best paths
    for i in range(world["n"]):
        key = "utt%03d" % i
        paths = [(l.split()[0], [int(x) for x in l.split()[1:] if "=" not in x]) for l in lines if l.split()[0].startswith(key + "-") and "#" not in l.split()[0]]
        assert paths, key
        res = dec.sentence_posteriors([[w for _, w in paths]], [i], graph_scale=gs, acoustic_scale=as_)[0]
        for (head, w), a in zip(paths, res):
            line = [l for l in lines if l.split()[0] == head]
            assert a["found"] and len(line) == 1 and near(field(line[0], "sentpost"), a["logpost"]), head
            if scales:    # the posterior of all paths that spell the words is at least the aligned one's
                assert float(field(line[0], "sentpost")) >= float(field(line[0], "logpost")) - 1e-8, line[0]
            n_paths += 1
    # the sequences of the file
    res = dec.sentence_posteriors(world["asked"], graph_scale=gs, acoustic_scale=as_)
    for i, (seqs, answers) in enumerate(zip(world["asked"], res)):
        for q, a in enumerate(answers):
            head = "utt%03d align %d" % (i, q + 1)
            line = [l for l in lines if l.startswith(head + " ")]
            assert len(line) == 1 and ("found=%d" % a["found"]) in line[0], head
            if a["found"]:
                assert near(field(line[0], "sentpost"), a["logpost"]), head
                n_found += 1
            else:
                assert "sentpost" not in line[0]
                n_absent += 1
    # the phrases
    res = dec.phrase_posteriors(world["phrases"], graph_scale=gs, acoustic_scale=as_, hit_mass=True)
    for i, (seqs, answers) in enumerate(zip(world["phrases"], res)):
        for q, a in enumerate(answers):
            head = "utt%03d phrase %d " % (i, q + 1)
            line = [l for l in lines if l.startswith(head)]
            assert len(line) == 1 and field(line[0], "found") == "%d" % a["found"], head
            assert near(field(line[0], "count"), a["count"]) and near(field(line[0], "conf"), a["conf"]), line[0]
            peak = int(field(line[0], "peak"))
            if a["found"]:     # the lowest frame whose mass is the largest, up to the sums' rounding
                h = a["hit_mass"]
                assert 0 <= peak < len(h) and h[peak] >= h.max() - 1e-12 and (peak == 0 or h[:peak].max() <= h[peak] + 1e-12), line[0]
            else:
                assert peak == -1 and a["count"] == 0.0
            n_phrases += 1
            n_said += a["found"]
    assert n_paths >= world["n"] and n_found >= world["n"] and n_absent >= world["n"] and n_phrases >= 2 * world["n"] and n_said >= world["n"]


def test_the_flags_need_their_company(world):
    p = subprocess.run(world["head"] + ["--sentence-posterior"] + world["tail"], capture_output=True, text=True)
    assert p.returncode == 1 and "--sentence-posterior goes with --nbest-word-times or --align-words=FILE" in p.stderr
    p = subprocess.run(world["head"] + ["--threads=2", "--phrase-posterior=" + world["phrase_file"]] + world["tail"], capture_output=True, text=True)
    assert p.returncode == 1 and "--phrase-posterior goes with the batch shape or --single-stream" in p.stderr
