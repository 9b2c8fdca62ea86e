"""-m gpu: the lattice path nearest a transcript through the C++ mirror -- wfst-decode --nearest-words=FILE in the batch shape
(GpuBatchDecoder::NearestWords) and with --single-stream (GpuLatticeDecoder::NearestWords on a private decoder): the lines equal what
the Python binding's nearest_words says for the same references on the same utterances, and the closing line sums them."""
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


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    tmp = tmp_path_factory.mktemp("nearestcli")
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
    best = [[int(x) for x in w[0]] for w in dec.words()]
    # per utterance: its best path's words, those words with a word the lattice cannot hold in front, without their first, and no word
    asked = [[w, [100000] + w, w[1:], []] for w in best]
    with open(tmp / "refs.txt", "w") as f:
        for i, refs in enumerate(asked):
            for s in refs:
                f.write("utt%03d%s\n" % (i, "".join(" %d" % x for x in s)))
    head = [CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin")]
    tail = [str(tmp / "decoder.conf"), gp, str(tmp / "ll.bin")]
    yield dict(dec=dec, head=head, tail=tail, asked=asked, refs_file=str(tmp / "refs.txt"), n=len(mats))
    dec.free()
    graph.free()


def run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.splitlines()


@pytest.mark.parametrize("shape", [[], ["--batch=4"], ["--single-stream"]])
def test_nearest_words_file_equals_the_binding(world, shape):
    plain = run(world["head"] + shape + world["tail"])
    lines = run(world["head"] + shape + ["--nearest-words=" + world["refs_file"]] + world["tail"])
    assert [l for l in lines if not l.startswith("nearest ") and " nearest " not in l] == plain   # the other lines are unchanged
    res = world["dec"].nearest_words(world["asked"])
    want, tot = [], dict(err=0, words=0, ins=0, dele=0, sub=0)
    for i, (refs, answers) in enumerate(zip(world["asked"], res)):
        for q, (ref, a) in enumerate(zip(refs, answers)):
            assert a["found"] and a["status"] == 0
            head = "utt%03d nearest %d" % (i, q + 1)
            want.append("%s err=%d cor=%d sub=%d ins=%d del=%d arcs=%d tot=%.9g lm=%.9g" % (head, a["n_err"], a["n_cor"], a["n_sub"], a["n_ins"],
                                                                                           a["n_del"], a["n_arcs"], a["tot"], a["lm"]))
            want += ["%s#%d %d %d %d" % (head, j + 1, w, b, e) for j, (w, b, e) in enumerate(zip(a["hyp_words"], a["begin"], a["end"]))]
            tot["err"] += a["n_err"]; tot["words"] += len(ref); tot["ins"] += a["n_ins"]; tot["dele"] += a["n_del"]; tot["sub"] += a["n_sub"]
    got = [l for l in lines if " nearest " in l]
    assert sorted(got) == sorted(want)
    assert sum(" err=0 " in l for l in got) >= world["n"] and sum(" err=1 " in l for l in got) >= world["n"]
    assert lines[-1] == "nearest %%WER %.2f [ %d / %d, %d ins, %d del, %d sub ]" % (100.0 * tot["err"] / tot["words"], tot["err"], tot["words"],
                                                                                   tot["ins"], tot["dele"], tot["sub"])
    assert tot["err"] >= world["n"]
