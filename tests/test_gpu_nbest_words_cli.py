"""-m gpu: the n-best text through the C++ mirror -- wfst-decode --chunk=10 --partial-nbest=3 in --single-stream mode
(GpuLatticeDecoder::GetNbestWords on a private decoder), with --threads=4 --pool=4 (the GpuChannelPool request kind kNbestWords: one
wfst_decoder_get_nbest_words per batcher pass and question) and in the batch shape (GpuBatchDecoder::GetNbestWords): the lines
"KEY@frames nbest k: words... tot=.. lm=.." equal, line for line, a replay through the Python binding."""
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
SOURCES = [(0, 22), (1, 20), (11, 17), (9, 22), (6, 12), (4, 21)]   # (utterance, frames): tests/test_gpu_nbest_words.py says why so short
CHUNK, N = 10, 3


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    tmp = tmp_path_factory.mktemp("nbwcli")
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
    # the replay: every utterance on a channel of its own, chunk by chunk, one list call for the channels still running
    W = G.wfstdec
    graph = W.Graph.load(gp)
    graph.set_tid2pdf(m)
    dec = W.BatchDecoder(graph, G.gpu_config(CD), len(mats), max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
    dev = G.upload(mats)
    dec.init()
    want = {}
    T = [x.shape[0] for x in mats]
    for upto in range(CHUNK, max(T), CHUNK):
        dec.advance([t.data_ptr() for t in dev], [min(upto, t) for t in T], 300)
        live = [c for c in range(len(mats)) if upto < T[c]]
        for c, (status, paths) in zip(live, dec.nbest_words(N, channels=live, use_final_probs=False)):
            assert status == 0 and paths
            want[(c, upto)] = ["utt%03d@%d nbest %d:%s tot=%.9g lm=%.9g" % (c, upto, k + 1, "".join(" %d" % w for w in p["words"]), p["tot"], p["lm"])
                               for k, p in enumerate(paths)]
    dec.free()
    graph.free()
    lines = [l for c in range(len(mats)) for upto in range(CHUNK, T[c], CHUNK) for l in want[(c, upto)]]
    head = [CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin"), "--chunk=%d" % CHUNK, "--partial-nbest=%d" % N]
    tail = [str(tmp / "decoder.conf"), gp, str(tmp / "ll.bin")]
    return head, tail, lines


def _nbest_lines(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [l for l in p.stdout.splitlines() if " nbest " in l], p.stdout


@pytest.mark.parametrize("shape", [["--single-stream"], ["--threads=4", "--pool=4"]])
def test_cli_partial_nbest_equals_the_binding(world, shape):
    head, tail, want = world
    got, out = _nbest_lines(head + shape + tail)
    assert len(want) >= 2 * 6 and got == want   # utterance by utterance, chunk by chunk, path by path
    assert sum(1 for l in out.splitlines() if l.split() and l.split()[0].startswith("utt") and "@" not in l.split()[0]) == len(SOURCES)   # the final results follow


def test_cli_partial_nbest_batch_shape(world):
    head, tail, want = world
    got, _ = _nbest_lines(head + ["--batch=4"] + tail)   # (two batches; within one the lines come chunk by chunk)
    assert sorted(got) == sorted(want)


def test_the_flag_needs_its_chunks(world):
    head, tail, _ = world
    p = subprocess.run([CLI, "--partial-nbest=3", "--single-stream"] + tail, capture_output=True, text=True)
    assert p.returncode == 1 and "--partial-nbest=K" in p.stderr
