"""-m gpu: pruned live lattices through the C++ mirror -- wfst-decode --chunk=25 --partial-nbest=3 --live-lattice-prune in
--single-stream mode (GpuLatticeDecoder::SetLiveLatticePrune on a private decoder), with --threads=4 --pool=4 (the same call over a
GpuChannelPool: the shared decoder's mode) and in the batch shape
(GpuBatchDecoder::SetLiveLatticePrune): the lines "KEY@frames nbest k: words... tot=.. lm=.." equal, line for line, what the Python
binding's mode-1 nbest_words gives at the same frames.  The flag without --partial-nbest is a usage error."""
import os
import struct
import subprocess

import numpy as np
import pytest

from live_prune_util import LENGTHS, LIM, config, small_graph, utterances

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
CHUNK, N = 25, 3


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    tmp = tmp_path_factory.mktemp("lpcli")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    g, m, gp = small_graph(synth, tmp)
    mats = [np.ascontiguousarray(x) for x in utterances(synth, g, m)]
    m.astype("<i4").tofile(str(tmp / "tid2pdf.bin"))
    (tmp / "decoder.conf").write_text("--beam=11\n--max-active=1000000\n--min-active=0\n--lattice-beam=7\n--prune-interval=25\n")
    with open(tmp / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = ("utt%03d" % i).encode()
            f.write(struct.pack("<i", len(key)) + key + struct.pack("<ii", x.shape[0], x.shape[1]) + x.tobytes())
    # the replay: every utterance on a channel of its own, chunk by chunk, one mode-1 list call for the channels still running
    W = G.wfstdec
    graph = W.Graph.load(gp)
    graph.set_tid2pdf(m)
    dec = W.BatchDecoder(graph, G.gpu_config(config(7.0)), len(mats), **LIM)
    dec.set_live_lattice_prune(True)
    dev = G.upload(mats)
    dec.init()
    want = {}
    for upto in range(CHUNK, max(LENGTHS), CHUNK):
        dec.advance([t.data_ptr() for t in dev], [min(upto, t) for t in LENGTHS], int(mats[0].shape[1]))
        live = [c for c in range(len(mats)) if upto < LENGTHS[c]]
        for c, (status, paths) in zip(live, dec.nbest_words(N, channels=live, use_final_probs=False)):
            assert status == 0 and paths, (c, upto, status)
            want[(c, upto)] = ["utt%03d@%d nbest %d:%s tot=%.9g lm=%.9g" % (c, upto, k + 1, "".join(" %d" % w for w in p["words"]), p["tot"], p["lm"])
                               for k, p in enumerate(paths)]
    dec.free()
    graph.free()
    lines = [l for c in range(len(mats)) for upto in range(CHUNK, LENGTHS[c], CHUNK) for l in want[(c, upto)]]
    head = [CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin"), "--chunk=%d" % CHUNK, "--partial-nbest=%d" % N]
    tail = [str(tmp / "decoder.conf"), gp, str(tmp / "ll.bin")]
    return head, tail, lines


def _nbest_lines(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [l for l in p.stdout.splitlines() if " nbest " in l], p.stdout


@pytest.mark.parametrize("shape", [["--single-stream"], ["--threads=4", "--pool=4"]])
def test_cli_single_stream_and_pool_equal_the_bindings_mode_1(world, shape):
    """--threads/--pool: GpuLatticeDecoder::SetLiveLatticePrune over a GpuChannelPool sets the shared decoder's mode in the batcher thread"""
    head, tail, want = world
    got, out = _nbest_lines(head + ["--live-lattice-prune"] + shape + tail)
    assert len(want) >= 7 and got == want   # utterance by utterance, chunk by chunk, path by path (7 questions: at frame 25 of four streams, at 50 of three)
    assert sum(1 for l in out.splitlines() if l.split() and l.split()[0].startswith("utt") and "@" not in l.split()[0]) == len(LENGTHS)   # the final results follow


def test_cli_batch_shape_equals_the_bindings_mode_1(world):
    head, tail, want = world
    got, _ = _nbest_lines(head + ["--live-lattice-prune", "--batch=4"] + tail)
    assert sorted(got) == sorted(want)


def test_the_flag_needs_partial_nbest(world):
    head, tail, _ = world
    p = subprocess.run([CLI, "--chunk=%d" % CHUNK, "--live-lattice-prune", "--single-stream"] + tail, capture_output=True, text=True)
    assert p.returncode == 1 and "--live-lattice-prune goes with" in p.stderr
