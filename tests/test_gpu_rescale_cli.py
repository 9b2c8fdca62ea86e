"""-m gpu: wfst-decode --rescale=GS,AS,WIP[:...] (the host mirror's RescaledWords over wfst_decoder_rescaled_words) in its three
shapes -- the batch decoder over all utterances at once, --batch=4 and --single-stream -- against the Python binding on the same
utterances, and the tool's other output with and without the flag, byte for byte."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
N_TID = 600
FRAMES = [50, 21, 3, 33, 40]
SETTINGS = [(1.0, 1.0, 0.0), (1.0, 0.1, 0.5), (0.0, 0.0, 0.0), (1.0, 1.0, -3.0), (0.5, 1.0, 2.25)]
FLAG = "--rescale=" + ":".join("%r,%r,%r" % s for s in SETTINGS)
LINE = re.compile(r"^(\S+) rescale (\d+) gs=(\S+) as=(\S+) wip=(\S+) found=([01]) cost=(\S+) tot=(\S+) lm=(\S+) :(.*)$")


@pytest.fixture(scope="module")
def setup(synth, tmp_path_factory):
    import gpu_util as G

    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    tmp = tmp_path_factory.mktemp("rescale_cli")
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    gpath = str(tmp / "g.bin")
    g.write(gpath)
    m = np.asarray(synth.default_tid2pdf(N_TID), np.int32)
    m.astype("<i4").tofile(str(tmp / "tid2pdf.bin"))
    (tmp / "decoder.conf").write_text("--beam=12\n--max-active=1000000\n--min-active=0\n--lattice-beam=5\n--prune-interval=10\n")
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=900 + i, mu=-2.2)[0] for i, T in enumerate(FRAMES)]
    with open(tmp / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = ("utt%03d" % i).encode()
            f.write(struct.pack("<i", len(key)) + key + struct.pack("<ii", x.shape[0], x.shape[1]) + x.tobytes())
    # the binding's answer on the same utterances
    W = G.wfstdec
    graph = W.Graph.load(gpath)
    graph.set_tid2pdf(m)
    dec = W.BatchDecoder(graph, G.gpu_config(dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=5.0, prune_interval=10)), len(mats),
                         max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], FRAMES, N_TID // 2)
        dec.finalize()
        want = dec.rescaled_words(SETTINGS)
    finally:
        dec.free()
        graph.free()
    return dict(tmp=tmp, gpath=gpath, want=want)


def run(setup, *flags):
    tmp = setup["tmp"]
    p = subprocess.run([CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin")] + list(flags) + [str(tmp / "decoder.conf"), setup["gpath"], str(tmp / "ll.bin")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p


@pytest.mark.parametrize("shape,flags", [("batch", []), ("batch4", ["--batch=4"]), ("single", ["--single-stream"])])
def test_the_tool_against_the_binding(shape, flags, setup):
    plain = run(setup, *flags).stdout
    p = run(setup, FLAG, *flags)
    lines = p.stdout.splitlines(keepends=True)
    mine = [l for l in lines if LINE.match(l.rstrip("\n"))]
    # the other output is what it is without the flag, byte for byte
    assert "".join(l for l in lines if l not in mine) == plain and len(plain.splitlines()) == len(FRAMES) and " rescale " not in plain
    assert len(mine) == len(FRAMES) * len(SETTINGS)
    seen, n_words = set(), 0
    for l in mine:
        key, q, gs, as_, wip, found, cost, tot, lm, rest = LINE.match(l.rstrip("\n")).groups()
        i, q = int(key[3:]), int(q) - 1
        w = setup["want"][i][q]
        seen.add((i, q))
        assert (float(gs), float(as_), float(wip)) == SETTINGS[q] and int(found) == int(w["found"]) and w["status"] == 0, l
        assert float(cost) == w["scaled_cost"], "seventeen digits: the float64 itself"
        assert np.float32(float(tot)) == w["tot"] and np.float32(float(lm)) == w["lm"], l
        words = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"(\d+)\((\d+),(\d+)\)", rest)]
        assert len(words) == len(rest.split()) == w["n_hyp"], l
        assert [x[0] for x in words] == w["hyp_words"].tolist() and [x[1] for x in words] == w["begin"].tolist() and [x[2] for x in words] == w["end"].tolist(), l
        n_words += len(words)
    assert len(seen) == len(mine) and n_words > 20
    print("%s: %d lines, %d words compared" % (shape, len(mine), n_words))
