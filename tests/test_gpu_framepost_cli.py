"""-m gpu: wfst-decode --frame-post=FILE (the host mirror's FramePosteriors over wfst_decoder_frame_posteriors) in its three shapes --
the batch decoder over all utterances at once, --batch=4 and --single-stream -- against the Python binding on the same
utterances, and the tool's other output with and without the flag, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
N_TID = 600
FRAMES = [50, 21, 3, 33, 40]


def parse(text):
    """Kaldi's text posteriors: {key: [[(class, post), ...] per frame]}"""
    out = {}
    for line in text.strip().splitlines():
        key, _, rest = line.partition(" ")
        frames = []
        for chunk in rest.split("]")[:-1]:
            tok = chunk.replace("[", " ").split()
            assert len(tok) % 2 == 0, line[:200]
            frames.append([(int(tok[i]), float(tok[i + 1])) for i in range(0, len(tok), 2)])
        out[key] = frames
    return out


@pytest.fixture(scope="module")
def setup(synth, tmp_path_factory):
    import gpu_util as G

    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    tmp = tmp_path_factory.mktemp("framepost_cli")
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    gpath = str(tmp / "g.bin")
    g.write(gpath)
    m = np.asarray(synth.default_tid2pdf(N_TID), np.int32)
    m.astype("<i4").tofile(str(tmp / "tid2pdf.bin"))
    phone = ((np.arange(N_TID + 1, dtype=np.int32) - 1) // 12 + 1).astype(np.int32)
    phone[0] = 0
    phone.astype("<i4").tofile(str(tmp / "tid2phone.bin"))
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
        want = dict(tid=dec.frame_posteriors(), pdf=dec.frame_posteriors(label_map=m),
                    phone=dec.frame_posteriors(label_map=phone, graph_scale=1.0, acoustic_scale=0.1, min_post=0.01))
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


def against(got, want, what):
    assert sorted(got) == ["utt%03d" % i for i in range(len(FRAMES))], what
    n = 0
    for i in range(len(FRAMES)):
        frames, w = got["utt%03d" % i], want[i]
        assert w["status"] == 0 and len(frames) == w["n_frames"] == FRAMES[i], (what, i)
        for f, lst in enumerate(frames):
            a, b = w["frame_off"][f], w["frame_off"][f + 1]
            assert [c for c, _ in lst] == w["classes"][a:b].tolist(), (what, i, f)
            # nine significant digits in the file (5e-9 relative); the order of a sum is each launch's own
            assert np.allclose([x for _, x in lst], w["posts"][a:b], rtol=1e-8, atol=1e-12), (what, i, f)
            n += len(lst)
    return n


SHAPES = dict(batch=[], batch4=["--batch=4"], single=["--single-stream"])
_PLAIN = {}   # shape -> the tool's output without the flag


@pytest.mark.parametrize("cls", ["tid", "pdf", "phone"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_tool_against_the_binding(shape, cls, setup):
    tmp = setup["tmp"]
    flags = SHAPES[shape]
    if shape not in _PLAIN:
        _PLAIN[shape] = run(setup, *flags).stdout
    extra = dict(tid=[], pdf=["--frame-post-class=pdf"],
                 phone=["--frame-post-class=phone", "--tid2phone=" + str(tmp / "tid2phone.bin"), "--frame-post-scales=1,0.1", "--frame-post-min=0.01"])[cls]
    out = str(tmp / ("post_%s_%s.txt" % (shape, cls)))
    p = run(setup, "--frame-post=" + out, *(flags + extra))
    # the other output is what it was, byte for byte
    assert p.stdout == _PLAIN[shape] and len(p.stdout.splitlines()) == len(FRAMES)
    n = against(parse(open(out).read()), setup["want"][cls], "%s %s" % (shape, cls))
    assert n > 300
    print("%s %s: %d entries compared" % (shape, cls, n))
