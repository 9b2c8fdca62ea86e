"""-m gpu: wfst-decode --seq-stats=FILE --seq-ref=FILE (the host mirror's SequenceStats over wfst_decoder_sequence_stats) in its two
shapes -- the batch decoder and --single-stream -- against the Python binding on the same utterances and references, and the tool's
other output with and without the flags, byte for byte."""
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
    """{key: ([[(class, value), ...] per frame], {name: number} of the seq-stats line)}"""
    lists, stats = {}, {}
    for line in text.strip().splitlines():
        key, _, rest = line.partition(" ")
        if rest.startswith("seq-stats "):
            stats[key] = dict(kv.split("=") for kv in rest.split()[1:])
            continue
        frames = []
        for chunk in rest.split("]")[:-1]:
            tok = chunk.replace("[", " ").split()
            assert len(tok) % 2 == 0, line[:200]
            frames.append([(int(tok[i]), float(tok[i + 1])) for i in range(0, len(tok), 2)])
        lists[key] = frames
    return lists, stats


@pytest.fixture(scope="module")
def setup(synth, tmp_path_factory):
    import gpu_util as G

    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    tmp = tmp_path_factory.mktemp("seqstat_cli")
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
    # the binding's answer on the same utterances and references
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
        tids = [np.asarray(b["tids"], np.int64) for b in dec.best_paths()]
        refs, sil = {}, {}
        for name, mp in (("pdf", m), ("phone", phone)):
            refs[name] = [mp[t].astype(np.int64) for t in tids]
            for r in refs[name]:
                r[::5] += 1          # every fifth frame changed
            refs[name][1] = refs[name][1][:10]     # a reference shorter than its utterance
            refs[name][2][1] = -1                  # an unlabelled frame
            with open(tmp / ("ref_%s.txt" % name), "w") as f:
                for i, r in enumerate(refs[name]):
                    if i != 3:                     # an utterance without a line is unlabelled throughout
                        f.write("utt%03d %s\n" % (i, " ".join(str(int(x)) for x in r)))
            refs[name][3] = np.zeros(0, np.int64)
        sil = sorted(set(int(x) for x in refs["pdf"][0][:8]))
        want = dict(smbr=dec.sequence_stats(refs["pdf"], criterion="smbr", label_map=m, sil_classes=sil),
                    mmi=dec.sequence_stats(refs["phone"], criterion="mmi", label_map=phone, graph_scale=1.0, acoustic_scale=0.1, drop_frames=True))
    finally:
        dec.free()
        graph.free()
    return dict(tmp=tmp, gpath=gpath, want=want, sil=sil)


def run(setup, *flags):
    tmp = setup["tmp"]
    p = subprocess.run([CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin")] + list(flags) + [str(tmp / "decoder.conf"), setup["gpath"], str(tmp / "ll.bin")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p


def against(got, want, crit, what):
    lists, stats = got
    assert sorted(lists) == sorted(stats) == ["utt%03d" % i for i in range(len(FRAMES))], what
    n = 0
    for i in range(len(FRAMES)):
        key = "utt%03d" % i
        frames, w, s = lists[key], want[i], stats[key]
        assert w["status"] == 0 and len(frames) == w["n_frames"] == FRAMES[i] == int(s["n_frames"]), (what, i)
        assert s["criterion"] == crit and int(s["n_ref_frames"]) == w["n_ref_frames"] and int(s["n_dropped"]) == w["n_dropped"], (what, i)
        # 17 digits in the file; the order of a sum is each launch's own
        assert abs(float(s["tot_acc"]) - w["tot_acc"]) <= 1e-9 and abs(float(s["log_z"]) - w["log_z"]) <= 1e-9 * max(1.0, abs(w["log_z"])), (what, i)
        for f, lst in enumerate(frames):
            a, b = w["frame_off"][f], w["frame_off"][f + 1]
            assert [c for c, _ in lst] == w["classes"][a:b].tolist(), (what, i, f)
            assert np.allclose([x for _, x in lst], w["values"][a:b], rtol=0, atol=1e-9), (what, i, f)
            n += len(lst)
    return n


SHAPES = dict(batch=[], single=["--single-stream"])
_PLAIN = {}   # shape -> the tool's output without the flags


@pytest.mark.parametrize("crit", ["smbr", "mmi"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_tool_against_the_binding(shape, crit, setup):
    tmp = setup["tmp"]
    flags = SHAPES[shape]
    if shape not in _PLAIN:
        _PLAIN[shape] = run(setup, *flags).stdout
    extra = dict(smbr=["--seq-ref=" + str(tmp / "ref_pdf.txt"), "--seq-class=pdf", "--seq-silence=" + ":".join(str(x) for x in setup["sil"])],
                 mmi=["--seq-ref=" + str(tmp / "ref_phone.txt"), "--seq-criterion=mmi", "--seq-class=phone", "--tid2phone=" + str(tmp / "tid2phone.bin"),
                      "--seq-scales=1,0.1", "--seq-drop-frames"])[crit]
    out = str(tmp / ("seq_%s_%s.txt" % (shape, crit)))
    p = run(setup, "--seq-stats=" + out, *(flags + extra))
    # the other output is what it was, byte for byte
    assert p.stdout == _PLAIN[shape] and len(p.stdout.splitlines()) == len(FRAMES)
    n = against(parse(open(out).read()), setup["want"][crit], crit, "%s %s" % (shape, crit))
    assert n > 300
    if crit == "mmi":
        assert sum(w["n_dropped"] for w in setup["want"]["mmi"]) > 0, "the changed frames' classes are outside the lattice somewhere"
    print("%s %s: %d entries compared" % (shape, crit, n))
