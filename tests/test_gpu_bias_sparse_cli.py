"""-m gpu: wfst-decode --bias=FILE through the sparse call (the host mirror's BiasBooks / BiasedWordsSparse over
wfst_decoder_biased_words_sparse): a file whose lists have 300 nodes is answered -- the dense call refuses such a list -- and equals
the Python binding; --bias-sparse on a 40-node file prints what the run without the flag prints, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_bias_cli import CLI, LINE, N_TID, compare

pytestmark = pytest.mark.gpu
FRAMES = [50, 21, 33]
SETTINGS = [(1.0, 1.0, 0.0, 1.0), (1.0, 0.1, 0.5, 4.0), (0.5, 1.0, 2.25, 30.0)]
FLAG = "--bias-settings=" + ":".join("%r,%r,%r,%r" % s for s in SETTINGS)


@pytest.fixture(scope="module")
def setup(synth, tmp_path_factory):
    import gpu_util as G

    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    tmp = tmp_path_factory.mktemp("bias_sparse_cli")
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
        alt = dec.rescaled_words([(1.0, 1.0, 0.0), (1.0, 0.1, -2.0)])
        own = {}
        for i in range(len(mats)):
            words = alt[i][1]["hyp_words"].tolist()
            runs = [(tuple(words[k:k + 2]), 1.5) for k in range(0, max(len(words) - 1, 0), 3)] + [(tuple(words[-1:]), 0.5)] if words else []
            own[i] = [r for k, r in enumerate(runs) if r[0] and r not in runs[:k]][:6]
        want = {}
        for name, pad in (("small", 30), ("large", 290)):   # the common phrases: one-word phrases of words no lattice holds
            common = [((100001 + k,), 0.25) for k in range(pad)]
            with open(tmp / (name + ".txt"), "w") as f:
                for ws, b in common:
                    f.write("* %r %s\n" % (b, " ".join(str(w) for w in ws)))
                for i, ph in own.items():
                    for ws, b in ph:
                        f.write("utt%03d %r %s\n" % (i, b, " ".join(str(w) for w in ws)))
            books = [common + own[i] for i in range(len(mats))]
            bk = W.BiasBooks.from_phrases(books)
            try:
                assert all((n > 256) == (name == "large") for n in bk.info()["n_nodes"]), bk.info()["n_nodes"]
                want[name] = dec.biased_words_sparse(bk, None, SETTINGS)
            finally:
                bk.free()
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


@pytest.mark.parametrize("flags", [[], ["--single-stream"]])
def test_a_file_of_300_node_lists_is_answered(flags, setup):
    p = run(setup, "--bias=" + str(setup["tmp"] / "large.txt"), FLAG, *flags)
    mine = [l for l in p.stdout.splitlines(keepends=True) if LINE.match(l.rstrip("\n"))]
    assert len(mine) == len(FRAMES) * len(SETTINGS)
    n_words, n_hits = compare(mine, setup["want"]["large"], SETTINGS)
    assert n_words > 0 and n_hits > 0, "the comparison is not empty: words and hits were compared"


def test_bias_sparse_prints_what_the_run_without_it_prints(setup):
    flag = "--bias=" + str(setup["tmp"] / "small.txt")
    dense = run(setup, flag, FLAG).stdout
    sparse = run(setup, flag, FLAG, "--bias-sparse").stdout
    assert sparse == dense and " bias " in dense
    mine = [l for l in sparse.splitlines(keepends=True) if LINE.match(l.rstrip("\n"))]
    compare(mine, setup["want"]["small"], SETTINGS)
