"""-m gpu: wfst-decode --bias=FILE [--bias-settings=...] (the host mirror's BiasLists / BiasedWords over wfst_decoder_biased_words) in
its three shapes -- the batch decoder over all utterances at once, --batch=4 and --single-stream -- against the Python binding on the
same utterances and lists, and the tool's other output with and without the flag, byte for byte."""
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
SETTINGS = [(1.0, 1.0, 0.0, 1.0), (1.0, 0.1, 0.5, 4.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, -3.0, 0.0), (0.5, 1.0, 2.25, 30.0)]
FLAG = "--bias-settings=" + ":".join("%r,%r,%r,%r" % s for s in SETTINGS)
LINE = re.compile(r"^(\S+) bias (\d+) gs=(\S+) as=(\S+) wip=(\S+) bs=(\S+) found=([01]) cost=(\S+) bonus=(\S+) tot=(\S+) lm=(\S+) hits=(\S*) :(.*)$")


@pytest.fixture(scope="module")
def setup(synth, tmp_path_factory):
    import gpu_util as G

    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    tmp = tmp_path_factory.mktemp("bias_cli")
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
        # the phrases: for every utterance word runs of its best paths under two penalties; utterance 3 has none of its own; two
        # phrases for everyone (one of them of words no lattice holds)
        alt = dec.rescaled_words([(1.0, 1.0, 0.0), (1.0, 0.1, -2.0)])
        common = [((100001, 100002), 3.0), (tuple(alt[0][1]["hyp_words"][:1].tolist()), 0.75)]
        own = {}
        for i in range(len(mats)):
            if i == 3:
                continue
            words = alt[i][1]["hyp_words"].tolist()
            runs = [(tuple(words[k:k + 2]), 1.5) for k in range(0, max(len(words) - 1, 0), 3)] + [(tuple(words[-1:]), 0.5)] if words else []
            own[i] = [r for k, r in enumerate(runs) if r[0] and r not in runs[:k] and r[0] not in [c[0] for c in common]][:6]
        with open(tmp / "bias.txt", "w") as f:
            for ws, b in common:
                f.write("* %r %s\n" % (b, " ".join(str(w) for w in ws)))
            for i, ph in own.items():
                for ws, b in ph:
                    f.write("utt%03d %r %s\n" % (i, b, " ".join(str(w) for w in ws)))
        lists = [common + own.get(i, []) for i in range(len(mats))]
        bl = W.BiasLists.from_phrases(lists)
        try:
            want = dec.biased_words(bl, None, SETTINGS)
            default = dec.biased_words(bl)
        finally:
            bl.free()
    finally:
        dec.free()
        graph.free()
    return dict(tmp=tmp, gpath=gpath, want=want, default=default)


def run(setup, *flags):
    tmp = setup["tmp"]
    p = subprocess.run([CLI, "--tid2pdf=" + str(tmp / "tid2pdf.bin")] + list(flags) + [str(tmp / "decoder.conf"), setup["gpath"], str(tmp / "ll.bin")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p


def compare(lines, want, settings):
    seen, n_words, n_hits = set(), 0, 0
    for l in lines:
        key, q, gs, as_, wip, bs, found, cost, bonus, tot, lm, hits, rest = LINE.match(l.rstrip("\n")).groups()
        i, q = int(key[3:]), int(q) - 1
        w = want[i][q]
        seen.add((i, q))
        assert (float(gs), float(as_), float(wip), float(bs)) == tuple(float(x) for x in settings[q]) and int(found) == int(w["found"]) and w["status"] == 0, l
        assert float(cost) == w["biased_cost"] and float(bonus) == w["bonus"], "seventeen digits: the float64 itself"
        assert np.float32(float(tot)) == w["tot"] and np.float32(float(lm)) == w["lm"], l
        words = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"(\d+)\((\d+),(\d+)\)", rest)]
        assert len(words) == len(rest.split()) == w["n_hyp"], l
        assert [x[0] for x in words] == w["hyp_words"].tolist() and [x[1] for x in words] == w["begin"].tolist() and [x[2] for x in words] == w["end"].tolist(), l
        got_hits = [tuple(int(x) for x in h.split("@")) for h in hits.split(",")] if hits else []
        assert got_hits == list(zip(w["hit_phrase"].tolist(), w["hit_word"].tolist())) and len(got_hits) == w["n_hits"], l
        n_words += len(words)
        n_hits += len(got_hits)
    assert len(seen) == len(lines)
    return n_words, n_hits


@pytest.mark.parametrize("shape,flags", [("batch", []), ("batch4", ["--batch=4"]), ("single", ["--single-stream"])])
def test_the_tool_against_the_binding(shape, flags, setup):
    plain = run(setup, *flags).stdout
    p = run(setup, "--bias=" + str(setup["tmp"] / "bias.txt"), FLAG, *flags)
    lines = p.stdout.splitlines(keepends=True)
    mine = [l for l in lines if LINE.match(l.rstrip("\n"))]
    # the other output is what it is without the flag, byte for byte
    assert "".join(l for l in lines if l not in mine) == plain and len(plain.splitlines()) == len(FRAMES) and " bias " not in plain
    assert len(mine) == len(FRAMES) * len(SETTINGS)
    n_words, n_hits = compare(mine, setup["want"], SETTINGS)
    assert n_words > 20 and n_hits > 5
    print("%s: %d lines, %d words and %d hits compared" % (shape, len(mine), n_words, n_hits))


def test_without_settings_the_tool_takes_one_one_zero_one(setup):
    p = run(setup, "--bias=" + str(setup["tmp"] / "bias.txt"))
    mine = [l for l in p.stdout.splitlines(keepends=True) if LINE.match(l.rstrip("\n"))]
    assert len(mine) == len(FRAMES)
    compare(mine, setup["default"], [(1, 1, 0, 1)])


def test_a_bad_file_is_a_named_usage_error(setup):
    tmp = setup["tmp"]
    for text in ("utt000 x 5 6\n", "utt000 1.5\n", "utt000 -1 5\n", "utt000 1.0 5 0\n", "utt000 1.0 5 six\n", "utt000 1.0 " + " ".join(["7"] * 17) + "\n"):
        (tmp / "bad.txt").write_text("* 1.0 4 5\n" + text)
        p = subprocess.run([CLI, "--bias=" + str(tmp / "bad.txt"), str(tmp / "decoder.conf"), setup["gpath"], str(tmp / "ll.bin")], capture_output=True, text=True)
        assert p.returncode == 1 and "--bias: line 2 of" in p.stderr and "KEY bonus w1 w2 ..." in p.stderr, (text, p.stderr)
