"""-m gpu: partial words through the C++ mirror -- wfst-decode --chunk=N --partial-words, single stream and 64 service threads over
one GpuChannelPool (GetPartialWords after every chunk, served as one list per batcher pass).  Every partial line "KEY@frames
n_stable words..." carries the oracle's partial best path at that frame count, its word part equals the line the CLI prints
without the flag (GetBestPath(use_final_probs = false)), and every stable prefix is a prefix of the utterance's later lines and of
its final words."""
import os
import re
import struct
import subprocess

import pytest

import pyoracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
CD = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)


def setup(synth, tmp_path, T):
    """(the graph, config and utterance seeds of tests/test_gpu_host_cli.py's streaming test)"""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    g = synth.make_hclg_like(4000, seed=9, n_tid=600, n_words=800)
    gpath = str(tmp_path / "g.bin")
    g.write(gpath)
    m = synth.default_tid2pdf(600)
    m.astype("<i4").tofile(str(tmp_path / "tid2pdf.bin"))
    (tmp_path / "decoder.conf").write_text("--beam=12\n--max-active=1000000\n--min-active=0\n--lattice-beam=6\n--prune-interval=10\n")
    mats = [synth.make_loglikes(g, t, 300, m, seed=300 + i, mu=-2.2)[0] for i, t in enumerate(T)]
    with open(tmp_path / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = ("utt%03d" % i).encode()
            f.write(struct.pack("<i", len(key)) + key + struct.pack("<ii", x.shape[0], x.shape[1]) + x.tobytes())
    tail = [str(tmp_path / "decoder.conf"), gpath, str(tmp_path / "ll.bin")]
    return g, gpath, m, mats, [CLI, "--tid2pdf=" + str(tmp_path / "tid2pdf.bin")], tail


def run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l.split() for l in p.stdout.strip().splitlines()]
    partial = {l[0]: [int(w) for w in l[1:]] for l in lines if re.fullmatch(r"utt\d+@\d+", l[0])}
    final = {l[0]: [int(w) for w in l[1:]] for l in lines if re.fullmatch(r"utt\d+", l[0])}
    return partial, final, p.stdout


def check(oracle, gpath, m, mats, T, chunk, partial, final):
    h = oracle.load_graph(gpath)
    n_part = n_stable_total = 0
    try:
        for i, x in enumerate(mats):
            k = "utt%03d" % i
            assert final[k] == oracle.decode(h, pyoracle.Config(**CD), x, m).words.tolist(), k
            prev = []
            for r in range(chunk, T[i], chunk):
                line = partial["%s@%d" % (k, r)]
                ns, words = line[0], line[1:]
                o = oracle.decode(h, pyoracle.Config(**CD), x[:r], m, finalize=False, use_final_probs=False)
                assert words == o.words.tolist(), (k, r)
                assert 0 <= ns <= len(words)
                for r0, ns0, w0 in prev:
                    assert ns >= ns0 and words[:ns0] == w0[:ns0], (k, r0, r)
                prev.append((r, ns, words))
                n_part += 1
            for r0, ns0, w0 in prev:
                assert final[k][:ns0] == w0[:ns0], (k, r0)
            n_stable_total += prev[-1][1] if prev else 0
            assert "%s@%d" % (k, T[i]) not in partial
    finally:
        oracle.free_graph(h)
    return n_part, n_stable_total


@pytest.mark.parametrize("lattice", [False, True])
def test_cli_partial_words_single_stream(lattice, synth, oracle, tmp_path):
    T = [83, 45, 7, 140]
    g, gpath, m, mats, head, tail = setup(synth, tmp_path, T)
    shape = ["--single-stream", "--chunk=25"] + (["--nbest=3"] if lattice else [])
    plain, plain_final, plain_out = run(head + shape + tail)
    part, final, out = run(head + shape + ["--partial-words"] + tail)
    assert final == plain_final
    assert sorted(part) == sorted(plain) and all(part[k][1:] == plain[k] for k in plain)   # the word part of every line
    # every other line -- the final results, and in lattice mode the partial n-best lines KEY@frames-k -- is the same with and without
    # the flag, in the same order
    rest = lambda text: [l for l in text.splitlines() if not re.fullmatch(r"utt\d+@\d+", l.split()[0])]
    assert rest(out) == rest(plain_out)
    assert (sum(bool(re.fullmatch(r"utt\d+@\d+-\d+", l.split()[0])) for l in out.splitlines()) >= 9) == lattice
    n_part, n_stable = check(oracle, gpath, m, mats, T, 25, part, final)
    assert n_part == 3 + 1 + 0 + 5 and n_stable > 0


@pytest.mark.parametrize("lattice", [False, True])
def test_sixty_four_threads_ask_for_partial_words_over_one_pool(lattice, synth, oracle, tmp_path):
    T = [30 + (37 * i) % 131 for i in range(96)]   # ragged: 30 .. 160 frames
    g, gpath, m, mats, head, tail = setup(synth, tmp_path, T)
    shape = ["--threads=64", "--pool=64", "--chunk=25", "--pull", "--partial-words"] + (["--nbest=3"] if lattice else [])   # (--nbest: a lattice decoder)
    part, final, out = run(head + shape + tail)
    assert any(re.fullmatch(r"utt\d+-1", l.split()[0]) for l in out.splitlines()) == lattice   # the n-best of the lattice leg was served
    n_part, n_stable = check(oracle, gpath, m, mats, T, 25, part, final)
    assert n_part == sum((t - 1) // 25 for t in T) and n_stable > 0
