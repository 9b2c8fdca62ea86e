"""-m gpu: word alternatives through the C++ mirror -- wfst-decode --nbest=3 --nbest-word-times --word-alternatives=3 and
--align-words=FILE --word-alternatives (with and without --word-confidence), in the batch shape, with --batch=4
(GpuBatchDecoder::WordAlternatives) and with --single-stream (GpuLatticeDecoder::WordAlternatives on a private decoder): the lines
equal what the Python binding's word_alternatives says for the same words on the same utterances, and without the flag every line is
what it is without this feature.

The tool prints the doubles with 9 significant digits (%.9g): at most 5e-9 of the value off, as tests/test_gpu_posterior_cli.py works
out; the sums' free order leaves about 1e-13 more, and 1e-12 covers it.  Two calls may order two words of a slot differently where
their masses differ by no more than that rounding, so the lists are compared word by word, not position by position: a word both
list has the same mass, and a word only one lists has, to that rounding, the mass at which the other list ends."""
import os
import subprocess

import pytest

from test_gpu_posterior_cli import CLI, N, near, run, world  # noqa: F401

pytestmark = pytest.mark.gpu


def strip(line):
    """a line without what --word-alternatives adds to it: none= and alts= of a word line"""
    return " ".join(x for x in line.split() if not x.startswith("none=") and not x.startswith("alts="))


def check_words(lines, head, words, a, k, conf):
    got = [l for l in lines if l.startswith(head + "#")]
    assert len(got) == len(words), head
    for j, (l, w) in enumerate(zip(got, words)):
        f = l[len(head):].split()
        assert f[:4] == ["#%d" % (j + 1), str(w), str(a["begin"][j]), str(a["end"][j])] and len(f) == (7 if conf else 6), l
        if conf:
            assert near(f[4], a["conf"][j]), l
        assert f[-2].startswith("none=") and near(f[-2][5:], a["none_post"][j]) and f[-1].startswith("alts="), l
        listed = [] if f[-1] == "alts=-" else [(int(x.split(":")[0]), float(x.split(":")[1])) for x in f[-1][5:].split(",")]
        want = a["alts"][j]
        assert len(listed) == len(want) == min(k, int(a["n_distinct"][j])), l
        assert all(x[1] >= y[1] for x, y in zip(listed, listed[1:])), l
        both = dict(want)
        for word, post in listed:
            assert near(post, both[word]) if word in both else near(post, want[-1][1]), l
        for word, post in want:
            assert word in dict(listed) or near(listed[-1][1], post), l


@pytest.mark.parametrize("shape", [[], ["--batch=4"], ["--single-stream"]])
def test_nbest_word_alternatives_equal_the_binding(world, shape):
    plain = run(world["head"] + shape + ["--nbest=%d" % N, "--nbest-word-times"] + world["tail"])
    lines = run(world["head"] + shape + ["--nbest=%d" % N, "--nbest-word-times", "--word-alternatives=3"] + world["tail"])
    assert [strip(l) for l in lines] == plain    # without the flag: byte for byte today's lines
    n_words = n_alts = 0
    for i in range(world["n"]):
        key = "utt%03d" % i
        paths = [(l.split()[0], [int(x) for x in l.split()[1:]]) for l in plain if l.split()[0].startswith(key + "-") and "#" not in l.split()[0]]
        assert paths, key
        res = world["dec"].word_alternatives([[w for _, w in paths]], [i], n_alts=3)[0]
        for (head, w), a in zip(paths, res):
            assert a["found"], "an n-best path's words are in the raw lattice"
            check_words(lines, head, w, a, 3, False)
            n_words += len(w)
            n_alts += sum(len(x) for x in a["alts"])
    assert n_words >= 6 and n_alts > n_words


@pytest.mark.parametrize("shape", [[], ["--batch=4"], ["--single-stream"]])
def test_align_words_file_with_alternatives_equals_the_binding(world, shape):
    conf = run(world["head"] + shape + ["--align-words=" + world["align_file"], "--word-confidence=1,0.1"] + world["tail"])
    lines = run(world["head"] + shape + ["--align-words=" + world["align_file"], "--word-confidence=1,0.1", "--word-alternatives"] + world["tail"])
    # the confidences are two calls' (their last digits may differ): the lines without them are today's
    cut = lambda l: " ".join(l.split()[:-1] if "#" in l and "notfound" not in l else [x for x in l.split() if not x.startswith("logpost=")])
    assert [cut(strip(l)) for l in lines] == [cut(l) for l in conf]
    res = world["dec"].word_alternatives(world["asked"], graph_scale=1.0, acoustic_scale=0.1)
    n_found = n_absent = 0
    for i, (seqs, answers) in enumerate(zip(world["asked"], res)):
        for q, (s, a) in enumerate(zip(seqs, answers)):
            head = "utt%03d align %d" % (i, q + 1)
            line = [l for l in lines if l.startswith(head + " ")]
            assert len(line) == 1 and line[0].startswith("%s found=%d arcs=%d tot=%.9g lm=%.9g" % (head, a["found"], a["n_arcs"], a["tot"], a["lm"])), head
            if a["found"]:
                assert near(line[0].split()[-1][8:], a["path_logpost"]) and line[0].split()[-1].startswith("logpost="), head
                check_words(lines, head, s, a, 5, True)
                n_found += 1
            else:
                assert not [l for l in lines if l.startswith(head + "#")]
                n_absent += 1
    assert n_found >= world["n"] and n_absent >= world["n"]


def test_usage_errors():
    p = subprocess.run([CLI, "--word-alternatives", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "--word-alternatives goes with --nbest-word-times or --align-words=FILE" in p.stderr
    p = subprocess.run([CLI, "--word-alternatives=0", "--nbest-word-times", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "--word-alternatives=K, 1 <= K <= 16" in p.stderr
