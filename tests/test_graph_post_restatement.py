"""CPU: the numpy restatement of wfst_decoder_graph_posteriors' recursion (tests/graph_post_util.py) against the enumeration of every
path in float64, and the identities the header implies.  No device, no library.

The tolerance is posterior_util's derivation applied to the (frame, state) table: tol_log = 8 (n_levels + 2) 2^-52 max(1, A) with
n_levels = (T + 1)(eps_depth + 1) and A the largest finite |alpha| or |beta|; a posterior v over k arcs 4 tol_log max(1, |v|) + k 2^-52;
an occupancy T + 1 times that.  On the 320 graphs below (seed 2024) the restatement reaches the fraction of it the last test prints."""
import numpy as np
import pytest

import graph_post_util as U

N_GRAPHS = 320
N_TID = 4


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for k in range(N_GRAPHS):
        g = U.random_small_graph(rng, max_states=7, n_tid=N_TID)
        T = int(rng.integers(0, 5))
        ll = rng.normal(-2.0, 1.5, size=(max(T, 1), N_TID + 1)).astype(np.float32)
        ll[rng.random(ll.shape) < 0.08] = -np.inf
        gs, as_ = (float(rng.uniform(0, 2)), float(rng.uniform(0, 2))) if k % 2 else (1.0, 1.0)
        out.append((g, ll[:T] if T else ll[:0], T, gs, as_))
    return out


@pytest.fixture(scope="module")
def results():
    out = []
    for g, ll, T, gs, as_ in cases():
        want = U.graph_posteriors(g, ll, T, None, None, gs, as_)
        enum = U.enumerate_posteriors(g, ll, T, None, None, gs, as_)
        out.append((g, ll, T, gs, as_, want, enum))
    return out


def test_restatement_against_enumeration(results):
    worst, worst_mass, n_found = 0.0, 0.0, 0
    for k, (g, ll, T, gs, as_, want, enum) in enumerate(results):
        assert want["found"] == enum["found"], k
        if not want["found"]:
            continue
        n_found += 1
        worst = max(worst, U.compare_dense(enum["post"], enum["arc_occ"], enum["log_like"], True, want, "graph %d" % k))
        if T:
            r = np.abs(want["frame_mass"] - 1.0) / U.post_tol(want, 1.0, want["k_class"].sum())
            assert r.max() <= 1.0, (k, r.max())
            worst_mass = max(worst_mass, float(r.max()))
    print("restatement against enumeration: %d graphs, %d found, largest difference / tolerance %.4f, |frame_mass - 1| %.4f"
          % (len(results), n_found, worst, worst_mass))
    assert n_found >= N_GRAPHS // 4


def test_alpha_at_the_end_is_beta_at_the_start(results):
    for k, (g, ll, T, gs, as_, want, enum) in enumerate(results):
        a, b = want["alpha"][T, g.final_state], want["beta"][0, g.start]
        assert np.isfinite(a) == np.isfinite(b), k
        if np.isfinite(a):
            assert abs(a - b) <= want["tol_log"], (k, a, b)


def test_zero_scales_count_the_paths(results):
    for k, (g, ll, T, gs, as_, want, enum) in enumerate(results):
        zero = U.graph_posteriors(g, ll, T, None, None, 0.0, 0.0)
        n = U.enumerate_posteriors(g, ll, T, None, None, 0.0, 0.0)["n_paths"]
        assert zero["found"] == (n > 0), k
        if n:
            assert abs(zero["log_like"] - np.log(n)) <= zero["tol_log"], (k, zero["log_like"], n)


def test_a_chain_has_one_path():
    rng = np.random.default_rng(5)
    hops = [(1, 0, 0.5), (0, 1, -0.25), (2, 0, 1.5), (3, 2, 0.125), (0, 0, 0.75), (2, 0, 0.0)]
    g = U.chain_graph(hops)
    ll = rng.normal(-2.0, 1.0, size=(4, N_TID + 1)).astype(np.float32)
    want = U.graph_posteriors(g, ll, 4, None, None, 0.7, 1.3)
    cost = U.hop_cost(g, ll, list(range(len(hops))), None, 0.7, 1.3)
    assert want["found"] and abs(want["log_like"] + cost) <= want["tol_log"]
    assert np.allclose(want["posts"], 1.0, rtol=0, atol=4 * want["tol_log"] + U.EPS) and list(want["classes"]) == [1, 2, 3, 2]
    assert np.allclose(want["arc_occ"], 1.0, rtol=0, atol=5 * (4 * want["tol_log"] + U.EPS))


def test_the_sum_is_no_worse_than_the_best_path(results):
    n = 0
    for k, (g, ll, T, gs, as_, want, enum) in enumerate(results):
        if (gs, as_) != (1.0, 1.0) or not np.all(np.isfinite(g.arcs["w"])):
            continue
        fa = U.force_align(g, ll, T)
        if not fa["found"]:
            continue
        assert want["found"], k
        n += 1
        assert -want["log_like"] <= U.hop_cost(g, ll, fa["hop_arc"]) + want["tol_log"], k
    assert n >= 40
