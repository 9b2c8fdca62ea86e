"""-m gpu: the expansion kernels at their tile and row-shape edges, on the graphs of tests/geometry_util.py (each aimed at one of
the constants the code is cut along; tests/test_geometry_graphs.py proves the shapes and that every triple decoded here is `ok`
and tie-free under the oracle).  Every leg names the kernel path it is about and asserts dec.path_flags(), so none can silently
run another; every decode is held bit for bit to the ORDER-FREE oracle:

* the best path of every utterance (words, transition-ids, per-hop labels, graph and acoustic cost bits, scores), decoded in one
  call and again frame by frame;
* frame by frame, the partial best path behind frames 1 and 2 (the frames right behind the one-token tile of the start state);
* frame by frame, the frontier: the relation tests/test_gpu_parity.py::test_per_frame_best_cost_and_token_subset asserts (the
  device's tokens are distinct states, each among the oracle's tokens of that frame at a bit-equal cost; the same best cost);
* in lattice legs the raw lattice, state by state and arc by arc.

Utterances of 8, 3 and 1 frames share a decoder: one channel ends while the others go on.  Both frame boundaries size the tiles by
tokens x channels of the launch: these decoders of three channels expand every (non-compacting) frontier in tiles of 128 tokens, so the
frontiers of 255 .. 1025 tokens are cut at 128 (frontier_of(127 / 128 / 129) stand at that cut itself); tiles of 256 tokens, and a
frontier of 5 x 256 and one more, are the `tiles256` leg's, with 72 channels; a round of 256 live tokens is the compacting leg's."""
import numpy as np
import pytest

import geometry_util as U
from golden_util import bits

pytestmark = pytest.mark.gpu

LIM = dict(max_frames=16, max_tokens_per_frame=16384, arena_tokens=1 << 18)
LAT = dict(LIM, lattice_links=1 << 20)
# leg -> decoder limits, graph options, decoder options, padding columns, how the matrices lie in memory, the path flags it must report
LEGS = {
    # stride % 4 == 0, stride <= 3072, 16-byte aligned rows: the frame's whole row staged in LDS
    "row": dict(flags=dict(staged=1, ll_row=1, degcode=1)),
    # the same matrices with one padding column: one 4-byte gather per arc slot
    "gather_stride": dict(pad=1, flags=dict(staged=1, ll_row=0, degcode=1)),
    # stride % 4 == 0, but the matrix begins 4 bytes into its buffer
    "gather_align": dict(lay="off4", flags=dict(staged=1, ll_row=0)),
    # the matrix moves from an aligned to a misaligned address between two advance calls of one utterance
    "row_to_gather": dict(lay="moves", flags=dict(staged=1, ll_row=0)),
    # an arena of more than 2^22 tokens leaves no room for degree codes in the tokens: every token reads its row header
    "header": dict(lim=dict(LIM, arena_tokens=(1 << 22) + 4096), flags=dict(staged=1, degcode=0)),
    # the graph loaded without fused closures: expand_kernel_plain and the closure pass
    "plain": dict(gopt=dict(fuse_closures=0), flags=dict(staged=0, degcode=0)),
    # a closure of 49 paths or 9 hops: the loader itself leaves the graph unfused
    "unfusable": dict(flags=dict(staged=0, degcode=0)),
    # max_active (min_active) below the frontier: compacting tiles, GetCutoff's selection at the frame boundary
    "compacting": dict(flags=dict(staged=1)),
    # an arena that leaves no room for a collection stride: the closure launch on every frame
    "three_launch": dict(lim=dict(LIM, arena_tokens=1 << 15), flags=dict(staged=1, two_launch=0, gc_stride=1)),
    "lattice": dict(lim=LAT, lattice=True, flags=dict(staged=1, degcode=0)),
    "lattice_iterated": dict(lim=LAT, lattice=True, opt=dict(debug=0x1000), flags=dict(staged=0)),   # the iterated closure pass
    "small_tiles": dict(opt=dict(tile_tokens=64), flags=dict(staged=1, ll_row=1)),
    # 72 channels in one group: frontiers of 1.3 k tokens and more are cut into tiles of 256 tokens -- every other leg's decoders,
    # of three channels, cut theirs into tiles of 128 (U.plain_tile_tokens); the channels share the three utterances
    "tiles256": dict(channels=U.MANY_CHANNELS, opt=dict(channel_groups=1), lim=dict(max_frames=16, max_tokens_per_frame=4096, arena_tokens=1 << 16),
                     flags=dict(staged=1, ll_row=1, degcode=1, channel_groups=1)),
    # expand_kernel_biglm, against the fixed-mode oracle
    "biglm": dict(biglm=True, lim=dict(LIM, lm_pairs=1 << 16), flags=dict(staged=0)),
}
CASES = [(leg, name, cfg) for leg, cases in U.leg_cases().items() for name, cfg in cases]
assert set(LEGS) == set(U.leg_cases())


_Gpu = U.Gpu


@pytest.fixture(scope="module")
def gpu(synth, oracle, tmp_path_factory):
    g = _Gpu(U.World(synth, oracle, str(tmp_path_factory.mktemp("geometry"))))
    yield g
    g.free()


def _upload(mats, off4):
    """The matrices in HBM; off4: each 4 bytes into a buffer of its own (4-byte aligned, not 16)."""
    import torch

    out = []
    for m in mats:
        flat = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32).reshape(-1))
        if off4:
            buf = torch.zeros(flat.numel() + 1, dtype=torch.float32, device="cuda:0")
            buf[1:].copy_(flat)
            t = buf[1:]
            assert t.data_ptr() % 16 == 4
        else:
            t = flat.to("cuda:0")
            assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


_same_lattice = U.same_lattice


def _tile_tokens(n, max_active):
    """Tokens per compacting tile of a frame of n tokens under a binding max_active: a restatement of wfst_kernels.hip
    super_tile_tokens, which prep_frame and frame_boundary_fused call where max_active_cutoff < beam_cutoff (the non-compacting
    sizes: U.plain_tile_tokens).  When that sizing changes, the plateau case below fails (second_round) rather than lose its aim."""
    return min(1024, max(256, ((256 - 32) * n // max_active) & ~63))


@pytest.mark.parametrize("leg,name,cfg", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_leg(gpu, leg, name, cfg):
    G, W, world = gpu.G, gpu.W, gpu.world
    spec = LEGS[leg]
    flags = dict(spec["flags"])
    if name == "wide3076":
        flags["ll_row"] = 0   # 3076 columns do not fit the staged row
    cd = U.CFGS[cfg]
    biglm, lattice, lay = spec.get("biglm", False), spec.get("lattice", False), spec.get("lay")
    graph = gpu.graph(name, spec.get("gopt"))
    utts = world.mats(name)
    B = spec.get("channels", len(utts))
    utt = [c % len(utts) for c in range(B)]   # the utterance channel c decodes
    mats = [utts[u] for u in utt]
    T = [int(x.shape[0]) for x in mats]
    pad = spec.get("pad", 0)
    fed = [np.ascontiguousarray(np.pad(x, ((0, 0), (0, pad)))) for x in utts] if pad else utts
    stride = int(fed[0].shape[1])
    assert (stride % 4 == 0) == (pad == 0)
    dev = _upload(fed, lay == "off4")
    dev_moved = _upload(fed, True) if lay == "moves" else None
    ptrs = [dev[u].data_ptr() for u in utt]
    ptrs_moved = [dev_moved[u].data_ptr() for u in utt] if dev_moved else None
    row_ok = int(name != "wide3076")   # (row_to_gather: the form while the matrices are aligned)
    kw = dict(spec.get("lim", LIM))
    if spec.get("opt"):
        kw["options"] = W.Options(**spec["opt"])
    if biglm:
        kw["old_lm"], kw["new_lm"] = gpu.lm_pair()
    want = [(world.oracle_biglm if biglm else world.oracle_decode)(name, cfg, u) for u in utt]
    dec = W.BatchDecoder(graph, G.gpu_config(cd), B, **kw)

    def check_flags(expect, when):
        pf = dec.path_flags()
        assert {k: pf[k] for k in expect} == expect, "%s %s %s, %s: path flags %s" % (leg, name, cfg, when, pf)

    def check_best(when):
        for ui, d in enumerate(dec.best_paths()):
            assert want[ui].ok and want[ui].extra["ties"] == 0
            G.assert_same_as_oracle(G.GpuResult(d), want[ui], "%s %s %s utt %d, %s" % (leg, name, cfg, ui, when))
        assert all(dec.degraded_frames(c) == 0 for c in range(B)), "degraded frames"

    try:
        # ---- one call (row_to_gather: two, the matrices at another address for the second) ----
        dec.init()
        if lay == "moves":
            dec.advance(ptrs, [min(2, t) for t in T], stride)
            check_flags(dict(flags, ll_row=row_ok), "aligned")
            dec.advance(ptrs_moved, T, stride)
        else:
            dec.advance(ptrs, T, stride)
        dec.finalize()
        check_flags(flags, "one call")
        check_best("one call")
        if lattice:
            for ui in range(B):
                _same_lattice(dec.raw_lattice(ui), world.oracle_lattice(name, cfg, utt[ui]), "%s %s %s utt %d" % (leg, name, cfg, ui))

        # ---- frame by frame: the frontier of every frame, the partial best path behind frames 1 and 2 ----
        dec.init()
        second_round = one_round = 0
        tiles = set()   # (tile size, tokens in the frontier's last tile) of the frontiers that are expanded in non-compacting tiles
        for r in range(0, max(T) + 1):
            if r:
                moved = lay == "moves" and r >= 3
                dec.advance(ptrs_moved if moved else ptrs, [min(r, t) for t in T], stride)
                if lay == "moves":
                    check_flags(dict(flags, ll_row=0 if moved else row_ok), "frame %d" % r)
            for c in range(B):
                if r > T[c]:
                    continue
                what = "%s %s %s utt %d frame %d" % (leg, name, cfg, c, r)
                st, co = dec.frontier(c)
                if biglm:
                    # a biglm token is a (graph state, LM state pair): the oracle dumps no such list, its trace holds the frame's
                    # token count and best cost
                    tr = world.oracle_biglm_trace(name, cfg, utt[c])
                    assert len(st) == tr.frame_ntoks[r], what + ": %d tokens, the oracle %d" % (len(st), tr.frame_ntoks[r])
                    assert bits([co.min()]) == bits([tr.frame_best[r]]), what + " best cost"
                    continue
                ost, oco, on = world.oracle_dump(name, cfg, utt[c], r)
                assert on == len(ost) and 0 < len(st) <= on and len(set(st.tolist())) == len(st), what + ": %d tokens, the oracle %d" % (len(st), on)
                # (more than that test asks: against the ORDER-FREE oracle the sets are equal, on its 50k-arc graph as here)
                assert len(st) == on, what + ": %d tokens, the oracle %d" % (len(st), on)
                ref = dict(zip(ost.tolist(), bits(oco).tolist()))
                for a, b in zip(st.tolist(), bits(co).tolist()):
                    assert ref.get(a) == b, what + " state %d" % a
                assert bits([co.min()]) == bits([oco.min()]), what + " best cost"
                if r and r < T[c] and cd["max_active"] >= len(co) and spec["flags"]["staged"]:
                    t = U.plain_tile_tokens(len(co), B, (spec.get("opt") or {}).get("tile_tokens", 256))
                    tiles.add((t, (len(co) - 1) % t + 1))
                if leg == "compacting" and cd["max_active"] < len(co) and cfg in ("max200", "max600") and len(co) > 256:
                    # the tiles this frontier is expanded in (the limit binds: compacting tiles), from the token order the device
                    # holds: tokens at or below the max_active-th cheapest cost are live
                    cut, t = np.sort(co)[cd["max_active"] - 1], _tile_tokens(len(co), cd["max_active"])
                    live = [int((co[k:k + t] <= cut).sum()) for k in range(0, len(co), t)]
                    second_round += int(max(live) > 256 and r < T[c])
                    one_round += int(max(live) <= 256 and r < T[c])
            if r in (1, 2):
                for ui, d in enumerate(dec.best_paths(use_final_probs=False)):
                    k = min(r, T[ui])
                    po = (world.oracle_biglm if biglm else world.oracle_decode)(name, cfg, utt[ui], frames=k, partial=True)
                    assert po.ok and po.extra["ties"] == 0
                    G.assert_same_as_oracle(G.GpuResult(d), po, "%s %s %s utt %d, partial at frame %d" % (leg, name, cfg, ui, k))
        dec.finalize()
        check_flags(flags, "frame by frame")
        check_best("frame by frame")
        # the tile cuts a case is named for, at the tile size its decoder's channel count gives
        if leg == "tiles256" and name.startswith("frontier"):
            assert tiles == {(256, 256 if name == "frontier1280" else 1)}, tiles
        if leg == "tiles256":   # (the hub's graph: the frontiers right behind the hub; its later ones shrink below 700 x 128 / 72)
            assert 256 in {t for t, _ in tiles}, tiles
        if leg in ("row", "gather_stride", "gather_align", "row_to_gather") and name in ("frontier127", "frontier128", "frontier129"):
            assert tiles == {(128, {"frontier127": 127, "frontier128": 128, "frontier129": 1}[name])}, tiles
        if leg == "compacting" and cfg == "max200" and name in ("frontier1025", "hub3000"):
            # max_active 200 of 1025 (3000 and more) tokens: tiles of 1024 tokens, a fifth (a fifteenth) of them live -- one round
            assert one_round >= 2 and second_round == 0, (one_round, second_round)
        if leg == "compacting" and name == "plateau1025":
            # max_active 600 falls on the plateau of 860 equal costs: 84 % of the tokens and more stay live, in tiles of 320 cut for
            # 600 live ones in 1025 (58 %): about 270 live tokens a tile, a second round of the compacting tile -- on the frontiers
            # of frames 1 and 2 (tests/test_geometry_graphs.py)
            assert second_round >= 2, (one_round, second_round)
    finally:
        dec.free()
