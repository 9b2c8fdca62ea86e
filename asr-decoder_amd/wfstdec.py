"""ctypes binding of the C ABI in include/wfst_decoder.h (libwfstdec.so).

Thin plumbing for tests, bench.py and the smoke entry: numpy in, numpy out; device matrices
are passed as raw device pointers (e.g. ``torch.Tensor.data_ptr()``).  There is no CPU
fallback: if the HIP library is missing or no MI355X is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (WFST_LIB_VARIANT: kernel experiments only -- tools/ab_bench.sh builds variants of the library beside the product one with
# `build.py --variant NAME -D...` and times them on one box; the product path never sets it)
LIB_PATH = os.path.join(HERE, "lib", "libwfstdec%s.so" % (("_" + os.environ["WFST_LIB_VARIANT"]) if os.environ.get("WFST_LIB_VARIANT") else ""))

WFST_OK = 0
# wfst_decoder_advance_chunk: element types of a chunk, and "no producer stream" (the rows are complete)
WFST_DTYPE_F32, WFST_DTYPE_F16, WFST_DTYPE_BF16 = 0, 1, 2
WFST_STREAM_NONE = C.c_void_p(-1).value
# wfst_decoder_sequence_stats: the criteria
WFST_SEQ_MMI, WFST_SEQ_SMBR = 0, 1
ERR_NAMES = {-1: "WFST_E_ARG", -2: "WFST_E_IO", -3: "WFST_E_DEVICE", -4: "WFST_E_CAPACITY",
             -5: "WFST_E_STATE", -6: "WFST_E_FORMAT"}

# every symbol include/wfst_decoder.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "wfst_config_default", "wfst_last_error", "wfst_device_count", "wfst_graph_load", "wfst_graph_convert_file",
    "wfst_graph_from_arrays", "wfst_graph_set_tid2pdf", "wfst_graph_info", "wfst_graph_free",
    "wfst_decoder_create", "wfst_decoder_free", "wfst_decoder_init", "wfst_decoder_advance",
    "wfst_decoder_advance_host", "wfst_decoder_finalize", "wfst_decoder_sync",
    "wfst_decoder_num_frames_decoded", "wfst_decoder_get_best_path", "wfst_lattice_to_vector", "wfst_lattice_to_vector_batch",
    "wfst_decoder_get_stats", "wfst_decoder_get_frontier", "wfst_decoder_set_profiling",
    "wfst_decoder_get_profile", "wfst_decoder_get_profile_busy", "wfst_decoder_channel_groups", "wfst_decoder_get_raw_lattice", "wfst_decoder_get_nbest",
    "wfst_options_default", "wfst_graph_options_default", "wfst_graph_load_ex", "wfst_graph_from_arrays_ex",
    "wfst_decoder_create_ex", "wfst_lm_load", "wfst_lm_from_arrays", "wfst_lm_info", "wfst_lm_table_stats", "wfst_lm_free",
    "wfst_decoder_create_biglm", "wfst_decoder_get_determinized_lattice", "wfst_decoder_get_lattice_stats", "wfst_decoder_get_rescored_lattice", "wfst_decoder_get_nbest_paths",
    "wfst_decoder_get_degraded_frames", "wfst_decoder_get_prune_raw_abandoned", "wfst_host_alloc", "wfst_host_free", "wfst_decoder_busy", "wfst_decoder_calls_in_flight", "wfst_decoder_get_determinizer_ms", "wfst_decoder_best_path_enqueue", "wfst_decoder_best_path_ready", "wfst_decoder_best_path_fetch", "wfst_decoder_prefetch_nbest", "wfst_decoder_get_prefetched_nbest_paths", "wfst_decoder_get_path_flags", "wfst_decoder_rescore_lattices", "wfst_decoder_nbest_paths_batch",
    "wfst_decoder_prefetch_determinized", "wfst_lattice_labels_batch",
    "wfst_decoder_prefetch_determinized_detached", "wfst_decoder_get_prefetched_lattice", "wfst_decoder_harvest_prefetched",
    "wfst_endpoint_config_default", "wfst_graph_set_tid2phone", "wfst_decoder_set_endpoint_config", "wfst_decoder_endpoint_detected",
    "wfst_endpoint_rules",
    "wfst_decoder_partial_enqueue", "wfst_decoder_partial_ready", "wfst_decoder_partial_fetch", "wfst_decoder_get_partial",
    "wfst_decoder_set_silence_phones", "wfst_decoder_words_enqueue", "wfst_decoder_words_ready", "wfst_decoder_words_fetch",
    "wfst_decoder_get_words",
    "wfst_decoder_set_score_transform", "wfst_decoder_advance_chunk", "wfst_decoder_get_scores",
    "wfst_decoder_get_nbest_words", "wfst_decoder_get_determinizer_slots",
    "wfst_decoder_set_live_lattice_prune", "wfst_decoder_get_live_lattice_prune",
    "wfst_decoder_align_words", "wfst_decoder_nearest_words", "wfst_decoder_word_confidence",
    "wfst_decoder_sequence_posterior", "wfst_decoder_word_alternatives", "wfst_decoder_frame_posteriors",
    "wfst_decoder_rescaled_words", "wfst_decoder_sequence_stats",
    "wfst_align_graphs_create", "wfst_align_graphs_load", "wfst_align_graphs_info", "wfst_align_graphs_free", "wfst_decoder_force_align",
    "wfst_decoder_force_align_workspace", "wfst_decoder_graph_posteriors", "wfst_decoder_graph_posteriors_workspace",
    "wfst_bias_compile", "wfst_bias_lists_create", "wfst_bias_lists_info", "wfst_bias_lists_free", "wfst_decoder_biased_words",
    "wfst_bias_book_compile", "wfst_bias_books_create", "wfst_bias_books_info", "wfst_bias_books_free", "wfst_decoder_biased_words_sparse",
]


class _LazyList(object):
    """A read-only sequence whose items are put together from the batch's host arrays when first looked at, and kept."""

    def __init__(self, n, make):
        self._items = [None] * n
        self._make = make

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self._items)))]
        if i < 0:
            i += len(self._items)
        if self._items[i] is None:
            self._items[i] = self._make(i)
        return self._items[i]

    def __iter__(self):
        for i in range(len(self._items)):
            yield self[i]

    def __eq__(self, other):
        return list(self) == list(other)


class _BestPaths(object):
    """What best_paths() returns: a read-only sequence of per-channel dicts over the batch's hop arrays.  Everything the call
    computes -- hops, scores, the words and transition-ids of every path -- is in host arrays when it returns (the epsilons are
    dropped for the whole batch at once, wfst_lattice_labels_batch); an utterance's dict is put together when it is first looked at and kept (a service
    that decodes 128 utterances per step does not pay a Python loop over them inside the step)."""

    def __init__(self, il, ol, g, ac, nh, tot_s, lm_s, words, woff, tids, toff):
        self._a = (il, ol, g, ac, nh, tot_s, lm_s)
        self._words, self._woff, self._tids, self._toff = words, woff, tids, toff   # (wfst_lattice_labels_batch: path after path, hop order)
        self._items = [None] * len(nh)

    def __len__(self):
        return len(self._items)

    def _make(self, i):
        il, ol, g, ac, nh, tot_s, lm_s = self._a
        k = int(nh[i])
        return dict(ok=k > 0, ilabel=il[i, :k], olabel=ol[i, :k], graph=g[i, :k], ac=ac[i, :k],
                    words=self._words[self._woff[i]:self._woff[i + 1]], tids=self._tids[self._toff[i]:self._toff[i + 1]],
                    tot_score=float(tot_s[i]) if k else 0.0, lm_score=float(lm_s[i]) if k else 0.0)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self._items)))]
        if i < 0:
            i += len(self._items)
        if self._items[i] is None:
            self._items[i] = self._make(i)
        return self._items[i]

    def __iter__(self):
        for i in range(len(self._items)):
            yield self[i]


# BatchDecoder.frame_posteriors: the entries per decoded frame its first call has room for
FRAME_POST_ENTRIES_PER_FRAME = 64


def frame_post_lookup(result, classes_per_frame):
    """The posterior of ONE class per frame out of a BatchDecoder.frame_posteriors() dict: classes_per_frame[f] is looked up among the
    entries of frame f, 0.0 where it is not listed.  With a best path's transition-ids (one per frame) this is the hypothesis'
    frame-level confidence trace.  Pure numpy; frames beyond the result's n_frames give 0.0."""
    want = np.asarray(classes_per_frame, dtype=np.int64).reshape(-1)
    off, cls, post = np.asarray(result["frame_off"], np.int64), np.asarray(result["classes"], np.int64), np.asarray(result["posts"], np.float64)
    out = np.zeros(len(want), np.float64)
    n = min(len(want), max(len(off) - 1, 0))
    if n == 0 or len(cls) == 0:
        return out
    # the entries are ordered by (frame, class): one search in the combined key
    frame_of = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    span = int(max(cls.max(), want.max(initial=0))) + 2
    key = frame_of * span + cls
    ask = np.arange(n, dtype=np.int64) * span + np.clip(want[:n], -1, span - 2)
    at = np.searchsorted(key, ask)
    hit = (at < len(key)) & (want[:n] >= 0)
    hit[hit] = key[at[hit]] == ask[hit]
    out[:n][hit] = post[at[hit]]
    return out


class WfstError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "WFST_E_?"), code, msg))
        self.code = code


class Config(C.Structure):
    """wfst_config == LatticeFasterDecoderConfig (reference
    src/my-decoder/lattice-faster-decoder-conf.h:21-44), reference defaults."""

    _fields_ = [("beam", C.c_float), ("max_active", C.c_int32), ("min_active", C.c_int32),
                ("lattice_beam", C.c_float), ("prune_interval", C.c_int32), ("beam_delta", C.c_float),
                ("hash_ratio", C.c_float), ("prune_scale", C.c_float)]

    def __init__(self, beam=16.0, max_active=2147483647, min_active=200, lattice_beam=10.0,
                 prune_interval=25, beam_delta=0.5, hash_ratio=2.0, prune_scale=0.1):
        super().__init__(beam, max_active, min_active, lattice_beam, prune_interval, beam_delta,
                         hash_ratio, prune_scale)


class EndpointRule(C.Structure):
    """wfst_endpoint_rule == Kaldi's OnlineEndpointRule."""

    _fields_ = [("must_contain_nonsilence", C.c_int32), ("min_trailing_silence", C.c_float), ("max_relative_cost", C.c_float),
                ("min_utterance_length", C.c_float)]


class _EndpointConfigC(C.Structure):
    _fields_ = [("rule", EndpointRule * 5), ("frame_shift", C.c_float), ("n_silence_phones", C.c_int32),
                ("silence_phones", C.POINTER(C.c_int32))]


class EndpointConfig(object):
    """wfst_endpoint_config == Kaldi's OnlineEndpointConfig: rules[0..4] are rule1..rule5 (dicts of must_contain_nonsilence,
    min_trailing_silence, max_relative_cost, min_utterance_length), frame_shift in seconds, silence_phones a non-empty list.
    Defaults from the library (Kaldi's)."""

    def __init__(self, silence_phones=(), frame_shift=None, rules=None):
        c = _EndpointConfigC()
        lib().wfst_endpoint_config_default(C.byref(c))
        self.rules = [dict(must_contain_nonsilence=bool(r.must_contain_nonsilence), min_trailing_silence=r.min_trailing_silence,
                           max_relative_cost=r.max_relative_cost, min_utterance_length=r.min_utterance_length) for r in c.rule]
        self.frame_shift = c.frame_shift if frame_shift is None else float(frame_shift)
        for k, r in (rules or {}).items():   # {rule index 0..4: {field: value}}
            self.rules[k].update(r)
        self.silence_phones = [int(p) for p in silence_phones]

    def as_c(self):
        """The C struct; its silence list is kept alive on the returned object."""
        c = _EndpointConfigC()
        for k, r in enumerate(self.rules):
            c.rule[k] = EndpointRule(int(bool(r["must_contain_nonsilence"])), r["min_trailing_silence"], r["max_relative_cost"],
                                     r["min_utterance_length"])
        c.frame_shift = self.frame_shift
        c._sil = np.ascontiguousarray(self.silence_phones, dtype=np.int32)
        c.n_silence_phones = int(c._sil.shape[0])
        c.silence_phones = _i32(c._sil) if c._sil.shape[0] else None
        return c

    def rule_fired(self, num_frames_decoded, trailing_frames, relative_cost):
        """wfst_endpoint_rules: the first rule (1..5) that fires for these inputs, 0 if none -- on the host."""
        r = C.c_int32()
        c = self.as_c()
        _check(lib().wfst_endpoint_rules(C.byref(c), int(num_frames_decoded), int(trailing_frames), C.c_float(relative_cost), C.byref(r)))
        return r.value


class Limits(C.Structure):
    _fields_ = [("max_frames", C.c_int32), ("max_tokens_per_frame", C.c_int32), ("arena_tokens", C.c_int64),
                ("lattice_links", C.c_int64), ("lm_pairs", C.c_int64), ("det_raw_states", C.c_int32), ("det_raw_arcs", C.c_int32),
                ("det_workspace_bytes", C.c_int64)]


class Options(C.Structure):
    """wfst_options: scheduling choices of a decoder (never a result bit); defaults from the library."""

    _fields_ = [("channel_groups", C.c_int32), ("use_hip_graph", C.c_int32), ("log2_partitions", C.c_int32),
                ("log2_lds_slots", C.c_int32), ("joint_max", C.c_int32), ("expand_workgroups", C.c_int32),
                ("insert_workgroups", C.c_int32), ("upload_slice_frames", C.c_int32), ("tile_tokens", C.c_int32), ("debug", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().wfst_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown wfst_options field %r" % k)
            setattr(self, k, int(v))


class GraphOptions(C.Structure):
    _fields_ = [("row_align_slots", C.c_int32), ("flatten_closures", C.c_int32), ("fuse_closures", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().wfst_graph_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown wfst_graph_options field %r" % k)
            setattr(self, k, int(v))


_lib = None


def lib():
    """Load libwfstdec.so; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  If
        # this library were dlopen'ed first it would bind /opt/rocm's copy and torch would then
        # bring up a second runtime ("No HIP GPUs are available").  Loading torch first lets the
        # loader satisfy our DT_NEEDED libamdhip64.so.7 with the copy already in the process.
        if os.environ.get("WFST_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        L.wfst_last_error.restype = C.c_char_p
        L.wfst_decoder_get_frontier.restype = C.c_int
        _lib = L
    return _lib


def _check(rc):
    if rc != WFST_OK:
        raise WfstError(rc, lib().wfst_last_error().decode())


def _i32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _f32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _chunk_dtype(dt):
    """WFST_DTYPE_* of a torch / numpy dtype (by name: the tensors of advance_chunk are duck-typed)."""
    name = str(dt).split(".")[-1]
    try:
        return {"float32": WFST_DTYPE_F32, "float16": WFST_DTYPE_F16, "half": WFST_DTYPE_F16, "bfloat16": WFST_DTYPE_BF16}[name]
    except KeyError:
        raise ValueError("chunks must be float32, float16 or bfloat16, not %s" % (dt,))


def device_count():
    return int(lib().wfst_device_count())


class Graph:
    """HCLG resident in HBM (replaces the reference's ``Fst``)."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def load(path, device=0, options=None):
        h = C.c_void_p()
        _check(lib().wfst_graph_load_ex(path.encode(), int(device), C.byref(options) if options is not None else None,
                                        C.byref(h)))
        return Graph(h)

    @staticmethod
    def from_arrays(start, final_state, state_info, arcs, device=0, options=None):
        si = np.ascontiguousarray(state_info)
        ar = np.ascontiguousarray(arcs)
        assert si.dtype.itemsize == 12 and ar.dtype.itemsize == 16
        h = C.c_void_p()
        _check(lib().wfst_graph_from_arrays_ex(int(start), int(final_state), int(si.shape[0]), int(ar.shape[0]),
                                               si.ctypes.data_as(C.c_void_p), ar.ctypes.data_as(C.c_void_p),
                                               int(device), C.byref(options) if options is not None else None,
                                               C.byref(h)))
        return Graph(h)

    def set_tid2pdf(self, tid2pdf):
        m = np.ascontiguousarray(tid2pdf, dtype=np.int32)
        _check(lib().wfst_graph_set_tid2pdf(self.h, _i32(m), int(m.shape[0] - 1)))

    def set_tid2phone(self, tid2phone):
        """TransitionIdToPhone as a table (entry 0 unused): what the endpoint's silence phones are looked up in."""
        m = np.ascontiguousarray(tid2phone, dtype=np.int32)
        _check(lib().wfst_graph_set_tid2phone(self.h, _i32(m), int(m.shape[0] - 1)))

    def info(self):
        s, f, ns, na = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        b = C.c_int64()
        _check(lib().wfst_graph_info(self.h, C.byref(s), C.byref(f), C.byref(ns), C.byref(na), C.byref(b)))
        return dict(start=s.value, final_state=f.value, n_states=ns.value, n_arcs=na.value, device_bytes=b.value)

    def free(self):
        if self.h:
            lib().wfst_graph_free(self.h)
            self.h = None


class AlignGraphs:
    """A set of small per-utterance graphs resident in HBM, for BatchDecoder.force_align (wfst_align_graphs)."""

    def __init__(self, handle, n_graphs):
        self.h = handle
        self.n_graphs = int(n_graphs)

    @staticmethod
    def from_arrays(graphs, device=0):
        """graphs: a list of (start, final_state, state_info, arcs), each as Graph.from_arrays takes them."""
        graphs = list(graphs)
        k = len(graphs)
        start = np.ascontiguousarray([int(g[0]) for g in graphs], dtype=np.int32)
        final = np.ascontiguousarray([int(g[1]) for g in graphs], dtype=np.int32)
        sis = [np.ascontiguousarray(g[2]) for g in graphs]
        ars = [np.ascontiguousarray(g[3]) for g in graphs]
        assert all(x.dtype.itemsize == 12 for x in sis) and all(x.dtype.itemsize == 16 for x in ars)
        ns = np.ascontiguousarray([x.shape[0] for x in sis], dtype=np.int32)
        na = np.ascontiguousarray([x.shape[0] for x in ars], dtype=np.int32)
        si = np.frombuffer(b"".join(x.tobytes() for x in sis), dtype=np.uint8)
        ar = np.frombuffer(b"".join(x.tobytes() for x in ars), dtype=np.uint8)
        h = C.c_void_p()
        _check(lib().wfst_align_graphs_create(k, _i32(start), _i32(final), _i32(ns), _i32(na),
                                              si.ctypes.data_as(C.c_void_p) if si.size else None,
                                              ar.ctypes.data_as(C.c_void_p) if ar.size else None, int(device), C.byref(h)))
        return AlignGraphs(h, k)

    @staticmethod
    def load(paths, device=0):
        """One graph per file, in any format Graph.load reads (wfst_align_graphs_load)."""
        paths = [p.encode() for p in paths]
        h = C.c_void_p()
        _check(lib().wfst_align_graphs_load(len(paths), (C.c_char_p * max(len(paths), 1))(*paths), int(device), C.byref(h)))
        return AlignGraphs(h, len(paths))

    def info(self):
        k = self.n_graphs
        n, ts, ta, b = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        v = [np.zeros(k, np.int32) for _ in range(5)]
        _check(lib().wfst_align_graphs_info(self.h, C.byref(n), C.byref(ts), C.byref(ta), *[_i32(x) for x in v], C.byref(b)))
        return dict(n_graphs=n.value, total_states=ts.value, total_arcs=ta.value, n_states=v[0], n_arcs=v[1], max_ilabel=v[2],
                    eps_depth=v[3], n_labels=v[4], device_bytes=b.value)

    def free(self):
        if self.h:
            lib().wfst_align_graphs_free(self.h)
            self.h = None


def _f64(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _flat_phrases(lists):
    """[[(words, bonus), ...], ...] as the arrays wfst_bias_lists_create takes: n_phrases per list, then the phrases' lengths,
    words and bonuses, one list after the other"""
    lists = [[(list(ws), float(b)) for ws, b in ph] for ph in lists]
    n_ph = np.ascontiguousarray([len(ph) for ph in lists], dtype=np.int32)
    ln = np.ascontiguousarray([len(ws) for ph in lists for ws, _ in ph], dtype=np.int32)
    words = np.ascontiguousarray([int(w) for ph in lists for ws, _ in ph for w in ws], dtype=np.int32)
    bonus = np.ascontiguousarray([b for ph in lists for _, b in ph], dtype=np.float64)
    return n_ph, ln, words, bonus


def bias_compile(phrases, cap_nodes=256):
    """The phrase automaton of ONE bias list [(words, bonus), ...] (wfst_bias_compile; host only, no device): dict of n_nodes and the
    nodes' parent (-1: the root), word (0: the root), fail, phrase (index in the list or -1) and beta (float64), nodes in
    breadth-first order."""
    _, ln, words, bonus = _flat_phrases([phrases])
    cap = int(cap_nodes)
    n = C.c_int32()
    v = [np.zeros(max(cap, 1), np.int32) for _ in range(4)]
    beta = np.zeros(max(cap, 1), np.float64)
    _check(lib().wfst_bias_compile(len(ln), _i32(ln), _i32(words), _f64(bonus), cap, C.byref(n), *([_i32(x) for x in v] + [_f64(beta)])))
    k = n.value
    return dict(n_nodes=k, parent=v[0][:k].copy(), word=v[1][:k].copy(), fail=v[2][:k].copy(), phrase=v[3][:k].copy(), beta=beta[:k].copy())


class BiasLists:
    """A set of bias lists resident in HBM, for BatchDecoder.biased_words (wfst_bias_lists)."""

    def __init__(self, handle, n_lists):
        self.h = handle
        self.n_lists = int(n_lists)

    @staticmethod
    def from_phrases(lists, device=0):
        """lists: [[(words, bonus), ...], ...] -- per list its phrases, each 1..16 word ids (> 0) and a bonus >= 0."""
        lists = list(lists)
        n_ph, ln, words, bonus = _flat_phrases(lists)
        h = C.c_void_p()
        _check(lib().wfst_bias_lists_create(len(lists), _i32(n_ph), _i32(ln), _i32(words), _f64(bonus), int(device), C.byref(h)))
        return BiasLists(h, len(lists))

    def info(self):
        k = self.n_lists
        n, tp, tn, b = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        v = [np.zeros(k, np.int32) for _ in range(3)]
        _check(lib().wfst_bias_lists_info(self.h, C.byref(n), C.byref(tp), C.byref(tn), *([_i32(x) for x in v] + [C.byref(b)])))
        return dict(n_lists=n.value, total_phrases=tp.value, total_nodes=tn.value, n_phrases=v[0], n_nodes=v[1], n_words=v[2],
                    device_bytes=b.value)

    def free(self):
        if self.h:
            lib().wfst_bias_lists_free(self.h)
            self.h = None


def bias_book_compile(phrases, cap_nodes=65536):
    """bias_compile for a BOOK, a bias list of up to 65 536 nodes (wfst_bias_book_compile; host only, no device)."""
    _, ln, words, bonus = _flat_phrases([phrases])
    cap = int(cap_nodes)
    n = C.c_int32()
    v = [np.zeros(max(cap, 1), np.int32) for _ in range(4)]
    beta = np.zeros(max(cap, 1), np.float64)
    _check(lib().wfst_bias_book_compile(len(ln), _i32(ln), _i32(words), _f64(bonus), cap, C.byref(n), *([_i32(x) for x in v] + [_f64(beta)])))
    k = n.value
    return dict(n_nodes=k, parent=v[0][:k].copy(), word=v[1][:k].copy(), fail=v[2][:k].copy(), phrase=v[3][:k].copy(), beta=beta[:k].copy())


class BiasBooks:
    """A set of books -- bias lists of up to 65 536 nodes -- resident in HBM, for BatchDecoder.biased_words_sparse (wfst_bias_books)."""

    def __init__(self, handle, n_books):
        self.h = handle
        self.n_books = int(n_books)

    @staticmethod
    def from_phrases(books, device=0):
        """books: [[(words, bonus), ...], ...] -- per book its phrases, each 1..16 word ids (> 0) and a bonus >= 0."""
        books = list(books)
        n_ph, ln, words, bonus = _flat_phrases(books)
        h = C.c_void_p()
        _check(lib().wfst_bias_books_create(len(books), _i32(n_ph), _i32(ln), _i32(words), _f64(bonus), int(device), C.byref(h)))
        return BiasBooks(h, len(books))

    def info(self):
        k = self.n_books
        n, tp, tn, b = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        v = [np.zeros(k, np.int32) for _ in range(3)]
        _check(lib().wfst_bias_books_info(self.h, C.byref(n), C.byref(tp), C.byref(tn), *([_i32(x) for x in v] + [C.byref(b)])))
        return dict(n_books=n.value, total_phrases=tp.value, total_nodes=tn.value, n_phrases=v[0], n_nodes=v[1], n_words=v[2],
                    device_bytes=b.value)

    def free(self):
        if self.h:
            lib().wfst_bias_books_free(self.h)
            self.h = None


class ForcedAlignment(object):
    """One channel's answer of BatchDecoder.force_align: status (WFST_OK or the CHANNEL's own error code), found, n_frames,
    path_cost / tot_score / lm_score (numpy float32), hop_arc (arc indices of the channel's graph), alignment (one class per
    frame), words and word_frame (int32 arrays)."""

    __slots__ = ("status", "found", "n_frames", "path_cost", "tot_score", "lm_score", "n_hops", "hop_arc", "alignment", "n_words",
                 "words", "word_frame")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        return "ForcedAlignment(status=%d, found=%r, n_frames=%d, path_cost=%r, n_hops=%d, n_words=%d)" % (
            self.status, self.found, self.n_frames, self.path_cost, self.n_hops, self.n_words)


class GraphPosteriors(object):
    """One channel's answer of BatchDecoder.graph_posteriors: status (WFST_OK or the CHANNEL's own error code), found, n_frames,
    log_like (float: the log of the sum over the graph's paths of exp(-cost)), n_entries, frame_off (int32, n_frames + 1), classes and posts (the
    entries of frame f are frame_off[f] .. frame_off[f + 1], by class ascending), n_distinct (int32 per frame), frame_mass (float64
    per frame) and arc_occ (float64 per arc of the channel's graph, or None).  r["frame_off"] reads a field as r.frame_off does, so
    that frame_post_lookup takes the object as it stands."""

    __slots__ = ("status", "found", "n_frames", "log_like", "n_entries", "n_arcs", "frame_off", "classes", "posts", "n_distinct",
                 "frame_mass", "arc_occ")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def __getitem__(self, key):
        return getattr(self, key)

    def __repr__(self):
        return "GraphPosteriors(status=%d, found=%r, n_frames=%d, log_like=%r, n_entries=%d)" % (
            self.status, self.found, self.n_frames, self.log_like, self.n_entries)


class Lm:
    """A back-off n-gram LM automaton resident in HBM (replaces the reference's ``ArpaLm``); `scale`
    is ArpaLm::Rescale -- the biglm CLI loads the OLD LM with -1."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def load(path, scale=1.0, device=0):
        h = C.c_void_p()
        _check(lib().wfst_lm_load(path.encode(), C.c_float(scale), int(device), C.byref(h)))
        return Lm(h)

    @staticmethod
    def from_arrays(bos, eos, unk, states, arcs, scale=1.0, device=0):
        st = np.ascontiguousarray(states)
        ar = np.ascontiguousarray(arcs)
        assert st.dtype.itemsize == 12 and ar.dtype.itemsize == 12
        h = C.c_void_p()
        _check(lib().wfst_lm_from_arrays(int(bos), int(eos), int(unk), int(st.shape[0]), st.ctypes.data_as(C.c_void_p),
                                         int(ar.shape[0]), ar.ctypes.data_as(C.c_void_p), C.c_float(scale), int(device), C.byref(h)))
        return Lm(h)

    def info(self):
        v = [C.c_int32() for _ in range(5)]
        b = C.c_int64()
        _check(lib().wfst_lm_info(self.h, *[C.byref(x) for x in v], C.byref(b)))
        return dict(bos=v[0].value, eos=v[1].value, n_states=v[2].value, n_arcs=v[3].value, n_words=v[4].value, device_bytes=b.value)

    def table_stats(self):
        """The device (state, word) table as the upload left it (wfst_lm_table_stats): table_size slots, `used` occupied,
        longest_run (cyclic) of occupied slots, max_displacement of an entry from its home slot, wraps (a run over the last slot and slot 0)."""
        size = C.c_int64()
        v = [C.c_int32() for _ in range(4)]
        _check(lib().wfst_lm_table_stats(self.h, C.byref(size), *[C.byref(x) for x in v]))
        return dict(table_size=size.value, used=v[0].value, longest_run=v[1].value, max_displacement=v[2].value, wraps=bool(v[3].value))

    def free(self):
        if self.h:
            lib().wfst_lm_free(self.h)
            self.h = None


class BatchDecoder:
    """A batch of decoding channels (one channel == one reference decoder object).  old_lm / new_lm:
    biglm mode (the reference's OnlineLatticeDecoderMempoolBiglm)."""

    def __init__(self, graph, cfg, n_channels, max_frames=0, max_tokens_per_frame=0, arena_tokens=0, stream=None,
                 lattice_links=0, options=None, old_lm=None, new_lm=None, lm_pairs=0, det_raw_states=0, det_raw_arcs=0,
                 det_workspace_bytes=0):
        self.graph = graph
        self.n = int(n_channels)
        lim = Limits(int(max_frames), int(max_tokens_per_frame), int(arena_tokens), int(lattice_links), int(lm_pairs),
                     int(det_raw_states), int(det_raw_arcs), int(det_workspace_bytes))
        self.lattice_links = int(lattice_links)
        h = C.c_void_p()
        _check(lib().wfst_decoder_create_biglm(graph.h, C.byref(cfg), self.n, C.byref(lim),
                                               C.byref(options) if options is not None else None,
                                               old_lm.h if old_lm is not None else None, new_lm.h if new_lm is not None else None,
                                               C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self._score_cols = 0   # columns of a row of the library-held history (scores())

    def free(self):
        if self.h:
            lib().wfst_decoder_free(self.h)
            self.h = None

    def _chan(self, channels):
        if channels is None:
            return None, 0
        ch = np.ascontiguousarray(channels, dtype=np.int32)
        return ch, int(ch.shape[0])

    def init(self, channels=None):
        ch, n = self._chan(channels)
        _check(lib().wfst_decoder_init(self.h, _i32(ch), n))

    def advance(self, ll_ptrs, n_frames_ready, stride, channels=None, max_num_frames=-1):
        """ll_ptrs: device addresses (ints) of row 0 of each listed channel's matrix."""
        ch, n = self._chan(channels)
        cnt = n if ch is not None else self.n
        ptrs = (C.c_void_p * cnt)(*[int(p) for p in ll_ptrs])
        nr = np.ascontiguousarray(n_frames_ready, dtype=np.int32)
        assert nr.shape[0] == cnt
        _check(lib().wfst_decoder_advance(self.h, _i32(ch), n, ptrs, _i32(nr), int(stride), int(max_num_frames)))

    def advance_host(self, mats, n_frames_ready, channels=None, max_num_frames=-1):
        """mats: list of C-contiguous float32 [frames][stride] numpy arrays (host)."""
        ch, n = self._chan(channels)
        cnt = n if ch is not None else self.n
        mats = [np.ascontiguousarray(m, dtype=np.float32) for m in mats]
        stride = int(mats[0].shape[1])
        assert all(m.shape[1] == stride for m in mats)
        ptrs = (C.c_void_p * cnt)(*[m.ctypes.data for m in mats])
        nr = np.ascontiguousarray(n_frames_ready, dtype=np.int32)
        self._score_cols = stride
        _check(lib().wfst_decoder_advance_host(self.h, _i32(ch), n, ptrs, _i32(nr), stride, int(max_num_frames)))

    def set_score_transform(self, acoustic_scale=1.0, log_priors=None):
        """What advance_chunk makes of a raw value x in column j: (float32(x) - log_priors[j]) * acoustic_scale
        (wfst_decoder_set_score_transform).  Not while an utterance holds ingested frames."""
        pri = None if log_priors is None else np.ascontiguousarray(log_priors, dtype=np.float32).reshape(-1)
        _check(lib().wfst_decoder_set_score_transform(self.h, C.c_float(acoustic_scale), _f32(pri), 0 if pri is None else int(pri.shape[0])))

    def advance_chunk(self, chunks, channels=None, max_num_frames=-1, stream="current"):
        """Hands the NEW rows of each listed channel over where the acoustic model left them (wfst_decoder_advance_chunk).
        chunks: per listed channel a 2-D device tensor [new frames][n_cols] -- anything with data_ptr(), shape, stride() and
        dtype; float32, float16 or bfloat16, the last dimension contiguous, one dtype and width for all -- or None (no rows).
        stream: "current" = torch's current stream, whose enqueued work writes the rows; a raw hipStream_t (int); None = the
        rows are complete and kept by the caller until sync() or a getter (WFST_STREAM_NONE)."""
        ch, n = self._chan(channels)
        cnt = n if ch is not None else self.n
        chunks = list(chunks)
        assert len(chunks) == cnt
        dtype = cols = None
        ptrs, nf, pitch = (C.c_void_p * cnt)(), np.zeros(cnt, np.int32), np.zeros(cnt, np.int64)
        for i, t in enumerate(chunks):
            if t is None:
                continue
            if len(t.shape) != 2:
                raise ValueError("chunk %d is not 2-D" % i)
            dt = _chunk_dtype(t.dtype)
            if dtype is None:
                dtype, cols = dt, int(t.shape[1])
            if dt != dtype or int(t.shape[1]) != cols:
                raise ValueError("chunks differ in dtype or width")
            if int(t.shape[0]) == 0:
                continue
            st = t.stride()
            if cols > 1 and int(st[1]) != 1:
                raise ValueError("the last dimension of chunk %d is not contiguous" % i)
            ptrs[i] = int(t.data_ptr())
            nf[i] = int(t.shape[0])
            pitch[i] = int(st[0]) if int(t.shape[0]) > 1 else max(int(st[0]), cols)
        if dtype is None:
            raise ValueError("no chunk to take the dtype and width from")
        pitch[nf == 0] = cols
        if stream == "current":
            import torch
            stream = int(torch.cuda.current_stream().cuda_stream)
        elif stream is None:
            stream = WFST_STREAM_NONE
        self._score_cols = cols
        _check(lib().wfst_decoder_advance_chunk(self.h, _i32(ch), n, ptrs, _i32(nf), pitch.ctypes.data_as(C.POINTER(C.c_int64)), dtype, cols,
                                                C.c_void_p(int(stream)), int(max_num_frames)))

    def scores(self, channel, first_frame, n_frames):
        """Rows of the channel's library-held score history as float32 [n_frames][n_cols] (wfst_decoder_get_scores); for tests."""
        out = np.empty((int(n_frames), self._score_cols), np.float32)
        _check(lib().wfst_decoder_get_scores(self.h, int(channel), int(first_frame), int(n_frames), _f32(out)))
        return out

    def finalize(self, channels=None):
        ch, n = self._chan(channels)
        _check(lib().wfst_decoder_finalize(self.h, _i32(ch), n))

    def sync(self):
        _check(lib().wfst_decoder_sync(self.h))

    def num_frames_decoded(self, channel):
        return int(lib().wfst_decoder_num_frames_decoded(self.h, int(channel)))

    def best_paths(self, channels=None, use_final_probs=True, cap=2048):
        """Returns one dict per listed channel: ok, ilabel, olabel, graph, ac, words, tids,
        tot_score, lm_score (LatticeToVector applied to the hop list)."""
        ch, n = self._chan(channels)
        cnt = n if ch is not None else self.n
        il = np.empty((cnt, cap), np.int32)    # (the call fills all of it)
        ol = np.empty((cnt, cap), np.int32)
        g = np.empty((cnt, cap), np.float32)
        ac = np.empty((cnt, cap), np.float32)
        nh = np.zeros(cnt, np.int32)
        _check(lib().wfst_decoder_get_best_path(self.h, _i32(ch), n, int(bool(use_final_probs)), int(cap),
                                                _i32(il), _i32(ol), _f32(g), _f32(ac), _i32(nh)))
        # LatticeToVector (newfst/lattice-functions.cc:179-217) for all channels at once: the float32 running sums
        # tot += (g + a), lm += g in forward order, by the C entry point (tests/test_capi_symbols.py holds it against
        # wfst_lattice_to_vector and against numpy's sequential cumsum)
        tot_s = np.zeros(cnt, np.float32)
        lm_s = np.zeros(cnt, np.float32)
        nw, nt = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32)
        _check(lib().wfst_lattice_to_vector_batch(_i32(il), _i32(ol), _f32(g), _f32(ac), _i32(nh), cnt, int(cap), _f32(tot_s), _f32(lm_s),
                                                  _i32(nw), _i32(nt)))
        words, tids = np.empty(max(1, int(nw.sum())), np.int32), np.empty(max(1, int(nt.sum())), np.int32)
        woff, toff = np.zeros(cnt + 1, np.int32), np.zeros(cnt + 1, np.int32)
        _check(lib().wfst_lattice_labels_batch(_i32(il), _i32(ol), _i32(nh), cnt, int(cap), _i32(words), _i32(woff), _i32(tids), _i32(toff)))
        return _BestPaths(il, ol, g, ac, nh, tot_s, lm_s, words, woff, tids, toff)

    def stats(self, channel):
        s = (C.c_int64 * 8)()
        _check(lib().wfst_decoder_get_stats(self.h, int(channel), s))
        lat = self.lattice_links > 0
        return dict(frames=s[0], N=s[1], E=s[2], Z=s[3], tokens=s[4], peak_tokens=s[5], records=s[6], links=s[7] if lat else 0,
                    collections=0 if lat else s[7])

    def degraded_frames(self, channel):
        """Frames of the utterance on which the per-frame token limit acted as a max_active (wfst_decoder_get_degraded_frames)."""
        n = C.c_int32(0)
        _check(lib().wfst_decoder_get_degraded_frames(self.h, int(channel), C.byref(n)))
        return int(n.value)

    def busy(self):
        """1 while work enqueued on the decoder's stream has not finished, else 0 (wfst_decoder_busy; never blocks)."""
        rc = lib().wfst_decoder_busy(self.h)
        if rc < 0:
            _check(rc)
        return int(rc)

    def calls_in_flight(self):
        """How many enqueued init / advance / finalize calls have not finished (wfst_decoder_calls_in_flight; never blocks)."""
        rc = lib().wfst_decoder_calls_in_flight(self.h)
        if rc < 0:
            _check(rc)
        return int(rc)

    def determinizer_ms(self, channel):
        """Device time of the channel's own determinization (wfst_decoder_get_determinizer_ms); None if no lattice of it is held."""
        ms = C.c_float(0)
        rc = lib().wfst_decoder_get_determinizer_ms(self.h, int(channel), C.byref(ms))
        return float(ms.value) if rc == WFST_OK else None

    def prune_raw_abandoned(self, channel):
        """Back-pruning passes whose several-workgroup raw pricing was abandoned and done over by the one-workgroup walk (-1: that pass is off)."""
        n = C.c_int32(0)
        _check(lib().wfst_decoder_get_prune_raw_abandoned(self.h, int(channel), C.byref(n)))
        return int(n.value)

    def lattice_stats(self, channel):
        s = (C.c_int64 * 5)()
        _check(lib().wfst_decoder_get_lattice_stats(self.h, int(channel), s))
        return dict(links_recorded=s[0], walk_links=s[1], walk_tokens=s[2], compaction_scanned=s[3], compaction_moved=s[4])

    def raw_lattice(self, channel, use_final_probs=True):
        """GetRawLattice of a finalized channel (lattice mode).  Returns a dict of numpy arrays, or
        None for the reference's `return false`."""
        ns, na = C.c_int32(0), C.c_int32(0)
        rc = lib().wfst_decoder_get_raw_lattice(self.h, int(channel), int(bool(use_final_probs)), 0, 0, C.byref(ns),
                                                C.byref(na), *([None] * 10))
        if rc != WFST_OK and not (rc == -4 and ns.value > 0):  # -4 with sizes = "give me bigger buffers"
            _check(rc)
        if ns.value == 0:
            return None
        S, A = ns.value, na.value
        fin, fr, gs = (np.zeros(S, np.int32) for _ in range(3))
        co = np.zeros(S, np.float32)
        src, dst, il, ol = (np.zeros(A, np.int32) for _ in range(4))
        gr, ac = np.zeros(A, np.float32), np.zeros(A, np.float32)
        _check(lib().wfst_decoder_get_raw_lattice(self.h, int(channel), int(bool(use_final_probs)), S, A, C.byref(ns),
                                                  C.byref(na), _i32(fin), _i32(fr), _i32(gs), _f32(co), _i32(src), _i32(dst),
                                                  _i32(il), _i32(ol), _f32(gr), _f32(ac)))
        return dict(n_states=S, st_final=fin, st_frame=fr, st_state=gs, st_cost=co, a_src=src, a_dst=dst, a_ilabel=il,
                    a_olabel=ol, a_graph=gr, a_acoustic=ac)

    def prefetch_determinized(self, detached=False, nbest=0):
        """Start the determinization of every finalized channel now, on a side stream (wfst_decoder_prefetch_determinized):
        best_paths() / nbest() run beside it, determinized_lattice(c) finds the work done or waits.  detached=True: init /
        advance / finalize do not wait for it either -- the channels decode their next utterances beside it -- and the lattices
        are fetched with prefetched_lattice(c) (wfst_decoder_prefetch_determinized_detached)."""
        if nbest > 0:   # GetNbest behind GetLattice on the determinizer's stream (wfst_decoder_prefetch_nbest)
            _check(lib().wfst_decoder_prefetch_nbest(self.h, int(nbest), int(bool(detached))))
            return
        _check((lib().wfst_decoder_prefetch_determinized_detached if detached else lib().wfst_decoder_prefetch_determinized)(self.h))

    def _nbest_fetch_all(self, f, extra, n):
        """f(handle, channel, *extra, cap_paths, cap_arcs, &n_paths, &total_arcs, off, tot, olabel, graph, acoustic) for every channel, over
        one buffer: per channel a list of dicts {words, olabel, graph, acoustic, tot} in ascending cost (words = the nonzero olabels), or
        None where the call reports no result."""
        K, A = int(n), int(n) * 256
        stride = (K + 1) + K + 3 * A
        buf = np.zeros((self.n, stride), np.int32)
        base = buf.ctypes.data
        npth, na = C.c_int32(0), C.c_int32(0)
        pn, pa = C.byref(npth), C.byref(na)
        vp = C.c_void_p
        fbuf = buf.view(np.float32)
        found = np.full(self.n, -1, np.int32)
        for c in range(self.n):
            p = base + 4 * stride * c
            rc = f(self.h, c, *extra, K, A, pn, pa, vp(p), vp(p + 4 * (K + 1)), vp(p + 4 * (2 * K + 1)), vp(p + 4 * (2 * K + 1 + A)), vp(p + 4 * (2 * K + 1 + 2 * A)))
            if rc == WFST_OK:
                found[c] = npth.value
        o0 = 2 * K + 1

        def make(c):   # (the dicts of a channel are put together when the channel is first looked at: _LazyList)
            k = int(found[c])
            if k < 0:
                return None
            off = buf[c, : k + 1]
            paths = []
            for i in range(k):
                a, b = int(off[i]), int(off[i + 1])
                ol = buf[c, o0 + a:o0 + b]
                paths.append(dict(olabel=ol, words=ol[ol != 0], graph=fbuf[c, o0 + A + a:o0 + A + b], acoustic=fbuf[c, o0 + 2 * A + a:o0 + 2 * A + b],
                                  tot=float(fbuf[c, K + 1 + i])))
            return paths

        return _LazyList(self.n, make)

    def prefetched_nbest(self, n):
        """The n-best paths a harvested detached prefetch (prefetch_determinized(detached=True, nbest=n)) computed, for every channel."""
        return self._nbest_fetch_all(lib().wfst_decoder_get_prefetched_nbest_paths, (), n)

    def nbest_paths_all(self, n, use_final_probs=True):
        """nbest_paths(c, n) for every channel in one sweep (after prefetch_determinized(nbest=n) or nbest_paths_batch(n): no device work)."""
        return self._nbest_fetch_all(lib().wfst_decoder_get_nbest_paths, (int(n), int(bool(use_final_probs)), None, None), n)

    def harvest_prefetched(self):
        """Wait for a prefetch in flight and take its lattices over (wfst_decoder_harvest_prefetched)."""
        _check(lib().wfst_decoder_harvest_prefetched(self.h))

    def prefetched_lattice(self, channel):
        """The determinized lattice the last HARVESTED detached prefetch made of `channel`'s utterance (never waits: right behind
        the prefetch call for utterance k it returns utterance k - 1's)."""
        return self._det_fetch(lambda *a: lib().wfst_decoder_get_prefetched_lattice(self.h, int(channel), *a))

    def determinized_lattice(self, channel, use_final_probs=True):
        """GetLattice (GetRawLattice + DeterminizeLatticeWrapper) of a channel: dict of numpy arrays, or None."""
        return self._det_fetch(lambda *a: lib().wfst_decoder_get_determinized_lattice(self.h, int(channel), int(bool(use_final_probs)), *a))

    def prefetched_lattices(self):
        """prefetched_lattice(c) for every channel, in one sweep over one buffer (the per-call work of the binding -- seven pointer
        casts, an allocation, a closure -- is most of what a lattice of a hundred states costs to fetch)."""
        return self._det_fetch_all(lib().wfst_decoder_get_prefetched_lattice, ())

    def determinized_lattices(self, use_final_probs=True):
        """determinized_lattice(c) for every channel (the first call runs the determinizer for all finalized channels)."""
        return self._det_fetch_all(lib().wfst_decoder_get_determinized_lattice, (int(bool(use_final_probs)),))

    def _det_fetch_all(self, f, extra):
        S, A = 1024, 2048
        stride = S + 6 * A
        buf = np.empty((self.n, stride), np.int32)
        base = buf.ctypes.data
        ns, na = C.c_int32(0), C.c_int32(0)
        pns, pna = C.byref(ns), C.byref(na)
        vp = C.c_void_p
        out = [None] * self.n
        for c in range(self.n):
            p = base + 4 * stride * c
            rc = f(self.h, c, *extra, S, A, pns, pna, vp(p), vp(p + 4 * S), vp(p + 4 * (S + A)), vp(p + 4 * (S + 2 * A)), vp(p + 4 * (S + 3 * A)),
                   vp(p + 4 * (S + 4 * A)), vp(p + 4 * (S + 5 * A)))
            if rc != WFST_OK:   # (larger than the common case, or an error: the careful path)
                out[c] = self._det_fetch(lambda *a: f(self.h, c, *extra, *a))
                continue
            s_, a_ = ns.value, na.value
            if s_ == 0:
                continue
            row = buf[c]
            out[c] = dict(n_states=s_, st_final=row[:s_], a_src=row[S:S + a_], a_dst=row[S + A:S + A + a_], a_ilabel=row[S + 2 * A:S + 2 * A + a_],
                          a_olabel=row[S + 3 * A:S + 3 * A + a_], a_graph=row[S + 4 * A:S + 4 * A + a_].view(np.float32),
                          a_acoustic=row[S + 5 * A:S + 5 * A + a_].view(np.float32))
        return out

    def _det_fetch(self, call):
        ns, na = C.c_int32(0), C.c_int32(0)
        S, A = 1024, 2048   # (a determinized lattice is a narrow chain: one call as a rule; a second one with the sizes it returned otherwise)
        for attempt in range(2):
            buf = np.empty(S + 6 * A, np.int32)   # one block per call: final flags | src | dst | ilabel | olabel | graph | acoustic
            p = buf.ctypes.data
            I32, F32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
            at = lambda k, T: C.cast(p + 4 * (S + k * A), T)
            rc = call(S, A, C.byref(ns), C.byref(na), C.cast(p, I32), at(0, I32), at(1, I32), at(2, I32), at(3, I32), at(4, F32), at(5, F32))
            if rc == -4 and attempt == 0 and (ns.value > S or na.value > A):
                S, A = max(S, ns.value), max(A, na.value)
                continue
            _check(rc)
            break
        if ns.value == 0:
            return None
        s_, a_ = ns.value, na.value
        seg = lambda k: buf[S + k * A: S + k * A + a_]
        return dict(n_states=s_, st_final=buf[:s_], a_src=seg(0), a_dst=seg(1), a_ilabel=seg(2), a_olabel=seg(3),
                    a_graph=seg(4).view(np.float32), a_acoustic=seg(5).view(np.float32))

    def rescored_lattice(self, channel, old_lm, new_lm, use_final_probs=True):
        """GetLattice under --use-second: determinized lattice o old LM (scale -1) o new LM, composed on the device."""
        ns, na = C.c_int32(0), C.c_int32(0)
        rc = lib().wfst_decoder_get_rescored_lattice(self.h, int(channel), int(bool(use_final_probs)), old_lm.h, new_lm.h, 0, 0,
                                                     C.byref(ns), C.byref(na), *([None] * 7))
        if rc != WFST_OK and not (rc == -4 and ns.value > 0):
            _check(rc)
        if ns.value == 0:
            return None
        S, A = ns.value, na.value
        fin = np.zeros(S, np.int32)
        src, dst, il, ol = (np.zeros(A, np.int32) for _ in range(4))
        gr, ac = np.zeros(A, np.float32), np.zeros(A, np.float32)
        _check(lib().wfst_decoder_get_rescored_lattice(self.h, int(channel), int(bool(use_final_probs)), old_lm.h, new_lm.h, S, A,
                                                       C.byref(ns), C.byref(na), _i32(fin), _i32(src), _i32(dst), _i32(il), _i32(ol),
                                                       _f32(gr), _f32(ac)))
        return dict(n_states=S, st_final=fin, a_src=src, a_dst=dst, a_ilabel=il, a_olabel=ol, a_graph=gr, a_acoustic=ac)

    def rescore_lattices(self, old_lm, new_lm, channels=None, use_final_probs=True):
        """The second LM pass of a BATCH of finalized channels (None: all of them) in one launch per stage
        (wfst_decoder_rescore_lattices); rescored_lattice(c, ...) with the same LMs then returns the kept result."""
        ch = None if channels is None else np.ascontiguousarray(channels, np.int32)
        _check(lib().wfst_decoder_rescore_lattices(self.h, _i32(ch) if ch is not None else None, 0 if ch is None else len(ch),
                                                   int(bool(use_final_probs)), old_lm.h, new_lm.h))

    def nbest_paths_batch(self, n, old_lm=None, new_lm=None, channels=None, use_final_probs=True):
        """GetNbest of a BATCH of finalized channels (None: all of them): one launch per stage (wfst_decoder_nbest_paths_batch);
        nbest_paths(c, n, ...) with the same arguments then returns the kept result."""
        ch = None if channels is None else np.ascontiguousarray(channels, np.int32)
        _check(lib().wfst_decoder_nbest_paths_batch(self.h, _i32(ch) if ch is not None else None, 0 if ch is None else len(ch), int(n),
                                                    int(bool(use_final_probs)), old_lm.h if old_lm is not None else None,
                                                    new_lm.h if new_lm is not None else None))

    def nbest_paths(self, channel, n, old_lm=None, new_lm=None, use_final_probs=True):
        """GetNbest as lattices: NShortestPath over the determinized lattice (with LMs: over its second-pass rescoring), on the
        device.  List of paths in ascending cost, each dict(olabel, graph, acoustic: per-arc arrays front to back, the last arc
        the final weight's; tot: the path's cost)."""
        npth, na = C.c_int32(0), C.c_int32(0)
        lm1 = old_lm.h if old_lm is not None else None
        lm2 = new_lm.h if new_lm is not None else None
        K, A = int(n), min(int(n) * 256, 1 << 22)   # (one call in the common case; a second one with the sizes it returned otherwise)
        for attempt in range(2):
            off = np.zeros(K + 1, np.int32)
            tot = np.zeros(K, np.float32)
            ol = np.zeros(A, np.int32)
            gr, ac = np.zeros(A, np.float32), np.zeros(A, np.float32)
            rc = lib().wfst_decoder_get_nbest_paths(self.h, int(channel), int(n), int(bool(use_final_probs)), lm1, lm2, K, A,
                                                    C.byref(npth), C.byref(na), _i32(off), _f32(tot), _i32(ol), _f32(gr), _f32(ac))
            if rc == -4 and attempt == 0 and (npth.value > K or na.value > A):
                K, A = max(K, npth.value), max(A, na.value)
                continue
            _check(rc)
            break
        K = npth.value
        return [dict(olabel=ol[off[i]:off[i + 1]].copy(), graph=gr[off[i]:off[i + 1]].copy(), acoustic=ac[off[i]:off[i + 1]].copy(),
                     tot=float(tot[i])) for i in range(K)]

    def determinizer_slots(self):
        """(lattices one determinize launch takes, bytes of one workspace slot) (wfst_decoder_get_determinizer_slots)."""
        s, b = C.c_int32(0), C.c_int64(0)
        _check(lib().wfst_decoder_get_determinizer_slots(self.h, C.byref(s), C.byref(b)))
        return s.value, b.value

    def set_live_lattice_prune(self, on):
        """on: the live getters (raw_lattice, determinized_lattice, rescored_lattice, nbest_paths, nbest_words, nbest on a channel
        that is not finalized) serve the lattice the channel would hold if the utterance ended at this frame -- FinalizeDecoding's
        pruning on a snapshot, the channel itself untouched -- instead of everything alive (wfst_decoder_set_live_lattice_prune)."""
        _check(lib().wfst_decoder_set_live_lattice_prune(self.h, 1 if on else 0))

    def live_lattice_prune(self):
        """(mode, bytes of the snapshot scratch) (wfst_decoder_get_live_lattice_prune)."""
        m, b = C.c_int32(0), C.c_int64(0)
        _check(lib().wfst_decoder_get_live_lattice_prune(self.h, C.byref(m), C.byref(b)))
        return m.value, b.value

    def nbest_words(self, n_paths, channels=None, old_lm=None, new_lm=None, use_final_probs=True, cap_words=256):
        """GetNbestTxt of a LIST of channels (None: all), live and finalized ones mixed, in one launch per stage
        (wfst_decoder_get_nbest_words): per channel (status, [dict(words, tot, lm, path_tot)]), cheapest path first -- what
        nbest_paths(c, n_paths, ...) + wfst_lattice_to_vector give, the text made on the device.  status: WFST_OK or the channel's own
        error code; with WFST_E_CAPACITY for words (more than cap_words on a path) the dicts carry n_words, the needed size."""
        ch = np.arange(self.n, dtype=np.int32) if channels is None else np.ascontiguousarray(channels, np.int32)
        cnt, n = len(ch), int(n_paths)
        status, got = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32)
        nw = np.zeros((cnt, max(n, 1)), np.int32)
        words = np.zeros((cnt, max(n, 1), max(int(cap_words), 1)), np.int32)
        tot, lm, ptot = (np.zeros((cnt, max(n, 1)), np.float32) for _ in range(3))
        _check(lib().wfst_decoder_get_nbest_words(self.h, _i32(ch), cnt, n, int(bool(use_final_probs)),
                                                  old_lm.h if old_lm is not None else None, new_lm.h if new_lm is not None else None,
                                                  int(cap_words), _i32(status), _i32(got), _i32(nw), _i32(words), _f32(tot), _f32(lm), _f32(ptot)))
        return [(int(status[i]), [dict(words=words[i, k, : min(int(nw[i, k]), int(cap_words))].copy(), n_words=int(nw[i, k]), tot=np.float32(tot[i, k]),
                                       lm=np.float32(lm[i, k]), path_tot=np.float32(ptot[i, k])) for k in range(int(got[i]))])
                for i in range(cnt)]

    def _pack_seqs(self, seqs, channels, what):
        """The inputs of a word query (align_words, nearest_words, word_confidences): (ch, cnt, ns, cap, words, lens) -- the channel
        list (None: all), its length, the most sequences of a channel and the most words of a sequence (at least 1), words[cnt][ns][cap]
        padded with 0 and lens[cnt][ns] (-1: None, or no such sequence).  what: "sequences" / "references", for the error."""
        ch = np.arange(self.n, dtype=np.int32) if channels is None else np.ascontiguousarray(channels, np.int32)
        cnt = len(ch)
        if len(seqs) != cnt:
            raise ValueError("one list of %s per listed channel" % what)
        ns = max([len(s) for s in seqs] + [1])
        cap = max([len(w) for s in seqs for w in s if w is not None] + [1])
        words = np.zeros((cnt, ns, cap), np.int32)
        lens = np.full((cnt, ns), -1, np.int32)
        for i, s in enumerate(seqs):
            for q, w in enumerate(s):
                if w is not None:
                    lens[i, q] = len(w)
                    words[i, q, :len(w)] = np.asarray(w, np.int32)
        return ch, cnt, ns, cap, words, lens

    @staticmethod
    def _word_results(cnt, ns, width):
        """The result arrays the word queries share: status[cnt], found, n_arcs [cnt][ns], begin, end [cnt][ns][width], tot, lm."""
        pair = lambda t: np.zeros((cnt, ns), t)
        return (np.zeros(cnt, np.int32), pair(np.int32), pair(np.int32), np.zeros((cnt, ns, width), np.int32), np.zeros((cnt, ns, width), np.int32),
                pair(np.float32), pair(np.float32))

    def align_words(self, seqs, channels=None, use_final_probs=True, max_cells=0):
        """Lattice-constrained word alignment of a LIST of channels (None: all), live and finalized ones mixed
        (wfst_decoder_align_words): seqs[i] = the word sequences to align on channels[i] (each a sequence of word ids > 0, possibly
        empty; None: skipped).  Per channel a list with one dict per sequence: found, begin / end (int32 arrays, frames, end
        exclusive), tot, lm (float32: the aligned path's LatticeToVector scores), n_arcs, and status -- WFST_OK or the CHANNEL's
        own error code (then nothing of it is found)."""
        ch, cnt, ns, cap, words, lens = self._pack_seqs(seqs, channels, "sequences")
        status, found, na, begin, end, tot, lm = self._word_results(cnt, ns, cap)
        _check(lib().wfst_decoder_align_words(self.h, _i32(ch), cnt, int(bool(use_final_probs)), ns, cap, _i32(words), _i32(lens),
                                              C.c_int64(int(max_cells)), _i32(status), _i32(found), _i32(na), _i32(begin), _i32(end),
                                              _f32(tot), _f32(lm)))
        return [[dict(found=bool(found[i, q]), begin=begin[i, q, :max(int(lens[i, q]), 0)].copy(), end=end[i, q, :max(int(lens[i, q]), 0)].copy(),
                      tot=np.float32(tot[i, q]), lm=np.float32(lm[i, q]), n_arcs=int(na[i, q]), status=int(status[i]))
                 for q in range(len(seqs[i]))] for i in range(cnt)]

    def nearest_words(self, refs, channels=None, use_final_probs=True, max_cells=0, cap_hyp=0):
        """Lattice edit distance of a LIST of channels (None: all), live and finalized ones mixed (wfst_decoder_nearest_words):
        refs[i] = the reference word sequences for channels[i] (each a sequence of word ids > 0, possibly empty; None: skipped).  Per
        channel a list with one dict per reference -- the lattice path nearest it: found, n_err, n_cor, n_sub, n_ins, n_del, n_arcs,
        n_hyp, hyp_words, begin / end (int32 arrays per hypothesis word, frames, end exclusive; min(n_hyp, cap_hyp) entries),
        ref_hyp (per reference word the hypothesis word's index, -1: deleted), tot, lm (float32) and status -- WFST_OK or the
        CHANNEL's own error code.  cap_hyp = 0: room for every path -- the call is made again, with n_hyp's room, if a path
        has more words than the first guess (the longest reference + 16) holds; a cap_hyp of the caller's is taken as it is."""
        ch, cnt, ns, cap, words, lens = self._pack_seqs(refs, channels, "references")
        hcap = int(cap_hyp) if cap_hyp else cap + 16
        while True:
            status, found, na, begin, end, tot, lm = self._word_results(cnt, ns, hcap)
            ne, nc, nsub, ni, ndel, nh = (np.zeros((cnt, ns), np.int32) for _ in range(6))
            hyp, rh = np.zeros((cnt, ns, hcap), np.int32), np.zeros((cnt, ns, cap), np.int32)
            _check(lib().wfst_decoder_nearest_words(self.h, _i32(ch), cnt, int(bool(use_final_probs)), ns, cap, _i32(words), _i32(lens), hcap,
                                                    C.c_int64(int(max_cells)), _i32(status), _i32(found), _i32(ne), _i32(nc), _i32(nsub),
                                                    _i32(ni), _i32(ndel), _i32(na), _i32(nh), _i32(hyp), _i32(begin), _i32(end), _i32(rh),
                                                    _f32(tot), _f32(lm)))
            if cap_hyp or int(nh.max()) <= hcap:
                break
            hcap = int(nh.max())   # (a path with more words than the guess: once more, with room for it)
        out = []
        for i in range(cnt):
            row = []
            for q in range(len(refs[i])):
                m, ln = min(int(nh[i, q]), hcap), max(int(lens[i, q]), 0)
                row.append(dict(found=bool(found[i, q]), n_err=int(ne[i, q]), n_cor=int(nc[i, q]), n_sub=int(nsub[i, q]), n_ins=int(ni[i, q]),
                                n_del=int(ndel[i, q]), n_arcs=int(na[i, q]), n_hyp=int(nh[i, q]), hyp_words=hyp[i, q, :m].copy(),
                                begin=begin[i, q, :m].copy(), end=end[i, q, :m].copy(), ref_hyp=rh[i, q, :ln].copy(),
                                tot=np.float32(tot[i, q]), lm=np.float32(lm[i, q]), status=int(status[i])))
            out.append(row)
        return out

    def word_confidences(self, seqs, channels=None, use_final_probs=True, graph_scale=1.0, acoustic_scale=1.0, max_cells=0):
        """Word confidences from the posteriors of the raw lattice, for a LIST of channels (None: all), live and finalized ones mixed
        (wfst_decoder_word_confidence): seqs[i] = the word sequences on channels[i], as align_words takes them.  Per channel a list
        with one dict per sequence: align_words' fields (found, begin, end, tot, lm, n_arcs, status: the aligned path's own, unscaled)
        plus word_post (float64 per word: the posterior mass of the arcs that say the word in the word's cell of the time axis,
        unclamped), conf = min(1, word_post), path_logpost (the log posterior of the aligned path) and log_z (the channel's).  The
        arcs cost graph_scale * graph + acoustic_scale * acoustic, in float64; the sums' order is the device's, so the floats are
        reproducible to rounding, not bit for bit."""
        ch, cnt, ns, cap, words, lens = self._pack_seqs(seqs, channels, "sequences")
        status, found, na, begin, end, tot, lm = self._word_results(cnt, ns, cap)
        log_z, wp, plp = np.zeros(cnt, np.float64), np.zeros((cnt, ns, cap), np.float64), np.zeros((cnt, ns), np.float64)
        f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _check(lib().wfst_decoder_word_confidence(self.h, _i32(ch), cnt, int(bool(use_final_probs)), C.c_double(float(graph_scale)),
                                                  C.c_double(float(acoustic_scale)), ns, cap, _i32(words), _i32(lens),
                                                  C.c_int64(int(max_cells)), _i32(status), f64(log_z), _i32(found), _i32(na), _i32(begin),
                                                  _i32(end), f64(wp), f64(plp), _f32(tot), _f32(lm)))
        out = []
        for i in range(cnt):
            row = []
            for q in range(len(seqs[i])):
                ln = max(int(lens[i, q]), 0)
                post = wp[i, q, :ln].copy()
                row.append(dict(found=bool(found[i, q]), begin=begin[i, q, :ln].copy(), end=end[i, q, :ln].copy(), tot=np.float32(tot[i, q]),
                                lm=np.float32(lm[i, q]), n_arcs=int(na[i, q]), status=int(status[i]), word_post=post,
                                conf=np.minimum(1.0, post), path_logpost=float(plp[i, q]), log_z=float(log_z[i])))
            out.append(row)
        return out

    def word_alternatives(self, seqs, channels=None, use_final_probs=True, graph_scale=1.0, acoustic_scale=1.0, n_alts=5, max_cells=0):
        """Word alternatives per slot -- a confusion network pinned to each sequence -- for a LIST of channels (None: all), live and
        finalized ones mixed (wfst_decoder_word_alternatives): seqs[i] = the word sequences on channels[i], as align_words takes them.
        Per channel a list with one dict per sequence: word_confidences' fields plus alts (per word a list of (word, post): the words
        the lattice says in that word's cell of the time axis, by posterior mass descending and word id ascending, the first n_alts of
        them, 1 <= n_alts <= 16, unclamped), n_distinct (int32 per word: how many words the cell has in all) and none_post (float64 per
        word: the share of the lattice's weight on the paths that say nothing in the cell).  The floats are reproducible to rounding,
        not bit for bit; a list is ordered on the device's own sums."""
        ch, cnt, ns, cap, words, lens = self._pack_seqs(seqs, channels, "sequences")
        K = int(n_alts)
        status, found, na, begin, end, tot, lm = self._word_results(cnt, ns, cap)
        log_z, wp, plp = np.zeros(cnt, np.float64), np.zeros((cnt, ns, cap), np.float64), np.zeros((cnt, ns), np.float64)
        nonep, nd = np.zeros((cnt, ns, cap), np.float64), np.zeros((cnt, ns, cap), np.int32)
        aw, ap = np.zeros((cnt, ns, cap, max(K, 1)), np.int32), np.zeros((cnt, ns, cap, max(K, 1)), np.float64)
        f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _check(lib().wfst_decoder_word_alternatives(self.h, _i32(ch), cnt, int(bool(use_final_probs)), C.c_double(float(graph_scale)),
                                                    C.c_double(float(acoustic_scale)), K, ns, cap, _i32(words), _i32(lens),
                                                    C.c_int64(int(max_cells)), _i32(status), f64(log_z), _i32(found), _i32(na), _i32(begin),
                                                    _i32(end), f64(wp), f64(nonep), _i32(nd), _i32(aw), f64(ap), f64(plp), _f32(tot), _f32(lm)))
        out = []
        for i in range(cnt):
            row = []
            for q in range(len(seqs[i])):
                ln = max(int(lens[i, q]), 0)
                post = wp[i, q, :ln].copy()
                w, p, cnt_k = aw[i, q, :ln].tolist(), ap[i, q, :ln].tolist(), nd[i, q, :ln].tolist()
                alts = [list(zip(w[k][:cnt_k[k]], p[k][:cnt_k[k]])) for k in range(ln)]   # (rows of n_alts: a longer count takes all)
                row.append(dict(found=bool(found[i, q]), begin=begin[i, q, :ln].copy(), end=end[i, q, :ln].copy(), tot=np.float32(tot[i, q]),
                                lm=np.float32(lm[i, q]), n_arcs=int(na[i, q]), status=int(status[i]), word_post=post,
                                conf=np.minimum(1.0, post), path_logpost=float(plp[i, q]), log_z=float(log_z[i]), alts=alts,
                                none_post=nonep[i, q, :ln].copy(), n_distinct=nd[i, q, :ln].copy()))
            out.append(row)
        return out

    def _sequence_posterior(self, mode, seqs, channels, use_final_probs, graph_scale, acoustic_scale, max_cells, cap_frames):
        """wfst_decoder_sequence_posterior: (lens, status[cnt], log_z[cnt], n_frames[cnt], found, logpost [cnt][ns],
        hit_mass [cnt][ns][cap_frames] or None)"""
        ch, cnt, ns, cap, words, lens = self._pack_seqs(seqs, channels, "sequences")
        status, nf = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32)
        log_z, found, lp = np.zeros(cnt, np.float64), np.zeros((cnt, ns), np.int32), np.zeros((cnt, ns), np.float64)
        hit = np.zeros((cnt, ns, int(cap_frames)), np.float64) if cap_frames else None
        f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        _check(lib().wfst_decoder_sequence_posterior(self.h, _i32(ch), cnt, int(bool(use_final_probs)), C.c_double(float(graph_scale)),
                                                     C.c_double(float(acoustic_scale)), int(mode), ns, cap, _i32(words), _i32(lens),
                                                     C.c_int64(int(max_cells)), int(cap_frames), _i32(status), f64(log_z), _i32(nf),
                                                     _i32(found), f64(lp), f64(hit)))
        return lens, status, log_z, nf, found, lp, hit

    def sentence_posteriors(self, seqs, channels=None, use_final_probs=True, graph_scale=1.0, acoustic_scale=1.0, max_cells=0):
        """Sentence posteriors on the raw lattice, for a LIST of channels (None: all), live and finalized ones mixed
        (wfst_decoder_sequence_posterior, mode 0): seqs[i] = the word sequences on channels[i], as align_words takes them.  Per
        channel a list with one dict per sequence: found, logpost (the log of the share of the lattice's weight on ALL paths that
        spell the sequence; 0.0 where none does), log_z (the channel's) and status.  Reproducible to rounding, not bit for bit."""
        _, status, log_z, _, found, lp, _ = self._sequence_posterior(0, seqs, channels, use_final_probs, graph_scale, acoustic_scale,
                                                                      max_cells, 0)
        return [[dict(found=bool(found[i, q]), logpost=float(lp[i, q]), log_z=float(log_z[i]), status=int(status[i]))
                 for q in range(len(seqs[i]))] for i in range(len(seqs))]

    def phrase_posteriors(self, phrases, channels=None, use_final_probs=True, graph_scale=1.0, acoustic_scale=1.0, max_cells=0,
                          hit_mass=False, cap_frames=0):
        """Phrase posteriors on the raw lattice (wfst_decoder_sequence_posterior, mode 1): phrases[i] = the phrases (each at least
        one word id > 0; None: skipped) looked for on channels[i].  Per channel a list with one dict per phrase: found, count (the
        expected number of times a path says the phrase, overlapping occurrences included: it may pass 1), log_count (what the
        call returns: count = exp(log_count)), conf = min(1, count), log_z, n_frames (the channel's) and status; with
        hit_mass=True also hit_mass, a float64 array of n_frames entries: the count by the frame at which the phrase's last word
        begins.  cap_frames = 0: room for every lattice -- the rows are sized by the listed channels' decoded frames, and the call
        is made again with n_frames' room if a lattice has more; a cap_frames of the caller's is taken as it is, and a channel whose
        lattice outgrows it carries WFST_E_CAPACITY in status and hit_mass None."""
        capf = 0
        if hit_mass:
            ch = range(self.n) if channels is None else channels
            capf = int(cap_frames) if cap_frames else 1 + max([self.num_frames_decoded(c) for c in ch] + [0])
        while True:
            lens, status, log_z, nf, found, lp, hit = self._sequence_posterior(1, phrases, channels, use_final_probs, graph_scale,
                                                                               acoustic_scale, max_cells, capf)
            if not hit_mass or cap_frames or int(nf.max(initial=0)) <= capf:
                break
            capf = int(nf.max())   # (a lattice with more frames than the guess: once more, with room for it)
        out = []
        for i in range(len(phrases)):
            row = []
            for q in range(len(phrases[i])):
                count = float(np.exp(lp[i, q])) if found[i, q] else 0.0
                d = dict(found=bool(found[i, q]), count=count, log_count=float(lp[i, q]), conf=min(1.0, count), log_z=float(log_z[i]),
                         n_frames=int(nf[i]), status=int(status[i]))
                if hit_mass:
                    d["hit_mass"] = hit[i, q, :int(nf[i])].copy() if int(nf[i]) <= capf else None
                row.append(d)
            out.append(row)
        return out

    def frame_posteriors(self, channels=None, use_final_probs=True, graph_scale=1.0, acoustic_scale=1.0, label_map=None, min_post=0.0,
                         max_cells=0):
        """Frame posteriors on the raw lattice, for a LIST of channels (None: all), live and finalized ones mixed
        (wfst_decoder_frame_posteriors): per frame the posterior mass of every class of the frame's emitting arcs -- the
        transition-id, or label_map[transition-id] (an int32 array of n_tid + 1 entries >= 0, entry 0 unused: a tid -> pdf or
        tid -> phone map) -- Kaldi's lattice-to-post.  Per channel one dict: status, log_z, n_frames, frame_off (int32,
        n_frames + 1), classes and posts (the entries of frame f are frame_off[f] .. frame_off[f + 1], by class ascending; only
        classes with a mass > 0 and >= min_post), n_distinct (int32 per frame: the classes with a mass > 0, before the threshold)
        and frame_mass (float64 per frame: the sum over all classes, before the threshold).  Room is taken from the frames decoded;
        the call is made once more where a channel reports that it needs more.  Reproducible to rounding, not bit for bit."""
        ch = np.ascontiguousarray(list(range(self.n)) if channels is None else [int(c) for c in channels], dtype=np.int32)
        cnt = int(ch.shape[0])
        m, n_tid = None, 0
        if label_map is not None:
            m = np.ascontiguousarray(label_map, dtype=np.int32)
            n_tid = int(m.shape[0]) - 1
        frames = max([self.num_frames_decoded(int(c)) for c in ch] + [1]) if cnt else 1
        capf, cape = max(frames, 1), max(frames, 1) * FRAME_POST_ENTRIES_PER_FRAME
        f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        for attempt in range(2):
            status, nf, ne = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32), np.zeros(cnt, np.int32)
            log_z = np.zeros(cnt, np.float64)
            off, nd, mass = np.zeros((cnt, capf + 1), np.int32), np.zeros((cnt, capf), np.int32), np.zeros((cnt, capf), np.float64)
            cls, post = np.zeros((cnt, cape), np.int32), np.zeros((cnt, cape), np.float64)
            _check(lib().wfst_decoder_frame_posteriors(self.h, _i32(ch), cnt, int(bool(use_final_probs)), C.c_double(float(graph_scale)),
                                                       C.c_double(float(acoustic_scale)), _i32(m) if m is not None else None, n_tid,
                                                       C.c_double(float(min_post)), C.c_int64(int(max_cells)), capf, cape, _i32(status),
                                                       f64(log_z), _i32(nf), _i32(ne), _i32(off), _i32(nd), f64(mass), _i32(cls), f64(post)))
            short = (status == -4) & ((nf > capf) | (ne > cape))
            if attempt or not short.any():
                break
            capf, cape = max(capf, int(nf.max())), max(cape, int(ne.max()))   # (a channel needs more room: once more, with it)
        out = []
        for i in range(cnt):
            k, e = (int(nf[i]), int(ne[i])) if status[i] == 0 else (0, 0)
            out.append(dict(status=int(status[i]), log_z=float(log_z[i]), n_frames=int(nf[i]), n_entries=int(ne[i]),
                            frame_off=off[i, :k + 1].copy(), classes=cls[i, :e].copy(), posts=post[i, :e].copy(),
                            n_distinct=nd[i, :k].copy(), frame_mass=mass[i, :k].copy()))
        return out

    def sequence_stats(self, refs, channels=None, criterion="smbr", use_final_probs=True, graph_scale=1.0, acoustic_scale=1.0,
                       label_map=None, sil_classes=(), drop_frames=False, grad=None, grad_scale=1.0, stream="current", max_cells=0,
                       lists=True):
        """Sequence-training statistics on the raw lattice, for a LIST of channels (None: all), live and finalized ones mixed
        (wfst_decoder_sequence_stats; Kaldi's LatticeForwardBackwardMpeVariants "smbr" and LatticeForwardBackwardMmi): refs = per
        listed channel the numerator alignment's class per frame (an int sequence; < 0 or beyond its end: unlabelled), classes as
        frame_posteriors takes them (transition-ids, or label_map of them).  Per channel one dict: status, log_z, tot_acc (the
        expected number of correct frames; 0 under "mmi"), n_frames, n_ref_frames, n_dropped, n_entries, frame_off (int32,
        n_frames + 1), classes, posts and values (the entries of frame f are frame_off[f] .. frame_off[f + 1], by class ascending):
        value is the derivative of the criterion with respect to the class' score at that frame.
        grad: None, or per listed channel a 2-D float32 DEVICE tensor [frames][n_cols] (anything with data_ptr(), shape and stride(),
        the last dimension contiguous; one width for all) or None: rows 0 .. min(n_frames, frames) - 1 become zeros with
        float32(grad_scale * value) at each listed class' column.  stream: "current" = torch's current stream, which then waits for the
        rows; a raw hipStream_t (int); None = WFST_STREAM_NONE.  lists=False: no lists are fetched (the dense rows and the numbers
        only).  The call is made once more where a channel reports that its lists need more room."""
        ch = np.ascontiguousarray(list(range(self.n)) if channels is None else [int(c) for c in channels], dtype=np.int32)
        cnt = int(ch.shape[0])
        crit = {"mmi": WFST_SEQ_MMI, "smbr": WFST_SEQ_SMBR}.get(criterion, criterion)
        if not isinstance(crit, int):
            raise ValueError("criterion is 'smbr' or 'mmi'")
        refs = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1) for r in refs]
        if len(refs) != cnt:
            raise ValueError("one reference per listed channel")
        cap_ref = max([len(r) for r in refs] + [1])
        ref, n_ref = np.full((max(cnt, 1), cap_ref), -1, np.int32), np.zeros(max(cnt, 1), np.int32)
        for i, r in enumerate(refs):
            ref[i, :len(r)] = r
            n_ref[i] = len(r)
        m, n_tid = None, 0
        if label_map is not None:
            m = np.ascontiguousarray(label_map, dtype=np.int32)
            n_tid = int(m.shape[0]) - 1
        sil = np.ascontiguousarray(list(sil_classes), dtype=np.int32).reshape(-1)
        ptrs = pitch = rows = None
        n_cols = 0
        if grad is not None:
            grad = list(grad)
            if len(grad) != cnt:
                raise ValueError("one grad tensor (or None) per listed channel")
            ptrs, pitch, rows = (C.c_void_p * max(cnt, 1))(), np.zeros(max(cnt, 1), np.int64), np.zeros(max(cnt, 1), np.int32)
            for i, t in enumerate(grad):
                if t is None:
                    continue
                if len(t.shape) != 2:
                    raise ValueError("grad %d is not 2-D" % i)
                if "float32" not in str(t.dtype):
                    raise ValueError("grad %d is not float32" % i)
                cols = int(t.shape[1])
                if n_cols and cols != n_cols:
                    raise ValueError("grad tensors differ in width")
                n_cols = cols
                st = t.stride()
                if cols > 1 and int(st[1]) != 1:
                    raise ValueError("the last dimension of grad %d is not contiguous" % i)
                ptrs[i] = int(t.data_ptr())
                rows[i] = int(t.shape[0])
                pitch[i] = int(st[0]) if int(t.shape[0]) > 1 else max(int(st[0]), cols)
            if not n_cols:
                ptrs = None
        if stream == "current":
            stream = WFST_STREAM_NONE
            if ptrs is not None:
                import torch
                stream = int(torch.cuda.current_stream().cuda_stream)
        elif stream is None:
            stream = WFST_STREAM_NONE
        frames = max([self.num_frames_decoded(int(c)) for c in ch] + [1]) if cnt else 1
        capf, cape = (max(frames, 1), max(frames, 1) * FRAME_POST_ENTRIES_PER_FRAME) if lists else (0, 0)
        f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        for attempt in range(2):
            status, nf, ne = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32), np.zeros(cnt, np.int32)
            nr, ndrop = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32)
            log_z, tot = np.zeros(cnt, np.float64), np.zeros(cnt, np.float64)
            off = np.zeros((cnt, capf + 1), np.int32)
            cls, post, val = np.zeros((cnt, cape), np.int32), np.zeros((cnt, cape), np.float64), np.zeros((cnt, cape), np.float64)
            _check(lib().wfst_decoder_sequence_stats(
                self.h, _i32(ch), cnt, int(crit), int(bool(use_final_probs)), C.c_double(float(graph_scale)), C.c_double(float(acoustic_scale)),
                _i32(m) if m is not None else None, n_tid, _i32(ref), _i32(n_ref), cap_ref, _i32(sil) if len(sil) else None, int(len(sil)),
                int(bool(drop_frames)), C.c_int64(int(max_cells)), capf, cape, ptrs,
                pitch.ctypes.data_as(C.POINTER(C.c_int64)) if ptrs is not None else None, _i32(rows) if ptrs is not None else None,
                int(n_cols), C.c_double(float(grad_scale)), C.c_void_p(int(stream)), _i32(status), f64(log_z), f64(tot), _i32(nf), _i32(nr),
                _i32(ndrop), _i32(ne), _i32(off), _i32(cls), f64(post), f64(val)))
            short = (status == -4) & ((nf > capf) | (ne > cape))
            if attempt or not lists or not short.any():
                break
            capf, cape = max(capf, int(nf.max())), max(cape, int(ne.max()))   # (a channel needs more room: once more, with it)
        out = []
        for i in range(cnt):
            k, e = (int(nf[i]), int(ne[i])) if status[i] == 0 and lists else (0, 0)
            out.append(dict(status=int(status[i]), log_z=float(log_z[i]), tot_acc=float(tot[i]), n_frames=int(nf[i]),
                            n_ref_frames=int(nr[i]), n_dropped=int(ndrop[i]), n_entries=int(ne[i]), frame_off=off[i, :k + 1].copy(),
                            classes=cls[i, :e].copy(), posts=post[i, :e].copy(), values=val[i, :e].copy()))
        return out

    def rescaled_words(self, settings, channels=None, use_final_probs=True, cap_words=256, cap_tids=0, max_cells=0):
        """The best path of the raw lattice again under other scales and a word penalty, for a LIST of channels (None: all), live and
        finalized ones mixed (wfst_decoder_rescaled_words; Kaldi's lattice-best-path-score): settings = up to 64 triples
        (graph_scale, acoustic_scale, word_penalty), shared by the listed channels.  Per channel a list with one dict per setting:
        found, n_arcs, n_hyp, hyp_words, begin / end (int32 arrays per word, frames, end exclusive), scaled_cost (float64: the
        path's cost at the setting), tot, lm (float32: the path's own UNSCALED LatticeToVector scores), status -- WFST_OK or the
        CHANNEL's own error code -- and, with cap_tids > 0, n_tids and tids (the alignment: the path's transition-ids).  Bit for
        bit reproducible.  A path with more words or transition-ids than cap_words / cap_tids hold: the call is made once more,
        with the room needed."""
        ch = np.ascontiguousarray(list(range(self.n)) if channels is None else [int(c) for c in channels], dtype=np.int32)
        cnt = int(ch.shape[0])
        st = np.ascontiguousarray(settings, dtype=np.float64).reshape(-1, 3)
        ns = int(st.shape[0])
        cap, tcap, want_tids = int(cap_words), int(cap_tids), int(cap_tids) != 0
        f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        for attempt in range(2):
            status, found, na, begin, end, tot, lm = self._word_results(cnt, max(ns, 1), max(cap, 1))
            nh, nt = np.zeros((cnt, max(ns, 1)), np.int32), np.zeros((cnt, max(ns, 1)), np.int32)
            hyp, cost = np.zeros((cnt, max(ns, 1), max(cap, 1)), np.int32), np.zeros((cnt, max(ns, 1)), np.float64)
            tids = np.zeros((cnt, max(ns, 1), max(tcap, 1)), np.int32)
            _check(lib().wfst_decoder_rescaled_words(self.h, _i32(ch), cnt, int(bool(use_final_probs)), ns, f64(st), cap, tcap,
                                                     C.c_int64(int(max_cells)), _i32(status), _i32(found), _i32(na), _i32(nh), _i32(nt),
                                                     _i32(hyp), _i32(begin), _i32(end), _i32(tids) if want_tids else None, f64(cost),
                                                     _f32(tot), _f32(lm)))
            short = (nh > cap) | ((nt > tcap) if want_tids else False)
            if attempt or not np.any(short):
                break
            cap = max(cap, int(nh.max()))   # (a path needs more room: once more, with it)
            if want_tids:
                tcap = max(tcap, int(nt.max()))
        out = []
        for i in range(cnt):
            row = []
            for q in range(ns):
                m = min(int(nh[i, q]), cap)
                d = dict(found=bool(found[i, q]), n_arcs=int(na[i, q]), n_hyp=int(nh[i, q]), hyp_words=hyp[i, q, :m].copy(),
                         begin=begin[i, q, :m].copy(), end=end[i, q, :m].copy(), scaled_cost=float(cost[i, q]), tot=np.float32(tot[i, q]),
                         lm=np.float32(lm[i, q]), status=int(status[i]))
                if want_tids:
                    d.update(n_tids=int(nt[i, q]), tids=tids[i, q, :min(int(nt[i, q]), tcap)].copy())
                row.append(d)
            out.append(row)
        return out

    def biased_words(self, lists, list_of=None, settings=((1, 1, 0, 1),), channels=None, use_final_probs=True, cap_words=256, cap_hits=64,
                     max_cells=0):
        """Phrase boosting: the best path of the raw lattice again under scales, a word penalty and a bonus for every occurrence of a
        phrase of the channel's bias list, for a LIST of channels (None: all), live and finalized ones mixed
        (wfst_decoder_biased_words).  lists = a BiasLists set (None: no channel has a list), list_of[i] = the list of listed channel
        i (None: list i where the set has one, else none; -1: none), settings = up to 16 quadruples (graph_scale, acoustic_scale,
        word_penalty, boost_scale) shared by the listed channels.  Per channel a list with one dict per setting: found, n_arcs, n_hyp,
        hyp_words, begin / end (int32 arrays per word, frames, end exclusive), biased_cost and bonus (float64), tot, lm (float32: the
        path's own UNSCALED scores), n_hits, hit_phrase / hit_word (int32 arrays: the phrase's index in the list, the index in
        hyp_words of the occurrence's last word) and status -- WFST_OK or the CHANNEL's own error code.  Bit for bit reproducible.
        A path with more words or hits than cap_words / cap_hits hold: the call is made once more, with the room needed.
        lists may also be a BiasBooks set: the call is then biased_words_sparse's."""
        if isinstance(lists, BiasBooks):
            return self.biased_words_sparse(lists, list_of, settings, channels, use_final_probs, cap_words, cap_hits, max_cells)
        ch = np.ascontiguousarray(list(range(self.n)) if channels is None else [int(c) for c in channels], dtype=np.int32)
        cnt = int(ch.shape[0])
        if list_of is None:
            k = lists.n_lists if lists is not None else 0
            list_of = [i if i < k else -1 for i in range(cnt)]
        lo = np.ascontiguousarray([int(x) for x in list_of], dtype=np.int32)
        if lo.shape[0] != cnt:
            raise ValueError("list_of must have one entry per listed channel")
        st = np.ascontiguousarray(settings, dtype=np.float64).reshape(-1, 4)
        ns = int(st.shape[0])
        cap, hcap = int(cap_words), int(cap_hits)
        for attempt in range(2):
            status, found, na, begin, end, tot, lm = self._word_results(cnt, max(ns, 1), max(cap, 1))
            pair = lambda t: np.zeros((cnt, max(ns, 1)), t)
            nh, nk, cost, bonus = pair(np.int32), pair(np.int32), pair(np.float64), pair(np.float64)
            hyp = np.zeros((cnt, max(ns, 1), max(cap, 1)), np.int32)
            hp, hw = np.zeros((cnt, max(ns, 1), max(hcap, 1)), np.int32), np.zeros((cnt, max(ns, 1), max(hcap, 1)), np.int32)
            _check(lib().wfst_decoder_biased_words(self.h, _i32(ch), cnt, int(bool(use_final_probs)), lists.h if lists is not None else None,
                                                   _i32(lo), ns, _f64(st), cap, hcap, C.c_int64(int(max_cells)), _i32(status), _i32(found),
                                                   _i32(na), _i32(nh), _i32(nk), _i32(hyp), _i32(begin), _i32(end), _i32(hp), _i32(hw),
                                                   _f64(cost), _f64(bonus), _f32(tot), _f32(lm)))
            if attempt or not (np.any(nh > cap) or np.any(nk > hcap)):
                break
            cap, hcap = max(cap, int(nh.max())), max(hcap, int(nk.max()))   # (a path needs more room: once more, with it)
        out = []
        for i in range(cnt):
            row = []
            for q in range(ns):
                m, k = min(int(nh[i, q]), cap), min(int(nk[i, q]), hcap)
                row.append(dict(found=bool(found[i, q]), n_arcs=int(na[i, q]), n_hyp=int(nh[i, q]), hyp_words=hyp[i, q, :m].copy(),
                                begin=begin[i, q, :m].copy(), end=end[i, q, :m].copy(), biased_cost=float(cost[i, q]),
                                bonus=float(bonus[i, q]), tot=np.float32(tot[i, q]), lm=np.float32(lm[i, q]), n_hits=int(nk[i, q]),
                                hit_phrase=hp[i, q, :k].copy(), hit_word=hw[i, q, :k].copy(), status=int(status[i])))
            out.append(row)
        return out

    def biased_words_sparse(self, books, book_of=None, settings=((1, 1, 0, 1),), channels=None, use_final_probs=True, cap_words=256,
                            cap_hits=64, max_cells=0, round_cells=0):
        """biased_words for books, bias lists of up to 65 536 nodes (wfst_decoder_biased_words_sparse): the same answers from the
        cells a path can reach.  books = a BiasBooks set (None: no channel has a book), book_of as biased_words' list_of.  Every dict
        of biased_words, and n_cells beside them: the channel's reachable (state, node) pairs, -1 where they pass max_cells (which
        bounds ONE channel's n_cells here; 0: 4 Mi).  round_cells: the cost cells of one round of the sweep (0: 32 Mi)."""
        ch = np.ascontiguousarray(list(range(self.n)) if channels is None else [int(c) for c in channels], dtype=np.int32)
        cnt = int(ch.shape[0])
        if book_of is None:
            k = books.n_books if books is not None else 0
            book_of = [i if i < k else -1 for i in range(cnt)]
        lo = np.ascontiguousarray([int(x) for x in book_of], dtype=np.int32)
        if lo.shape[0] != cnt:
            raise ValueError("book_of must have one entry per listed channel")
        st = np.ascontiguousarray(settings, dtype=np.float64).reshape(-1, 4)
        ns = int(st.shape[0])
        cap, hcap = int(cap_words), int(cap_hits)
        for attempt in range(2):
            status, found, na, begin, end, tot, lm = self._word_results(cnt, max(ns, 1), max(cap, 1))
            pair = lambda t: np.zeros((cnt, max(ns, 1)), t)
            nh, nk, cost, bonus = pair(np.int32), pair(np.int32), pair(np.float64), pair(np.float64)
            nc = np.zeros(max(cnt, 1), np.int64)
            hyp = np.zeros((cnt, max(ns, 1), max(cap, 1)), np.int32)
            hp, hw = np.zeros((cnt, max(ns, 1), max(hcap, 1)), np.int32), np.zeros((cnt, max(ns, 1), max(hcap, 1)), np.int32)
            _check(lib().wfst_decoder_biased_words_sparse(self.h, _i32(ch), cnt, int(bool(use_final_probs)), books.h if books is not None else None,
                                                          _i32(lo), ns, _f64(st), cap, hcap, C.c_int64(int(max_cells)), C.c_int64(int(round_cells)),
                                                          _i32(status), nc.ctypes.data_as(C.POINTER(C.c_int64)), _i32(found), _i32(na), _i32(nh),
                                                          _i32(nk), _i32(hyp), _i32(begin), _i32(end), _i32(hp), _i32(hw), _f64(cost), _f64(bonus),
                                                          _f32(tot), _f32(lm)))
            if attempt or not (np.any(nh > cap) or np.any(nk > hcap)):
                break
            cap, hcap = max(cap, int(nh.max())), max(hcap, int(nk.max()))   # (a path needs more room: once more, with it)
        out = []
        for i in range(cnt):
            row = []
            for q in range(ns):
                m, k = min(int(nh[i, q]), cap), min(int(nk[i, q]), hcap)
                row.append(dict(found=bool(found[i, q]), n_arcs=int(na[i, q]), n_hyp=int(nh[i, q]), hyp_words=hyp[i, q, :m].copy(),
                                begin=begin[i, q, :m].copy(), end=end[i, q, :m].copy(), biased_cost=float(cost[i, q]),
                                bonus=float(bonus[i, q]), tot=np.float32(tot[i, q]), lm=np.float32(lm[i, q]), n_hits=int(nk[i, q]),
                                hit_phrase=hp[i, q, :k].copy(), hit_word=hw[i, q, :k].copy(), status=int(status[i]), n_cells=int(nc[i])))
            out.append(row)
        return out

    def force_align(self, graphs, graph_of=None, channels=None, n_frames=None, label_map=None, max_cells=0, cap_frames=None,
                    cap_hops=None, cap_words=None):
        """Forced alignment of the listed channels' scores (None: all) against per-utterance graphs (wfst_decoder_force_align):
        graphs = an AlignGraphs set, graph_of[i] = the graph of listed channel i (None: graph i), n_frames[i] = the frames to
        align (None or -1: all the channel holds), label_map = class per transition-id for `alignment` (entry 0 unused).  Works on
        every kind of decoder and on live, finalized and never-decoded channels alike; only reads the decoder.  Per channel one
        ForcedAlignment, bit for bit reproducible.  The capacities are chosen from the frames held; where a channel answers that
        its path needs more room the call is made once more, with it."""
        ch = np.ascontiguousarray(list(range(self.n)) if channels is None else [int(c) for c in channels], dtype=np.int32)
        cnt = int(ch.shape[0])
        gof = np.ascontiguousarray(list(range(cnt)) if graph_of is None else [int(g) for g in graph_of], dtype=np.int32)
        if gof.shape[0] != cnt:
            raise ValueError("one graph per listed channel")
        nfi = None
        if n_frames is not None:
            nfi = np.ascontiguousarray([-1 if t is None else int(t) for t in n_frames], dtype=np.int32)
            if nfi.shape[0] != cnt:
                raise ValueError("one frame count per listed channel")
        m, n_tid = None, 0
        if label_map is not None:
            m = np.ascontiguousarray(label_map, dtype=np.int32)
            n_tid = int(m.shape[0]) - 1
        # (a first guess at the frames: a channel that holds more than it has decoded answers with the room it needs)
        guess = max([int(t) for t in nfi if t >= 0] + [1]) if nfi is not None and (nfi >= 0).all() else \
            max([max(self.num_frames_decoded(int(c)), 0) for c in ch] + [1]) if cnt else 1
        capf = int(cap_frames) if cap_frames is not None else guess
        caph = int(cap_hops) if cap_hops is not None else 2 * guess + 8
        capw = int(cap_words) if cap_words is not None else guess + 8
        for attempt in range(2):
            k = max(cnt, 1)
            status, found, nf, nh, nw = (np.zeros(k, np.int32) for _ in range(5))
            cost, tot, lm = (np.zeros(k, np.float32) for _ in range(3))
            hops, ali = np.zeros((k, max(caph, 1)), np.int32), np.zeros((k, max(capf, 1)), np.int32)
            words, wf = np.zeros((k, max(capw, 1)), np.int32), np.zeros((k, max(capw, 1)), np.int32)
            _check(lib().wfst_decoder_force_align(self.h, _i32(ch), cnt, graphs.h, _i32(gof), _i32(nfi), _i32(m), n_tid,
                                                  C.c_int64(int(max_cells)), max(capf, 1), max(caph, 1), max(capw, 1), _i32(status),
                                                  _i32(found), _i32(nf), _f32(cost), _f32(tot), _f32(lm), _i32(nh), _i32(hops),
                                                  _i32(ali), _i32(nw), _i32(words), _i32(wf)))
            short = (status[:cnt] == -4) & ((nf[:cnt] > max(capf, 1)) | (nh[:cnt] > max(caph, 1)) | (nw[:cnt] > max(capw, 1)))
            if attempt or not short.any():
                break
            capf, caph, capw = max(capf, int(nf.max())), max(caph, int(nh.max())), max(capw, int(nw.max()))
        out = []
        for i in range(cnt):
            ok = bool(found[i])
            t, h, w = (min(int(nf[i]), max(capf, 1)), min(int(nh[i]), max(caph, 1)), min(int(nw[i]), max(capw, 1))) if ok else (0, 0, 0)
            out.append(ForcedAlignment(status=int(status[i]), found=ok, n_frames=int(nf[i]), path_cost=np.float32(cost[i]),
                                       tot_score=np.float32(tot[i]), lm_score=np.float32(lm[i]), n_hops=int(nh[i]),
                                       hop_arc=hops[i, :h].copy(), alignment=ali[i, :t].copy(), n_words=int(nw[i]),
                                       words=words[i, :w].copy(), word_frame=wf[i, :w].copy()))
        return out

    def force_align_workspace(self):
        """Bytes of the decoder's forced-alignment workspace (wfst_decoder_force_align_workspace)."""
        b = C.c_int64()
        _check(lib().wfst_decoder_force_align_workspace(self.h, C.byref(b)))
        return int(b.value)

    def graph_posteriors(self, graphs, graph_of=None, channels=None, n_frames=None, label_map=None, graph_scale=1.0, acoustic_scale=1.0,
                         min_post=0.0, arc_occupancy=False, grad=None, grad_scale=1.0, n_cols=None, consumer_stream=None, max_cells=0,
                         lists=True, cap_frames=None, cap_entries=None, cap_arcs=None):
        """Forward-backward of the listed channels' scores (None: all) over per-utterance graphs (wfst_decoder_graph_posteriors):
        graphs, graph_of, n_frames and label_map as force_align takes them; the scales are finite and >= 0.  Per channel one
        GraphPosteriors: log_like = the log of the sum over the graph's paths, per frame the posterior of every class (the
        transition-id, or label_map of it) in frame_posteriors' list format (frame_post_lookup reads it), and with
        arc_occupancy=True arc_occ, the expected count of every arc of the channel's graph.
        grad: None, or per listed channel a 2-D float32 DEVICE tensor [frames][n_cols] or None, as sequence_stats takes them: rows
        0 .. min(n_frames, frames) - 1 become zeros with float32(grad_scale * post) at each class' column.  consumer_stream: None =
        torch's current stream where there are dense rows; a torch stream; a raw hipStream_t (int), WFST_STREAM_NONE among them.
        lists=False: no lists are fetched.  Works on every kind of decoder and on live, finalized and never-decoded channels alike;
        only reads the decoder.  The call is made once more where a channel reports that it needs more room."""
        ch = np.ascontiguousarray(list(range(self.n)) if channels is None else [int(c) for c in channels], dtype=np.int32)
        cnt = int(ch.shape[0])
        gof = np.ascontiguousarray(list(range(cnt)) if graph_of is None else [int(g) for g in graph_of], dtype=np.int32)
        if gof.shape[0] != cnt:
            raise ValueError("one graph per listed channel")
        nfi = None
        if n_frames is not None:
            nfi = np.ascontiguousarray([-1 if t is None else int(t) for t in n_frames], dtype=np.int32)
            if nfi.shape[0] != cnt:
                raise ValueError("one frame count per listed channel")
        m, n_tid = None, 0
        if label_map is not None:
            m = np.ascontiguousarray(label_map, dtype=np.int32)
            n_tid = int(m.shape[0]) - 1
        ptrs = pitch = rows = None
        width = 0
        if grad is not None:
            grad = list(grad)
            if len(grad) != cnt:
                raise ValueError("one grad tensor (or None) per listed channel")
            ptrs, pitch, rows = (C.c_void_p * max(cnt, 1))(), np.zeros(max(cnt, 1), np.int64), np.zeros(max(cnt, 1), np.int32)
            for i, t in enumerate(grad):
                if t is None:
                    continue
                if len(t.shape) != 2:
                    raise ValueError("grad %d is not 2-D" % i)
                if "float32" not in str(t.dtype):
                    raise ValueError("grad %d is not float32" % i)
                cols = int(t.shape[1]) if n_cols is None else int(n_cols)
                if cols > int(t.shape[1]) or (width and cols != width):
                    raise ValueError("grad tensors differ in width, or are narrower than n_cols")
                width = cols
                st = t.stride()
                if int(t.shape[1]) > 1 and int(st[1]) != 1:
                    raise ValueError("the last dimension of grad %d is not contiguous" % i)
                ptrs[i] = int(t.data_ptr())
                rows[i] = int(t.shape[0])
                pitch[i] = int(st[0]) if int(t.shape[0]) > 1 else max(int(st[0]), cols)
            if not width:
                ptrs = None
        if consumer_stream is None:
            consumer_stream = WFST_STREAM_NONE
            if ptrs is not None:
                import torch
                consumer_stream = int(torch.cuda.current_stream().cuda_stream)
        elif hasattr(consumer_stream, "cuda_stream"):
            consumer_stream = int(consumer_stream.cuda_stream)
        # (a first guess at the frames: a channel that holds more than it has decoded answers with the room it needs)
        guess = max([int(t) for t in nfi if t >= 0] + [1]) if nfi is not None and (nfi >= 0).all() else \
            max([max(self.num_frames_decoded(int(c)), 0) for c in ch] + [1]) if cnt else 1
        capf, cape = (0, 0) if not lists else (int(cap_frames) if cap_frames is not None else guess,
                                               int(cap_entries) if cap_entries is not None else guess * FRAME_POST_ENTRIES_PER_FRAME)
        capa = 0
        if arc_occupancy:
            capa = int(cap_arcs) if cap_arcs is not None else max([int(graphs.info()["n_arcs"][g]) for g in gof] + [1])
        f64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
        k = max(cnt, 1)
        for attempt in range(2):
            status, found, nf, ne, na = (np.zeros(k, np.int32) for _ in range(5))
            ll = np.zeros(k, np.float64)
            off = nd = mass = cls = post = occ = None
            if lists:
                off, nd, mass = np.zeros((k, capf + 1), np.int32), np.zeros((k, capf), np.int32), np.zeros((k, capf), np.float64)
                cls, post = np.zeros((k, cape), np.int32), np.zeros((k, cape), np.float64)
            if arc_occupancy:
                occ = np.zeros((k, max(capa, 1)), np.float64)
            _check(lib().wfst_decoder_graph_posteriors(
                self.h, _i32(ch), cnt, graphs.h, _i32(gof), _i32(nfi), _i32(m), n_tid, C.c_double(float(graph_scale)),
                C.c_double(float(acoustic_scale)), C.c_double(float(min_post)), C.c_int64(int(max_cells)), capf, cape, capa, ptrs,
                pitch.ctypes.data_as(C.POINTER(C.c_int64)) if ptrs is not None else None, _i32(rows) if ptrs is not None else None,
                int(width), C.c_double(float(grad_scale)), C.c_void_p(int(consumer_stream)), _i32(status), _i32(found), _i32(nf), f64(ll),
                _i32(ne), _i32(na), _i32(off), _i32(nd), f64(mass), _i32(cls), f64(post), f64(occ)))
            short = (status[:cnt] == -4) & (((nf[:cnt] > capf) | (ne[:cnt] > cape) if lists else False) | ((na[:cnt] > capa) if arc_occupancy else False))
            if attempt or not np.any(short):
                break
            capf, cape, capa = max(capf, int(nf.max())) if lists else 0, max(cape, int(ne.max())) if lists else 0, max(capa, int(na.max())) if arc_occupancy else 0
        out = []
        for i in range(cnt):
            ok = bool(found[i]) and lists and int(nf[i]) <= capf and int(ne[i]) <= cape
            t, e = (int(nf[i]), int(ne[i])) if ok else (0, 0)
            z = lambda dt: np.zeros(0, dt)
            out.append(GraphPosteriors(
                status=int(status[i]), found=bool(found[i]), n_frames=int(nf[i]), log_like=float(ll[i]), n_entries=int(ne[i]), n_arcs=int(na[i]),
                frame_off=off[i, :t + 1].copy() if lists else np.zeros(1, np.int32), classes=cls[i, :e].copy() if lists else z(np.int32),
                posts=post[i, :e].copy() if lists else z(np.float64), n_distinct=nd[i, :t].copy() if lists else z(np.int32),
                frame_mass=mass[i, :t].copy() if lists else z(np.float64),
                arc_occ=occ[i, :int(na[i])].copy() if arc_occupancy and int(na[i]) <= capa else None))
        return out

    def graph_posteriors_workspace(self):
        """Bytes of the decoder's graph-posterior workspace (wfst_decoder_graph_posteriors_workspace)."""
        b = C.c_int64()
        _check(lib().wfst_decoder_graph_posteriors_workspace(self.h, C.byref(b)))
        return int(b.value)

    def nbest_words_timed(self, n_paths, channels=None, old_lm=None, new_lm=None, use_final_probs=True, cap_words=256, max_cells=0):
        """nbest_words(...) with word times: every path's words aligned on its channel's raw lattice (align_words); the dicts of
        nbest_words gain found, begin, end, n_arcs and align_tot / align_lm (the aligned path's own scores: the determinizer
        re-associates the sums, so they may differ from tot / lm in the last bits)."""
        res = self.nbest_words(n_paths, channels, old_lm, new_lm, use_final_probs, cap_words)
        ch = list(range(self.n)) if channels is None else [int(c) for c in channels]
        seqs = [[p["words"] if p["n_words"] <= int(cap_words) else None for p in paths] for _, paths in res]
        al = self.align_words(seqs, ch, use_final_probs, max_cells)
        for (_, paths), a in zip(res, al):
            for p, x in zip(paths, a):
                p.update(found=x["found"], begin=x["begin"], end=x["end"], n_arcs=x["n_arcs"], align_tot=x["tot"], align_lm=x["lm"],
                         align_status=x["status"])
        return res

    def nbest_words_conf(self, n_paths, channels=None, old_lm=None, new_lm=None, use_final_probs=True, cap_words=256, max_cells=0,
                         graph_scale=1.0, acoustic_scale=1.0, sentence_post=False, alternatives=0):
        """nbest_words_timed(...) with confidences: every path's words aligned on its channel's raw lattice and weighed against the
        lattice's posteriors (word_confidences); beside nbest_words_timed's keys the dicts carry conf, word_post, path_logpost and
        log_z.  sentence_post=True: also sent_logpost, the log posterior of the path's word sequence over ALL lattice paths that
        spell it (sentence_posteriors, at the same scales; 0.0 where found is False).  alternatives=K > 0: also alts, none_post and
        n_distinct, the K first alternatives of every word's slot (word_alternatives, which then answers in word_confidences' place)."""
        res = self.nbest_words(n_paths, channels, old_lm, new_lm, use_final_probs, cap_words)
        ch = list(range(self.n)) if channels is None else [int(c) for c in channels]
        seqs = [[p["words"] if p["n_words"] <= int(cap_words) else None for p in paths] for _, paths in res]
        if alternatives:
            al = self.word_alternatives(seqs, ch, use_final_probs, graph_scale, acoustic_scale, int(alternatives), max_cells)
            for (_, paths), a in zip(res, al):
                for p, x in zip(paths, a):
                    p.update(alts=x["alts"], none_post=x["none_post"], n_distinct=x["n_distinct"])
        else:
            al = self.word_confidences(seqs, ch, use_final_probs, graph_scale, acoustic_scale, max_cells)
        for (_, paths), a in zip(res, al):
            for p, x in zip(paths, a):
                p.update(found=x["found"], begin=x["begin"], end=x["end"], n_arcs=x["n_arcs"], align_tot=x["tot"], align_lm=x["lm"],
                         align_status=x["status"], conf=x["conf"], word_post=x["word_post"], path_logpost=x["path_logpost"],
                         log_z=x["log_z"])
        if sentence_post:
            sp = self.sentence_posteriors(seqs, ch, use_final_probs, graph_scale, acoustic_scale, max_cells)
            for (_, paths), a in zip(res, sp):
                for p, x in zip(paths, a):
                    p.update(sent_logpost=x["logpost"], sent_found=x["found"])
        return res

    def raw_lattices(self, channels=None, use_final_probs=True, threads=0):
        """GetRawLattice of many finalized channels.  The first call fetches the pruned lattices of all
        finalized channels from the device in one sweep; the per-lattice host work (numbering, arc
        order) then runs on `threads` host threads (0 = min(16, cpu count))."""
        import os
        from concurrent.futures import ThreadPoolExecutor

        ch = list(range(self.n)) if channels is None else [int(c) for c in channels]
        if not ch:
            return []
        first = self.raw_lattice(ch[0], use_final_probs)  # fills the host-side cache (single threaded)
        nt = threads or min(16, os.cpu_count() or 1)
        if nt <= 1 or len(ch) == 1:
            return [first] + [self.raw_lattice(c, use_final_probs) for c in ch[1:]]
        with ThreadPoolExecutor(max_workers=nt) as ex:
            rest = list(ex.map(lambda c: self.raw_lattice(c, use_final_probs), ch[1:]))
        return [first] + rest

    def nbest(self, n, channels=None, max_words=256):
        """GetNbest + LatticeToVector of finalized channels (lattice mode): per channel a list of
        dicts {words, tot_score, lm_score}, cheapest first."""
        ch = list(range(self.n)) if channels is None else [int(c) for c in channels]
        cnt = len(ch)
        arr = np.asarray(ch, np.int32)
        npaths = np.zeros(cnt, np.int32)
        nw = np.zeros((cnt, n), np.int32)
        words = np.zeros((cnt, n, max_words), np.int32)
        tot = np.zeros((cnt, n), np.float32)
        lm = np.zeros((cnt, n), np.float32)
        _check(lib().wfst_decoder_get_nbest(self.h, _i32(arr), cnt, int(n), int(max_words), _i32(npaths), _i32(nw), _i32(words),
                                            _f32(tot), _f32(lm)))
        return _LazyList(cnt, lambda i: [dict(words=words[i, k, : min(nw[i, k], max_words)].copy(), n_words=int(nw[i, k]), tot_score=float(tot[i, k]),
                                              lm_score=float(lm[i, k])) for k in range(npaths[i])])

    def path_flags(self):
        """Which kernel paths the decoder runs (wfst_decoder_get_path_flags)."""
        f = (C.c_int32 * 8)()
        _check(lib().wfst_decoder_get_path_flags(self.h, f))
        return dict(zip(("staged", "two_launch", "gc_stride", "degcode", "ll_row", "best_exp", "soft_limit", "channel_groups"), [int(x) for x in f]))

    @property
    def n_groups(self):
        return int(lib().wfst_decoder_channel_groups(self.h))

    def set_profiling(self, on):
        _check(lib().wfst_decoder_set_profiling(self.h, int(bool(on))))

    def profile(self):
        ms = (C.c_double * 3)()
        n = (C.c_int64 * 3)()
        _check(lib().wfst_decoder_get_profile(self.h, ms, n))
        busy = (C.c_double * 3)()
        _check(lib().wfst_decoder_get_profile_busy(self.h, busy))
        return dict(expand_ms=ms[0], expand_launches=n[0], insert_ms=ms[1], insert_launches=n[1],
                    closure_ms=ms[2], closure_launches=n[2], expand_busy_ms=busy[0], insert_busy_ms=busy[1], closure_busy_ms=busy[2])

    def set_endpoint_config(self, cfg):
        c = cfg.as_c()
        _check(lib().wfst_decoder_set_endpoint_config(self.h, C.byref(c)))

    def endpoint(self, channels=None):
        """EndpointDetected of the listed channels (all if None) in one device call: (detected bool[n], rule int32[n] (1..5, 0 none),
        trailing_frames int32[n] (-1: no path), relative_cost float32[n])."""
        ch = np.arange(self.n, dtype=np.int32) if channels is None else np.ascontiguousarray(channels, dtype=np.int32)
        n = int(ch.shape[0])
        det, rule, tr = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        rel = np.zeros(n, np.float32)
        _check(lib().wfst_decoder_endpoint_detected(self.h, _i32(ch), n, _i32(det), _i32(rule), _i32(tr), _f32(rel)))
        return det.astype(bool), rule, tr, rel

    def partial_enqueue(self, channels=None, cap_words=256):
        """First half of partial(): the work goes on the results stream behind the listed channels' own; returns at once."""
        ch = np.arange(self.n, dtype=np.int32) if channels is None else np.ascontiguousarray(channels, dtype=np.int32)
        _check(lib().wfst_decoder_partial_enqueue(self.h, _i32(ch), int(ch.shape[0]), int(cap_words)))
        self._partial_req = (int(ch.shape[0]), int(cap_words))

    def partial_ready(self):
        rc = lib().wfst_decoder_partial_ready(self.h)
        if rc < 0:
            _check(rc)
        return bool(rc)

    def partial_fetch(self):
        n, cap = self._partial_req
        words = np.zeros((n, cap), np.int32)
        nw, ns, sf = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(lib().wfst_decoder_partial_fetch(self.h, _i32(words), _i32(nw), _i32(ns), _i32(sf)))
        return [words[i, : nw[i]].copy() for i in range(n)], ns, sf

    def partial(self, channels=None, cap_words=256):
        """Partial words of the listed channels (all if None) mid-utterance (wfst_decoder_get_partial): (words: one int32 array per
        channel -- those of best_paths(use_final_probs=False) now --, n_stable int32[n]: how many of them can no longer change,
        stable_frame int32[n]: the frame of the commit token, 0 if none yet)."""
        self.partial_enqueue(channels, cap_words)
        return self.partial_fetch()

    def set_silence_phones(self, phones):
        """The silence phones that word end times skip (wfst_decoder_set_silence_phones); an empty list clears them."""
        a = np.ascontiguousarray(phones, dtype=np.int32).reshape(-1)
        _check(lib().wfst_decoder_set_silence_phones(self.h, _i32(a) if a.size else None, int(a.size)))

    def words_enqueue(self, channels=None, use_final_probs=True, cap_words=256):
        """First half of words(): the work goes on the results stream behind the listed channels' own; returns at once."""
        ch = np.arange(self.n, dtype=np.int32) if channels is None else np.ascontiguousarray(channels, dtype=np.int32)
        _check(lib().wfst_decoder_words_enqueue(self.h, _i32(ch), int(ch.shape[0]), int(bool(use_final_probs)), int(cap_words)))
        self._words_req = (int(ch.shape[0]), int(cap_words))

    def words_ready(self):
        rc = lib().wfst_decoder_words_ready(self.h)
        if rc < 0:
            _check(rc)
        return bool(rc)

    def words_fetch(self):
        n, cap = self._words_req
        words, begin, end = np.zeros((n, cap), np.int32), np.zeros((n, cap), np.int32), np.zeros((n, cap), np.int32)
        nw, nh = np.zeros(n, np.int32), np.zeros(n, np.int32)
        tot, lm = np.zeros(n, np.float32), np.zeros(n, np.float32)
        _check(lib().wfst_decoder_words_fetch(self.h, _i32(words), _i32(begin), _i32(end), _i32(nw), _i32(nh), _f32(tot), _f32(lm)))
        return [(words[i, : nw[i]].copy(), begin[i, : nw[i]].copy(), end[i, : nw[i]].copy(), tot[i], lm[i], int(nh[i])) for i in range(n)]

    def words(self, channels=None, use_final_probs=True, cap_words=256):
        """The best path of the listed channels (all if None) as words with times, in one launch (wfst_decoder_get_words): per
        channel (words int32[k], begin int32[k], end int32[k] -- frames, end exclusive --, tot_score float32, lm_score float32,
        n_hops).  More than cap_words words: WfstError (WFST_E_CAPACITY)."""
        self.words_enqueue(channels, use_final_probs, cap_words)
        return self.words_fetch()

    def frontier(self, channel, cap=1 << 20):
        st = np.zeros(cap, np.int32)
        co = np.zeros(cap, np.float32)
        n = lib().wfst_decoder_get_frontier(self.h, int(channel), int(cap), _i32(st), _f32(co))
        if n < 0:
            _check(n)
        k = min(n, cap)
        return st[:k].copy(), co[:k].copy()
