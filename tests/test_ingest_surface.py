"""CPU: the surface of the device-side chunk ingest (wfst_decoder_set_score_transform / _advance_chunk / _get_scores): the header,
the binding's symbol list and the library agree on the names; the header block cites the reference; the argument checks that need
no device; the host mirror builds with its ingest translation unit, which alone calls the new symbols; the CLI lists its flags and
refuses --acoustic-scale alone; what the compiler made of ingest_kernel (no scratch, no spills), with the default report still
that of the decode kernels."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wfst_decoder_set_score_transform", "wfst_decoder_advance_chunk", "wfst_decoder_get_scores"]


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("asr-decoder_amd")
    p.build.build()
    return p


def test_header_binding_and_library_agree(pkg):
    src = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    for define in ("#define WFST_DTYPE_F32 0", "#define WFST_DTYPE_F16 1", "#define WFST_DTYPE_BF16 2", "#define WFST_STREAM_NONE ((void *)(intptr_t)-1)"):
        assert define in src, define
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(wfst_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(pkg.wfstdec.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.wfstdec.SYMBOLS, name
        assert hasattr(lib, name), name
    for method in ("set_score_transform", "advance_chunk", "scores"):
        assert callable(getattr(pkg.wfstdec.BatchDecoder, method)), method
    W = pkg.wfstdec
    assert (W.WFST_DTYPE_F32, W.WFST_DTYPE_F16, W.WFST_DTYPE_BF16) == (0, 1, 2) and W.WFST_STREAM_NONE == ctypes.c_void_p(-1).value


def test_header_cites_the_reference_lines():
    src = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    block = src[src.index("acoustic-model chunks ingested on the device"):]
    for cite in ("kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:37-41,107", "nnet/nnet-nnet.h:212-232", "nnet/nnet-layer.cc:30", "nnet/nnet-nnet.cc:156-164",
                 "(float(x[r][j]) - log_priors[j]) * acoustic_scale"):
        assert cite in block, cite


def test_argument_checks_without_a_device(pkg):
    L = pkg.wfstdec.lib()
    one = (ctypes.c_int32 * 1)(1)
    ptr = (ctypes.c_void_p * 1)(None)
    out = (ctypes.c_float * 4)()
    assert L.wfst_decoder_set_score_transform(None, ctypes.c_float(0.1), None, 0) == -1
    assert b"NULL decoder" in L.wfst_last_error()
    assert L.wfst_decoder_advance_chunk(None, one, 1, ptr, one, None, 1, 4, None, -1) == -1
    assert b"NULL decoder" in L.wfst_last_error()
    assert L.wfst_decoder_get_scores(None, 0, 0, 1, out) == -1
    assert b"NULL decoder" in L.wfst_last_error()


def test_chunk_tensors_are_checked_by_the_binding(pkg):
    """advance_chunk's duck-typed tensors: dtype, width and layout are refused before the library is called."""
    import numpy as np

    class T:
        def __init__(self, shape, stride, dtype):
            self.shape, self._stride, self.dtype = shape, stride, dtype

        def stride(self):
            return self._stride

        def data_ptr(self):
            return 256

    dec = object.__new__(pkg.wfstdec.BatchDecoder)
    dec.n, dec.h = 2, None
    for chunks, msg in (([T((4, 8), (8, 1), np.dtype("int32")), None], "float32, float16 or bfloat16"),
                        ([T((4, 8), (8, 1), "torch.float16"), T((4, 8), (8, 1), "torch.bfloat16")], "differ in dtype or width"),
                        ([T((4, 8), (8, 1), "torch.float16"), T((4, 9), (9, 1), "torch.float16")], "differ in dtype or width"),
                        ([T((4, 8), (1, 4), "torch.float32"), None], "not contiguous"),
                        ([T((4,), (1,), "torch.float32"), None], "not 2-D"),
                        ([None, None], "no chunk")):
        with pytest.raises(ValueError, match=msg):
            dec.advance_chunk(chunks, stream=None)


def test_host_mirror_builds_with_the_ingest_translation_unit(pkg):
    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    assert "wfst-host-ingest.cc" in open(os.path.join(host, "Makefile")).read()
    host_cc = open(os.path.join(host, "wfst-host.cc")).read()
    for name in NAMES:   # the new C symbols are called from the new translation unit only
        assert name not in host_cc, name
    ingest_cc = open(os.path.join(host, "wfst-host-ingest.cc")).read()
    assert "wfst_decoder_set_score_transform" in ingest_cc and "wfst_decoder_advance_chunk" in ingest_cc
    so = os.path.join(ROOT, "asr-decoder_amd", "lib", "libwfsthost.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert "datemoon::GpuBatchDecoder::SetScoreTransform(" in syms and "datemoon::GpuBatchDecoder::AdvanceDecodingChunk(" in syms
    exe = os.path.join(host, "wfst-decode")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 1
    for flag in ("--device-chunks", "--chunk=N", "--acoustic-scale=S", "--log-priors=FILE", "--score-dtype=f32|f16|bf16"):
        assert flag in p.stderr, flag
    # the scale alone is refused before any device work: without --device-chunks the matrices are finished scores
    p = subprocess.run([exe, "--acoustic-scale=0.1", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "go with --device-chunks" in p.stderr
    p = subprocess.run([exe, "--device-chunks", "--acoustic-scale=0.1", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "--device-chunks goes with --chunk=N" in p.stderr


def test_ingest_kernels_use_no_scratch(pkg):
    res = pkg.build.kernel_resources(source=pkg.build.INGEST_SRC)
    kernels = {k: v for k, v in res.items() if "ingest_kernel" in k}
    assert len(kernels) == 3, sorted(res)   # float32, float16, bfloat16
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] == 0 and r["vgprs"] <= 64 and r["occupancy"] == 8, (name, r)


def test_default_resource_report_is_still_the_decode_kernels(pkg):
    b = pkg.build
    sig = inspect.signature(b.kernel_resources)
    assert list(sig.parameters) == ["extra", "source"] and sig.parameters["source"].default is None and sig.parameters["extra"].default == ()
    assert os.path.basename(b.SRCS[0]) == "wfst_kernels.hip"
    res = b.kernel_resources()
    assert any("words_kernel" in k for k in res) and any("closure_kernel" in k for k in res) and not any("ingest" in k for k in res)
