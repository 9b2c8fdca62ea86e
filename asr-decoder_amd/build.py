"""Build libwfstdec.so (HIP kernels + C ABI) for gfx950, in-tree.

hipcc cross-compiles without a GPU.  The result is asr-decoder_amd/lib/libwfstdec.so; it is
git-ignored (history stays source-only) but travels with the repo snapshot to the GPU box.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "csrc", "wfst_kernels.hip"), os.path.join(HERE, "csrc", "wfst_nbest.hip"),
        os.path.join(HERE, "csrc", "wfst_determinize.hip"), os.path.join(HERE, "csrc", "wfst_compose.hip"), os.path.join(HERE, "csrc", "wfst_ingest.hip"),
        os.path.join(HERE, "csrc", "wfst_capi.cc"), os.path.join(HERE, "csrc", "wfst_capi_words.cc"), os.path.join(HERE, "csrc", "wfst_capi_ingest.cc"),
        os.path.join(HERE, "csrc", "wfst_capi_nbwords.cc"), os.path.join(HERE, "csrc", "wfst_capi_liveprune.cc"),
        os.path.join(HERE, "csrc", "wfst_align.hip"), os.path.join(HERE, "csrc", "wfst_capi_align.cc"), os.path.join(HERE, "csrc", "wfst_capi_wordquery.cc"),
        os.path.join(HERE, "csrc", "wfst_nearest.hip"), os.path.join(HERE, "csrc", "wfst_capi_nearest.cc"),
        os.path.join(HERE, "csrc", "wfst_posterior.hip"), os.path.join(HERE, "csrc", "wfst_capi_posterior.cc"),
        os.path.join(HERE, "csrc", "wfst_seqpost.hip"), os.path.join(HERE, "csrc", "wfst_capi_seqpost.cc"),
        os.path.join(HERE, "csrc", "wfst_altern.hip"), os.path.join(HERE, "csrc", "wfst_capi_altern.cc"),
        os.path.join(HERE, "csrc", "wfst_framepost.hip"), os.path.join(HERE, "csrc", "wfst_capi_framepost.cc"),
        os.path.join(HERE, "csrc", "wfst_rescale.hip"), os.path.join(HERE, "csrc", "wfst_capi_rescale.cc"),
        os.path.join(HERE, "csrc", "wfst_bias.hip"), os.path.join(HERE, "csrc", "wfst_capi_bias.cc"),
        os.path.join(HERE, "csrc", "wfst_bias_sparse.hip"), os.path.join(HERE, "csrc", "wfst_capi_bias_sparse.cc"),
        os.path.join(HERE, "csrc", "wfst_seqstat.hip"), os.path.join(HERE, "csrc", "wfst_capi_seqstat.cc"),
        os.path.join(HERE, "csrc", "wfst_forced.hip"), os.path.join(HERE, "csrc", "wfst_capi_forced.cc"),
        os.path.join(HERE, "csrc", "wfst_graphpost.hip"), os.path.join(HERE, "csrc", "wfst_capi_graphpost.cc"),
        os.path.join(HERE, "csrc", "wfst_openfst.cc")]
HDRS = [os.path.join(HERE, "csrc", "wfst_device.h"), os.path.join(HERE, "csrc", "wfst_determinize.h"), os.path.join(HERE, "csrc", "wfst_determinize_wave.h"), os.path.join(HERE, "csrc", "wfst_openfst.h"), os.path.join(HERE, "csrc", "wfst_hip_own.h"), os.path.join(HERE, "csrc", "wfst_capi_words.h"), os.path.join(HERE, "csrc", "wfst_capi_ingest.h"), os.path.join(HERE, "csrc", "wfst_ingest.h"), os.path.join(HERE, "csrc", "wfst_capi_nbwords.h"), os.path.join(HERE, "csrc", "wfst_capi_liveprune.h"), os.path.join(HERE, "csrc", "wfst_capi_align.h"), os.path.join(HERE, "csrc", "wfst_align_index.h"), os.path.join(HERE, "csrc", "wfst_capi_nearest.h"), os.path.join(HERE, "csrc", "wfst_capi_posterior.h"), os.path.join(HERE, "csrc", "wfst_lattice_sweep.h"), os.path.join(HERE, "csrc", "wfst_capi_seqpost.h"), os.path.join(HERE, "csrc", "wfst_capi_altern.h"), os.path.join(HERE, "csrc", "wfst_capi_framepost.h"), os.path.join(HERE, "csrc", "wfst_capi_rescale.h"), os.path.join(HERE, "csrc", "wfst_capi_bias.h"), os.path.join(HERE, "csrc", "wfst_capi_bias_sparse.h"), os.path.join(HERE, "csrc", "wfst_capi_seqstat.h"), os.path.join(HERE, "csrc", "wfst_capi_forced.h"), os.path.join(HERE, "csrc", "wfst_capi_graphpost.h"),
        os.path.join(HERE, "..", "include", "wfst_decoder.h")]
LIB = os.path.join(HERE, "lib", "libwfstdec.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -ffp-contract=off: the search must round like the reference (no FMA; configure.ac:12-13)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
         "-Wall", "-Wno-unused-function"]


def up_to_date():
    if not os.path.exists(LIB):
        return False
    t = os.path.getmtime(LIB)
    return all(os.path.getmtime(p) <= t for p in SRCS + HDRS + [os.path.abspath(__file__)])


def build(force=False, verbose=False):
    if not force and up_to_date():
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    cmd = [HIPCC] + FLAGS + ["-o", LIB] + SRCS
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


def build_variant(name, defines):
    """Kernel experiments: the library built with extra -D flags as lib/libwfstdec_<name>.so (wfstdec.py loads it when
    WFST_LIB_VARIANT=<name>; tools/ab_bench.sh)."""
    out = os.path.join(HERE, "lib", "libwfstdec_%s.so" % name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([HIPCC] + FLAGS + list(defines) + ["-o", out] + SRCS)
    return out


INGEST_SRC = os.path.join(HERE, "csrc", "wfst_ingest.hip")


def kernel_resources(extra=(), source=None):
    """What the compiler made of the kernels of `source` (default: the decode kernels, wfst_kernels.hip; device code only, the library's own flags):
    {kernel name: {"vgprs", "agprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "occupancy", "lds"}} from
    -Rpass-analysis=kernel-resource-usage; "lds" is the static LDS in bytes.  Template instantiations keep their mangled names,
    plain kernels go by their function name.  (tests/test_kernel_resources.py; `python build.py --resources [source]` prints the lines.)"""
    import re
    import tempfile
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC] + flags + list(extra) + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                           "-o", os.path.join(tmp, "kernels.o"), source or SRCS[0]],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds"}
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(.*?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            plain = re.match(r"_ZN4wfstL?(\d+)", name)   # wfst::<name>(...): the plain kernels
            if plain and "I" not in name[len(plain.group(0)) + int(plain.group(1)):][:1]:
                a = len(plain.group(0))
                name = name[a:a + int(plain.group(1))]
            cur = out.setdefault(name, {})
        elif cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


if __name__ == "__main__":
    if "--resources" in sys.argv:   # --resources [source file]
        src = sys.argv[sys.argv.index("--resources") + 1:]
        for k, v in sorted(kernel_resources(source=src[0] if src else None).items()):
            print(k, " ".join("%s=%d" % kv for kv in sorted(v.items())))
    elif "--variant" in sys.argv:
        i = sys.argv.index("--variant")
        print(build_variant(sys.argv[i + 1], [a for a in sys.argv[i + 2:] if a.startswith("-D")]))
    else:
        build(force="--force" in sys.argv, verbose=True)
        print(LIB)
