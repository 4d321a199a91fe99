"""Register, scratch and LDS budget of the two MFMA update kernels, read from the code object's metadata (no GPU).

The dense-front kernel ssssm_front_f64_kernel<2,true> and the general kernel ssssm_tilesv_f64_kernel are written for four
wavefronts per SIMD (512 threads, two workgroups per CU): at most 128 vector registers, nothing spilled to scratch, and for the
front kernel two LDS stages of 34 816 bytes.  A change to either kernel (pg_hip_front.h) that crosses one of these lines halves the
occupancy or adds memory traffic without failing any numerical test: this file fails instead.

The R64 platform is compiled for gfx950 (device side only) with --save-temps; only .vgpr_count, .private_segment_fixed_size and
.group_segment_fixed_size of the two kernels are read.

Cost: one device-side compile of the whole R64 platform, once for both tests -- two to three minutes of one core on an idle machine,
more beside other work; by far the slowest file of the CPU suite, and the only one that sees these three numbers."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")
FRONT = "_Z22ssssm_front_f64_kernelILi2ELb1EE"  # ssssm_front_f64_kernel<2, true>(...)
TILESV = "_Z23ssssm_tilesv_f64_kernelPK"        # ssssm_tilesv_f64_kernel(...)
FIELDS = (".vgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    """{mangled kernel name: {field: int}} of every kernel of the R64 platform."""
    tmp = tmp_path_factory.mktemp("front_build")
    src = os.path.join(ROOT, "pangulu_amd", "csrc", "platform", "pg_hip_platform.hip")
    # the product's flags (pangulu_amd/csrc/Makefile: HIPFLAGS)
    cmd = [os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-DCALCULATE_TYPE_R64",
           "-Wno-unused-result", "--cuda-device-only", "--save-temps", "-c", src, "-o", "pg_hip_platform.o"]
    out = subprocess.run(cmd, cwd=str(tmp), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    asm = glob.glob(os.path.join(str(tmp), "*gfx950*.s"))
    assert len(asm) == 1, sorted(os.listdir(str(tmp)))
    text = open(asm[0]).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        if not name:
            continue
        kernels[name.group(1)] = {f: int(re.search(r"^\s*%s:\s*(\d+)" % re.escape(f), entry, re.M).group(1)) for f in FIELDS}
    return kernels


def _one(kernels, prefix):
    hits = [k for k in kernels if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    print(hits[0], kernels[hits[0]])
    return kernels[hits[0]]


def test_front_kernel_resources(kernel_metadata):
    k = _one(kernel_metadata, FRONT)
    assert k[".vgpr_count"] <= 128, k                   # four wavefronts per SIMD
    assert k[".private_segment_fixed_size"] == 0, k     # no scratch
    assert k[".group_segment_fixed_size"] == 69632, k   # two stages of 16 x 144 + 128 x 16 doubles


def test_general_kernel_resources(kernel_metadata):
    k = _one(kernel_metadata, TILESV)
    assert k[".vgpr_count"] <= 128, k
    assert k[".private_segment_fixed_size"] == 0, k
    assert k[".group_segment_fixed_size"] <= 81920, k   # two workgroups per CU (160 KiB of LDS)
