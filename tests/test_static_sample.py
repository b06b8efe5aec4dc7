"""Static checks of the sampler's compiled gfx950 code (CPU: hipcc cross-compiles; no GPU needed), in the style of
tests/test_static_asm.py: sample.hip is compiled on its own as the product build compiles it, and the compiler's resource-usage
remarks must show that no instantiation of sample_advance_kernel (nor the kernel-level entry's sample_rows_kernel) owns scratch or
spills - sixteen waves share one CU and up to 148 KiB of its LDS; a spilling variant would put the per-slot pick back on the step's
critical path."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aurora_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sample_advance_kernel_owns_no_scratch(tmp_path):
    from aurora_amd.build import COMMON, PER_FILE, SOURCES
    assert "sample.hip" in SOURCES
    cmd = [HIPCC, *COMMON, *PER_FILE.get("sample.hip", []), "-Rpass-analysis=kernel-resource-usage", "-c", "--cuda-device-only",
           "-o", str(tmp_path / "sample.o"), os.path.join(CSRC, "sample.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage = {}
    name = None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|VGPRs|LDS Size \[bytes/block\]|Dynamic Stack): (\S+)", ln)
        if m and name:
            usage[name][m.group(1)] = m.group(2)
    picks = {k: v for k, v in usage.items() if "sample_advance_kernel" in k}
    rows = {k: v for k, v in usage.items() if "sample_rows_kernel" in k}
    assert len(picks) == 2 and len(rows) == 2, sorted(usage)            # the LDS-staged and the re-reading instantiation of each
    for k, v in {**picks, **rows}.items():
        assert v["ScratchSize [bytes/lane]"] == "0" and v["SGPRs Spill"] == "0" and v["VGPRs Spill"] == "0" and v["Dynamic Stack"] == "False", (k, v)
        assert int(v["VGPRs"]) <= 128, (k, v)                               # 1024 threads: 4 waves per SIMD
        assert int(v["LDS Size [bytes/block]"]) + 148 * 1024 <= 160 * 1024, (k, v)   # bins + the staged row fit the CU's LDS


def test_sampler_sources_keep_to_plain_stores():
    """the sampler writes its results with ordinary stores in C++: no inline assembly in sample.hip or advance.h"""
    for f in ("sample.hip", "advance.h"):
        src = open(os.path.join(CSRC, f)).read()
        assert "asm" not in re.sub(r"//.*", "", src), f
