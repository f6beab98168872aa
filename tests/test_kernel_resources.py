"""Every kernel in the built librr.so stays out of scratch memory.

The split cores run at the register file's edge (242-256 VGPRs at two waves
per SIMD) and load through inline asm whose registers the compiler does not
track (csrc/h2_*.hip): a spill of such a register before its counted wait would
read an unloaded value.  This reads the gfx950 code-object metadata of the
library that ships (tools/kernel_resources.py) and fails if any kernel has a
private segment (scratch) -- no GPU needed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "research_image_retrieval_amd", "librr.so")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="ROCm llvm tools absent")
def test_no_kernel_uses_scratch():
    if not os.path.exists(LIB):
        pytest.fail("librr.so missing: build it first (make -C research_image_retrieval_amd/csrc)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--check", LIB],
                       capture_output=True, text=True, timeout=120)
    bad = [ln for ln in r.stdout.splitlines() if " scratch " in ln and not ln.split(" scratch ")[1].strip().startswith("0 ")]
    assert r.returncode == 0, "kernels using scratch:\n" + "\n".join(bad) + "\n" + r.stderr[-500:]
    # the f16x2 split-core kernels are all there (tiled, persistent, halo, stem, and the two helpers)
    for name in ("gemm_s3p_kernel<", "gemm_s3_kernel<", "gemm_s3q_kernel<", "gemm_h2_halo_kernel<",
                 "stem_pool_halo_kernel<", "split2h_kernel", "amax_kernel",
                 # the fp32 and the bf16 / fp8 one-tile GEMM cores
                 "gemm_f32_kernel<", "gemm_lp_kernel<"):
        assert name in r.stdout, name
