"""The thread-per-(destination, head) GAT kernels of re_gat.hip (gat_softmax_fwd_generic,
gat_softmax_bwd_generic, segment_sum_generic: head counts that are no power of two <= 32) built
for the host from their own source text and run with one thread per GPU thread
(tests/host/gat_generic_host.cpp), under AddressSanitizer and UBSan:
the backward's relation bins must not depend on 256 % H, the grid-stride loops must keep a
thread's head, and no index may leave its array. No GPU and no HIP library."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "re-gnn_amd", "csrc", "re_gat.hip")
HARNESS = os.path.join(ROOT, "tests", "host", "gat_generic_host.cpp")
KERNELS = ("gat_softmax_fwd_generic", "gat_softmax_bwd_generic", "segment_sum_generic")


def _kernel_text():
    text = open(SRC).read()
    m = re.search(r"^__host__ __device__ inline int gat_generic_act\(.*?^}\n", text, re.S | re.M)
    assert m, "gat_generic_act not found in re_gat.hip"
    out = [m.group(0)]
    for name in KERNELS:
        m = re.search(r"^__global__ void __launch_bounds__\(kBlock\)\n" + name + r"\(.*?^}\n", text,
                      re.S | re.M)
        assert m, f"{name} not found in re_gat.hip"
        out.append(m.group(0))
    body, n = re.subn(r"^ *extern __shared__ float bins\[\];.*$", "    // LDS: the global bins",
                      "\n".join(out), flags=re.M)
    assert n == 1
    return body


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler found (g++ / clang++)")


def test_generic_gat_kernels_on_host(tmp_path):
    (tmp_path / "gat_generic_kernels.inc").write_text(_kernel_text())
    exe = str(tmp_path / "host_kernel")
    base = [_compiler(), "-std=c++20", "-O1", "-g", "-pthread", "-I", str(tmp_path), HARNESS,
            "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr[-4000:]
