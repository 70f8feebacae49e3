"""The binder of the host forms' staged arrays (host_compose.h Bind: one declaration per array makes the pipeline's record and the way
back into the chunk's call) in a stand-alone host program (tests/hostsim/pipeline_bind.hip) under AddressSanitizer / UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_each_declared_array_is_staged_and_rebound_by_its_rule():
    src, exe = os.path.join(ROOT, "tests", "hostsim", "pipeline_bind.hip"), os.path.join(ROOT, "build", "pipeline_bind_san")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "circl_amd", "csrc"), "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "bind ok" in r.stdout, r.stdout[-3000:]
