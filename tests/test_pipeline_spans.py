"""The offset arithmetic of the host pipeline's ragged outputs and padded blobs (host_common.h span_start / span_bytes) in a
stand-alone host program (tests/hostsim/pipeline_spans.hip) under AddressSanitizer / UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spans_cover_a_ragged_blob_exactly_once():
    src, exe = os.path.join(ROOT, "tests", "hostsim", "pipeline_spans.hip"), os.path.join(ROOT, "build", "pipeline_spans_san")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "circl_amd", "csrc"), "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "spans ok" in r.stdout, r.stdout[-3000:]
