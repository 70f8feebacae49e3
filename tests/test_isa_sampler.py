"""The matrix sampler of the headline kernel (mlkem_encrypt_kernel<3, ENCAPS, 0, true, KM_ITEM>) in its gfx950 ISA: the three-block parse
(parse_shake128_block_fifo<false>, mlkem_kernels.h) checks its FIFO for a flush after candidates 32, 64, 96 and 112 of a block -- four
conditional flush sites, each moving 64 bytes (four 16-byte FIFO reads, four 16-byte row stores), where the parent had fourteen of 16 bytes --
inside the parent's register and scratch budget, and the kernel's LDS is what the launcher asks for.

Reads the assembly the library build leaves in build/ (python -m circl_amd.build); without one (or with one older than the kernel's
header) it compiles the headline kernel alone, as tests/test_isa_ring.py does.  `python tests/test_isa_sampler.py [<file.s>]` prints the
figures."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN5circl5mlkem20mlkem_encrypt_kernelILi3ELi0ELi0ELb1ELi0EEEv"  # <K = 3, ENCAPS, ABLATE 0, SCRATCH, KM_ITEM>
BUILT = os.path.join(ROOT, "build", "api_mlkem-hip-amdgcn-amd-amdhsa-gfx950.s")
HEADER = os.path.join(ROOT, "circl_amd", "csrc", "mlkem_kernels.h")

PARENT_NUM_VGPR = 128
PARENT_SCRATCH_BYTES = 192        # the parent's headline kernel inside the library build of api_mlkem.hip
PARENT_FLUSH_SITES = 14           # a check every 8 candidates
CU_LDS_BYTES = 160 * 1024


def _assembly(workdir):
    if os.path.exists(BUILT) and os.path.getmtime(BUILT) >= os.path.getmtime(HEADER):
        return open(BUILT).read()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, asm = os.path.join(workdir, "headline.hip"), os.path.join(workdir, "headline.s")
    with open(src, "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "mlkem_kernels.h"\n'
                "template __global__ void circl::mlkem::mlkem_encrypt_kernel<3, circl::mlkem::ENCAPS, 0, true, circl::mlkem::KM_ITEM>(\n"
                "    const uint8_t *, size_t, const uint8_t *, const uint8_t *, uint8_t *, uint8_t *, uint8_t *, const uint8_t *, const uint8_t *,\n"
                "    uint8_t *, unsigned *, size_t, const circl::KeyIdx, const int16_t *);\n")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", "-I", os.path.join(ROOT, "circl_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), src, "-o", asm], stderr=subprocess.DEVNULL)
    return open(asm).read()


def launcher_lds_bytes():
    """Geom<3>::LDS_SCRATCH_TOTAL as the header states it: the larger of the FIFO area (64 lanes x (2 bytes x slots + 16)) and the
    noise + exchange areas.  The big-batch launchers of api_mlkem.hip pass exactly this constant."""
    text = open(HEADER).read()
    flush = int(re.search(r"#define CIRCL_KEM_FIFO_FLUSH (\d+)", text).group(1))
    assert "FIFO_SLOTS = FIFO_FLUSH > 16 ? 2 * FIFO_FLUSH : 32;" in text and "FIFO_STRIDE = 2 * FIFO_SLOTS + 16;" in text
    assert "LDS_FIFO = 64 * FIFO_STRIDE;" in text
    slots = 2 * flush if flush > 16 else 32
    fifo = 64 * (2 * slots + 16)
    noise_xch = 7 * 7 * (64 * 2 + 8) + 1024      # G x NOISE x NOISE_STRIDE + LDS_XCH at K = 3
    api = open(os.path.join(ROOT, "circl_amd", "csrc", "api_mlkem.hip")).read()
    assert "Gm::LDS_SCRATCH_TOTAL" in api
    return max(fifo, noise_xch), fifo // 64


def sampler_stats(text):
    m = re.search(r"^(%s\w*):[^\n]*\n(.*?)^\.Lfunc_end(.*?)\.end_amdhsa_kernel" % KERNEL, text, re.M | re.S)
    assert m, "headline kernel not found in the ISA"
    name, body, tail = m.group(1), m.group(2), m.group(3)
    lines = [ln.split(";")[0].strip() for ln in body.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith(".") and not ln.endswith(":")]
    op = [ln.split()[0] for ln in lines]
    # the three-block parse body (the first parse in program order; a block has 112 candidates): from the kernel's first FIFO write to
    # the block loop's branch behind its 112th, the last flush site included
    writes = [i for i, o in enumerate(op) if o == "ds_write_b16"]
    assert len(writes) >= 112
    end = next((i for i in range(writes[111], len(op)) if op[i].startswith("s_cbranch_scc") or op[i] == "s_branch"), len(op))
    span = op[writes[0]:end]
    adds = [i for i, ln in enumerate(lines) if re.match(r"v_addc_co_u32_e32 (v\d+), vcc, 0, \1, vcc$", ln)]
    meta = re.search(r"\.name:\s+%s\n(?:    \..*\n)*" % re.escape(name), text)
    blk_start = text.rfind("  - .agpr_count", 0, meta.start())
    blk = text[blk_start:text.find("  - .agpr_count", meta.end()) if text.find("  - .agpr_count", meta.end()) > 0 else len(text)]

    def field(k):
        return int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
    occ = re.search(r"; Occupancy: (\d+)", tail)
    return {
        "num_vgpr": field("vgpr_count"), "scratch_bytes": field("private_segment_fixed_size"), "static_lds_bytes": field("group_segment_fixed_size"),
        "occupancy": int(occ.group(1)) if occ else -1,
        "accept_adds": len(adds), "accept_adds_behind_their_compare": sum(1 for i in adds if op[i - 1] == "v_cmp_gt_u32_e32"),
        "parse_fifo_writes": span.count("ds_write_b16"), "parse_flush_sites": span.count("s_and_saveexec_b64"),
        "parse_fifo_reads_b128": span.count("ds_read_b128"), "parse_row_stores_x4": span.count("global_store_dwordx4"),
        "fifo_lane_stride_0x90": len(re.findall(r"\b0x90\b", body)),
    }


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    return sampler_stats(_assembly(str(tmp_path_factory.mktemp("isa_sampler"))))


def test_register_scratch_and_lds_budget(stats):
    print(stats)
    lds, lane_stride = launcher_lds_bytes()
    assert stats["num_vgpr"] == PARENT_NUM_VGPR and stats["occupancy"] == 4, stats
    assert 0 <= stats["scratch_bytes"] <= PARENT_SCRATCH_BYTES, stats
    # all of the kernel's LDS is the launch's dynamic size: 9 216 bytes (64 lanes x 144), sixteen wavefronts of it in a CU's 160 KiB
    assert stats["static_lds_bytes"] == 0 and lds == 9216 and lane_stride == 144 and 16 * lds <= CU_LDS_BYTES, (stats, lds)
    assert stats["fifo_lane_stride_0x90"] >= 1, stats        # lane x 144 bytes addresses the FIFO


def test_accept_add_sits_directly_behind_its_compare(stats):
    assert stats["accept_adds"] >= 3 * 112, stats
    assert stats["accept_adds_behind_their_compare"] == stats["accept_adds"], stats


def test_three_block_parse_has_four_flush_sites(stats):
    assert stats["parse_fifo_writes"] == 112, stats
    assert stats["parse_flush_sites"] == 4 < PARENT_FLUSH_SITES, stats
    assert stats["parse_fifo_reads_b128"] == 16 and stats["parse_row_stores_x4"] == 16, stats   # 64 bytes a site


if __name__ == "__main__":
    if len(sys.argv) > 1:
        print(sampler_stats(open(sys.argv[1]).read()))
    else:
        with tempfile.TemporaryDirectory() as d:
            print(sampler_stats(_assembly(d)))
