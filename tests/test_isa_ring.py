"""The ring phase of the headline kernel (mlkem_encrypt_kernel<3, ENCAPS, 0, true, KM_ITEM>) in its gfx950 ISA, compiled here (hipcc
cross-compiles without a GPU): the transforms re-distribute their polynomial across the lanes (V_PERMLANE32/16_SWAP, DPP moves) instead
of through LDS, inside the same register budget.

The PARENT_* constants are the figures of the tree before the cross-lane exchange (the LDS form with barriers), taken from ITS ISA with
this file's own ring_stats() -- same compiler, same flags: run `python tests/test_isa_ring.py <tree>` on a checkout to print them."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN5circl5mlkem20mlkem_encrypt_kernelILi3ELi0ELi0ELb1ELi0EEEv"  # <K = 3, ENCAPS, ABLATE 0, SCRATCH, KM_ITEM>

# the parent's figures (see the module docstring): from the s_setprio 1 that opens the ring phase to the end of the kernel ...
PARENT_RING_DS_WRITE_B16 = 44
PARENT_RING_DS_READ_U16 = 40
PARENT_RING_WAITCNT = 67
# ... and of the whole kernel.  (Spilled dwords: 58 in this file's stand-alone translation unit, 56 for the same kernel inside the parent's
# library build of api_mlkem.hip; the bound is the lower of the two.)
PARENT_NUM_VGPR = 128
PARENT_VGPR_SPILL = 56
PARENT_KERNEL_S_NOP = 347


def ring_stats(root, workdir):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(workdir, "headline.hip")
    with open(src, "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "mlkem_kernels.h"\n'
                "template __global__ void circl::mlkem::mlkem_encrypt_kernel<3, circl::mlkem::ENCAPS, 0, true, circl::mlkem::KM_ITEM>(\n"
                "    const uint8_t *, size_t, const uint8_t *, const uint8_t *, uint8_t *, uint8_t *, uint8_t *, const uint8_t *, const uint8_t *,\n"
                "    uint8_t *, unsigned *, size_t, const circl::KeyIdx, const int16_t *);\n")
    asm = os.path.join(workdir, "headline.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", "-I", os.path.join(root, "circl_amd", "csrc"),
                           "-I", os.path.join(root, "include"), src, "-o", asm], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    m = re.search(r"^(%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % KERNEL, text, re.M | re.S)
    assert m, "headline kernel not found in the ISA"
    name, body = m.group(1), m.group(2)
    lines = [ln.split(";")[0].strip() for ln in body.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith(".") and not ln.endswith(":")]
    op = [ln.split()[0] for ln in lines]
    first_prio = next(i for i, ln in enumerate(lines) if re.match(r"s_setprio\s+1\b", ln))
    ring = op[first_prio:]
    nvgpr = re.search(r"\.set %s\.num_vgpr, (\d+)" % re.escape(name), text)
    spill = re.search(r"\.name:\s+%s\n(?:    \..*\n)*?    \.vgpr_spill_count:\s+(\d+)" % re.escape(name), text)
    # the sampler's accept counter (count_accept, mlkem_kernels.h): every add with carry-in and a zero addend ...
    adds = [i for i, ln in enumerate(lines) if re.match(r"v_addc_co_u32_e32 (v\d+), vcc, 0, \1, vcc$", ln)]
    stats = {
        "accept_adds": len(adds), "accept_adds_behind_their_compare": sum(1 for i in adds if op[i - 1] == "v_cmp_gt_u32_e32"),
        "ring_ds_write_b16": ring.count("ds_write_b16"), "ring_ds_read_u16": ring.count("ds_read_u16"),
        "ring_waitcnt": sum(1 for o in ring if o == "s_waitcnt"),
        "ring_permlane32_swap": sum(1 for o in ring if o.startswith("v_permlane32_swap")),
        "ring_permlane16_swap": sum(1 for o in ring if o.startswith("v_permlane16_swap")),
        "ring_dpp": sum(1 for ln in lines[first_prio:] if re.search(r"\b(quad_perm|row_shl|row_shr|row_ror)\b", ln)),
        "ring_insts": len(ring), "kernel_insts": len(op),
        "kernel_ds_write_b16": op.count("ds_write_b16"), "kernel_s_nop": op.count("s_nop"),
        "head_permlane_swaps": sum(1 for o in op[:first_prio] if o.startswith("v_permlane")),
        "num_vgpr": int(nvgpr.group(1)) if nvgpr else -1,
        "vgpr_spill": int(spill.group(1)) if spill else -1,
    }
    return stats


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    return ring_stats(ROOT, str(tmp_path_factory.mktemp("isa_ring")))


def test_ring_phase_exchanges_across_the_lanes(stats):
    print(stats)
    assert stats["ring_permlane32_swap"] > 0 and stats["ring_permlane16_swap"] > 0, stats
    assert stats["head_permlane_swaps"] == 0, stats  # (they belong to the ring phase, behind the s_setprio 1 that opens it)


def test_ring_phase_has_fewer_lds_round_trips_and_waits_than_the_parent(stats):
    assert stats["ring_ds_write_b16"] < PARENT_RING_DS_WRITE_B16, stats
    assert stats["ring_ds_read_u16"] < PARENT_RING_DS_READ_U16, stats
    assert stats["ring_waitcnt"] < PARENT_RING_WAITCNT, stats


def test_register_budget_is_the_parents(stats):
    assert stats["num_vgpr"] == PARENT_NUM_VGPR, stats
    assert 0 <= stats["vgpr_spill"] <= PARENT_VGPR_SPILL, stats


def test_accept_counter_is_compare_and_add_with_carry(stats):
    """... sits directly behind the v_cmp_gt_u32 that feeds it: no s_nop, no v_cndmask in between; the kernel as a whole loses most
    of its hazard waits (3 blocks of 112 candidates, unrolled, in two copies of the parser)."""
    assert stats["accept_adds"] >= 3 * 112, stats
    assert stats["accept_adds_behind_their_compare"] == stats["accept_adds"], stats
    assert stats["kernel_s_nop"] < PARENT_KERNEL_S_NOP // 2, stats


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(ring_stats(sys.argv[1] if len(sys.argv) > 1 else ROOT, d))
