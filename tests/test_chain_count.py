"""The instruction count of the chain that ends the cold one-launch tick (tools/chain_count.py: the QP of the hardest wavefront, nine trips and one drop)
stays at least 5 % below what it was before the diet of csrc/qp_struct16.hip.hpp (DIET).  A lone wavefront issues one instruction per ~5.5 cycles whatever
its kind, so a change that lengthens this chain lengthens the kernel; no functional test would notice."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# tools/chain_count.py on the commit in front of the diet ("Contact-input parity: all masks, steep normals, wide mu, per family"), hipcc of ROCm 7.2, gfx950:
# set-up 143 + 343, trip 256, add-commit 54, drop path 385, tail 83  ->  143 + 343 + 9 x (256 + 54) + 385 + 83
PARENT_CHAIN9 = 3744


def _tool():
    spec = importlib.util.spec_from_file_location("chain_count", os.path.join(ROOT, "tools", "chain_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_chain9_stays_five_per_cent_below_the_parent(tmp_path):
    mod = _tool()
    r = mod.analyse(mod.compile_unit(str(tmp_path / "k_fused_f64.s")))
    p = r["parts"]
    print("chain9 %d = %d + %d + 9 x (%d + %d) + %d + %d; parent %d" % (p["chain9"], p["setup_lever"], p["setup_wdes"], p["trip"], p["commit"], p["drop"], p["tail"], PARENT_CHAIN9))
    assert p["chain9"] == p["setup_lever"] + p["setup_wdes"] + 9 * (p["trip"] + p["commit"]) + p["drop"] + p["tail"]
    assert min(p["setup_lever"], p["setup_wdes"], p["trip"], p["commit"], p["drop"], p["tail"]) > 0, p     # every part was found
    assert p["chain9"] <= 0.95 * PARENT_CHAIN9, p


def test_the_counter_finds_the_parts_of_a_small_loop(tmp_path):
    """a hand-written kernel of the same shape: two flag waits, a bottom-tested loop with a skipped add-commit and a skipped drop region, a tail"""
    mod = _tool()
    lines = ["_ZN3wbc17fused_tick_kernelIdLb0ELb1ELb0EJPKdEEvv:", "\tv_mov_b32_e32 v0, 0",
             ".LBB0_1:", "\ts_sleep 1", "\tds_read_b32 v1, v0", "\ts_cbranch_vccnz .LBB0_1",
             ".LBB0_2:", "\tv_rsq_f64_e32 v[2:3], v[4:5]", "\tv_mul_f64 v[2:3], v[2:3], v[2:3]",
             ".LBB0_3:", "\ts_sleep 1", "\tds_read_b32 v1, v0", "\ts_cbranch_vccnz .LBB0_3",
             ".LBB0_4:", "\tv_add_f64 v[2:3], v[2:3], v[2:3]", "\tv_add_f64 v[2:3], v[2:3], v[2:3]", "\tv_add_f64 v[2:3], v[2:3], v[2:3]",
             ".LBB0_5:", "\tds_read_b64 v[6:7], v0", "\tv_rcp_f64_e32 v[8:9], v[6:7]", "\tv_cndmask_b32_e32 v1, v1, v2, vcc", "\ts_cbranch_vccz .LBB0_7",
             ".LBB0_6:", "\tv_rcp_f64_e32 v[8:9], v[6:7]", "\tds_write_b64 v0, v[8:9]",
             ".LBB0_7:", "\ts_and_b64 vcc, vcc, exec", "\ts_cbranch_vccz .LBB0_9",
             ".LBB0_8:", "\tds_bpermute_b32 v1, v1, v2", "\tv_rsq_f64_e32 v[2:3], v[4:5]", "\tv_mov_b32_e32 v1, v2",
             ".LBB0_9:", "\tv_cmp_lt_i32_e32 vcc, -1, v1", "\ts_cbranch_vccnz .LBB0_5",
             ".LBB0_10:", "\tv_mov_b32_e32 v1, v2", "\tglobal_store_dword v[2:3], v1, off", "\tv_mov_b32_e32 v1, v2", "\ts_endpgm", "\t.section\t.rodata"]
    p = tmp_path / "k.s"
    p.write_text("\n".join(lines) + "\n")
    r = mod.analyse(str(p))["parts"]
    assert (r["setup_lever"], r["setup_wdes"], r["trip"], r["commit"], r["drop"], r["tail"]) == (2, 3, 4 + 2 + 2, 2, 3, 2), r
    assert r["chain9"] == 2 + 3 + 9 * (8 + 2) + 3 + 2
