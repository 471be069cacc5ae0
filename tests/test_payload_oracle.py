"""CPU: the plant payload of wbc_*_plant_batch (ABI 10) -- the exactness claim against the oracle's merged model, the C-ABI surface,
and the register / LDS budget of the PAYLOAD kernels in the compiled gfx950 ISA."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import payload_ref
from tests.util import unpack_M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_payload_changes_only_the_base_block_and_base_rows(flat_model, oracle):
    """500 random states and payloads up to 30 % of the total mass with CoM offsets up to 0.15 m: the merged model's dynamics minus the
    nominal model's is zero outside the 6x6 base block of M, in the joint rows of h, in Jc and in pf; inside, delta_terms is exact."""
    rng = np.random.default_rng(2026)
    from oracle import oracle_py
    from wbc_quadruped_dob_amd import synth
    n = 500
    m_total = float(np.sum(flat_model["mass"]))
    B = synth.make_batch(4, n, m_total, rank=5)
    q, v = B["q"], B["v"]
    q[:, 3:7] = rng.normal(size=(n, 4))   # any attitude (not normalised: the dynamics normalise the quaternion)
    v[:, 3:6] = rng.uniform(-3, 3, (n, 3))
    pays = payload_ref.random_payloads(rng, n, m_max=0.3 * m_total, c_max=0.15, zero_every=0)
    nom = oracle.dynamics(q, v)
    g = np.asarray(flat_model["gravity"])
    worst_out, worst_in = 0.0, 0.0
    for i in range(n):
        m, c, I = payload_ref.unpack(pays[i])
        d = oracle_py.Oracle(payload_ref.merge_payload(flat_model, m, c, I)).dynamics(q[i:i + 1], v[i:i + 1])
        dM = unpack_M(d["M"][0] - nom["M"][i])
        dh = d["h"][0] - nom["h"][i]
        scale = max(1.0, np.abs(unpack_M(d["M"][0])).max(), np.abs(d["h"][0]).max())
        out_of_block = dM.copy()
        out_of_block[:6, :6] = 0
        worst_out = max(worst_out, np.abs(out_of_block).max(), np.abs(dh[6:]).max(), np.abs(d["Jc"][0] - nom["Jc"][i]).max(),
                        np.abs(d["pf"][0] - nom["pf"][i]).max())
        eM, eh = payload_ref.delta_terms(q[i], v[i], pays[i], g)
        worst_in = max(worst_in, np.abs(dM[:6, :6] - eM).max() / scale, np.abs(dh[:6] - eh).max() / scale)
    assert worst_out <= 1e-12, worst_out
    assert worst_in <= 1e-11, worst_in


def test_merge_payload_of_nothing_is_the_nominal_model(flat_model, oracle):
    from oracle import oracle_py
    from wbc_quadruped_dob_amd import synth
    B = synth.make_batch(3, 16, 20.0, rank=1)
    a = oracle.dynamics(B["q"], B["v"])
    b = oracle_py.Oracle(payload_ref.merge_payload(flat_model, 0.0, np.zeros(3), np.zeros((3, 3)))).dynamics(B["q"], B["v"])
    for k in ("M", "h", "Jc", "pf"):
        assert np.abs(a[k] - b[k]).max() <= 1e-13, k


def test_abi_exports_the_plant_calls(hip_lib):
    for name in ("wbc_integrate_plant_batch", "wbc_rollout_plant_batch", "wbc_rollout_tracking_plant_batch"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.wbc_abi_version() == 10


def test_plant_struct_layout_matches_the_header(hip_lib):
    """sizeof(wbc_plant) and its field offsets as a C compiler sees the header, against the binding's ctypes mirror."""
    import wbc_quadruped_dob_amd as W
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "wbc_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(wbc_plant), '
           'offsetof(wbc_plant, struct_size), offsetof(wbc_plant, tau_ext), offsetof(wbc_plant, payload), WBC_PAYLOAD_WORDS); return 0; }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c_path, exe = os.path.join(d, "plant.c"), os.path.join(d, "plant")
        open(c_path, "w").write(src)
        subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), c_path, "-o", exe], check=True,
                       capture_output=True, text=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.Plant), W.Plant.struct_size.offset, W.Plant.tau_ext.offset, W.Plant.payload.offset, W.PAYLOAD_WORDS]


def test_plant_calls_check_their_arguments_without_a_gpu(hip_lib):
    """struct_size too small -> WBC_E_INVALID before anything else (no solver needed: the struct is checked first)."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    pl = W.Plant()
    pl.struct_size = C.sizeof(W.Plant) - 8
    pl.payload = C.c_void_p(16)
    p = C.c_void_p(16)
    INVALID = 1
    assert L.wbc_integrate_plant_batch(p, 4, p, p, p, p, p, p, p, C.byref(pl), None) == INVALID
    assert L.wbc_rollout_plant_batch(p, 4, 2, p, p, p, C.byref(pl), None, None) == INVALID
    assert L.wbc_rollout_tracking_plant_batch(p, 4, 2, p, p, p, C.byref(pl), p, None, None, None) == INVALID


def test_payload_rows_layout():
    import wbc_quadruped_dob_amd as W
    I = np.array([[0.1, 0.01, 0.02], [0.01, 0.2, 0.03], [0.02, 0.03, 0.3]])
    rows = W.payload_rows([1.0, 2.0, 0.0], [[0.1, 0.0, -0.05], [0.0, 0.1, 0.0], [0.0, 0.0, 0.0]], np.stack([I, I, 0 * I]))
    assert rows.shape == (10, 3)
    np.testing.assert_array_equal(rows[:, 0], [1.0, 0.1, 0.0, -0.05, 0.1, 0.2, 0.3, 0.01, 0.02, 0.03])
    assert not rows[:, 2].any()
    m, c, I2 = payload_ref.unpack(rows[:, 1])
    assert m == 2.0 and np.array_equal(I2, I)


def _compile_rollout_asm(out, extra=(), units=("k_rollout",)):
    """device assembly of the rollout units (plain, tracking) x scalar type with the flags of tools/spill_lint.compile_asm, concatenated"""
    csrc = os.path.join(ROOT, "wbc_quadruped_dob_amd", "csrc")
    jobs = []
    for unit, defs in [(u, ()) for u in units] + [("k_rollout", ("-DWBC_ROLLOUT_TRACK=1",))]:
        for scalar in ("double", "float"):
            part = "%s.%s%d.%s.s" % (out, unit, len(defs), scalar)
            cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-DWBC_SCALAR=" + scalar, *defs, *extra, "-S",
                   "--cuda-device-only", "-w", "-o", part, unit + ".hip"]
            jobs.append((part, subprocess.Popen(cmd, cwd=csrc)))
    with open(out, "w") as f:
        for part, proc in jobs:
            assert proc.wait() == 0, part
            f.write(open(part).read())
            os.remove(part)
    return out


@pytest.fixture(scope="module")
def payload_isa(tmp_path_factory):
    """the gfx950 assembly of the PAYLOAD kernels (plain, tracking; their unit also holds integrate_kernel<T, true>) and of their siblings"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_lint
    d = tmp_path_factory.mktemp("payload_asm")
    base = _compile_rollout_asm(str(d / "base.s"), units=("k_rollout", "k_misc"))   # (k_misc: integrate_kernel<T>)
    pl = _compile_rollout_asm(str(d / "payload.s"), extra=("-DWBC_ROLLOUT_PAYLOAD=1",))
    return spill_lint, base, pl


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def test_payload_kernels_keep_their_siblings_budget(payload_isa):
    """Every PAYLOAD instantiation of rollout_kernel: the LDS and the waves per SIMD of its non-payload sibling; no scratch traffic in the
    4-state rollout workgroups (the form every rollout of up to 1 024 states runs).  The 16-state workgroups (two wavefronts per SIMD, 256
    registers) spill in several siblings already; there the payload may add at most 8 scratch instructions (measured: +4 / +5 in the fp64
    observer-off plain kernels, +6 in the tracking ones, none elsewhere).  integrate_kernel<T, true>: no scratch; fp64 keeps its one
    wavefront per SIMD (256 + 70 -> 256 + 105 registers), fp32 grows from 160 to 195 registers -- two wavefronts per SIMD instead of three;
    held to three (amdgpu_waves_per_eu) it spills 53 scratch instructions, so the drop is kept and stated in DESIGN.md 4.7."""
    spill_lint, base, pl = payload_isa
    rb, rp = spill_lint.resources(base), spill_lint.resources(pl)
    dem = _demangle(list(rb) + list(rp))
    sib = {dem[k].split("(")[0]: v for k, v in rb.items()}
    waves = lambda r: 512 // max(1, ((r["vgpr"] + 7) // 8 * 8 + r["agpr"]))
    seen = 0
    for k, v in rp.items():
        d = dem[k].split("(")[0]
        if not (d.startswith("void wbc::rollout_kernel<") or d.startswith("void wbc::integrate_kernel<")) or not d.endswith(", true>"):
            continue
        seen += 1
        stem = d[:-len(", true>")]
        s = sib.get(stem + ", false>") or sib[stem + ">"]   # (the defaulted PAYLOAD argument is spelt out, or not)
        assert v["lds"] == s["lds"], (d, v, s)
        if "integrate_kernel" in d:
            assert waves(v) >= (waves(s) if "double" in d else 2), (d, v, s)
        else:
            assert waves(v) >= waves(s), (d, v, s)
        if "integrate_kernel" in d or ", 4, " in d:
            assert v["scratch_insts"] == 0, (d, v)
        else:
            assert v["scratch_insts"] <= s["scratch_insts"] + 8, (d, v, s)
    assert seen == 2 * (16 + 1), seen   # rollout: 2 scalar types x observer x SPW x warm x (plain, tracking) = 32; integrate: 2
    assert spill_lint.lint(pl) == []
