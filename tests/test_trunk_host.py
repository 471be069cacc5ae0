"""The trunk reference from the velocity command without a GPU: the exported symbols, the struct layout as a C compiler sees the header, the defaults,
parameter validation in both directions for every field, and the calls' argument checks as far as they go before the device is touched."""
import ctypes as C
import os
import subprocess

import pytest

from tests import trunk_ref as TK

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("wbc_trunk_params_default", "wbc_solver_set_trunk_params", "wbc_reference_cmd_batch", "wbc_reference_cmd_swing_batch",
           "wbc_compute_reference_cmd")
OK, INVALID, CAPACITY = 0, 1, 7


def test_abi_exports_the_trunk_calls(hip_lib):
    for name in SYMBOLS:
        assert hasattr(hip_lib, name), name
    assert hip_lib.wbc_abi_version() == 10   # additive: the feature is detected by the symbols
    import wbc_quadruped_dob_amd as W
    assert W._trunk_lib() is W.lib()
    assert (W.TRUNK_WORDS, W.TRUNKREF_WORDS) == (TK.TRUNK_WORDS, TK.TRUNKREF_WORDS) == (6, 10)


def test_trunk_struct_layout_matches_the_header(hip_lib, tmp_path):
    import wbc_quadruped_dob_amd as W
    names = [n for n, _ in W.TrunkParams._fields_]
    args = ["sizeof(wbc_trunk_params)"] + ["offsetof(wbc_trunk_params, %s)" % n for n in names] + ["(size_t)WBC_TRUNK_WORDS", "(size_t)WBC_TRUNKREF_WORDS"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "wbc_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (
        " ".join(["%zu"] * len(args)), ", ".join(args))
    c_path, exe = tmp_path / "trunk.c", tmp_path / "trunk"
    c_path.write_text(src)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c_path), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.TrunkParams)] + [getattr(W.TrunkParams, n).offset for n in names] + [6, 10]


def test_trunk_params_default_values(hip_lib):
    import wbc_quadruped_dob_amd as W
    p = W.TrunkParams.default()
    assert p.struct_size == C.sizeof(W.TrunkParams)
    assert p.as_dict() == TK.DEFAULT_PARAMS == dict(height=0.4, leash=0.05, yaw_leash=0.5, a_s=2.0 ** -5, tilt=1.0, nz_min=0.5, det_min=1e-6)
    q = W.TrunkParams.from_dict(dict(a_s=0.5, leash=float("inf")))
    assert q.as_dict() == dict(TK.DEFAULT_PARAMS, a_s=0.5, leash=float("inf"))
    with pytest.raises(KeyError):
        W.TrunkParams.from_dict(dict(nope=1))


def _set(L, solver, **kw):
    import wbc_quadruped_dob_amd as W
    p = W.TrunkParams.default()
    for k, val in kw.items():
        setattr(p, k, val)
    return L.wbc_solver_set_trunk_params(solver, C.byref(p)), p


def test_trunk_params_validation_in_both_directions(hip_lib):
    """Every refusal comes from the check it names, before the solver is touched (a fake handle); every boundary value that is allowed is accepted and
    stored (a zeroed block stands in for the solver: the setter does nothing but store)."""
    import math
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    fake = C.c_void_p(16)
    nan, inf = float("nan"), float("inf")
    p = W.TrunkParams.default()
    p.struct_size -= 8
    assert L.wbc_solver_set_trunk_params(fake, C.byref(p)) == INVALID and b"struct_size" in L.wbc_last_error()
    assert L.wbc_solver_set_trunk_params(None, C.byref(p)) == INVALID and L.wbc_solver_set_trunk_params(fake, None) == INVALID
    bad = [("height", (nan, inf, -inf)), ("leash", (0.0, -0.05, nan, -inf)), ("yaw_leash", (0.0, -0.5, math.pi + 1e-9, nan, inf)),
           ("a_s", (-1e-12, 1.0 + 1e-12, nan, inf)), ("tilt", (-1e-12, 1.0 + 1e-12, nan, inf)), ("nz_min", (0.0, -0.5, 1.0 + 1e-12, nan, inf)),
           ("det_min", (0.0, -1e-6, nan, inf))]
    for word, values in bad:
        for val in values:
            rc, _ = _set(L, fake, **{word: val})
            assert rc == INVALID and word.encode() in L.wbc_last_error(), (word, val, L.wbc_last_error())
    block = C.create_string_buffer(1 << 20)
    good = [dict(), dict(height=0.0), dict(height=-0.3), dict(leash=inf), dict(leash=1e-300), dict(yaw_leash=math.pi), dict(yaw_leash=1e-300),
            dict(a_s=0.0), dict(a_s=1.0), dict(tilt=0.0), dict(tilt=1.0), dict(nz_min=1.0), dict(nz_min=1e-300), dict(det_min=1e-300),
            dict(det_min=1e300)]
    for kw in good:
        rc, p = _set(L, C.cast(block, C.c_void_p), **kw)
        assert rc == OK, (kw, L.wbc_last_error())
        assert bytes(p) in block.raw, kw          # stored as given


def test_trunk_params_bounds_hold_in_the_solvers_scalar_type(hip_lib):
    """The kernels hold the values in the solver's scalar type.  A zeroed block whose first word (wbc_solver's dtype) is WBC_F32 stands in for an fp32
    solver: a leash, nz_min or det_min that rounds to 0 in float32 and a det_min or height that overflows there are refused; the same values are
    stored on the fp64 stand-in; values float32 holds are accepted on both."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    b32, b64 = C.create_string_buffer(1 << 20), C.create_string_buffer(1 << 20)
    C.cast(b32, C.POINTER(C.c_int))[0] = 1                       # WBC_F32
    s32, s64 = C.cast(b32, C.c_void_p), C.cast(b64, C.c_void_p)
    for word, val in (("leash", 1e-300), ("nz_min", 1e-300), ("nz_min", 1e-46), ("det_min", 1e-300), ("det_min", 1e300), ("height", 1e300),
                      ("height", -1e39)):
        rc, _ = _set(L, s32, **{word: val})
        assert rc == INVALID and word.encode() in L.wbc_last_error() and b"scalar type" in L.wbc_last_error(), (word, val, L.wbc_last_error())
        rc, p = _set(L, s64, **{word: val})
        assert rc == OK and bytes(p) in b64.raw, (word, val)
    for kw in (dict(), dict(leash=float("inf")), dict(leash=1e-30), dict(nz_min=1e-30), dict(det_min=1e-30), dict(det_min=1e30), dict(height=-1e30)):
        rc, p = _set(L, s32, **kw)
        assert rc == OK and bytes(p) in b32.raw, (kw, L.wbc_last_error())


def test_calls_check_their_arguments_before_the_device(hip_lib):
    """No solver; N == 0 returns OK without looking at anything; each required pointer in turn; the optional ones NULL; N beyond max_batch (a zeroed
    block stands in for a solver of max_batch 0: the capacity check comes before the device is touched)."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    buf = C.create_string_buffer(1 << 12)
    x = C.cast(buf, C.c_void_p)
    block = C.create_string_buffer(1 << 20)
    zero = C.cast(block, C.c_void_p)
    # q v cmd normals height | reset | trunk w_des vdot_des | com ref
    ref_full = [x] * 5 + [None] + [x] * 3 + [None, None]
    ref_required = (0, 1, 2, 3, 4, 6, 7, 8)
    # q v cmd normals height | reset | trunk mask swing w_des vdot_des | com ref foot
    fused_full = [x] * 5 + [None] + [x] * 5 + [None, None, None]
    fused_required = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)
    assert L.wbc_reference_cmd_batch(None, 1, *ref_full, None) == INVALID
    assert L.wbc_reference_cmd_swing_batch(None, 1, *fused_full, None) == INVALID
    assert L.wbc_reference_cmd_batch(zero, 0, *([None] * 11), None) == OK
    assert L.wbc_reference_cmd_swing_batch(zero, 0, *([None] * 14), None) == OK
    for i in ref_required:
        a = list(ref_full); a[i] = None
        assert L.wbc_reference_cmd_batch(zero, 1, *a, None) == INVALID, i
    for i in fused_required:
        a = list(fused_full); a[i] = None
        assert L.wbc_reference_cmd_swing_batch(zero, 1, *a, None) == INVALID, i
    assert L.wbc_reference_cmd_batch(zero, 1, *ref_full, None) == CAPACITY
    assert L.wbc_reference_cmd_swing_batch(zero, 1, *fused_full, None) == CAPACITY
    a = list(ref_full); a[5] = a[9] = a[10] = x
    assert L.wbc_reference_cmd_batch(zero, 1, *a, None) == CAPACITY            # with reset, com and ref
    a = list(fused_full); a[5] = a[11] = a[12] = a[13] = x
    assert L.wbc_reference_cmd_swing_batch(zero, 1, *a, None) == CAPACITY
    one = [x, x, x, x, x, 0, x, x, x, None, None]       # q v cmd normals height reset trunk w_des vdot_des com ref
    for i in (0, 1, 2, 3, 4, 6, 7, 8):
        a = list(one); a[i] = None
        assert L.wbc_compute_reference_cmd(zero, *a) == INVALID, i
    assert L.wbc_compute_reference_cmd(None, *one) == INVALID


def test_header_compiles_from_c(tmp_path):
    c = tmp_path / "trunk_c.c"
    c.write_text('#include "wbc_hip.h"\nint f(wbc_solver* s, wbc_trunk_params* p, int* w) { wbc_trunk_params_default(p); '
                 'if (wbc_solver_set_trunk_params(s, p)) return 1; return wbc_reference_cmd_batch(s, 0, 0, 0, 0, 0, 0, w, 0, 0, 0, 0, 0, 0) + '
                 'wbc_reference_cmd_swing_batch(s, 0, 0, 0, 0, 0, 0, w, 0, w, 0, 0, 0, 0, 0, 0, 0) + '
                 'wbc_compute_reference_cmd(s, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "trunk_c.o")],
                   check=True, capture_output=True, text=True)
