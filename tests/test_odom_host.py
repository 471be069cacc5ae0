"""The base estimate without a GPU: the exported symbols, the struct layout as a C compiler sees the header, the defaults, parameter validation in
both directions, and the calls' argument checks as far as they go before the device is touched."""
import ctypes as C
import os
import subprocess

import pytest

from tests import odom_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("wbc_odom_params_default", "wbc_solver_set_odom_params", "wbc_base_estimate_batch", "wbc_gait_estimated_odom_batch",
           "wbc_compute_base_estimate")
OK, INVALID, CAPACITY = 0, 1, 7


def test_abi_exports_the_odom_calls(hip_lib):
    for name in SYMBOLS:
        assert hasattr(hip_lib, name), name
    assert hip_lib.wbc_abi_version() == 10   # additive: the feature is detected by the symbols
    import wbc_quadruped_dob_amd as W
    assert W._odom_lib() is W.lib()


def test_odom_struct_layout_matches_the_header(hip_lib, tmp_path):
    import wbc_quadruped_dob_amd as W
    names = [n for n, _ in W.OdomParams._fields_]
    args = ["sizeof(wbc_odom_params)"] + ["offsetof(wbc_odom_params, %s)" % n for n in names]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "wbc_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (
        " ".join(["%zu"] * len(args)), ", ".join(args))
    c_path, exe = tmp_path / "odom.c", tmp_path / "odom"
    c_path.write_text(src)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c_path), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.OdomParams)] + [getattr(W.OdomParams, n).offset for n in names]


def test_odom_params_default_values(hip_lib):
    import wbc_quadruped_dob_amd as W
    p = W.OdomParams.default()
    assert p.struct_size == C.sizeof(W.OdomParams)
    assert p.as_dict() == R.DEFAULT_PARAMS == dict(a_v=2.0 ** -3, a_p=2.0 ** -2)       # dyadic: the blends' products are exact
    q = W.OdomParams.from_dict(dict(a_p=0.5))
    assert q.as_dict() == dict(a_v=0.125, a_p=0.5)
    with pytest.raises(KeyError):
        W.OdomParams.from_dict(dict(nope=1))


def _set(L, solver, **kw):
    import wbc_quadruped_dob_amd as W
    p = W.OdomParams.default()
    for k, val in kw.items():
        setattr(p, k, val)
    return L.wbc_solver_set_odom_params(solver, C.byref(p)), p


def test_odom_params_validation_in_both_directions(hip_lib):
    """Every refusal comes from the check it names, before the solver is touched (a fake handle); every boundary value that is allowed is accepted and
    stored (a zeroed block stands in for the solver: the setter does nothing but store)."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    fake = C.c_void_p(16)
    nan, inf = float("nan"), float("inf")
    p = W.OdomParams.default()
    p.struct_size -= 8
    assert L.wbc_solver_set_odom_params(fake, C.byref(p)) == INVALID and b"struct_size" in L.wbc_last_error()
    assert L.wbc_solver_set_odom_params(None, C.byref(p)) == INVALID and L.wbc_solver_set_odom_params(fake, None) == INVALID
    bad = [("a_v", dict(a_v=0.0)), ("a_v", dict(a_v=-0.125)), ("a_v", dict(a_v=1.0 + 1e-12)), ("a_v", dict(a_v=nan)), ("a_v", dict(a_v=inf)),
           ("a_p", dict(a_p=-1e-12)), ("a_p", dict(a_p=1.0 + 1e-12)), ("a_p", dict(a_p=nan)), ("a_p", dict(a_p=inf)), ("a_p", dict(a_p=-inf))]
    for word, kw in bad:
        rc, _ = _set(L, fake, **kw)
        assert rc == INVALID and word.encode() in L.wbc_last_error(), (kw, L.wbc_last_error())
    block = C.create_string_buffer(1 << 20)
    good = [dict(), dict(a_v=1.0), dict(a_v=1e-300), dict(a_p=0.0), dict(a_p=1.0), dict(a_v=1.0, a_p=1.0)]
    for kw in good:
        rc, p = _set(L, C.cast(block, C.c_void_p), **kw)
        assert rc == OK, (kw, L.wbc_last_error())
        assert bytes(p) in block.raw, kw          # stored as given


def test_calls_check_their_arguments_before_the_device(hip_lib):
    """No solver; N == 0 returns OK without looking at the buffers; each required pointer in turn; normals without height and the reverse; N beyond
    max_batch (a zeroed block stands in for a solver of max_batch 0: the capacity check comes before the device is touched)."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    buf = C.create_string_buffer(1 << 12)
    x = C.cast(buf, C.c_void_p)
    block = C.create_string_buffer(1 << 20)
    zero = C.cast(block, C.c_void_p)
    # q v contact mask normals height base anchor odo q_est v_est
    est_full = [x] * 11
    est_required = (0, 1, 2, 3, 6, 7, 8, 9, 10)
    # q v cmd Jc r f_prev normals contact phase mask swing | events f_est height | base anchor odo q_est v_est
    fused_full = [x] * 11 + [None, None, None] + [x] * 5
    fused_required = tuple(range(11)) + (14, 15, 16, 17, 18)
    assert L.wbc_base_estimate_batch(None, 1, *est_full, None) == INVALID
    assert L.wbc_gait_estimated_odom_batch(None, 1, *fused_full, None) == INVALID
    assert L.wbc_base_estimate_batch(zero, 0, *([None] * 11), None) == OK
    assert L.wbc_gait_estimated_odom_batch(zero, 0, *([None] * 19), None) == OK
    for i in est_required:
        a = list(est_full); a[i] = None
        assert L.wbc_base_estimate_batch(zero, 1, *a, None) == INVALID, i
    for i in (4, 5):                                   # the planes: together or not at all
        a = list(est_full); a[i] = None
        assert L.wbc_base_estimate_batch(zero, 1, *a, None) == INVALID and b"together" in L.wbc_last_error(), i
    for i in fused_required:
        a = list(fused_full); a[i] = None
        assert L.wbc_gait_estimated_odom_batch(zero, 1, *a, None) == INVALID, i
    assert L.wbc_base_estimate_batch(zero, 1, *est_full, None) == CAPACITY
    a = list(est_full); a[4] = a[5] = None
    assert L.wbc_base_estimate_batch(zero, 1, *a, None) == CAPACITY            # no planes: a valid call
    assert L.wbc_gait_estimated_odom_batch(zero, 1, *fused_full, None) == CAPACITY
    a = list(fused_full); a[13] = x
    assert L.wbc_gait_estimated_odom_batch(zero, 1, *a, None) == CAPACITY      # with height
    ow = C.c_int(0)
    one = [x, x, 0, 0, x, x, x, x, C.cast(C.byref(ow), C.c_void_p), x, x]       # q v contact mask normals height base anchor odo q_est v_est
    for i in (0, 1, 6, 7, 8, 9, 10):
        a = list(one); a[i] = None
        assert L.wbc_compute_base_estimate(zero, *a) == INVALID, i
    for i in (4, 5):
        a = list(one); a[i] = None
        assert L.wbc_compute_base_estimate(zero, *a) == INVALID and b"together" in L.wbc_last_error(), i
    assert L.wbc_compute_base_estimate(None, *one) == INVALID


def test_header_compiles_from_c(tmp_path):
    c = tmp_path / "odom_c.c"
    c.write_text('#include "wbc_hip.h"\nint f(wbc_solver* s, wbc_odom_params* p, int* w) { wbc_odom_params_default(p); '
                 'if (wbc_solver_set_odom_params(s, p)) return 1; return wbc_base_estimate_batch(s, 0, 0, 0, w, w, 0, 0, 0, 0, w, 0, 0, 0) + '
                 'wbc_gait_estimated_odom_batch(s, 0, 0, 0, 0, 0, 0, 0, 0, w, 0, w, 0, w, 0, 0, 0, 0, w, 0, 0, 0) + '
                 'wbc_compute_base_estimate(s, 0, 0, 1, 1, 0, 0, 0, 0, w, 0, 0); }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "odom_c.o")],
                   check=True, capture_output=True, text=True)
