"""Foothold selection without a GPU: the exported symbols, wbc_foothold_params' layout as a C compiler sees the header, the documented defaults, the
setter's validation, and the four calls' argument checks in their order, as far as they go before the device is touched."""
import ctypes as C
import os
import subprocess

from tests import foothold_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("wbc_foothold_params_default", "wbc_solver_set_foothold_params", "wbc_terrain_cost_batch", "wbc_foothold_select_batch",
           "wbc_gait_terrain_select_batch", "wbc_gait_estimated_terrain_select_batch")
OK, INVALID, CAPACITY = 0, 1, 7


def test_abi_exports_the_foothold_calls(hip_lib):
    for name in SYMBOLS:
        assert hasattr(hip_lib, name), name
    assert hip_lib.wbc_abi_version() == 10   # additive: the feature is detected by the symbols
    import wbc_quadruped_dob_amd as W
    assert W._foothold_lib() is W.lib()
    for name in ("FootholdParams", "Solver"):
        assert hasattr(W, name)
    for name in ("set_foothold_params", "terrain_cost", "foothold_select", "gait_terrain_select", "gait_estimated_terrain_select"):
        assert hasattr(W.Solver, name), name


def test_params_struct_layout_matches_the_header(hip_lib, tmp_path):
    import wbc_quadruped_dob_amd as W
    names = [n for n, _ in W.FootholdParams._fields_]
    args = ["sizeof(wbc_foothold_params)"] + ["offsetof(wbc_foothold_params, %s)" % n for n in names]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "wbc_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (
        " ".join(["%zu"] * len(args)), ", ".join(args))
    c_path, exe = tmp_path / "foothold.c", tmp_path / "foothold"
    c_path.write_text(src)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c_path), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.FootholdParams)] + [getattr(W.FootholdParams, n).offset for n in names]


def test_defaults_are_the_documented_ones(hip_lib):
    import wbc_quadruped_dob_amd as W
    p = W.FootholdParams.default()
    assert p.struct_size == C.sizeof(W.FootholdParams)
    assert p.as_dict() == dict(radius=3, margin=1, w_step=1.0, w_slope=2.0 ** -7, w_dist=4.0, cost_ok=0.00875, u_max=0.75)
    assert p.as_dict() == R.DEFAULTS                      # the numpy restatement walks with the library's values
    header = open(os.path.join(ROOT, "include", "wbc_hip.h")).read()
    assert "radius = 3, margin = 1, w_step = 1, w_slope = 2^-7, w_dist = 4 (1/m), cost_ok = 8.75e-3, u_max = 0.75" in header
    q = W.FootholdParams.from_dict(dict(radius=2, cost_ok=0.5))
    assert (q.radius, q.cost_ok, q.margin, q.w_dist) == (2, 0.5, 1, 4.0)
    W.lib().wbc_foothold_params_default(None)             # a null pointer is ignored


def _solver_block():
    block = C.create_string_buffer(1 << 20)               # a zeroed block standing in for a solver of max_batch 0
    return block, C.cast(block, C.c_void_p)


def test_setter_validates_every_field(hip_lib):
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    block, zero = _solver_block()
    nan, inf = float("nan"), float("inf")
    good = W.FootholdParams.default()
    assert L.wbc_solver_set_foothold_params(zero, C.byref(good)) == OK
    assert L.wbc_solver_set_foothold_params(None, C.byref(good)) == INVALID and L.wbc_solver_set_foothold_params(zero, None) == INVALID
    bad = [("struct_size", dict(struct_size=C.sizeof(W.FootholdParams) - 8)), ("struct_size", dict(struct_size=0)),
           ("radius", dict(radius=-1)), ("radius", dict(radius=5)), ("margin", dict(margin=-1)), ("margin", dict(margin=3)),
           ("u_max", dict(u_max=1.0000001)), ("finite", dict(u_max=-0.1)), ("finite", dict(u_max=nan))]
    bad += [("finite", {k: val}) for k in ("w_step", "w_slope", "w_dist", "cost_ok") for val in (-1.0, nan, inf, -inf)]
    for word, kw in bad:
        p = W.FootholdParams.default()
        for k, val in kw.items():
            setattr(p, k, val)
        assert L.wbc_solver_set_foothold_params(zero, C.byref(p)) == INVALID and word.encode() in L.wbc_last_error(), (kw, L.wbc_last_error())
    for kw in (dict(radius=0), dict(radius=4), dict(margin=0), dict(margin=2), dict(u_max=0.0), dict(u_max=1.0), dict(w_step=0.0, w_slope=0.0, w_dist=0.0, cost_ok=0.0)):
        p = W.FootholdParams.default()
        for k, val in kw.items():
            setattr(p, k, val)
        assert L.wbc_solver_set_foothold_params(zero, C.byref(p)) == OK, kw


def _terrain_struct(**kw):
    import wbc_quadruped_dob_amd as W
    t = W.TerrainStruct(C.sizeof(W.TerrainStruct), 64, 48, 4, -0.5, -0.375, 2.0 ** -6, 4096, None)    # z: a fake device address, never followed
    for k, val in kw.items():
        setattr(t, k, val)
    return t


# the argument lists, every required pointer given: (name, arguments behind the solver, indices of the required pointers)
def _lists(tp, x, n):
    sel = [tp, x, n, x, x, x, x]                                  # terrain cost N mask swing hold latch
    gait = [n, x, x, x, None, x, x, x, None, tp, x, x, None, x, x, x]   # N q v cmd contact phase mask swing events terrain normals height surf cost hold latch
    est = [n] + [x] * 11 + [None, None, tp, x, None, x, x, x]     # N q v cmd Jc r f_prev normals contact phase mask swing events f_est terrain height surf cost hold latch
    return (("wbc_foothold_select_batch", sel, (0, 1, 3, 4, 5, 6)),
            ("wbc_gait_terrain_select_batch", gait, (1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15)),
            ("wbc_gait_estimated_terrain_select_batch", est, tuple(range(1, 12)) + (14, 15, 17, 18, 19)))


def test_calls_check_their_arguments_before_the_device(hip_lib):
    """No solver; N == 0 returns OK without looking at anything (a bad struct included); each required pointer in turn -- cost, hold and latch among
    them --; then the terrain struct's own checks; then N beyond max_batch."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    buf = C.create_string_buffer(1 << 12)
    x = C.cast(buf, C.c_void_p)
    block, zero = _solver_block()
    t, broken = _terrain_struct(), _terrain_struct(nx=1)
    for name, args, required in _lists(C.byref(t), x, 1):
        call = getattr(L, name)
        assert call(None, *args, None) == INVALID, name
        assert call(zero, *args, None) == CAPACITY, name                      # a good call gets as far as the capacity check
        for i in required:
            a = list(args); a[i] = None
            assert call(zero, *a, None) == INVALID and b"null" in L.wbc_last_error(), (name, i)
        bad = [C.byref(broken) if isinstance(v, type(C.byref(t))) else v for v in args]
        assert call(zero, *bad, None) == INVALID and b"nx and ny" in L.wbc_last_error(), name      # the struct's checks come before the capacity check
        for i in required:                                                   # a NULL pointer is reported before a bad struct
            a = list(bad); a[i] = None
            assert call(zero, *a, None) == INVALID and b"null" in L.wbc_last_error(), (name, i)
    for name, args, required in _lists(C.byref(broken), None, 0):             # N == 0: nothing is looked at
        a = [None if i in required else v for i, v in enumerate(args)]
        assert getattr(L, name)(zero, *a, None) == OK, name
    # the cost map has no N: solver, terrain, cost, then the struct
    assert L.wbc_terrain_cost_batch(None, C.byref(t), x, None) == INVALID
    assert L.wbc_terrain_cost_batch(zero, None, x, None) == INVALID and L.wbc_terrain_cost_batch(zero, C.byref(t), None, None) == INVALID
    for kw in (dict(nx=1), dict(n_tiles=0), dict(cell=0.0), dict(z=None), dict(struct_size=8)):
        assert L.wbc_terrain_cost_batch(zero, C.byref(_terrain_struct(**kw)), x, None) == INVALID, kw


def test_header_compiles_from_c(tmp_path):
    c = tmp_path / "foothold_c.c"
    c.write_text('#include "wbc_hip.h"\nint f(wbc_solver* s, int* w) { wbc_terrain t = {sizeof(wbc_terrain), 2, 2, 1, 0.0, 0.0, 1.0, 0, 0}; '
                 'wbc_foothold_params p; wbc_foothold_params_default(&p); '
                 'return wbc_solver_set_foothold_params(s, &p) + wbc_terrain_cost_batch(s, &t, 0, 0) + '
                 'wbc_foothold_select_batch(s, &t, 0, 0, w, 0, 0, w, 0) + '
                 'wbc_gait_terrain_select_batch(s, 0, 0, 0, 0, w, 0, w, 0, w, &t, 0, 0, 0, 0, 0, w, 0) + '
                 'wbc_gait_estimated_terrain_select_batch(s, 0, 0, 0, 0, 0, 0, 0, 0, w, 0, w, 0, w, 0, &t, 0, 0, 0, 0, w, 0); }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "foothold_c.o")],
                   check=True, capture_output=True, text=True)
