"""Terrain heightfield without a GPU: the exported symbols, wbc_terrain's layout as a C compiler sees the header, the struct's checks, and the four batch
calls' argument checks in their order, as far as they go before the device is touched."""
import ctypes as C
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("wbc_terrain_sample_batch", "wbc_terrain_feet_batch", "wbc_gait_terrain_batch", "wbc_gait_estimated_terrain_batch")
OK, INVALID, CAPACITY = 0, 1, 7


def test_abi_exports_the_terrain_calls(hip_lib):
    for name in SYMBOLS:
        assert hasattr(hip_lib, name), name
    assert hip_lib.wbc_abi_version() == 10   # additive: the feature is detected by the symbols
    import wbc_quadruped_dob_amd as W
    assert W._terrain_lib() is W.lib()


def test_terrain_struct_layout_matches_the_header(hip_lib, tmp_path):
    import wbc_quadruped_dob_amd as W
    names = [n for n, _ in W.TerrainStruct._fields_]
    args = ["sizeof(wbc_terrain)"] + ["offsetof(wbc_terrain, %s)" % n for n in names]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "wbc_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (
        " ".join(["%zu"] * len(args)), ", ".join(args))
    c_path, exe = tmp_path / "terrain.c", tmp_path / "terrain"
    c_path.write_text(src)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c_path), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.TerrainStruct)] + [getattr(W.TerrainStruct, n).offset for n in names]


def _struct(**kw):
    import wbc_quadruped_dob_amd as W
    t = W.TerrainStruct(C.sizeof(W.TerrainStruct), 64, 48, 4, -0.5, -0.375, 2.0 ** -6, 4096, None)    # z: a fake device address, never followed
    for k, val in kw.items():
        setattr(t, k, val)
    return t


def _calls(L, solver, t, x, n=1):
    """the four calls with every required pointer given, on N = n"""
    tp = C.byref(t) if t is not None else None
    return dict(sample=lambda: L.wbc_terrain_sample_batch(solver, tp, n, x, None, None, None, None),
                feet=lambda: L.wbc_terrain_feet_batch(solver, tp, n, x, None, None, x, x, None, None),
                gait=lambda: L.wbc_gait_terrain_batch(solver, n, x, x, x, None, x, x, x, None, tp, x, x, None, None),
                estimated=lambda: L.wbc_gait_estimated_terrain_batch(solver, n, *([x] * 11), None, None, tp, x, None, None))


def test_every_invalid_field_is_refused_with_a_message(hip_lib):
    """On a zeroed block standing in for a solver of max_batch 0: the struct's checks come before the capacity check, and a good struct gets as far
    as that check in all four calls."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    buf = C.create_string_buffer(1 << 12)
    x = C.cast(buf, C.c_void_p)
    block = C.create_string_buffer(1 << 20)
    zero = C.cast(block, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", dict(struct_size=C.sizeof(W.TerrainStruct) - 8)), ("struct_size", dict(struct_size=C.sizeof(W.TerrainStruct) + 8)),
           ("struct_size", dict(struct_size=0)),
           ("nx and ny", dict(nx=1)), ("nx and ny", dict(ny=1)), ("nx and ny", dict(nx=0)), ("nx and ny", dict(ny=-3)),
           ("n_tiles", dict(n_tiles=0)), ("n_tiles", dict(n_tiles=-1)),
           ("x0 and y0", dict(x0=nan)), ("x0 and y0", dict(x0=inf)), ("x0 and y0", dict(y0=nan)), ("x0 and y0", dict(y0=-inf)),
           ("cell", dict(cell=0.0)), ("cell", dict(cell=-1.0)), ("cell", dict(cell=nan)), ("cell", dict(cell=inf)),
           ("z is null", dict(z=None)),
           ("2^28", dict(nx=1 << 14, ny=1 << 14, n_tiles=1)), ("2^28", dict(nx=1 << 10, ny=1 << 10, n_tiles=1 << 8)),
           ("2^28", dict(nx=(1 << 31) - 1, ny=(1 << 31) - 1, n_tiles=(1 << 31) - 1))]
    for word, kw in bad:
        for name, call in _calls(L, zero, _struct(**kw), x).items():
            assert call() == INVALID and word.encode() in L.wbc_last_error(), (name, kw, L.wbc_last_error())
    good = [dict(), dict(nx=2, ny=2, n_tiles=1), dict(nx=1 << 14, ny=1 << 13, n_tiles=1), dict(nx=(1 << 14) - 1, ny=1 << 14, n_tiles=1), dict(cell=1e-9),
            dict(x0=-1e30, y0=1e30)]
    for kw in good:
        for name, call in _calls(L, zero, _struct(**kw), x).items():
            assert call() == CAPACITY, (name, kw, L.wbc_last_error())


def test_batch_calls_check_their_arguments_before_the_device(hip_lib):
    """No solver; N == 0 returns OK without looking at anything (a bad struct included); each required pointer in turn; mask and swing both or neither;
    N beyond max_batch (a zeroed block stands in for a solver of max_batch 0)."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    buf = C.create_string_buffer(1 << 12)
    x = C.cast(buf, C.c_void_p)
    block = C.create_string_buffer(1 << 20)
    zero = C.cast(block, C.c_void_p)
    t = _struct()
    tp = C.byref(t)
    for name, call in _calls(L, None, t, x).items():
        assert call() == INVALID, name
    for name, call in _calls(L, zero, _struct(nx=0, z=None), None, n=0).items():
        assert call() == OK, name
    for name, call in _calls(L, zero, None, None, n=0).items():
        assert call() == OK, name
    for name, call in _calls(L, zero, None, x).items():          # no terrain
        assert call() == INVALID, name
    for name, call in _calls(L, zero, t, x).items():
        assert call() == CAPACITY, name
    # each required pointer in turn
    assert L.wbc_terrain_sample_batch(zero, tp, 1, None, x, x, x, None) == INVALID
    feet = [x, None, None, x, x, None]                    # q mask swing normals height | surf
    for i in (0, 3, 4):
        a = list(feet); a[i] = None
        assert L.wbc_terrain_feet_batch(zero, tp, 1, *a, None) == INVALID, i
    assert L.wbc_terrain_feet_batch(zero, tp, 1, x, x, None, x, x, None, None) == INVALID       # mask without swing
    assert L.wbc_terrain_feet_batch(zero, tp, 1, x, None, x, x, x, None, None) == INVALID       # swing without mask
    assert L.wbc_terrain_feet_batch(zero, tp, 1, x, x, x, x, x, x, None) == CAPACITY
    gait = [x, x, x, None, x, x, x, None, tp, x, x, None]   # q v cmd contact phase mask swing events terrain normals height surf
    for i in (0, 1, 2, 4, 5, 6, 8, 9, 10):
        a = list(gait); a[i] = None
        assert L.wbc_gait_terrain_batch(zero, 1, *a, None) == INVALID, i
    est = [x] * 11 + [None, None, tp, x, None]             # q v cmd Jc r f_prev normals contact phase mask swing events f_est terrain height surf
    for i in list(range(11)) + [13, 14]:
        a = list(est); a[i] = None
        assert L.wbc_gait_estimated_terrain_batch(zero, 1, *a, None) == INVALID, i
    assert L.wbc_gait_estimated_terrain_batch(zero, 1, *est, None) == CAPACITY


def test_header_compiles_from_c(tmp_path):
    c = tmp_path / "terrain_c.c"
    c.write_text('#include "wbc_hip.h"\nint f(wbc_solver* s, int* w) { wbc_terrain t = {sizeof(wbc_terrain), 2, 2, 1, 0.0, 0.0, 1.0, 0, 0}; '
                 'return wbc_terrain_sample_batch(s, &t, 0, 0, 0, 0, 0, 0) + wbc_terrain_feet_batch(s, &t, 0, 0, w, 0, 0, 0, 0, 0) + '
                 'wbc_gait_terrain_batch(s, 0, 0, 0, 0, w, 0, w, 0, w, &t, 0, 0, 0, 0) + '
                 'wbc_gait_estimated_terrain_batch(s, 0, 0, 0, 0, 0, 0, 0, 0, w, 0, w, 0, w, 0, &t, 0, 0, 0); }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "terrain_c.o")],
                   check=True, capture_output=True, text=True)
