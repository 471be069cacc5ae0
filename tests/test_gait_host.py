"""Gait scheduler without a GPU: the exported symbols, the struct layout as a C compiler sees the header, parameter validation in both directions,
wbc_gait_params_default against the models' hip origins, and the C++ host class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gait_ref as GR, limit_models

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("wbc_gait_params_default", "wbc_solver_set_gait_params", "wbc_gait_batch", "wbc_compute_gait")
INVALID = 1


def test_abi_exports_the_gait_calls(hip_lib):
    for name in SYMBOLS:
        assert hasattr(hip_lib, name), name
    assert hip_lib.wbc_abi_version() == 10   # additive: the feature is detected by the symbols


def test_gait_struct_layout_matches_the_header(hip_lib, tmp_path):
    import wbc_quadruped_dob_amd as W
    names = [n for n, _ in W.GaitParams._fields_]
    args = ["sizeof(wbc_gait_params)"] + ["offsetof(wbc_gait_params, %s)" % n for n in names] + ["(size_t)WBC_GAIT_CMD_WORDS"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "wbc_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (
        " ".join(["%zu"] * len(args)), ", ".join(args))
    c_path, exe = tmp_path / "gait.c", tmp_path / "gait"
    c_path.write_text(src)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c_path), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.GaitParams)] + [getattr(W.GaitParams, n).offset for n in names] + [W.GAIT_CMD_WORDS]
    assert W.GAIT_CMD_WORDS == 4


def test_gait_params_default_values(hip_lib):
    import wbc_quadruped_dob_amd as W
    p = W.GaitParams.default()   # no model: zeros for base_xy
    assert p.struct_size == C.sizeof(W.GaitParams)
    assert p.period == 0.4 and list(p.duty) == [0.6] * 4 and list(p.offset) == [0.0, 0.5, 0.5, 0.0]
    assert p.clearance == 0.05 and p.k_v == 0.03 and p.late == 0.5 and p.retarget == 1
    assert all(r[0] == 0.0 and r[1] == 0.0 for r in p.base_xy)
    d = p.as_dict()
    assert {k: d[k] for k in GR.DEFAULT_PARAMS} == GR.DEFAULT_PARAMS
    p = W.GaitParams.from_dict(dict(duty=0.5, offset=[0.0, 0.25, 0.5, 0.75], retarget=0, base_xy=[[1, 2], [3, 4], [5, 6], [7, 8]]))
    assert list(p.duty) == [0.5] * 4 and list(p.offset) == [0.0, 0.25, 0.5, 0.75] and p.retarget == 0 and p.period == 0.4
    assert [tuple(r) for r in p.base_xy] == [(1, 2), (3, 4), (5, 6), (7, 8)]
    with pytest.raises(KeyError):
        W.GaitParams.from_dict(dict(nope=1))


def test_gait_params_default_takes_the_hip_origins_of_the_model(gpu_model, flat_model, tmp_path):
    """base_xy[k] = x, y of the first joint's origin of foot k's leg, caller's foot order: the synthetic model, and the two descriptions whose foot
    and joint order is not leg-major (the Gazebo-like model among them), against the independent URDF parser."""
    want = GR.base_xy(flat_model)
    assert np.abs(want).min() > 0.05 and len({tuple(np.sign(r)) for r in want}) == 4    # four distinct quadrants: an order mix-up would show
    got = np.array(gpu_model.gait_params_default().as_dict()["base_xy"])
    assert np.array_equal(got, want)
    for name, spec in limit_models.specs(tmp_path).items():
        want = GR.base_xy(spec.flat)
        got = np.array(spec.model.gait_params_default().as_dict()["base_xy"])
        assert len({tuple(np.sign(r)) for r in want}) == 4, name
        assert np.allclose(got, want, rtol=0, atol=1e-15), (name, got, want)


def _set(L, solver, **kw):
    import wbc_quadruped_dob_amd as W
    p = W.GaitParams.default()
    for k, val in kw.items():
        if isinstance(val, tuple):       # (index, value) of an array field
            f = getattr(p, k)
            if k == "base_xy":
                f[val[0]][val[1]] = val[2]
            else:
                f[val[0]] = val[1]
        else:
            setattr(p, k, val)
    return L.wbc_solver_set_gait_params(solver, C.byref(p)), p


def test_gait_params_validation_in_both_directions(hip_lib):
    """Every refusal comes from the range check it names, before the solver is touched (a fake handle); every boundary value that is allowed is
    accepted and stored (a zeroed block stands in for the solver: the setter does nothing but store)."""
    import wbc_quadruped_dob_amd as W
    L = W.lib()
    L.wbc_last_error.restype = C.c_char_p
    fake = C.c_void_p(16)
    nan, inf = float("nan"), float("inf")
    p = W.GaitParams.default()
    p.struct_size -= 8
    assert L.wbc_solver_set_gait_params(fake, C.byref(p)) == INVALID and b"struct_size" in L.wbc_last_error()
    assert L.wbc_solver_set_gait_params(None, C.byref(p)) == INVALID and L.wbc_solver_set_gait_params(fake, None) == INVALID
    bad = [("period", dict(period=0.0)), ("period", dict(period=-0.4)), ("period", dict(period=nan)), ("period", dict(period=inf)),
           ("duty", dict(duty=(2, 0.0))), ("duty", dict(duty=(0, -0.1))), ("duty", dict(duty=(3, 1.0 + 1e-12))), ("duty", dict(duty=(1, nan))),
           ("offset", dict(offset=(0, -1e-12))), ("offset", dict(offset=(3, 1.0))), ("offset", dict(offset=(2, nan))), ("offset", dict(offset=(1, inf))),
           ("clearance", dict(clearance=-1e-9)), ("clearance", dict(clearance=nan)), ("clearance", dict(clearance=inf)),
           ("k_v", dict(k_v=nan)), ("k_v", dict(k_v=inf)), ("k_v", dict(k_v=-inf)),
           ("late", dict(late=0.0)), ("late", dict(late=-0.5)), ("late", dict(late=1.0 + 1e-12)), ("late", dict(late=nan)),
           ("retarget", dict(retarget=2)), ("retarget", dict(retarget=-1)),
           ("base_xy", dict(base_xy=(2, 1, nan))), ("base_xy", dict(base_xy=(0, 0, inf)))]
    for word, kw in bad:
        rc, _ = _set(L, fake, **kw)
        assert rc == INVALID and word.encode() in L.wbc_last_error(), (kw, L.wbc_last_error())
    block = C.create_string_buffer(1 << 20)
    good = [dict(), dict(period=1e-3), dict(duty=(0, 1.0)), dict(duty=(1, 1e-6)), dict(offset=(2, 0.0)), dict(offset=(3, 1.0 - 1e-12)), dict(clearance=0.0),
            dict(k_v=-0.1), dict(k_v=0.0), dict(late=1.0), dict(late=1e-6), dict(retarget=0), dict(base_xy=(1, 0, -3.0))]
    for kw in good:
        rc, p = _set(L, C.cast(block, C.c_void_p), **kw)
        assert rc == 0, (kw, L.wbc_last_error())
        assert bytes(p) in block.raw, kw          # stored as given


def test_host_class_names_the_gait_methods(tmp_path):
    """A translation unit that includes quadruped_wbc.hpp and takes the address of every new member compiles with the host compiler."""
    src = r'''
#include "wbc/quadruped_wbc.hpp"
using W = wbc::QuadrupedWBC;
wbc_gait_params (W::*dflt)() const = &W::gaitParamsDefault;
void (W::*set_gait)(const wbc_gait_params&) = &W::setGaitParams;
void (W::*gait)(const wbc::BaseState&, const wbc::JointState&, const wbc::GaitCommand&, wbc::GaitState&, const bool*) = &W::gait;
wbc::Command tick(W& w, const wbc::BaseState& b, const wbc::JointState& js, wbc::ContactState& cs, const wbc::ComPlan& cp, wbc::GaitState& st) {
  wbc_gait_params g = w.gaitParamsDefault();
  g.period = 0.5; g.duty[2] = 1.0; g.base_xy[3][1] = -0.1;
  w.setGaitParams(g);
  const wbc::GaitCommand gc{0.2, 0.0, 0.1, -0.05};
  const bool sensed[4] = {true, false, false, true};
  w.gait(b, js, gc, st, sensed);
  w.gait(b, js, gc, st);
  for (int f = 0; f < 4; ++f) cs.stance[f] = st.stance[f];
  double cmd[WBC_GAIT_CMD_WORDS] = {gc.vx, gc.vy, gc.wz, gc.ground_z};
  (void)cmd;
  return w.referenceSwing(b, js, cs, cp, st.swing, 0.0);
}
'''
    cpp = tmp_path / "gait_host.cpp"
    cpp.write_text(src)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "gait_host.o")],
                   check=True, capture_output=True, text=True)
    # and the C header alone, from C
    c = tmp_path / "gait_c.c"
    c.write_text('#include "wbc_hip.h"\nint f(wbc_solver* s, wbc_gait_params* p) { wbc_gait_params_default(0, p); return wbc_solver_set_gait_params(s, p); }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "gait_c.o")],
                   check=True, capture_output=True, text=True)
