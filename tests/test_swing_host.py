"""Swing-foot references without a GPU: the exported symbols, the struct layout as a C compiler sees the header, and the C++ host class."""
import ctypes as C
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("wbc_swing_params_default", "wbc_solver_set_swing_params", "wbc_swing_reference_batch", "wbc_reference_swing_batch",
           "wbc_compute_swing_reference")


def test_abi_exports_the_swing_calls(hip_lib):
    for name in SYMBOLS:
        assert hasattr(hip_lib, name), name
    assert hip_lib.wbc_abi_version() == 10   # additive: the feature is detected by the symbols


def test_swing_struct_layout_matches_the_header(hip_lib, tmp_path):
    import wbc_quadruped_dob_amd as W
    names = [n for n, _ in W.SwingParams._fields_]
    args = ["sizeof(wbc_swing_params)"] + ["offsetof(wbc_swing_params, %s)" % n for n in names] + ["(size_t)WBC_SWING_WORDS", "(size_t)WBC_FOOT_WORDS"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "wbc_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (
        " ".join(["%zu"] * len(args)), ", ".join(args))
    c_path, exe = tmp_path / "swing.c", tmp_path / "swing"
    c_path.write_text(src)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c_path), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.SwingParams)] + [getattr(W.SwingParams, n).offset for n in names] + [W.SWING_WORDS, W.FOOT_WORDS]


def test_host_class_names_the_swing_methods(tmp_path):
    """A translation unit that includes quadruped_wbc.hpp and takes the address of every new member compiles with the host compiler."""
    src = r'''
#include "wbc/quadruped_wbc.hpp"
using W = wbc::QuadrupedWBC;
void (W::*set_gains)(const wbc_swing_params&) = &W::setSwingGains;
void (W::*swing_ref)(const wbc::BaseState&, const wbc::JointState&, const wbc::ContactState&, const std::array<wbc::SwingPlan, 4>&, double,
                     wbc::Command&, double*) = &W::swingReference;
wbc::Command (W::*ref_swing)(const wbc::BaseState&, const wbc::JointState&, const wbc::ContactState&, const wbc::ComPlan&,
                             const std::array<wbc::SwingPlan, 4>&, double, double*, double*) = &W::referenceSwing;
wbc::Command tick(W& w, const wbc::BaseState& b, const wbc::JointState& js, const wbc::ContactState& cs, const wbc::ComPlan& cp) {
  std::array<wbc::SwingPlan, 4> sp{};
  sp[1] = wbc::SwingPlan{{0.3, -0.2, 0.0}, {0.36, -0.2, 0.0}, 0.05, 0.16, 0.0};
  wbc_swing_params g;
  wbc_swing_params_default(&g);
  w.setSwingGains(g);
  double foot[WBC_FOOT_WORDS];
  wbc::Command c = w.referenceSwing(b, js, cs, cp, sp, 0.01, nullptr, foot);
  w.swingReference(b, js, cs, sp, 0.011, c);
  return c;
}
'''
    cpp = tmp_path / "swing_host.cpp"
    cpp.write_text(src)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "swing_host.o")],
                   check=True, capture_output=True, text=True)
