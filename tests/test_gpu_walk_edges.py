"""GPU: the walking kernels added since the envelope tests -- ground plant, stiction, contact sensing, leg odometry, terrain feet, cost map and the
one-launch gait calls built on them -- on the inputs of tests/walk_edges.py: wide states (joints over +- 7 pi, attitudes over the sphere, bases 50 m
out), unit normals over the whole sphere, mu from 0.05 to 1.5.  tests/test_walk_edges_oracle.py pins the referee on the same inputs on the CPU,
asserts the cases' conditions and measures what float32 costs on them.

Gates.  Integer words (contact, singular, stick, odo): equal; in float32 against the float32 restatement's words, which the builders made equal to
the float64 ones; outside the capped skip sets of the contact and ramp cases.  Words a law does not write: the input's bits.  Everything finite.
fp64: util.gate -- util.elementwise_excess at the project's standing tolerances; q', v' of the plant steps 1e-9 of the largest entry (TIGHT64).
fp32: 8 x the walk_edges.F32_* figure of that output, of the largest entry -- measured on the reference, never on the device.
Fused against unfused: bit for bit, NaN for NaN, on every state (those envelope.heading_ok drops included); the planes of the terrain calls as
tests/test_gpu_terrain.py::_same and tests/test_gpu_foothold.py::_same hold them -- and, found here and now written into include/wbc_hip.h, the
p0 of a foot that lifts off in a fused terrain call to rounding as well (_planes_as_same)."""
import functools

import numpy as np
import pytest

from tests import contact_ref as CR, foothold_ref as FR, ground_ref as GND, limit_models, limit_ref, odom_ref as OD, stick_ref as ST, \
    terrain_ref as TR, walk_dev as WD, walk_edges as WE
from tests.util import elementwise_excess, gate, to_dev, to_host, torch_dtype as _td

pytestmark = pytest.mark.gpu
SIZES = WE.SIZES
MARGIN = 8.0
TIGHT64 = 1e-9
STANDING32 = 5e-4       # the planes of a fused call against terrain_feet's, as the existing _same functions gate them
JUNK = 7.5
_x8 = lambda d: {k: MARGIN * x for k, x in d.items()}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _nd(dtype):
    return np.float64 if dtype == "f64" else np.float32


def _ints(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _junk(torch, shape, dtype):
    return torch.full(shape, JUNK, dtype=_td(torch, dtype), device="cuda")


def _bits_equal(a, b):
    """bit patterns equal (NaN for NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_tensor(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and _bits_equal(x.cpu().numpy(), y.cpu().numpy())


def _plant_gate(got, ref, dtype, what, n, f32_gate):
    """q', v' of a plant step: of the largest entry in both scalar types"""
    e = WE.rel(got, ref)
    tol = TIGHT64 if dtype == "f64" else f32_gate[what]
    print("%s %s n=%d: %.3g of the largest entry (gate %.3g)" % (what, dtype, n, e, tol))
    assert np.all(np.isfinite(got)) and e < tol, (what, e, tol)


# ---- 1. parity: ground plant and stiction
def _plant_dev(torch, c, dtype, stick):
    td = _td(torch, dtype)
    d = {k: to_dev(c[k], torch, td) for k in ("q", "v", "normals", "height", "mu", "tau", "tau_ext") + (("anchor",) if stick else ())}
    d.update({k: to_dev(c["dyn"][k], torch, td) for k in ("M", "h", "Jc")})
    if stick:
        d["stick"] = _ints(torch, c["stick"])
    return d


def _plant_outs(torch, n, dtype):
    return dict(f_gr=_junk(torch, (12, n), dtype), contact=torch.full((n,), -1, dtype=torch.int32, device="cuda"), gap=_junk(torch, (4, n), dtype))


def _ground_parity(torch, solver, c, dtype, n, legs, f32_gate, what=""):
    """ground_force and integrate_ground on a ground_ref-shaped case against its ref64 / ref32"""
    q_ref, v_ref, g = c["ref64"]
    words = c["ref64" if dtype == "f64" else "ref32"][2]
    d = _plant_dev(torch, c, dtype, False)
    o = _plant_outs(torch, n, dtype)
    solver.ground_force(d["q"], d["v"], d["Jc"], d["normals"], d["height"], d["mu"], f_gr=o["f_gr"], contact=o["contact"], gap=o["gap"])
    torch.cuda.synchronize()
    law = dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]))
    o = _plant_outs(torch, n, dtype)
    q, v = d["q"].clone(), d["v"].clone()
    solver.integrate_ground(q, v, d["M"], d["h"], d["Jc"], d["tau"], d["normals"], d["height"], d["mu"], tau_ext=d["tau_ext"], f_gr=o["f_gr"],
                            contact=o["contact"], gap=o["gap"])
    torch.cuda.synchronize()
    one = dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]))
    for got in (law, one):
        assert np.array_equal(got["contact"], words["contact"]), what
        gate(got["f_gr"], g["f_gr"], dtype, "f_gr", n, f32_gate)
        gate(got["gap"], g["gap"], dtype, "gap", n, f32_gate)
    _plant_gate(to_host(q), q_ref, dtype, "q", n, f32_gate)
    _plant_gate(to_host(v), v_ref, dtype, "v", n, f32_gate)
    assert not np.array_equal(to_host(q), c["q"].astype(_nd(dtype)))
    return law


def _stick_parity(torch, solver, c, dtype, n, f32_gate, what=""):
    q_ref, v_ref, g = c["ref64"]
    words = c["ref64" if dtype == "f64" else "ref32"][2]
    d = _plant_dev(torch, c, dtype, True)
    anchor_in = to_host(d["anchor"])
    wr = np.repeat(g["loaded"] & (g["slid"] | ~g["had"]), 3, 1)
    assert wr.any() and (~wr).any()

    def check(got):
        assert np.array_equal(got["stick"], words["stick"]) and np.array_equal(got["contact"], words["contact"]), what
        gate(got["f_gr"], g["f_gr"], dtype, "f_gr", n, f32_gate)
        gate(got["gap"], g["gap"], dtype, "gap", n, f32_gate)
        assert _bits_equal(got["anchor"][~wr], anchor_in[~wr])            # unloaded feet and sticking anchored feet: the input's bits
        gate(got["anchor"][wr], g["anchor"][wr], dtype, "anchor", n, f32_gate)

    o = _plant_outs(torch, n, dtype)
    anchor, stick = d["anchor"].clone(), d["stick"].clone()
    solver.ground_stick_force(d["q"], d["v"], d["Jc"], d["normals"], d["height"], d["mu"], anchor, stick, f_gr=o["f_gr"], contact=o["contact"],
                              gap=o["gap"])
    torch.cuda.synchronize()
    check(dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]), anchor=to_host(anchor), stick=stick.cpu().numpy()))
    o = _plant_outs(torch, n, dtype)
    q, v, anchor, stick = d["q"].clone(), d["v"].clone(), d["anchor"].clone(), d["stick"].clone()
    solver.integrate_ground_stick(q, v, d["M"], d["h"], d["Jc"], d["tau"], d["normals"], d["height"], d["mu"], anchor, stick, tau_ext=d["tau_ext"],
                                  f_gr=o["f_gr"], contact=o["contact"], gap=o["gap"])
    torch.cuda.synchronize()
    check(dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]), anchor=to_host(anchor), stick=stick.cpu().numpy()))
    _plant_gate(to_host(q), q_ref, dtype, "q", n, f32_gate)
    _plant_gate(to_host(v), v_ref, dtype, "v", n, f32_gate)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_ground_force_and_integrate_ground_on_wide_states(torch_cuda, gpu_model, flat_model, dtype, n):
    c = WE.wide_ground_case(flat_model, gpu_model.total_mass, n)
    assert GND.branches_taken(GND.params(), c["ref64"][2]) == GND.ALL_BRANCHES
    solver = WD.solver(gpu_model, dtype, max_batch=n)
    law = _ground_parity(torch_cuda, solver, c, dtype, n, limit_ref.leg_joints(flat_model), _x8(WE.F32_GROUND))
    rest = c["kinds"][:, 0] == -1
    assert rest.any() and np.array_equal(law["f_gr"][rest][:, [0, 1, 3, 4, 6, 7, 9, 10]], np.zeros((rest.sum(), 8)))     # v_t = 0 exactly


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_ground_stick_force_and_integrate_ground_stick_on_wide_states(torch_cuda, gpu_model, flat_model, dtype, n):
    c = WE.wide_stick_case(flat_model, gpu_model.total_mass, n)
    assert ST.branches_taken(c["ref64"][2]) == ST.ALL_BRANCHES
    solver = WD.solver(gpu_model, dtype, max_batch=n)
    _stick_parity(torch_cuda, solver, c, dtype, n, _x8(WE.F32_STICK))


# ---- contact sensing
def _contact_parity(torch, solver, c, dtype, n, f32_gate):
    e = c["e64"]
    keep = ~c["skip"]
    assert c["skip"].mean() <= WE.SKIP_CAP
    td = _td(torch, dtype)
    d = {k: to_dev(c[k], torch, td) for k in ("Jc", "r", "f_prev", "normals")}
    word = _ints(torch, c["contact"])
    o = dict(f_est=_junk(torch, (12, n), dtype), fn_est=_junk(torch, (4, n), dtype), singular=torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    solver.contact_estimate(d["Jc"], d["r"], d["f_prev"], d["normals"], word, **o)
    torch.cuda.synchronize()
    got = dict(contact=word.cpu().numpy(), f_est=to_host(o["f_est"]), fn=to_host(o["fn_est"]), singular=o["singular"].cpu().numpy())
    assert np.array_equal(WE._bits(got["contact"])[keep], WE._bits(e["contact"])[keep])
    assert np.array_equal(WE._bits(got["singular"])[keep], WE._bits(e["singular"])[keep])
    assert np.all(got["contact"] & ~15 == c["contact"] & ~15) and np.all(got["singular"] & ~15 == 0)
    assert np.all(np.isfinite(got["f_est"])) and np.all(np.isfinite(got["fn"]))              # singular legs included: nothing divides by a small det
    k3 = np.repeat(keep, 3, 1)
    gate(got["f_est"][k3], e["f_est"][k3], dtype, "f_est", n, f32_gate)
    gate(got["fn"][keep], e["fn"][keep], dtype, "fn", n, f32_gate)
    sing = np.repeat(WE._bits(e["singular"]) & keep, 3, 1)
    assert sing.any() and _bits_equal(got["f_est"][sing], to_host(d["f_prev"])[sing])       # a singular leg: f_est = f_prev exactly
    return got


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_contact_estimate_on_wide_states(torch_cuda, gpu_model, flat_model, dtype, n):
    c = WE.wide_contact_case(flat_model, gpu_model.total_mass, n)
    fig = WE.contact_figures(flat_model, c)
    assert fig["neg"] >= 1.0 / 3.0 and np.all(fig["per_foot"] >= 1) and CR.branches_taken(CR.params(), c["e64"]) == CR.ALL_BRANCHES
    solver = WD.solver(gpu_model, dtype, max_batch=n, observer=1)
    _contact_parity(torch_cuda, solver, c, dtype, n, _x8(WE.F32_CONTACT))


# ---- leg odometry
def _odom_dev(torch, c, dtype):
    td = _td(torch, dtype)
    d = {k: (None if c[k] is None else to_dev(c[k], torch, td)) for k in ("q", "v", "normals", "height", "base", "anchor")}
    d.update({k: _ints(torch, c[k]) for k in ("contact", "mask", "odo")})
    return d


def _odom_parity(torch, solver, c, dtype, n, f32_gate, what=""):
    nd = _nd(dtype)
    ref = c["ref64"]
    d = _odom_dev(torch, c, dtype)
    o = dict(base=d["base"].clone(), anchor=d["anchor"].clone(), odo=d["odo"].clone(), q_est=torch.full_like(d["q"], JUNK),
             v_est=torch.full_like(d["v"], JUNK))
    solver.base_estimate(d["q"], d["v"], d["contact"], d["mask"], o["base"], o["anchor"], o["odo"], normals=d["normals"], height=d["height"],
                         q_est=o["q_est"], v_est=o["v_est"])
    torch.cuda.synchronize()
    got = {k: (x.cpu().numpy() if k == "odo" else to_host(x)) for k, x in o.items()}
    assert np.array_equal(got["odo"], ref["odo"]), what
    w = OD.written(ref)
    assert w.any() and _bits_equal(got["anchor"][~w], c["anchor"].astype(nd)[~w]), what                 # untouched: NaN stays NaN
    assert _bits_equal(got["q_est"][:, 3:], c["q"].astype(nd)[:, 3:]) and _bits_equal(got["v_est"][:, 3:], c["v"].astype(nd)[:, 3:]), what
    assert _bits_equal(got["q_est"][:, 0:3], got["base"][:, 0:3]) and _bits_equal(got["v_est"][:, 0:3], got["base"][:, 3:6]), what
    gate(got["base"][:, 0:3], ref["base"][:, 0:3], dtype, "p", n, f32_gate)
    gate(got["base"][:, 3:6], ref["base"][:, 3:6], dtype, "v", n, f32_gate)
    gate(got["anchor"][w], ref["anchor"][w], dtype, "anchor", n, f32_gate)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_base_estimate_on_wide_states_with_unnormalised_attitudes(torch_cuda, gpu_model, flat_model, dtype, n):
    """The attitudes have lengths from 0.5 to 2.  include/wbc_hip.h ("Base state from leg odometry") takes the attitude as a sensor gives it and the
    law normalises it before it forms R (odom.hip.hpp, the leg chain of wbc_swing_reference_batch): any non-zero quaternion is a valid input, and
    tests/test_walk_edges_oracle.py shows that a law without the normalisation fails these gates."""
    solver = WD.solver(gpu_model, dtype, max_batch=n, dt=OD.BRANCH_DT, observer=1)
    for planes in (True, False):
        c = WE.wide_odom_case(flat_model, gpu_model.total_mass, n, planes=planes)
        ln = np.linalg.norm(c["q"][:, 3:7], axis=1)
        assert ln.min() < 0.7 and ln.max() > 1.5
        _odom_parity(torch_cuda, solver, c, dtype, n, _x8(WE.F32_ODOM), "planes %s" % planes)


# ---- terrain feet
def _terrain(torch, T, dtype, tile=None):
    import wbc_quadruped_dob_amd as W
    z = torch.from_numpy(np.ascontiguousarray(T["z"])).to(_td(torch, dtype)).cuda().contiguous()
    return W.Terrain(z, T["x0"], T["y0"], T["cell"], None if tile is None else _ints(torch, tile))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", WE.FEET_KINDS)
def test_terrain_feet_on_wide_states(torch_cuda, gpu_model, flat_model, dtype, kind):
    """fit: every foot on the map; far: the map and the batch 50 m out; clamped: feet beyond every edge of the 64 x 48 grid"""
    torch = torch_cuda
    td = _td(torch, dtype)
    f32_gate = _x8(WE.F32_FEET[kind])
    for n in WE.feet_sizes(kind):
        c = WE.wide_feet_case(flat_model, gpu_model.total_mass, kind, n)
        ref = c["ref64"]
        assert ref["inside"] == (kind != "clamped") and ref["margin"] >= TR.MARGIN64 and c["ref32"]["margin"] >= TR.MARGIN32
        solver = WD.solver(gpu_model, dtype, max_batch=n)
        terr = _terrain(torch, c["T"], dtype, c["tile"])
        q, swing, mask = to_dev(c["q"], torch, td), to_dev(c["swing"], torch, td), _ints(torch, c["mask"])
        swing_in = to_host(swing)
        o = dict(normals=_junk(torch, (12, n), dtype), height=_junk(torch, (4, n), dtype), surf=_junk(torch, (4, n), dtype))
        solver.terrain_feet(terr, q, mask=mask, swing=swing, **o)
        torch.cuda.synchronize()
        for key in ("normals", "height", "surf"):
            gate(to_host(o[key]), ref[key], dtype, key, n, f32_gate)
        got = to_host(swing)
        p1z = WE.p1z_words(c["mask"])
        assert _bits_equal(got[~p1z], swing_in[~p1z])
        gate(got[p1z], ref["swing"][p1z], dtype, "p1_z", n, f32_gate)
        assert np.array_equal(mask.cpu().numpy(), c["mask"])


# ---- 2. fused against unfused on wide states
def _gait_dev(torch, c, td, near=False, nan_base=False):
    g, cc = c["gait"], c["contact"]
    d = {k: to_dev(g[k], torch, td) for k in ("v", "cmd", "swing")}
    d["q"] = to_dev(c["q_near"] if near else g["q"], torch, td)
    if nan_base:
        d["q"][0:3] = float("nan")
        d["v"][0:3] = float("nan")
    d["phase"] = torch.from_numpy(np.ascontiguousarray(g["phase"])).to(td).cuda()
    d["mask"], d["sensed"], d["contact"] = _ints(torch, g["mask"]), _ints(torch, g["contact"]), _ints(torch, cc["contact"])
    d.update({k: to_dev(cc[k], torch, td) for k in ("Jc", "r", "f_prev", "normals")})
    return d


def _gait_io(torch, d, n, td, estimated=True, planes=False, select=False):
    """the in/out buffers of one side: fresh copies, outputs prefilled with junk"""
    x = dict(phase=d["phase"].clone(), mask=d["mask"].clone(), swing=d["swing"].clone(), events=torch.full_like(d["mask"], -1))
    if estimated:
        x.update(contact=d["contact"].clone(), f_est=torch.full((12, n), JUNK, dtype=td, device="cuda"))
    if planes:
        x.update(normals=torch.full((12, n), JUNK, dtype=td, device="cuda"), height=torch.full((4, n), JUNK, dtype=td, device="cuda"),
                 surf=torch.full((4, n), JUNK, dtype=td, device="cuda"))
    if select:
        x.update(hold=torch.zeros((8, n), dtype=td, device="cuda"), latch=torch.zeros(n, dtype=torch.int32, device="cuda"))
    return x


def _all_bits(one, two, what, keep=None):
    """every output bit for bit, NaN for NaN, on every state.  Were they to differ on the states heading_ok drops alone, the message says so."""
    for key in one:
        if not _same_tensor(one[key], two[key]):
            a, b = one[key].cpu().numpy(), two[key].cpu().numpy()
            diff = (a.view(np.int64 if a.itemsize == 8 else np.int32) != b.view(np.int64 if b.itemsize == 8 else np.int32))
            states = np.nonzero(diff.reshape(-1, diff.shape[-1]).any(0))[0]
            only_dropped = keep is not None and not keep[states].any()
            raise AssertionError("%s: %s differs on states %s%s" % (what, key, states[:10], " (only states heading_ok drops)" if only_dropped else ""))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_gait_estimated_equals_contact_estimate_then_gait_on_wide_states(torch_cuda, gpu_model, flat_model, dtype, n):
    torch = torch_cuda
    td = _td(torch, dtype)
    c = WE.wide_gait_case(flat_model, gpu_model.total_mass, n)
    solver = WD.solver(gpu_model, dtype, max_batch=n, observer=1)
    d = _gait_dev(torch, c, td)
    one, two = _gait_io(torch, d, n, td), _gait_io(torch, d, n, td)
    solver.gait_estimated(d["q"], d["v"], d["cmd"], d["Jc"], d["r"], d["f_prev"], d["normals"], one["contact"], one["phase"], one["mask"], one["swing"],
                          events=one["events"], f_est=one["f_est"])
    solver.contact_estimate(d["Jc"], d["r"], d["f_prev"], d["normals"], two["contact"], f_est=two["f_est"])
    solver.gait(d["q"], d["v"], d["cmd"], two["phase"], two["mask"], two["swing"], contact=two["contact"], events=two["events"])
    torch.cuda.synchronize()
    _all_bits(one, two, "gait_estimated %s n=%d" % (dtype, n), c["gait"]["keep"])
    keep = torch.from_numpy(c["gait"]["keep"]).cuda()
    assert bool(torch.isfinite(one["swing"][:, keep]).all()) and bool(torch.isfinite(one["f_est"]).all())
    assert not torch.equal(one["mask"], d["mask"]) and not torch.equal(one["contact"], d["contact"]) and bool((one["events"] != -1).all())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_gait_estimated_odom_equals_base_estimate_then_gait_estimated_on_wide_states(torch_cuda, gpu_model, flat_model, dtype, n):
    """with and without height; the base rows of q and v hold NaN in the copies both sides read"""
    torch = torch_cuda
    td = _td(torch, dtype)
    c = WE.wide_gait_case(flat_model, gpu_model.total_mass, n)
    oc = c["odom"]
    solver = WD.solver(gpu_model, dtype, max_batch=n, dt=OD.BRANCH_DT, observer=1)
    d = _gait_dev(torch, c, td, nan_base=True)
    base, anchor, odo, height = to_dev(oc["base"], torch, td), to_dev(oc["anchor"], torch, td), _ints(torch, oc["odo"]), to_dev(oc["height"], torch, td)
    anchored = False
    for hgt in (height, None):
        def io():
            x = _gait_io(torch, d, n, td)
            x.update(base=base.clone(), anchor=anchor.clone(), odo=odo.clone(), q_est=torch.full((19, n), JUNK, dtype=td, device="cuda"),
                     v_est=torch.full((18, n), JUNK, dtype=td, device="cuda"))
            return x
        one, two = io(), io()
        solver.gait_estimated_odom(d["q"], d["v"], d["cmd"], d["Jc"], d["r"], d["f_prev"], d["normals"], one["contact"], one["phase"], one["mask"],
                                   one["swing"], one["base"], one["anchor"], one["odo"], height=hgt, q_est=one["q_est"], v_est=one["v_est"],
                                   events=one["events"], f_est=one["f_est"])
        solver.base_estimate(d["q"], d["v"], two["contact"], two["mask"], two["base"], two["anchor"], two["odo"],
                             normals=None if hgt is None else d["normals"], height=hgt, q_est=two["q_est"], v_est=two["v_est"])
        solver.gait_estimated(two["q_est"], two["v_est"], d["cmd"], d["Jc"], d["r"], d["f_prev"], d["normals"], two["contact"], two["phase"],
                              two["mask"], two["swing"], events=two["events"], f_est=two["f_est"])
        torch.cuda.synchronize()
        _all_bits(one, two, "gait_estimated_odom %s n=%d height %s" % (dtype, n, hgt is not None), c["gait"]["keep"])
        assert bool(torch.isfinite(one["base"]).all()) and bool(torch.isfinite(one["q_est"][0:3]).all())
        anchored = anchored or bool(((one["odo"] >> 4) != 0).any())
    assert anchored


def _rounding(a, b, dtype):
    """the standing tolerances the existing _same functions hold the planes to"""
    return elementwise_excess(a, b) if dtype == "f64" else elementwise_excess(a, b, rtol=0.0, atol_frac=STANDING32)


def _planes_as_same(one, two, what, dtype, parent=None):
    """tests/test_gpu_terrain.py::_same (parent None) and tests/test_gpu_foothold.py::_same: every word bit for bit but the planes, which descend from
    p_f -- hipcc contracts the leg chain inside gait's body and inside terrain_feet_kernel differently -- and are held to terrain_feet's at the
    standing tolerances, and bit for bit to the existing one-launch call's where there is one.
    FOUND HERE: the p0 of a foot that lifts off in the call (swing words 9k .. 9k+2 := p_f) descends from p_f too, and gait_kernel and the fused
    kernels, which share gait_body.inc.hpp as text, do not contract it alike either.  On the walking loop's states the existing tests see equal
    bits; on these states 9 to 24 of the lifted feet's p0 words of a case differ in their last bits (5.6e-15 relative in fp64, 1.9e-6 in fp32).
    include/wbc_hip.h now says so, and p0 is held like the planes: to rounding against the unfused launches.  Every other swing word -- p1_x, p1_y,
    p1_z, t0, hgt, T and all nine words of a foot that did not lift -- stays bit for bit."""
    for key in one:
        if key in ("normals", "height", "surf"):
            if parent is not None:
                assert _same_tensor(one[key], parent[key]), (what, key)
            a, b = to_host(one[key]), to_host(two[key]).astype(np.float64)
            ex = _rounding(a, b, dtype)
            print("%s %s %s: %d of %d words differ from terrain_feet's, excess %.3g" % (what, key, dtype, int((a != b).sum()), a.size, ex))
            assert np.all(np.isfinite(a)) and ex <= 1.0, (what, key, ex)
        elif key == "swing":
            assert _same_tensor(one["events"], two["events"])
            ev = two["events"].cpu().numpy()
            p0 = np.zeros((len(ev), 36), bool)
            for k in range(4):
                p0[((ev >> k) & 1) == 1, 9 * k:9 * k + 3] = True
            a, b = to_host(one["swing"]), to_host(two["swing"])
            assert p0.any() and _bits_equal(a[~p0], b[~p0]), (what, "swing words other than a lifted foot's p0")
            ex = _rounding(a[p0], b[p0].astype(np.float64), dtype)
            vs = "" if parent is None else "; %d from the call's without selection" % int((a[p0] != to_host(parent["swing"])[p0]).sum())
            print("%s p0 %s: %d of %d words differ from gait's%s, excess %.3g" % (what, dtype, int((a[p0] != b[p0]).sum()), int(p0.sum()), vs, ex))
            assert np.all(np.isfinite(a[p0])) and ex <= 1.0, (what, "p0", ex)
        else:
            assert _same_tensor(one[key], two[key]), (what, key)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_terrain_calls_equal_the_launches_they_replace_on_wide_states(torch_cuda, gpu_model, flat_model, dtype, n):
    """gait_terrain = gait -> terrain_feet and gait_estimated_terrain = gait_estimated -> terrain_feet; then, on the same grid with ridges and a cost
    map, gait_terrain_select = gait -> foothold_select -> terrain_feet and gait_estimated_terrain_select = gait_estimated -> foothold_select ->
    terrain_feet, their planes bit for bit those of the call without selection.  Wide joints and attitudes, the base within a metre of the origin
    (one map holds the batch), every foot on the map."""
    torch = torch_cuda
    td = _td(torch, dtype)
    c = WE.wide_gait_case(flat_model, gpu_model.total_mass, n)
    sv = WD.solver(gpu_model, dtype, max_batch=n, observer=1)
    d = _gait_dev(torch, c, td, near=True)
    q, v, cmd, Jc, r, fp, nrm = (d[k] for k in ("q", "v", "cmd", "Jc", "r", "f_prev", "normals"))
    selected = 0
    for select in (False, True):
        T = FR.ridges(c["T"], 4) if select else c["T"]
        tr = _terrain(torch, T, dtype, c["tile"])
        cm = sv.terrain_cost(tr) if select else None
        mk = functools.partial(_gait_io, torch, d, n, td, planes=True, select=select)
        pl = lambda x: dict(normals=x["normals"], height=x["height"], surf=x["surf"])
        # the plain gait rule, given a sensed word
        one, two = mk(estimated=False), mk(estimated=False)
        if select:
            par = _gait_io(torch, d, n, td, estimated=False, planes=True)
            sv.gait_terrain_select(tr, cm, one["hold"], one["latch"], q, v, cmd, one["phase"], one["mask"], one["swing"], contact=d["sensed"],
                                   events=one["events"], **pl(one))
            sv.gait_terrain(tr, q, v, cmd, par["phase"], par["mask"], par["swing"], contact=d["sensed"], events=par["events"], **pl(par))
        else:
            par = None
            sv.gait_terrain(tr, q, v, cmd, one["phase"], one["mask"], one["swing"], contact=d["sensed"], events=one["events"], **pl(one))
        sv.gait(q, v, cmd, two["phase"], two["mask"], two["swing"], contact=d["sensed"], events=two["events"])
        if select:
            sv.foothold_select(tr, cm, two["mask"], two["swing"], two["hold"], two["latch"])
        sv.terrain_feet(tr, q, mask=two["mask"], swing=two["swing"], **pl(two))
        torch.cuda.synchronize()
        _planes_as_same(one, two, "gait_terrain%s n=%d" % ("_select" if select else "", n), dtype, par)
        if select:
            selected += int(((one["latch"] >> 4) != 0).sum())
        # the estimated word; normals is in/out: the planes of the contact law go in
        one, two = mk(), mk()
        one["normals"] = nrm.clone()
        if select:
            par = _gait_io(torch, d, n, td, planes=True)
            par["normals"] = nrm.clone()
            sv.gait_estimated_terrain_select(tr, cm, one["hold"], one["latch"], q, v, cmd, Jc, r, fp, one["normals"], one["contact"], one["phase"],
                                             one["mask"], one["swing"], events=one["events"], f_est=one["f_est"], height=one["height"], surf=one["surf"])
            sv.gait_estimated_terrain(tr, q, v, cmd, Jc, r, fp, par["normals"], par["contact"], par["phase"], par["mask"], par["swing"],
                                      events=par["events"], f_est=par["f_est"], height=par["height"], surf=par["surf"])
        else:
            sv.gait_estimated_terrain(tr, q, v, cmd, Jc, r, fp, one["normals"], one["contact"], one["phase"], one["mask"], one["swing"],
                                      events=one["events"], f_est=one["f_est"], height=one["height"], surf=one["surf"])
        sv.gait_estimated(q, v, cmd, Jc, r, fp, nrm, two["contact"], two["phase"], two["mask"], two["swing"], events=two["events"], f_est=two["f_est"])
        if select:
            sv.foothold_select(tr, cm, two["mask"], two["swing"], two["hold"], two["latch"])
        sv.terrain_feet(tr, q, mask=two["mask"], swing=two["swing"], **pl(two))
        torch.cuda.synchronize()
        _planes_as_same(one, two, "gait_estimated_terrain%s n=%d" % ("_select" if select else "", n), dtype, par)
        assert not torch.equal(one["normals"], nrm) and not torch.equal(one["mask"], d["mask"])
        if select:
            selected += int(((one["latch"] >> 4) != 0).sum())
    print("n = %d %s: %d selections among the calls compared" % (n, dtype, selected))
    assert selected > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_gait_terrain_planes_on_a_steep_ramp_feed_ground_force(torch_cuda, gpu_model, flat_model, dtype, n):
    """The normals and heights gait_terrain writes on a ramp of slope 2 (63 degrees off e_z) go straight into ground_force of the same states, and the
    chain is held end to end against terrain_ref.feet -> ground_ref.ground_force.  The robots are at rest, so f_gr = f_n n: the planes alone."""
    torch = torch_cuda
    td = _td(torch, dtype)
    c = WE.ramp_case(flat_model, gpu_model.total_mass, n)
    ref, own = c["ref64"], c["ref" + dtype[1:]]
    keep = ~c["skip"]
    assert c["skip"].mean() <= WE.SKIP_CAP
    f32_gate = _x8(WE.F32_RAMP)
    solver = WD.solver(gpu_model, dtype, max_batch=n)
    terr = _terrain(torch, c["T"], dtype)
    d = {k: to_dev(c[k], torch, td) for k in ("q", "v", "cmd", "swing", "mu", "Jc")}
    phase, mask = torch.from_numpy(np.ascontiguousarray(c["phase"])).to(td).cuda(), _ints(torch, c["mask"])
    normals, height = _junk(torch, (12, n), dtype), _junk(torch, (4, n), dtype)
    solver.gait_terrain(terr, d["q"], d["v"], d["cmd"], phase, mask, d["swing"], contact=_ints(torch, c["contact"]), normals=normals, height=height)
    o = _plant_outs(torch, n, dtype)
    solver.ground_force(d["q"], d["v"], d["Jc"], normals, height, d["mu"], f_gr=o["f_gr"], contact=o["contact"], gap=o["gap"])
    torch.cuda.synchronize()
    gate(to_host(normals), ref["feet"]["normals"], dtype, "normals", n, f32_gate)
    gate(to_host(height), ref["feet"]["height"], dtype, "height", n, f32_gate)
    got = o["contact"].cpu().numpy()
    assert np.array_equal(WE._bits(got)[keep], WE._bits(own["ground"]["contact"])[keep]) and np.all(got & ~15 == 0)
    gate(to_host(o["f_gr"]), ref["ground"]["f_gr"], dtype, "f_gr", n, f32_gate)
    gate(to_host(o["gap"]), ref["ground"]["gap"], dtype, "gap", n, f32_gate)


# ---- 3. cost-map grids whose last workgroups are not the first and lie partly outside the map
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("grid", WE.COST_GRIDS)
def test_cost_map_on_ragged_grids(torch_cuda, gpu_model, dtype, grid):
    """the gates of tests/test_gpu_foothold.py::test_cost_map_parity"""
    torch = torch_cuda
    T = WE.cost_grid(grid)
    solver = WD.solver(gpu_model, dtype, max_batch=16)
    terr = _terrain(torch, T, dtype)
    tol = 1e-9 if dtype == "f64" else 5e-4
    for margin in (0, 1, 2):
        for w_slope in (0.0, 0.375, FR.DEFAULTS["w_slope"]):
            P = FR.params(margin=margin, w_slope=w_slope)
            solver.set_foothold_params(P)
            cost = torch.full_like(terr.z, JUNK)
            assert solver.terrain_cost(terr, cost) is cost
            torch.cuda.synchronize()
            got = cost.cpu().numpy()
            own, ref = FR.cost_map(T, P, _nd(dtype)), FR.cost_map(T, P)["cost"]
            err = np.abs(got.astype(np.float64) - ref).max()
            print("cost %s %s margin %d w_slope %g: max |diff| %.3g of %.3g" % (grid, dtype, margin, w_slope, err, np.abs(ref).max()))
            assert np.all(np.isfinite(got)) and not np.any(got == JUNK)
            if w_slope == 0.0:
                assert np.array_equal(got, own["step"])
            else:
                assert err <= tol * np.abs(ref).max()


# ---- 4. descriptions whose joint and foot order is not leg-major
@pytest.mark.parametrize("which", ["G", "P"])
def test_wide_cases_on_reordered_models(torch_cuda, hip_lib, tmp_path, which):
    """jidx_of_leg is not the identity: the contact, ground, stiction and odometry wide cases built on that description, fp64, one size"""
    torch = torch_cuda
    n, dtype = 65, "f64"
    spec = limit_models.specs(tmp_path)[which]
    assert [j for js in spec.legs for j in js] != list(range(12))
    none = dict.fromkeys(("f_gr", "gap", "q", "v", "anchor", "f_est", "fn", "p"), 0.0)      # fp64 only: no float32 gate is consulted
    c = WE.wide_contact_case(spec.flat, spec.total_mass, n)
    fig = WE.contact_figures(spec.flat, c)
    print("%s contact: det < 0 on %.1f %%, singular %.1f %%, cond up to %.1f" % (which, 100 * fig["neg"], 100 * fig["singular"], fig["cond"]))
    assert fig["singular"] > 0 and 0.2 < fig["neg"] < 0.8
    _contact_parity(torch, WD.solver(spec.model, dtype, max_batch=n, observer=1), c, dtype, n, none)
    solver = WD.solver(spec.model, dtype, max_batch=n)
    c = WE.wide_ground_case(spec.flat, spec.total_mass, n)
    assert GND.branches_taken(GND.params(), c["ref64"][2]) == GND.ALL_BRANCHES
    _ground_parity(torch, solver, c, dtype, n, spec.legs, none, which)
    c = WE.wide_stick_case(spec.flat, spec.total_mass, n)
    assert ST.branches_taken(c["ref64"][2]) == ST.ALL_BRANCHES
    _stick_parity(torch, solver, c, dtype, n, none, which)
    c = WE.wide_odom_case(spec.flat, spec.total_mass, n)
    _odom_parity(torch, WD.solver(spec.model, dtype, max_batch=n, dt=OD.BRANCH_DT, observer=1), c, dtype, n, none, which)
    # the leg's own joint columns matter: dealt to the legs in leg-major order, the same joint angles put the feet elsewhere
    lever, _ = OD.leg_terms(spec.flat, c["q"], c["v"])
    perm = c["q"].copy()
    perm[:, 7:] = c["q"][:, 7 + np.array([j for js in spec.legs for j in js])]
    assert np.abs(lever - OD.leg_terms(spec.flat, perm, c["v"])[0]).max() > 1e-2
