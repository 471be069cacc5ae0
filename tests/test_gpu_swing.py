"""GPU: swing-foot references (wbc_swing_reference_batch, wbc_reference_swing_batch, wbc_compute_swing_reference) through the C-ABI against the numpy
restatement tests/swing_ref.py: parity in both scalar types on ragged sizes, untouched data bit for bit, the fused call against the two-call sequence,
models whose joint and foot order is not leg-major, a singular leg, argument checks, a captured per-tick loop and the closed loop.

Gates.  fp64: 1e-6 of every entry (util.elementwise_excess, the project's gate).  fp32: tests/swing_ref.py evaluated in float32 against float64 on the
inputs of this file's cases (sizes 1, 15, 16, 17, 33), error relative to the largest entry of the array: written rows of vdot_des 7.4e-6 (the
near-singular folded right legs of the synthetic batch carry it), foot 2.2e-7.  The device uses its own rsqrt / sincos and another operation order, so
the gates are 8 x those: 5.9e-5 and 1.8e-6."""
import functools

import numpy as np
import pytest

from tests import limit_models, limit_ref, swing_ref as SR, walk_dev as WD
from tests.util import elementwise_excess, relerr, to_dev, to_host
from wbc_quadruped_dob_amd import synth

pytestmark = pytest.mark.gpu
SIZES = (1, 15, 16, 17, 33)
F32_GATE_VDOT, F32_GATE_FOOT = 5.9e-5, 1.8e-6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _solver(model, dtype="f64", max_batch=64, ref=True, ref_params=None):
    return WD.solver(model, dtype, max_batch, ref_params=(ref_params or synth.default_ref_params()) if ref else None)


@functools.lru_cache(maxsize=None)
def _case(flat_id, n):
    """(case, plan, reference vdot_des, reference foot) in float64: computed once per (model, size), read only"""
    flat, tm = _FLATS[flat_id]
    c = SR.swing_case(flat, tm, n, rank=n)
    plan = synth.make_plan(dict(q=c["q"]), rank=n)
    vd, foot = SR.swing_reference(flat, c["q"], c["v"], c["mask"], c["swing"], c["t"], c["vdot_des"])
    return c, plan, vd, foot


_FLATS = {}


def _register(name, flat, total_mass):
    _FLATS[name] = (flat, total_mass)
    return name


def _written(flat, mask):
    """bool [N, 18]: the entries of vdot_des a swing call writes"""
    w = np.zeros((len(mask), 18), bool)
    for k, js in enumerate(limit_ref.leg_joints(flat)):
        lifted = ((mask >> k) & 1) == 0
        for j in js:
            w[lifted, 6 + j] = True
    return w


def _gate(got, ref, dtype, f32_gate, what):
    ex = elementwise_excess(got, ref) if dtype == "f64" else elementwise_excess(got, ref, rtol=0.0, atol_frac=f32_gate)
    print("%s %s: excess %.3g (max |ref| %.3g, max |diff| %.3g)" % (what, dtype, ex, np.abs(ref).max() if ref.size else 0.0,
                                                                     np.abs(np.asarray(got, np.float64) - ref).max() if ref.size else 0.0))
    assert np.all(np.isfinite(got)), what
    assert ex <= 1.0, (what, ex)


def _dev_case(torch, c, plan, dtype):
    td = torch.float64 if dtype == "f64" else torch.float32
    d = {k: to_dev(c[k], torch, td) for k in ("q", "v", "swing", "vdot_des")}
    d["plan"] = to_dev(plan, torch, td)
    d["mask"] = torch.from_numpy(np.ascontiguousarray(c["mask"])).to(torch.int32).cuda()
    return d


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_parity_and_untouched_rows(torch_cuda, gpu_model, flat_model, dtype, n):
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, plan, ref_vd, ref_foot = _case(fid, n)
    solver = _solver(gpu_model, dtype, max_batch=n, ref=False)
    d = _dev_case(torch, c, plan, dtype)
    before = to_host(d["vdot_des"])
    got = solver.swing_reference(d["q"], d["v"], d["mask"], d["swing"], c["t"], vdot_des=d["vdot_des"], want_foot=True)
    torch.cuda.synchronize()
    vd, foot = to_host(got["vdot_des"]), to_host(got["foot"])
    w = _written(flat_model, c["mask"])
    assert np.array_equal(vd[~w], before[~w])      # base rows and stance-leg rows: the buffer as it was
    if w.any():
        _gate(vd[w], ref_vd[w], dtype, F32_GATE_VDOT, "vdot_des n=%d" % n)
    _gate(foot, ref_foot, dtype, F32_GATE_FOOT, "foot n=%d" % n)


def test_all_stance_mask_leaves_vdot_des_untouched(torch_cuda, gpu_model, flat_model):
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, plan, _, ref_foot = _case(fid, 17)
    solver = _solver(gpu_model, "f64", max_batch=17, ref=False)
    d = _dev_case(torch, c, plan, "f64")
    before = d["vdot_des"].clone()
    got = solver.swing_reference(d["q"], d["v"], torch.full_like(d["mask"], 0b1111), d["swing"], c["t"], vdot_des=d["vdot_des"], want_foot=True)
    torch.cuda.synchronize()
    assert torch.equal(got["vdot_des"], before)
    _gate(to_host(got["foot"]), ref_foot, "f64", F32_GATE_FOOT, "foot, all stance")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", (17, 33))
def test_fused_call_against_the_two_call_sequence(torch_cuda, gpu_model, flat_model, dtype, n):
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, plan, _, ref_foot = _case(fid, n)
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, plan, dtype)
    ref = solver.reference(d["q"], d["v"], d["plan"], c["t"], want_com=True)
    fused = solver.reference_swing(d["q"], d["v"], d["plan"], d["mask"], d["swing"], c["t"], want_com=True, want_foot=True)
    torch.cuda.synchronize()
    assert torch.equal(fused["w_des"], ref["w_des"]) and torch.equal(fused["com"], ref["com"])
    w = _written(flat_model, c["mask"])
    fv, rv = to_host(fused["vdot_des"]), to_host(ref["vdot_des"])
    assert np.array_equal(fv[~w], rv[~w])          # base rows and stance-leg rows: wbc_reference_batch's bits
    two = solver.swing_reference(d["q"], d["v"], d["mask"], d["swing"], c["t"], vdot_des=ref["vdot_des"].clone(), want_foot=True)
    torch.cuda.synchronize()
    tv = to_host(two["vdot_des"])
    print("swing rows bit-identical to the two-call sequence:", bool(np.array_equal(fv[w], tv[w])), "foot:", bool(torch.equal(fused["foot"], two["foot"])))
    _gate(fv[w], np.asarray(tv[w], np.float64), dtype, F32_GATE_VDOT, "fused swing rows n=%d" % n)
    _gate(to_host(fused["foot"]), ref_foot, dtype, F32_GATE_FOOT, "fused foot n=%d" % n)
    # and against the numpy reference fed with the oracle-side base rows the device wrote
    ref_vd, _ = SR.swing_reference(flat_model, c["q"], c["v"], c["mask"], c["swing"], c["t"], np.asarray(rv, np.float64))
    _gate(fv[w], ref_vd[w], dtype, F32_GATE_VDOT, "fused swing rows vs swing_ref n=%d" % n)


@pytest.mark.parametrize("which", ["G", "P"])
def test_reordered_models(torch_cuda, hip_lib, tmp_path, which):
    """Joint and foot order not leg-major: rows land in the caller's joint order, foot in the caller's foot order."""
    torch = torch_cuda
    spec = limit_models.specs(tmp_path)[which]
    assert [j for js in spec.legs for j in js] != list(range(12))
    fid = _register(which, spec.flat, spec.total_mass)
    n = 17
    c, plan, ref_vd, ref_foot = _case(fid, n)
    solver = _solver(spec.model, "f64", max_batch=n)
    d = _dev_case(torch, c, plan, "f64")
    before = to_host(d["vdot_des"])
    got = solver.swing_reference(d["q"], d["v"], d["mask"], d["swing"], c["t"], vdot_des=d["vdot_des"], want_foot=True)
    torch.cuda.synchronize()
    vd, foot = to_host(got["vdot_des"]), to_host(got["foot"])
    w = _written(spec.flat, c["mask"])
    assert np.array_equal(vd[~w], before[~w])
    _gate(vd[w], ref_vd[w], "f64", F32_GATE_VDOT, "%s vdot_des" % which)
    _gate(foot, ref_foot, "f64", F32_GATE_FOOT, "%s foot" % which)
    fused = solver.reference_swing(d["q"], d["v"], d["plan"], d["mask"], d["swing"], c["t"], want_foot=True)
    ref = solver.reference(d["q"], d["v"], d["plan"], c["t"])
    torch.cuda.synchronize()
    fv, rv = to_host(fused["vdot_des"]), to_host(ref["vdot_des"])
    assert np.array_equal(fv[~w], rv[~w]) and torch.equal(fused["w_des"], ref["w_des"])
    ref2, _ = SR.swing_reference(spec.flat, c["q"], c["v"], c["mask"], c["swing"], c["t"], rv)
    _gate(fv[w], ref2[w], "f64", F32_GATE_VDOT, "%s fused" % which)


def test_singular_leg(torch_cuda, gpu_model, flat_model):
    """Foot 0's knee at the angle where det J_kl vanishes (|det| <= 1e-6 of its value in the nominal stance): finite, and the reference's numbers
    at the fp64 gate with the default damping."""
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, plan, _, _ = _case(fid, 16)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    nominal = np.zeros(19); nominal[2] = 0.4; nominal[6] = 1.0; nominal[7:] = synth.default_ref_params()["q_nom"]
    det_nom = abs(SR.leg_det(flat_model, 0, nominal[None])[0])
    for s in range(16):
        qs, det, _ = SR.singular_knee(flat_model, 0, c["q"][s])
        assert det <= 1e-6 * det_nom, (det, det_nom)
        c["q"][s] = qs
    c["mask"] = np.full(16, 0b1110, np.int32)
    ref_vd, ref_foot = SR.swing_reference(flat_model, c["q"], c["v"], c["mask"], c["swing"], c["t"], c["vdot_des"])
    solver = _solver(gpu_model, "f64", max_batch=16, ref=False)
    d = _dev_case(torch, c, plan, "f64")
    got = solver.swing_reference(d["q"], d["v"], d["mask"], d["swing"], c["t"], vdot_des=d["vdot_des"], want_foot=True)
    torch.cuda.synchronize()
    w = _written(flat_model, c["mask"])
    _gate(to_host(got["vdot_des"])[w], ref_vd[w], "f64", F32_GATE_VDOT, "singular leg vdot_des")
    _gate(to_host(got["foot"]), ref_foot, "f64", F32_GATE_FOOT, "singular leg foot")


def test_argument_checks(torch_cuda, gpu_model):
    import ctypes as C
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    solver = _solver(gpu_model, "f64", max_batch=16)
    L = W.lib()
    z = lambda r, n=16: torch.zeros((r, n), dtype=torch.float64, device="cuda")
    q = z(19); q[6] = 1.0
    mask = torch.zeros(16, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    # N = 0: WBC_OK without looking at the buffers
    assert L.wbc_swing_reference_batch(solver._h, 0, None, None, None, None, C.c_double(0), None, None, None) == 0
    assert L.wbc_reference_swing_batch(solver._h, 0, None, None, None, None, None, C.c_double(0), None, None, None, None, None) == 0
    # a NULL swing
    assert L.wbc_swing_reference_batch(solver._h, 16, p(q), p(z(18)), p(mask), None, C.c_double(0), p(z(18)), None, None) == 1
    assert L.wbc_reference_swing_batch(solver._h, 16, p(q), p(z(18)), p(z(12)), p(mask), None, C.c_double(0), p(z(6)), p(z(18)), None, None, None) == 1
    # N > max_batch
    with pytest.raises(W.WbcError) as e:
        solver.swing_reference(z(19, 17), z(18, 17), torch.zeros(17, dtype=torch.int32, device="cuda"), z(36, 17), vdot_des=z(18, 17))
    assert e.value.code == 7   # WBC_E_CAPACITY
    # a negative or non-finite entry
    for bad in (dict(damping=-1e-4), dict(kp=[1.0, -1.0, 1.0]), dict(kd=float("nan")), dict(damping=float("inf"))):
        with pytest.raises(W.WbcError):
            solver.set_swing_params(bad)
    solver.set_swing_params(dict(kp=100.0, kd=20.0, damping=0.0))
    torch.cuda.synchronize()


def test_set_swing_params_reaches_the_kernel(torch_cuda, gpu_model, flat_model):
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, plan, _, _ = _case(fid, 15)
    sp = dict(kp=(100.0, 200.0, 300.0), kd=(10.0, 20.0, 30.0), damping=1e-3)
    ref_vd, _ = SR.swing_reference(flat_model, c["q"], c["v"], c["mask"], c["swing"], c["t"], c["vdot_des"], sp)
    solver = _solver(gpu_model, "f64", max_batch=15, ref=False)
    solver.set_swing_params(sp)
    d = _dev_case(torch, c, plan, "f64")
    got = solver.swing_reference(d["q"], d["v"], d["mask"], d["swing"], c["t"], vdot_des=d["vdot_des"])
    torch.cuda.synchronize()
    w = _written(flat_model, c["mask"])
    _gate(to_host(got["vdot_des"])[w], ref_vd[w], "f64", F32_GATE_VDOT, "custom gains")


# ---- the tick without a gait call: reference_swing -> step -> integrate with the case's fixed mask and plan (walk_dev.tick, gait=False)
def test_captured_tick_replays_bit_for_bit(torch_cuda, gpu_model, flat_model, oracle):
    """reference_swing -> step -> integrate at N = 17, captured once: three replays from the same start = three eager ticks, bit for bit."""
    torch = torch_cuda
    n, t = 17, 0.02
    case = SR.loop_case(flat_model, oracle, n)
    solver = _solver(gpu_model, "f64", max_batch=n, ref_params=SR.loop_ref_params())
    d = WD.buffers(torch, case)
    start = WD.state(torch, case)
    st = {k: x.clone() for k, x in start.items()}
    for _ in range(3):
        WD.tick(solver, d, st, gait=False, t=t)
    torch.cuda.synchronize()
    eager = {k: x.clone() for k, x in st.items()}
    eager["tau"] = d["tick"]["tau"].clone()
    WD.capture_replay(torch, lambda: WD.tick(solver, d, st, gait=False, t=t), WD.rewinder(st, start), 3,
                      lambda: solver.set_swing_params(dict(kp=1.0)))   # a captured graph keeps the gains it was captured with
    assert torch.equal(st["q"], eager["q"]) and torch.equal(st["v"], eager["v"]) and torch.equal(d["tick"]["tau"], eager["tau"])
    assert not torch.equal(st["q"], start["q"])


def test_closed_loop_matches_the_cpu_loop_and_lands(torch_cuda, gpu_model, flat_model, oracle):
    """The loop of tests/test_swing_oracle.py on the device, 16 robots, fp64: end-of-loop q, v and swing-foot positions agree with the CPU loop to 1e-6
    (of the largest entry), and every swing foot ends within 0.1 |p1 - p0| of its touchdown point."""
    torch = torch_cuda
    n = 16
    case = SR.loop_case(flat_model, oracle, n)
    cpu = SR.closed_loop(flat_model, oracle, case)
    assert cpu["status_ok"]
    solver = _solver(gpu_model, "f64", max_batch=n, ref_params=SR.loop_ref_params())
    d = WD.buffers(torch, case)
    st = WD.state(torch, case)
    dt = synth.default_params()["dt"]
    for k in range(SR.LOOP_TICKS):
        WD.tick(solver, d, st, gait=False, t=k * dt)
    foot = solver.swing_reference(st["q"], st["v"], st["mask"], st["swing"], 0.0, vdot_des=d["ref"]["vdot_des"], want_foot=True)["foot"]
    torch.cuda.synchronize()
    q, v, foot = to_host(st["q"]), to_host(st["v"]), to_host(foot)
    lifted = ((case["mask"][:, None] >> np.arange(4)[None]) & 1) == 0
    pos = lambda f: f.reshape(n, 4, 6)[:, :, :3][lifted]
    eq, ev, ef = relerr(q, cpu["q"]), relerr(v, cpu["v"]), relerr(pos(foot), pos(cpu["foot"]))
    err = SR.landing_errors(case, foot)
    print("closed loop: q %.3g v %.3g swing feet %.3g; landing errors / step: worst %.4f" % (eq, ev, ef, err[lifted].max()))
    assert eq < 1e-6 and ev < 1e-6 and ef < 1e-6
    assert np.all(err[lifted] < 0.1), err


def test_single_robot_call_equals_the_batch_call(torch_cuda, gpu_model, flat_model):
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, plan, _, _ = _case(fid, 15)
    solver = _solver(gpu_model, "f64", max_batch=1, ref=False)
    for s in (0, 6, 9):
        one = {k: (v[s:s + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        d = _dev_case(torch, one, plan[s:s + 1], "f64")
        got = solver.swing_reference(d["q"], d["v"], d["mask"], d["swing"], c["t"], vdot_des=d["vdot_des"], want_foot=True)
        torch.cuda.synchronize()
        vd, foot = solver.compute_swing_reference(c["q"][s], c["v"][s], int(c["mask"][s]), c["swing"][s], c["vdot_des"][s], c["t"])
        assert np.array_equal(vd, to_host(got["vdot_des"])[0]) and np.array_equal(foot, to_host(got["foot"])[0])
