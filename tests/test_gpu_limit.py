"""GPU: joint torque limits behind the tick (wbc_step_limited_batch / wbc_limit_torques_batch) against the numpy reference tests/limit_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import limit_ref
from tests.util import Dev, _compare, _host, _nd, _obs_state, elementwise_excess, to_host
from wbc_quadruped_dob_amd import synth

pytestmark = pytest.mark.gpu
KEYS = ("tau", "f", "status", "limited")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _solver(gpu_model, dtype="f64", obs=0, n=256, lim=None, **kw):
    import wbc_quadruped_dob_amd as W
    P = synth.default_params(observer_order=obs, dtype=dtype)
    P.update(kw)
    s = W.Solver(gpu_model, W.Params.from_dict(P, dtype), dtype=dtype, device=0, max_batch=n, options={})
    if lim is not None:
        s.set_torque_limits(lim)
    return s, P


def _same_bits(torch, a, b, keys=KEYS + ("iters",)):
    torch.cuda.synchronize()
    return all(torch.equal(a[k], b[k]) for k in keys)


@functools.lru_cache(maxsize=None)
def _case(oracle, total_mass, cfg, n, dtype, obs, lim):
    B = synth.make_batch(cfg, n, total_mass, rank=3)
    P = synth.default_params(observer_order=obs, dtype=dtype)
    integ, r = _obs_state(oracle, B, dtype, obs)
    ref = limit_ref.step_limited(oracle, P, B, lim, _nd(dtype), None if integ is None else integ.copy(), None if r is None else r.copy())
    return B, integ, r, ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("cfg", [3, 4])
@pytest.mark.parametrize("dtype,obs", [("f64", 0), ("f64", 1), ("f32", 1)])
def test_parity_with_the_reference(torch_cuda, gpu_model, oracle, dtype, obs, cfg, n):
    torch = torch_cuda
    B, integ, r, ref = _case(oracle, gpu_model.total_mass, cfg, n, dtype, obs, 45.0)
    solver, _ = _solver(gpu_model, dtype, obs, n, 45.0)
    got = _host(torch, Dev(torch, B, dtype, integ, r).step_limited(solver))
    _compare(got, ref, dtype, 45.0)
    if n >= 63:
        assert (ref["limited"] == 0).any() and (ref["limited"] == 1).any()
        assert solver.limited_count() == int((got["limited"] == 1).sum())


@pytest.mark.parametrize("dtype,obs", [("f64", 0), ("f64", 1), ("f32", 1)])
def test_swing_leg_torques_are_clipped(torch_cuda, gpu_model, oracle, dtype, obs):
    torch = torch_cuda
    B = limit_ref.swing_case(gpu_model.total_mass)
    P = synth.default_params(observer_order=obs, dtype=dtype)
    integ, r = _obs_state(oracle, B, dtype, obs)
    ref = limit_ref.step_limited(oracle, P, B, 45.0, _nd(dtype), None if integ is None else integ.copy(), None if r is None else r.copy())
    assert (ref["limited"] == 2).sum() >= 8
    solver, _ = _solver(gpu_model, dtype, obs, 64, 45.0)
    got = _host(torch, Dev(torch, B, dtype, integ, r).step_limited(solver))
    _compare(got, ref, dtype, 45.0)


@pytest.mark.parametrize("dtype,obs", [("f64", 0), ("f64", 1), ("f32", 1)])
def test_infeasible_limits_clamp_and_keep_the_forces(torch_cuda, gpu_model, oracle, dtype, obs):
    torch = torch_cuda
    B = synth.make_batch(2, 64, gpu_model.total_mass, rank=3)
    P = synth.default_params(observer_order=obs, dtype=dtype)
    P["fn_min"] = 20.0
    integ, r = _obs_state(oracle, B, dtype, obs)
    ref = limit_ref.step_limited(oracle, P, B, 0.05, _nd(dtype), None if integ is None else integ.copy(), None if r is None else r.copy())
    assert np.all(ref["qp_status"] == 2) and np.all(ref["limited"] == 2)
    solver, _ = _solver(gpu_model, dtype, obs, 64, 0.05, fn_min=20.0)
    dev = Dev(torch, B, dtype, integ, r)
    out = dev.step_limited(solver)
    plain = dev.step(solver)
    assert torch.equal(out["f"], plain["f"]) and torch.equal(out["status"], plain["status"]) and torch.equal(out["iters"], plain["iters"])
    _compare(_host(torch, out), ref, dtype, 0.05)


@pytest.mark.parametrize("dtype,obs", [("f64", 0), ("f32", 1)])
def test_untouched_states_are_untouched(torch_cuda, gpu_model, oracle, dtype, obs):
    torch = torch_cuda
    B, integ, r, _ = _case(oracle, gpu_model.total_mass, 4, 257, dtype, obs, 45.0)
    solver, _ = _solver(gpu_model, dtype, obs, 257, 45.0)
    dev = Dev(torch, B, dtype, integ, r)
    plain, out = dev.step(solver), dev.step_limited(solver)
    torch.cuda.synchronize()
    zero = out["limited"] == 0
    assert zero.any() and (~zero).any()
    for k in ("tau", "f"):
        assert torch.equal(out[k][:, zero], plain[k][:, zero]), k
    for k in ("status", "iters"):
        assert torch.equal(out[k][zero], plain[k][zero]), k
    assert not torch.equal(out["tau"][:, ~zero], plain["tau"][:, ~zero])
    for k in ("M", "h", "Jc", "pf", "obs_r"):
        assert plain[k] is None or torch.equal(out[k], plain[k]), k
    # no limit at all: nothing is launched, the whole output is the tick's
    solver.set_torque_limits(np.inf)
    free = dev.step_limited(solver)
    torch.cuda.synchronize()
    assert all(torch.equal(free[k], plain[k]) for k in ("tau", "f", "status", "iters")) and not free["limited"].any()
    assert solver.limited_count() == 0
    solver.set_torque_limits(None)    # back to the URDF's 60 N m
    assert solver.model.effort_limits()[0] == 60.0
    back = _host(torch, dev.step_limited(solver))
    assert 0 < (back["limited"] == 1).sum() < (_host(torch, out)["limited"] == 1).sum()


@pytest.mark.parametrize("obs", [0, 1])
def test_post_pass_alone_equals_the_combined_call(torch_cuda, gpu_model, oracle, obs):
    torch = torch_cuda
    B, integ, r, _ = _case(oracle, gpu_model.total_mass, 3, 257, "f64", obs, 45.0)
    solver, _ = _solver(gpu_model, "f64", obs, 257, 45.0)
    dev = Dev(torch, B, "f64", integ, r)
    both = dev.step_limited(solver)
    a = dev.a
    cold = dev.step(solver)
    solver.limit_torques(a["w_des"], a["normals"], a["mu"], dev.mask, cold, obs_r=cold["obs_r"])
    assert _same_bits(torch, cold, both, KEYS)
    # behind a warm-started tick whose sets were carried over from a previous tick of the same states
    first = dev.step(solver, warm=True)
    warm = dev.step(solver, active_in=first["active"].clone())
    solver.limit_torques(a["w_des"], a["normals"], a["mu"], dev.mask, warm, obs_r=warm["obs_r"])
    torch.cuda.synchronize()
    assert torch.equal(warm["limited"], both["limited"]) and torch.equal(warm["status"], both["status"])
    # (a warm start changes the tick's rounding, not its solution: the re-solved states agree to rounding, the untouched ones as the ticks do)
    assert elementwise_excess(to_host(warm["tau"]), to_host(both["tau"])) <= 1.0 and elementwise_excess(to_host(warm["f"]), to_host(both["f"])) <= 1.0


def test_a_list_longer_than_the_grid(torch_cuda, gpu_model, oracle):
    """8 N m: every state is re-solved.  N sits just above the number of wavefronts of limit_qp_kernel's grid (launch.hpp, limit_qp_grid: 16 per compute
    unit), so some wavefronts take a second entry."""
    torch = torch_cuda
    waves = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    assert waves <= 8192
    n = waves + 37
    B = synth.make_batch(4, n, gpu_model.total_mass, rank=3)
    solver, P = _solver(gpu_model, "f64", 0, n, 8.0)
    got = _host(torch, Dev(torch, B, "f64").step_limited(solver))
    assert np.all(got["limited"] == 1) and np.all(got["status"] == 0) and solver.limited_count() == n
    legs = limit_ref.leg_joints(oracle.flat)
    stance = np.zeros((n, 12), bool)
    for k in range(4):
        stance[:, legs[k]] = ((B["mask"] >> k) & 1).astype(bool)[:, None]
    assert (np.abs(got["tau"])[stance]).max() <= 8.0 + P["qp_tol"]
    sub = np.unique(np.concatenate([np.arange(0, n, n // 200), np.arange(n - 56, n)]))[:256]
    Bs = {k: v[sub] for k, v in B.items()}
    ref = limit_ref.step_limited(oracle, P, Bs, 8.0)
    _compare({k: got[k][sub] for k in KEYS}, ref, "f64", 8.0)


def test_order_independence(torch_cuda, gpu_model, oracle):
    torch = torch_cuda
    B, integ, r, _ = _case(oracle, gpu_model.total_mass, 4, 257, "f64", 1, 45.0)
    solver, _ = _solver(gpu_model, "f64", 1, 257, 45.0)
    dev = Dev(torch, B, "f64", integ, r)
    first = dev.step_limited(solver)
    for _ in range(19):
        assert _same_bits(torch, dev.step_limited(solver), first)


def test_capture_and_replay(torch_cuda, gpu_model, oracle):
    torch = torch_cuda
    B, integ, r, _ = _case(oracle, gpu_model.total_mass, 4, 257, "f64", 0, 45.0)
    solver, _ = _solver(gpu_model, "f64", 0, 257, 45.0)
    dev = Dev(torch, B, "f64")
    eager = dev.step_limited(solver)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = dev.step_limited(solver)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.step_limited(solver, out=out)
    solver.set_torque_limits(8.0)   # a captured graph keeps the limits it was captured with
    for _ in range(2):
        for k in KEYS + ("iters",):
            out[k].zero_()
        g.replay()
        assert _same_bits(torch, out, eager)
    assert (_host(torch, dev.step_limited(solver))["limited"] == 1).all()


def test_closed_loop(torch_cuda, gpu_model, oracle):
    """16 robots, 30 ticks of step_limited + wbc_integrate_batch at 30 N m against the same loop on the CPU (the tolerances of the closed-loop scenario
    tests, tests/test_gpu_scenarios.py: q 1e-8, v 1e-7 of the largest entry)."""
    from tests.util import relerr
    torch = torch_cuda
    n, H, lim = 16, 30, 30.0
    B = synth.make_batch(2, n, gpu_model.total_mass, rank=3)
    B["v"] = 0.1 * B["v"]
    solver, P = _solver(gpu_model, "f64", 0, n, lim)
    dev = Dev(torch, B, "f64")
    legs = limit_ref.leg_joints(oracle.flat)
    stance = [j for k in range(4) for j in legs[k]]
    Bo = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in B.items()}
    seen = np.zeros(3, int)
    for t in range(H):
        out = dev.step_limited(solver)
        solver.integrate(dev.a["q"], dev.a["v"], out["M"], out["h"], out["Jc"], out["tau"], out["f"])
        ref = limit_ref.step_limited(oracle, P, Bo, lim)
        limit_ref.integrate(P, ref["dyn"], ref["tau"], ref["f"], Bo["q"], Bo["v"])
        got = _host(torch, out)
        np.testing.assert_array_equal(got["limited"], ref["limited"])
        np.testing.assert_array_equal(got["status"], ref["status"])
        assert np.abs(got["tau"][:, stance]).max() <= lim + P["qp_tol"], t
        seen += np.bincount(ref["limited"], minlength=3)
    assert seen[1] > 0
    assert relerr(to_host(dev.a["q"]), Bo["q"]) < 1e-8 and relerr(to_host(dev.a["v"]), Bo["v"]) < 1e-7
    assert relerr(got["tau"], ref["tau"]) < 1e-7


def test_error_paths(torch_cuda, gpu_model, oracle, hip_lib):
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    B, _, _, _ = _case(oracle, gpu_model.total_mass, 3, 64, "f64", 0, 45.0)
    solver, _ = _solver(gpu_model, "f64", 0, 64, 45.0)
    dev = Dev(torch, B, "f64")
    for bad in (0.0, -1.0, float("nan")):
        lim = np.full(12, 45.0); lim[7] = bad
        with pytest.raises(W.WbcError, match="tau_max"):
            solver.set_torque_limits(lim)
    t = W.TorqueLimits()
    t.struct_size = 8
    assert hip_lib.wbc_solver_set_torque_limits(solver._h, C.byref(t)) == 1 and b"struct_size" in hip_lib.wbc_last_error()
    # no Jc: WBC_E_INVALID before anything is enqueued -- the outputs stay as they were
    out = {k: torch.full((rows, 64), 7.0, dtype=torch.float64, device="cuda") for k, rows in (("tau", 12), ("f", 12))}
    out["status"] = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    out["iters"] = out["status"].clone()
    limited = out["status"].clone()
    bi, bo, ob = solver._batch(64, *dev.args(None, None)[:7], out, None, None, dev.a["tau_prev"], dev.a["f_prev"])
    for fn in (hip_lib.wbc_step_limited_batch, hip_lib.wbc_limit_torques_batch):
        assert fn(solver._h, 64, C.byref(bi), C.byref(bo), C.byref(ob), C.c_void_p(limited.data_ptr()), solver._stream()) == 1
        assert b"Jc" in hip_lib.wbc_last_error()
    torch.cuda.synchronize()
    assert all(bool((out[k] == 7).all()) for k in out) and bool((limited == 7).all())
    assert hip_lib.wbc_step_limited_batch(solver._h, 65, C.byref(bi), C.byref(bo), C.byref(ob), None, solver._stream()) == 7   # WBC_E_CAPACITY
    # an empty batch needs no buffers, as for wbc_step_batch
    zi, zo = W._BatchIn(), W._BatchOut()
    assert hip_lib.wbc_step_batch(solver._h, 0, C.byref(zi), C.byref(zo), None, solver._stream()) == 0
    for fn in (hip_lib.wbc_step_limited_batch, hip_lib.wbc_limit_torques_batch):
        assert fn(solver._h, 0, C.byref(zi), C.byref(zo), None, None, solver._stream()) == 0
