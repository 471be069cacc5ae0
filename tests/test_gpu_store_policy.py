"""GPU: the one-launch tick's outputs under its store policy (device_types.hpp, store_out).

The tick's pure outputs (M, h, Jc, pf; tau, f, status, iters) may leave the chip by another cache policy than a plain store.  Whatever the
policy, a caller must find EVERY word written, and find it by every way it can look: a copy enqueued right behind the tick on the same stream, a
copy on another stream ordered by an event, and the host after a synchronize -- all three bit for bit the same.  Launches of the same tick give
the same bits, and keep_structural (which skips the structural constants of M / Jc from the second tick into a buffer pair on) leaves the same
M / Jc bits as the default."""
import numpy as np
import pytest

from tests.test_gpu_parity import _solver
from tests.util import to_dev
from wbc_quadruped_dob_amd import synth

pytestmark = pytest.mark.gpu
ROWS = dict(tau=12, f=12, M=171, h=18, Jc=216, pf=12)
ISENT = -123456789   # status / iters never take this value


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _bits(torch, t):
    """the tensor's bytes as integers: NaN-safe, sign-of-zero-exact comparison"""
    return t if t.dtype == torch.int32 else t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _sentinel_out(torch, n, td):
    out = {k: torch.full((r, n), float("nan"), dtype=td, device="cuda") for k, r in ROWS.items()}
    out["status"] = torch.full((n,), ISENT, dtype=torch.int32, device="cuda")
    out["iters"] = torch.full((n,), ISENT, dtype=torch.int32, device="cuda")
    return out


def _untouched(torch, t):
    return int(((t == ISENT) if t.dtype == torch.int32 else torch.isnan(t)).sum())


def _inputs(torch, gpu_model, cfg, n, td, rank):
    B = synth.make_batch(cfg, n, gpu_model.total_mass, rank=rank)
    ins = [to_dev(B[k], torch, td) for k in ("q", "v", "w_des", "vdot_des", "normals", "mu")]
    mask = torch.from_numpy(np.ascontiguousarray(B["mask"])).to(torch.int32).cuda()
    return B, ins, mask


@pytest.mark.parametrize("obs", [0, 1])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [4096, 4095, 1003, 17, 1002])   # (1 002: an even batch with a ragged last workgroup -- the 16-byte stores beside dead lanes)
def test_every_output_word_is_written_and_visible(torch_cuda, gpu_model, n, dtype, obs):
    torch = torch_cuda
    td = torch.float64 if dtype == "f64" else torch.float32
    solver, _ = _solver(gpu_model, dtype=dtype, obs=obs, max_batch=n)
    assert solver.plan_tick(n, want_mats=True)["fused"] == 1            # the default tick at these sizes is the one-launch tick
    B, ins, mask = _inputs(torch, gpu_model, 3 if obs else 2, n, td, rank=n + obs)
    extra = []
    if obs:
        ig = solver.dynamics(ins[0], ins[1], want=("p",))["p"].clone()
        extra = [to_dev(B["tau_prev"], torch, td), to_dev(B["f_prev"], torch, td), ig, torch.zeros_like(ig)]
    out = _sentinel_out(torch, n, td)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()                                            # the sentinels are in place before the tick is enqueued
    res = solver.step(*ins, mask, *extra, out=out, want_mats=True)
    same = {k: v.clone() for k, v in res.items()}                       # (i) same stream, nothing in between
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(side):
        side.wait_event(ev)
        other = {k: v.clone() for k, v in res.items()}                  # (ii) a second stream, ordered by an event
    torch.cuda.synchronize()
    host = {k: v.cpu() for k, v in res.items()}                         # (iii) the host, after a synchronize
    assert set(res) >= set(ROWS) | {"status", "iters"}
    for k in res:
        for tag, got in (("same stream", same[k]), ("second stream", other[k]), ("host", host[k])):
            assert _untouched(torch, got) == 0, (k, tag, _untouched(torch, got))
        assert torch.equal(_bits(torch, same[k]), _bits(torch, other[k])), k
        assert torch.equal(_bits(torch, same[k]).cpu(), _bits(torch, host[k])), k


def test_launches_of_the_same_tick_give_the_same_bits(torch_cuda, gpu_model):
    torch = torch_cuda
    n, td = 4096, torch.float64
    solver, _ = _solver(gpu_model, max_batch=n)
    _, ins, mask = _inputs(torch, gpu_model, 2, n, td, rank=5)
    sets = [_sentinel_out(torch, n, td) for _ in range(2)]
    torch.cuda.synchronize()
    seen = []
    for i in range(50):
        res = solver.step(*ins, mask, out=sets[i & 1], want_mats=True)
        seen.append({k: v.clone() for k, v in res.items()})             # read on the same stream, no synchronize (path (i) above)
    torch.cuda.synchronize()
    for k in seen[0]:
        assert _untouched(torch, seen[0][k]) == 0, k
        ref = _bits(torch, seen[0][k])
        for i in range(1, 50):
            assert torch.equal(ref, _bits(torch, seen[i][k])), (k, i)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_keep_structural_leaves_the_same_matrix_bits(torch_cuda, gpu_model, dtype):
    torch = torch_cuda
    n = 4096
    td = torch.float64 if dtype == "f64" else torch.float32
    _, ins, mask = _inputs(torch, gpu_model, 2, n, td, rank=9)
    got = {}
    for keep in (0, 1):
        solver, _ = _solver(gpu_model, dtype=dtype, max_batch=n, options={"keep_structural": keep})
        out = _sentinel_out(torch, n, td)
        torch.cuda.synchronize()
        ticks = []
        for _ in range(3):                                              # the same buffers: with keep = 1 ticks 2 and 3 skip the constants
            out = solver.step(*ins, mask, out=out, want_mats=True)
            ticks.append({k: out[k].clone() for k in ("M", "Jc")})
        torch.cuda.synchronize()
        got[keep] = ticks
    for t in range(3):
        for k in ("M", "Jc"):
            assert _untouched(torch, got[1][t][k]) == 0, (k, t)
            assert torch.equal(_bits(torch, got[0][t][k]), _bits(torch, got[1][t][k])), (k, t)
