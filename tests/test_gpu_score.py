"""Scored rollouts on the GPU: the on-chip cost against tests/score_ref.py on the CPU oracle's state path, the persistent kernel against
per-tick launches, the caller's loop, fp32, accumulate, the per-group selection, one captured graph, ranking and determinism."""
import ctypes as C

import numpy as np
import pytest

from tests import score_ref
from tests.test_score_host import _goal_near, _random_weights
from tests.util import relerr, to_dev, to_host
from wbc_quadruped_dob_amd import synth

pytestmark = pytest.mark.gpu

TIGHT64 = 1e-9
F32_GATE = 5e-4
ORACLE_GATE = 1e-6   # the rollout gates after 20 compounding ticks are 1e-8 (q, v) and 1e-7 (tau_traj); squares double them; x5 for (p - g_p)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _td(torch, dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def _solver(model, dtype="f64", obs=0, n=64, options=None, weights=None, **kw):
    import wbc_quadruped_dob_amd as W
    P = synth.default_params(observer_order=obs, dtype=dtype)
    P.update(kw)
    s = W.Solver(model, W.Params.from_dict(P, dtype), dtype=dtype, device=0, max_batch=n, options=options or {})
    if weights is not None:
        s.set_score_params(weights)
    return s, P


class Bufs:
    """device buffers of one rollout of batch B (row-per-state numpy in, component-major tensors)"""

    def __init__(self, torch, solver, B, dtype, H, goal, integ=None, plan=None, payload=None, want_traj=False):
        td = _td(torch, dtype)
        dv = lambda a: to_dev(a, torch, td)
        n = self.n = B["q"].shape[0]
        self.torch, self.solver, self.H = torch, solver, H
        self.q, self.v = dv(B["q"]), dv(B["v"])
        self.w_des, self.vdot_des = dv(B["w_des"]), dv(B["vdot_des"])
        self.normals, self.mu = dv(B["normals"]), dv(B["mu"])
        self.mask = torch.from_numpy(np.ascontiguousarray(B["mask"])).to(torch.int32).cuda()
        self.out = dict(tau=torch.zeros((12, n), dtype=td, device="cuda"), f=torch.zeros((12, n), dtype=td, device="cuda"),
                        status=torch.zeros(n, dtype=torch.int32, device="cuda"), iters=torch.zeros(n, dtype=torch.int32, device="cuda"),
                        M=solver.empty(171, n), h=solver.empty(18, n), Jc=solver.empty(216, n), pf=solver.empty(12, n))
        self.ig = None if integ is None else dv(integ)
        self.rr = None if integ is None else torch.zeros((18, n), dtype=td, device="cuda")
        self.plan = None if plan is None else dv(plan)
        self.payload = None if payload is None else dv(payload)
        self.goal = dv(goal)
        self.cost = torch.full((n,), -7.0, dtype=td, device="cuda")   # (a scored call without accumulate must not read it)
        self.fail = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.traj = torch.zeros((H, 12, n), dtype=td, device="cuda") if want_traj else None
        self._saved = None

    def save(self):
        self._saved = [t.clone() for t in self._state()]

    def restore(self):
        for t, s in zip(self._state(), self._saved):
            t.copy_(s)

    def _state(self):
        return [t for t in (self.q, self.v, self.w_des, self.vdot_des, self.out["tau"], self.out["f"], self.ig, self.rr, self.cost, self.fail) if t is not None]

    def scored(self, H=None, accumulate=False):
        return self.solver.rollout_scored(self.H if H is None else H, self.q, self.v, self.normals, self.mu, self.mask, self.out, self.w_des, self.vdot_des,
                                          self.goal, self.cost, self.fail, accumulate=accumulate, plan=self.plan, payload=self.payload,
                                          obs_integ=self.ig, obs_r=self.rr, tau_traj=self.traj)

    def plain(self, H=None):
        H = self.H if H is None else H
        if self.plan is None:
            self.solver.rollout(H, self.q, self.v, self.w_des, self.vdot_des, self.normals, self.mu, self.mask, self.out, self.ig, self.rr, None,
                                self.traj, payload=self.payload)
        else:
            self.solver.rollout_tracking(H, self.q, self.v, self.plan, self.normals, self.mu, self.mask, self.out, self.w_des, self.vdot_des,
                                         self.ig, self.rr, None, self.traj, payload=self.payload)

    def host(self):
        self.torch.cuda.synchronize()
        return dict(cost=self.cost.cpu().numpy().astype(np.float64), fail=self.fail.cpu().numpy(), q=to_host(self.q), v=to_host(self.v),
                    tau=to_host(self.out["tau"]), f=to_host(self.out["f"]), status=self.out["status"].cpu().numpy())


def _oracle_path(oracle, P, B, H, obs, G=None, plan=None):
    """the CPU oracle's state path, one tick per call (everything advances in place); with a plan, its elapsed time advances by dt per tick"""
    n = len(B["q"])
    q, v = B["q"].copy(), B["v"].copy()
    tp, fp = np.zeros((n, 12)), np.zeros((n, 12))
    integ = oracle.dynamics(q, v, nthreads=8)["p"] if obs else None
    r = np.zeros((n, 18)) if obs else None
    path = dict(q=[], v=[], tau=[], f=[], status=[])
    pl = None if plan is None else plan.copy()
    for _ in range(H):
        if pl is None:
            o = oracle.rollout(P, 1, q, v, B["w_des"], B["vdot_des"], B["normals"], B["mu"], B["mask"], None, tp, fp, integ, r, nthreads=8)
        else:
            o = oracle.rollout_tracking(P, G, 1, q, v, pl, B["normals"], B["mu"], B["mask"], None, tp, fp, integ, r, nthreads=8)
            pl[:, 7] += P["dt"]
        for k, a in (("q", q), ("v", v), ("tau", tp), ("f", fp), ("status", o["status"])):
            path[k].append(np.array(a, copy=True))
    return path


def _ref_cost(path, goal, W, **kw):
    return score_ref.rollout_cost(path["q"], path["v"], path["tau"], path["f"], path["status"], goal, W, **kw)


@pytest.mark.parametrize("config,n,H,obs", [(2, 1024, 20, 0), (3, 1000, 20, 1), (4, 333, 7, 2)])
def test_cost_vs_oracle_fp64(torch_cuda, gpu_model, oracle, config, n, H, obs):
    """The cost of the one-launch scored rollout (default options) against score_ref on the CPU oracle's state path.  Gate 1e-6 relative
    (ORACLE_GATE above); fail_ticks equal to the oracle's count exactly."""
    rng = np.random.default_rng(100 + config)
    W = _random_weights(rng)
    solver, P = _solver(gpu_model, obs=obs, n=n, weights=W)
    B = synth.make_batch(config, n, gpu_model.total_mass, rank=40 + config)
    goal = _goal_near(rng, B["q"], B["v"])
    integ = oracle.dynamics(B["q"], B["v"], nthreads=8)["p"] if obs else None
    bufs = Bufs(torch_cuda, solver, B, "f64", H, goal, integ)
    bufs.scored()
    got = bufs.host()
    path = _oracle_path(oracle, P, B, H, obs)
    ref, rfail = _ref_cost(path, goal, W)
    err = relerr(got["cost"], ref)
    per_state = float(np.max(np.abs(got["cost"] - ref) / ref))
    print("scored rollout vs oracle: config %d n %d H %d observer %d: relerr %.3g, worst per-state relative %.3g, failed ticks %d"
          % (config, n, H, obs, err, per_state, int(rfail.sum())))
    assert err < ORACLE_GATE
    assert np.array_equal(got["fail"], rfail)
    assert relerr(got["q"], path["q"][-1]) < 1e-8   # the rollout itself is the existing one


def test_fail_ticks_count_the_gpus_own_status(torch_cuda, gpu_model):
    """max_iter = 1: some ticks end at the iteration limit, and which ones is a property of the solver -- of its warm start too: the one-launch
    kernel starts every tick after the first from the previous tick's active set, a chain of rollout(1) calls starts every tick cold.  So the
    count is compared where the GPU's own per-tick status is known:
    (a) per-tick launches, cold (rollout_persistent = 0, rollout_warm = 0), H = 6: against H x {rollout(1), status};
    (b) the one-launch kernel as six scored launches of one tick with accumulate (each starts cold): against the same chain;
    (c) the one-launch kernel, H = 6 in one launch, w_fail the only weight: cost = w_fail x fail_ticks exactly, the last tick's status is
        counted, and (a horizon of one) fail_ticks = [status != 0]."""
    torch = torch_cuda
    n, H = 256, 6
    W = dict(w_fail=3.0)
    B = synth.make_batch(3, n, gpu_model.total_mass, rank=51)
    goal = _goal_near(np.random.default_rng(51), B["q"], B["v"])

    def chain(solver):
        b = Bufs(torch, solver, B, "f64", H, goal)
        cnt = np.zeros(n, np.int64)
        for _ in range(H):
            b.plain(1)
            cnt += b.host()["status"] != 0
        return cnt

    solver, P = _solver(gpu_model, n=n, options={"rollout_persistent": 0, "rollout_warm": 0}, weights=W, max_iter=1)
    a = Bufs(torch, solver, B, "f64", H, goal)
    a.scored()
    got, cnt = a.host(), chain(solver)
    assert cnt.sum() > 0, "the case is meant to hit the iteration limit"
    assert np.array_equal(got["fail"], cnt) and np.array_equal(got["cost"], 3.0 * cnt)

    solver, P = _solver(gpu_model, n=n, weights=W, max_iter=1)
    cnt = chain(solver)
    b = Bufs(torch, solver, B, "f64", H, goal)
    for k in range(H):
        b.scored(1, accumulate=k > 0)
        if k == 0:
            first = b.host()
            assert np.array_equal(first["fail"], (first["status"] != 0).astype(np.int32)) and first["fail"].sum() > 0
    got = b.host()
    assert np.array_equal(got["fail"], cnt) and np.array_equal(got["cost"], 3.0 * cnt)

    c = Bufs(torch, solver, B, "f64", H, goal)
    c.scored()
    got = c.host()
    assert got["fail"].sum() > 0 and got["fail"].max() <= H
    assert np.array_equal(got["cost"], 3.0 * got["fail"]) and np.all(got["fail"] >= (got["status"] != 0))


@pytest.mark.parametrize("payload", [False, True])
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("spw", [4, 16])
def test_persistent_equals_per_tick(torch_cuda, gpu_model, oracle, spw, track, payload):
    """The cost accumulated inside the persistent kernel against score_tick_kernel behind per-tick launches: 1e-9 relative, fail_ticks equal."""
    from tests import payload_ref
    torch = torch_cuda
    n, H, obs = 77, 8, 1
    rng = np.random.default_rng(61)
    W = _random_weights(rng)
    B = synth.make_batch(3, n, gpu_model.total_mass, rank=61)
    goal = _goal_near(rng, B["q"], B["v"])
    integ = oracle.dynamics(B["q"], B["v"], nthreads=8)["p"]
    plan = synth.make_plan(B, rank=61) if track else None
    pays = payload_ref.random_payloads(np.random.default_rng(61), n, m_max=8.0, c_max=0.15, zero_every=5) if payload else None
    res = {}
    for tag, opt in (("persistent", {"rollout_spw": spw}), ("per_tick", {"rollout_persistent": 0})):
        solver, P = _solver(gpu_model, obs=obs, n=n, options=opt, weights=W)
        if track:
            solver.set_ref_params(synth.default_ref_params())
        bufs = Bufs(torch, solver, B, "f64", H, goal, integ.copy(), plan, pays)
        bufs.scored()
        res[tag] = bufs.host()
    a, b = res["persistent"], res["per_tick"]
    print("persistent vs per-tick cost: spw %d track %d payload %d: %.3g" % (spw, track, payload, relerr(a["cost"], b["cost"])))
    assert relerr(a["q"], b["q"]) < TIGHT64
    assert relerr(a["cost"], b["cost"]) < TIGHT64
    assert np.array_equal(a["fail"], b["fail"])


def test_callers_loop_equals_one_scored_rollout(torch_cuda, gpu_model, oracle):
    """H x {rollout(1), Solver.score(is_last = k == H - 1)} = one rollout_scored(H), within 1e-9."""
    torch = torch_cuda
    n, H = 200, 9
    rng = np.random.default_rng(62)
    W = _random_weights(rng)
    solver, P = _solver(gpu_model, obs=2, n=n, weights=W)
    B = synth.make_batch(4, n, gpu_model.total_mass, rank=62)
    goal = _goal_near(rng, B["q"], B["v"])
    integ = oracle.dynamics(B["q"], B["v"], nthreads=8)["p"]
    a = Bufs(torch, solver, B, "f64", H, goal, integ.copy())
    a.scored()
    one = a.host()
    b = Bufs(torch, solver, B, "f64", H, goal, integ.copy())
    for k in range(H):
        b.plain(1)
        solver.score(b.q, b.v, b.out["tau"], b.out["f"], b.out["status"], b.goal, b.cost, b.fail, accumulate=k > 0, is_last=k == H - 1)
    loop = b.host()
    assert relerr(one["cost"], loop["cost"]) < TIGHT64 and np.array_equal(one["fail"], loop["fail"])


@pytest.mark.parametrize("persistent", [1, 0])
def test_cost_fp32(torch_cuda, gpu_model, oracle, persistent):
    """fp32: the cost against score_ref in float64 on the fp32 solver's OWN per-tick state path (H x rollout(1)): gate 5e-4 -- the accumulation,
    apart from the trajectory divergence that the existing fp32 tests bound."""
    torch = torch_cuda
    n, H = 512, 20
    rng = np.random.default_rng(63)
    W = _random_weights(rng)
    solver, P = _solver(gpu_model, "f32", obs=1, n=n, weights=W, options={"rollout_persistent": persistent})
    B = synth.make_batch(3, n, gpu_model.total_mass, rank=63)
    goal = _goal_near(rng, B["q"], B["v"])
    integ = oracle.dynamics(B["q"], B["v"], nthreads=8)["p"]
    a = Bufs(torch, solver, B, "f32", H, goal, integ.copy())
    a.scored()
    got = a.host()
    b = Bufs(torch, solver, B, "f32", H, goal, integ.copy())
    path = dict(q=[], v=[], tau=[], f=[], status=[])
    for _ in range(H):
        b.plain(1)
        h = b.host()
        for k in path:
            path[k].append(h[k].astype(np.float64) if k != "status" else h[k])
    ref, rfail = _ref_cost(path, goal.astype(np.float32).astype(np.float64), W)
    err = relerr(got["cost"], ref)
    print("fp32 cost vs float64 reference on its own path (persistent %d): %.3g" % (persistent, err))
    assert err < F32_GATE and np.array_equal(got["fail"], rfail)


def test_score_null_is_the_existing_path(torch_cuda, gpu_model, oracle):
    """wbc_rollout_scored_batch with score = NULL (and with score->cost = NULL) for each (plant, plan) combination: bit-identical to the
    matching existing entry point."""
    import wbc_quadruped_dob_amd as W
    from tests import payload_ref
    from wbc_quadruped_dob_amd import _BatchIn, _BatchOut, _ObsState
    torch = torch_cuda
    n, H = 96, 5
    solver, P = _solver(gpu_model, obs=1, n=n)
    solver.set_ref_params(synth.default_ref_params())
    B = synth.make_batch(3, n, gpu_model.total_mass, rank=64)
    goal = np.zeros((n, 10))
    integ = oracle.dynamics(B["q"], B["v"], nthreads=8)["p"]
    pays = payload_ref.random_payloads(np.random.default_rng(64), n, m_max=8.0, c_max=0.15, zero_every=5)
    L = W.lib()
    for track in (False, True):
        for payload in (False, True):
            plan = synth.make_plan(B, rank=64) if track else None
            ref = Bufs(torch, solver, B, "f64", H, goal, integ.copy(), plan, pays if payload else None, want_traj=True)
            ref.plain()
            ref.host()
            for empty_struct in (False, True):
                b = Bufs(torch, solver, B, "f64", H, goal, integ.copy(), plan, pays if payload else None, want_traj=True)
                p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
                bi = _BatchIn(p(b.q), p(b.v), p(b.w_des), p(b.vdot_des), p(b.normals), p(b.mu), p(b.mask), None, None)
                o = b.out
                bo = _BatchOut(p(o["tau"]), p(o["f"]), p(o["status"]), p(o["iters"]), p(o["M"]), p(o["h"]), p(o["Jc"]), p(o["pf"]))
                ob = _ObsState(p(b.ig), p(b.rr))
                pl = solver._plant(None, b.payload, n) if payload else None
                sc = W.RolloutScore()
                sc.struct_size = C.sizeof(W.RolloutScore)
                rc = L.wbc_rollout_scored_batch(solver._h, n, H, C.byref(bi), C.byref(bo), C.byref(ob), C.byref(pl) if pl is not None else None,
                                                p(b.plan), p(b.traj), None, C.byref(sc) if empty_struct else None, solver._stream())
                assert rc == 0
                torch.cuda.synchronize()
                for x, y in ((b.q, ref.q), (b.v, ref.v), (b.traj, ref.traj), (b.rr, ref.rr), (o["tau"], ref.out["tau"]), (o["f"], ref.out["f"]),
                             (o["iters"], ref.out["iters"]), (o["M"], ref.out["M"])):
                    assert torch.equal(x, y), (track, payload, empty_struct)
                assert float(b.cost[0]) == -7.0   # untouched


def test_accumulate_continues_a_horizon(torch_cuda, gpu_model, oracle):
    """Two scored rollouts of 10 ticks, accumulate on the second = score_ref of the 20-tick path with terminal = 1 (persistent and per-tick)."""
    torch = torch_cuda
    n, H = 128, 10
    rng = np.random.default_rng(65)
    W = dict(_random_weights(rng), terminal=1.0)
    B = synth.make_batch(3, n, gpu_model.total_mass, rank=65)
    goal = _goal_near(rng, B["q"], B["v"])
    for opt in ({}, {"rollout_persistent": 0}):
        solver, P = _solver(gpu_model, obs=0, n=n, weights=W, options=opt)
        a = Bufs(torch, solver, B, "f64", H, goal)
        a.scored()
        a.scored(accumulate=True)
        got = a.host()
        if not opt:
            path = _oracle_path(oracle, P, B, 2 * H, 0)
            ref, rfail = _ref_cost(path, goal, W)
        assert relerr(got["cost"], ref) < ORACLE_GATE and np.array_equal(got["fail"], rfail)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("G,K", [(16, 64), (1, 1024), (5, 37), (3, 4096), (1000, 1)])
def test_select_vs_reference(torch_cuda, dtype, G, K):
    """best exactly, weights within 1e-12 (fp64) / 2e-5 absolute (fp32; costs scaled so that (c - c_min) / lambda <= 30: the fp32 rounding of the
    exponent's argument alone is 30 x 6e-8), two launches bit-identical.  Tie / NaN / inf / all-NaN groups are written into the cost buffer."""
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    td = _td(torch, dtype)
    rng = np.random.default_rng(70 + G)
    lam = 0.5
    c = rng.permutation(G * K).astype(np.float64) / max(1, G * K) * 30 * lam + 1.0   # distinct, spread over 30 lambda
    c = c.astype(np.float32 if dtype == "f32" else np.float64).reshape(G, K)
    if K > 1:
        c[0, K // 3] = c[0, K - 1] = c[0].min() - 0.25          # a tie for the minimum: the lowest index
        c[G - 1, 0] = np.nan; c[G - 1, K - 1] = np.inf          # NaN / inf beside finite costs
        if G > 2:
            c[1, :] = np.nan; c[1, K // 2] = np.inf             # nothing finite
    else:
        c[3, 0] = np.nan; c[4, 0] = np.inf
    ct = torch.from_numpy(c.reshape(-1)).cuda()
    rb, rc, rw = score_ref.select(c.astype(np.float64).reshape(-1), K, lam)
    r1 = W.select_rollouts(ct, K, lam, want_weights=True)
    r2 = W.select_rollouts(ct, K, lam, want_weights=True)
    torch.cuda.synchronize()
    assert np.array_equal(r1["best"].cpu().numpy(), rb)
    assert np.array_equal(r1["best_cost"].cpu().numpy().astype(np.float64), rc)
    w = r1["weights"].cpu().numpy().astype(np.float64)
    print("select %s G %d K %d: max weight error %.3g" % (dtype, G, K, np.max(np.abs(w - rw))))
    assert np.max(np.abs(w - rw)) < (1e-12 if dtype == "f64" else 2e-5)
    for k in ("best", "best_cost", "weights"):
        assert torch.equal(r1[k], r2[k]) or (k != "best" and torch.equal(torch.nan_to_num(r1[k]), torch.nan_to_num(r2[k])))
    r0 = W.select_rollouts(ct, K, 0.0, want_weights=True)
    _, _, w0 = score_ref.select(c.astype(np.float64).reshape(-1), K, 0.0)
    assert np.array_equal(r0["weights"].cpu().numpy().astype(np.float64), w0)


def _candidates(gpu_model, oracle, robots, K, seed):
    """robots x K candidates, candidate-minor: the K candidates of a robot share its state and differ only in the plan's goal c1 (within 5 cm
    of the start CoM, at least 1 cm apart); the score goal g_p is candidate `truth`'s c1, moved by the offset between base origin and CoM."""
    rng = np.random.default_rng(seed)
    n = robots * K
    B1 = synth.make_batch(2, robots, gpu_model.total_mass, rank=seed)
    B1["v"][:] = 0.0
    B = {k: np.repeat(v, K, axis=0) for k, v in B1.items()}
    plan1 = synth.make_plan(B1, rank=seed, duration=0.15)
    plan1[:, 7] = 0.0
    plan1[:, 8:12] = B1["q"][:, 3:7]
    com0 = oracle.reference(synth.default_ref_params(), B1["q"], B1["v"], plan1, 0.0)["com"][:, 0:3]
    plan1[:, 0:3] = com0
    plan = np.repeat(plan1, K, axis=0)
    grid = np.array([[x, y, 0.0] for x in (-0.03, -0.01, 0.01, 0.03) for y in (-0.02, 0.02)])[:K]
    step = np.concatenate([grid[rng.permutation(K)] for _ in range(robots)])
    plan[:, 3:6] = plan[:, 0:3] + step
    truth = rng.integers(0, K, robots)
    goal = np.zeros((n, 10))
    goal[:, 3:7] = B["q"][:, 3:7]
    sel = np.arange(robots) * K + truth
    goal[:, 0:3] = np.repeat(B1["q"][:, 0:3] - com0 + plan[sel, 3:6], K, axis=0)
    return B, plan, goal, truth


RANK_H = 150   # (on this seed the CPU reference names the true candidate for 64 of 64 robots at 150 and at 300 ticks)
RANK_W = dict(w_pos=1.0, terminal=10.0, w_fail=0.0)


def test_best_names_the_candidate_that_reaches_the_goal(torch_cuda, gpu_model, oracle):
    """64 robots x 8 candidates that differ only in the plan's goal c1; the score goal g_p is the base position that candidate `truth` steers
    to.  With w_pos only and terminal = 10, best names `truth` for >= 95 % of the robots -- a floor against an inverted sign or a mis-indexed
    group.  The reference itself (oracle.rollout_tracking + score_ref on the same seed) is checked against the same floor first."""
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    robots, K, H = 64, 8, RANK_H
    B, plan, goal, truth = _candidates(gpu_model, oracle, robots, K, 81)
    n = robots * K
    G = synth.default_ref_params()
    P = synth.default_params(observer_order=0)
    path = _oracle_path(oracle, P, B, H, 0, G, plan)
    ref, _ = _ref_cost(path, goal, RANK_W)
    rbest, _, _ = score_ref.select(ref, K)
    ref_rate = float(np.mean(rbest == truth))
    print("ranking: the reference names the true candidate for %.1f %% of the robots" % (100 * ref_rate))
    assert ref_rate >= 0.95
    solver, P = _solver(gpu_model, n=n, weights=RANK_W)
    solver.set_ref_params(G)
    bufs = Bufs(torch, solver, B, "f64", H, goal, None, plan)
    cost = bufs.scored()
    best = W.select_rollouts(cost, K)["best"].cpu().numpy()
    rate = float(np.mean(best == truth))
    print("ranking: the GPU names the true candidate for %.1f %% of the robots" % (100 * rate))
    assert rate >= 0.95
    assert np.mean(best == rbest) >= 0.95


def test_scored_rollout_and_select_replay_from_one_graph(torch_cuda, gpu_model, oracle):
    """rollout_scored (persistent, 64 x 8 candidates, tracking, K different plan goals) + select captured with torch.cuda.graph and replayed
    twice on restored inputs: the same best and the same bits of cost as the eager run."""
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    robots, K, H = 64, 8, 12
    B, plan, goal, truth = _candidates(gpu_model, oracle, robots, K, 82)
    n = robots * K
    solver, P = _solver(gpu_model, n=n, weights=RANK_W)
    solver.set_ref_params(synth.default_ref_params())
    bufs = Bufs(torch, solver, B, "f64", H, goal, None, plan)
    bufs.save()
    bufs.scored()
    eager = W.select_rollouts(bufs.cost, K, 0.5, want_weights=True)
    torch.cuda.synchronize()
    e_cost, e_best, e_w = bufs.cost.clone(), eager["best"].clone(), eager["weights"].clone()
    bufs.restore()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm-up on the side stream (torch's capture recipe)
        bufs.scored()
        W.select_rollouts(bufs.cost, K, 0.5, want_weights=True)
    torch.cuda.current_stream().wait_stream(s)
    bufs.restore()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bufs.scored()
        sel = W.select_rollouts(bufs.cost, K, 0.5, want_weights=True)
    for _ in range(2):
        bufs.restore()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bufs.cost, e_cost) and torch.equal(sel["best"], e_best) and torch.equal(sel["weights"], e_w)


def test_scored_rollout_is_deterministic(torch_cuda, gpu_model, oracle):
    """One scored persistent rollout (1 024 x 20, observer 2) launched 50 times on restored inputs: cost bit-identical (the accumulator sits
    beside LDS hand-overs; an ordering mistake would show here)."""
    torch = torch_cuda
    n, H = 1024, 20
    rng = np.random.default_rng(83)
    solver, P = _solver(gpu_model, obs=2, n=n, weights=_random_weights(rng))
    B = synth.make_batch(4, n, gpu_model.total_mass, rank=83)
    goal = _goal_near(rng, B["q"], B["v"])
    integ = oracle.dynamics(B["q"], B["v"], nthreads=8)["p"]
    bufs = Bufs(torch, solver, B, "f64", H, goal, integ)
    bufs.save()
    first = None
    for _ in range(50):
        bufs.restore()
        bufs.scored()
        torch.cuda.synchronize()
        if first is None:
            first = (bufs.cost.clone(), bufs.fail.clone(), bufs.q.clone())
        else:
            assert torch.equal(bufs.cost, first[0]) and torch.equal(bufs.fail, first[1]) and torch.equal(bufs.q, first[2])
