"""GPU: the base state from leg odometry (wbc_base_estimate_batch, wbc_gait_estimated_odom_batch, wbc_compute_base_estimate) through the C-ABI against
the numpy restatement tests/odom_ref.py: parity in both scalar types on ragged sizes over every branch of the law with and without planes, NaN in
the rows the law must not read, aliased outputs, models whose joint and foot order is not leg-major, the one-robot host form, the parameters,
argument checks, the one launch against the two it replaces, a captured walking tick and the walking closed loop whose controller launches see only
the estimate.

Gates.  odo, the copied rows and the untouched anchor words: exact (bit patterns, NaN included).  p^, v^ and new anchors: util.gate -- fp64
elementwise_excess at the project's standing tolerances (1e-6 of every entry + 1e-9 of the largest); fp32 F32_MARGIN x odom_ref.F32_ERR of the
largest entry, the numpy float32-against-float64 error (tests/test_odom_oracle.py).  Fused against unfused, graph replay against eager: bit for bit.
Closed loop: the integer words of every tick equal the CPU loop's; q, v and base at the end within max(1e-6, 10 A 1e-9), A =
odom_ref.WALK_AMPLIFICATION."""
import functools

import numpy as np
import pytest

from tests import ground_ref as GND, limit_models, odom_ref as R, walk_dev as WD
from tests.util import gate, relerr, to_dev, to_host, torch_dtype as _td

pytestmark = pytest.mark.gpu
SIZES = R.PARITY_SIZES
F32_GATE = {k: R.F32_MARGIN * x for k, x in R.F32_ERR.items()}
JUNK = 7.5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _solver(model, dtype, n, **kw):
    return WD.solver(model, dtype, max_batch=n, dt=R.BRANCH_DT, observer=1, **kw)


_FLATS = {}


@functools.lru_cache(maxsize=None)
def _case(flat_id, n, planes, stand=True):
    """(case, reference in float64): computed once per size, read only"""
    flat, total_mass = _FLATS[flat_id]
    c = R.branch_case(flat, total_mass, n, rank=n, planes=planes, stand=stand)
    return c, R.run(R.params(), flat, c)


def _branch(flat, n, planes):
    _FLATS["synthetic"] = (flat, float(np.sum(flat["mass"])))
    return _case("synthetic", n, planes)


def _ints(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _dev_case(torch, c, dtype):
    td = _td(torch, dtype)
    d = {k: (None if c[k] is None else to_dev(c[k], torch, td)) for k in ("q", "v", "normals", "height", "base", "anchor")}
    d.update({k: _ints(torch, c[k]) for k in ("contact", "mask", "odo")})
    return d


def _estimate(torch, solver, d, alias=False):
    """the call on clones of the in/out buffers -> (host dict, device dict)"""
    n = d["q"].shape[1]
    o = dict(base=d["base"].clone(), anchor=d["anchor"].clone(), odo=d["odo"].clone())
    if alias:
        o.update(q_est=d["q"].clone(), v_est=d["v"].clone())
        q, v = o["q_est"], o["v_est"]
    else:
        o.update(q_est=torch.full_like(d["q"], JUNK), v_est=torch.full_like(d["v"], JUNK))
        q, v = d["q"], d["v"]
    solver.base_estimate(q, v, d["contact"], d["mask"], o["base"], o["anchor"], o["odo"], normals=d["normals"], height=d["height"],
                         q_est=o["q_est"], v_est=o["v_est"])
    torch.cuda.synchronize()
    assert n == o["q_est"].shape[1]
    return {k: (x.cpu().numpy() if k == "odo" else to_host(x)) for k, x in o.items()}, o


def _same_bits(a, b):
    """bit patterns equal (NaN included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(got, c, ref, dtype, n, what="", f32_gate=F32_GATE):
    nd = np.float64 if dtype == "f64" else np.float32
    assert np.array_equal(got["odo"], ref["odo"]), what
    w = R.written(ref)
    assert _same_bits(got["anchor"][~w], c["anchor"].astype(nd)[~w]), what                       # untouched: NaN stays NaN, junk stays junk
    assert _same_bits(got["q_est"][:, 3:], c["q"].astype(nd)[:, 3:]) and _same_bits(got["v_est"][:, 3:], c["v"].astype(nd)[:, 3:]), what
    assert _same_bits(got["q_est"][:, 0:3], got["base"][:, 0:3]) and _same_bits(got["v_est"][:, 0:3], got["base"][:, 3:6]), what
    gate(got["base"][:, 0:3], ref["base"][:, 0:3], dtype, "p", n, f32_gate)
    gate(got["base"][:, 3:6], ref["base"][:, 3:6], dtype, "v", n, f32_gate)
    if w.any():
        gate(got["anchor"][w], ref["anchor"][w], dtype, "anchor", n, f32_gate)


def _f32_gate_of(flat, c, P, ref):
    """the fp32 gate of another model or other gains by the rule of F32_ERR: numpy's float32 against float64 on the same case (not below the recorded
    figures), times the margin"""
    r32 = R.run(P, flat, c, dtype=np.float32)
    w = R.written(ref)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    g = dict(p=rel(r32["base"][:, 0:3], ref["base"][:, 0:3]), v=rel(r32["base"][:, 3:6], ref["base"][:, 3:6]), anchor=rel(r32["anchor"][w], ref["anchor"][w]))
    return {k: R.F32_MARGIN * max(x, R.F32_ERR[k]) for k, x in g.items()}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_base_estimate_parity_over_every_branch(torch_cuda, gpu_model, flat_model, dtype, n):
    torch = torch_cuda
    solver = _solver(gpu_model, dtype, n)
    for planes in (True, False):
        c, ref = _branch(flat_model, n, planes)
        if n >= 16:
            assert R.branches_taken({k: ref[k][:16] for k in ("S", "A", "had")}) == R.ALL_BRANCHES
        got, _ = _estimate(torch, solver, _dev_case(torch, c, dtype))
        _check(got, c, ref, dtype, n, "planes %s" % planes)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_base_rows_are_never_read_and_aliased_outputs_keep_their_rows(torch_cuda, gpu_model, flat_model, dtype):
    """The case carries NaN in rows 0-2 of q and v; with other junk there every output has the same bits.  With q_est = q and v_est = v the rows from
    3 on are not written (they hold what they held) and rows 0-2 receive the estimate."""
    torch = torch_cuda
    n = 33
    c, ref = _branch(flat_model, n, True)
    assert np.all(np.isnan(c["q"][:, 0:3])) and np.all(np.isnan(c["v"][:, 0:3]))
    solver = _solver(gpu_model, dtype, n)
    d = _dev_case(torch, c, dtype)
    got, _ = _estimate(torch, solver, d)
    d2 = dict(d, q=d["q"].clone(), v=d["v"].clone())
    d2["q"][0:3] = 123.0
    d2["v"][0:3] = -45.0
    other, _ = _estimate(torch, solver, d2)
    for key in got:
        assert _same_bits(got[key], other[key]), key
    alias, _ = _estimate(torch, solver, d, alias=True)
    for key in got:
        assert _same_bits(got[key], alias[key]), key
    _check(alias, c, ref, dtype, n, "aliased")


NAMED_FOOT = {"G": "fl_foot", "P": "back_left_foot"}      # feet whose leg joints are NOT the leg-major ones of their row (asserted below)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which", ["G", "P"])
def test_reordered_models(torch_cuda, hip_lib, tmp_path, which, dtype):
    """Joint and foot order not leg-major: parity over the branch case built on that model, and the leg's own joint columns matter -- read leg-major,
    the same inputs give another answer."""
    torch = torch_cuda
    n = 33
    spec = limit_models.specs(tmp_path)[which]
    assert [j for js in spec.legs for j in js] != list(range(12))
    b = spec.feet.index(NAMED_FOOT[which])
    assert spec.legs[b] != [3 * b, 3 * b + 1, 3 * b + 2]
    _FLATS[which] = (spec.flat, spec.total_mass)
    c, ref = _case(which, n, True, False)
    solver = _solver(spec.model, dtype, n)
    got, _ = _estimate(torch, solver, _dev_case(torch, c, dtype))
    _check(got, c, ref, dtype, n, which, _f32_gate_of(spec.flat, c, R.params(), ref))
    # with the joint angles dealt to the legs in leg-major order the feet lie elsewhere
    lever, _ = R.leg_terms(spec.flat, c["q"], c["v"])
    perm = c["q"].copy()
    perm[:, 7:] = c["q"][:, 7 + np.array([j for js in spec.legs for j in js])]
    lever_major, _ = R.leg_terms(spec.flat, perm, c["v"])
    assert np.abs(lever - lever_major).max() > 1e-2


def test_compute_base_estimate_is_the_batch_call_for_one_robot(torch_cuda, gpu_model, flat_model):
    torch = torch_cuda
    c, ref = _branch(flat_model, 16, True)
    solver = _solver(gpu_model, "f64", 1)
    for i in (0, 5, 7, 15):
        one = {k: (x[i:i + 1] if x is not None else None) for k, x in c.items() if k != "dt"}
        got, _ = _estimate(torch, solver, _dev_case(torch, one, "f64"))
        base, anchor, odo, qe, ve = solver.compute_base_estimate(c["q"][i], c["v"][i], int(c["contact"][i]), int(c["mask"][i]), c["base"][i],
                                                                 c["anchor"][i], odo=int(c["odo"][i]), normals=c["normals"][i], height=c["height"][i])
        assert odo == int(ref["odo"][i]) == int(got["odo"][0])
        for mine, theirs in ((base, got["base"][0]), (anchor, got["anchor"][0]), (qe, got["q_est"][0]), (ve, got["v_est"][0])):
            assert _same_bits(mine, theirs)
    # without planes
    c2, ref2 = _branch(flat_model, 16, False)
    base, anchor, odo, qe, ve = solver.compute_base_estimate(c2["q"][6], c2["v"][6], int(c2["contact"][6]), int(c2["mask"][6]), c2["base"][6],
                                                             c2["anchor"][6], odo=int(c2["odo"][6]))
    assert odo == int(ref2["odo"][6])
    gate(base[None], ref2["base"][6:7], "f64", "p", 1, F32_GATE)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_set_odom_params_reaches_the_kernel(torch_cuda, gpu_model, flat_model, dtype):
    torch = torch_cuda
    n = 33
    c, ref = _branch(flat_model, n, True)
    solver = _solver(gpu_model, dtype, n)
    d = _dev_case(torch, c, dtype)
    for P in (R.params(a_v=1.0, a_p=1.0), R.params(a_v=0.5, a_p=0.0)):
        other = R.run(P, flat_model, c)
        assert np.abs(other["base"] - ref["base"]).max() > 1e-3                  # a change that shows
        solver.set_odom_params(P)
        got, _ = _estimate(torch, solver, d)
        _check(got, c, other, dtype, n, str(P), _f32_gate_of(flat_model, c, P, other))
    # a_p = 0: dead reckoning on the new v^, in the device's own arithmetic (one product, one sum: at most one rounding apart when contracted)
    nd = np.float64 if dtype == "f64" else np.float32
    pp = c["base"].astype(nd)[:, 0:3] + nd(c["dt"]) * got["base"][:, 3:6]
    assert np.abs(got["base"][:, 0:3] - pp).max() <= 2 * np.finfo(nd).eps * np.abs(pp).max()
    solver.set_odom_params(R.params())
    got, _ = _estimate(torch, solver, d)
    _check(got, c, ref, dtype, n, "defaults again")


def test_argument_checks_through_the_binding(torch_cuda, gpu_model):
    import ctypes as C
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    solver = _solver(gpu_model, "f64", 16)
    L = W.lib()
    z = lambda r, n=16: torch.zeros((r, n), dtype=torch.float64, device="cuda")
    zi = lambda n=16: torch.zeros(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    q = z(19); q[6] = 1.0; q[2] = 0.4
    nrm = z(12); nrm[2::3] = 1.0
    keep = dict(q=q, v=z(18), cmd=z(4), Jc=z(216), r=z(18), fp=z(12), nrm=nrm, hgt=z(4), w=zi(), phase=z(1), mask=zi(), swing=z(36), base=z(6),
                anchor=z(12), odo=zi(), qe=z(19), ve=z(18))
    est = [p(keep[k]) for k in ("q", "v", "w", "mask", "nrm", "hgt", "base", "anchor", "odo", "qe", "ve")]
    assert L.wbc_base_estimate_batch(solver._h, 0, *([None] * 11), None) == 0
    assert L.wbc_base_estimate_batch(solver._h, 16, *est, None) == 0
    for i in range(11):
        a = list(est); a[i] = None
        assert L.wbc_base_estimate_batch(solver._h, 16, *a, None) == 1, i           # the planes too: one without the other
    a = list(est); a[4] = a[5] = None
    assert L.wbc_base_estimate_batch(solver._h, 16, *a, None) == 0
    assert L.wbc_base_estimate_batch(None, 16, *est, None) == 1
    fused = ([p(keep[k]) for k in ("q", "v", "cmd", "Jc", "r", "fp", "nrm", "w", "phase", "mask", "swing")] + [None, None, p(keep["hgt"])] +
             [p(keep[k]) for k in ("base", "anchor", "odo", "qe", "ve")])
    assert L.wbc_gait_estimated_odom_batch(solver._h, 0, *([None] * 19), None) == 0
    assert L.wbc_gait_estimated_odom_batch(solver._h, 16, *fused, None) == 0
    for i in list(range(11)) + [14, 15, 16, 17, 18]:
        a = list(fused); a[i] = None
        assert L.wbc_gait_estimated_odom_batch(solver._h, 16, *a, None) == 1, i
    a = list(fused); a[13] = None
    assert L.wbc_gait_estimated_odom_batch(solver._h, 16, *a, None) == 0            # height may be NULL
    assert L.wbc_gait_estimated_odom_batch(None, 16, *fused, None) == 1
    torch.cuda.synchronize()
    with pytest.raises(W.WbcError) as e:
        solver.base_estimate(z(19, 17), z(18, 17), zi(17), zi(17), z(6, 17), z(12, 17), zi(17))
    assert e.value.code == 7   # WBC_E_CAPACITY
    with pytest.raises(W.WbcError) as e:
        solver.gait_estimated_odom(z(19, 17), z(18, 17), z(4, 17), z(216, 17), z(18, 17), z(12, 17), z(12, 17), zi(17), z(1, 17), zi(17), z(36, 17),
                                   z(6, 17), z(12, 17), zi(17))
    assert e.value.code == 7
    with pytest.raises(ValueError):
        solver.base_estimate(z(19), z(18), zi(), zi(), None, z(12), zi())
    for bad in (dict(a_v=0.0), dict(a_v=float("nan")), dict(a_p=-0.5), dict(a_p=float("inf")), dict(a_v=1.5)):
        with pytest.raises(W.WbcError):
            solver.set_odom_params(bad)
    assert W.OdomParams.default().as_dict() == R.DEFAULT_PARAMS


# ---- the walking tick on the estimated base state:
#   gait_estimated_odom -> reference_swing(q_est, v_est) -> step(q_est, v_est; observer on) -> integrate_ground_stick(the true q, v)
# The buffers of walk_dev.tick's "estimate" mode (which tau / f pair belongs where: tests/walk_dev.py) + base, odo_anchor, odo in the state and
# q_est, v_est among the buffers.  The first tick of a loop has no step behind it: base_estimate and the plain gait call.
def _walk(torch, model, flat, case, dtype="f64"):
    n = case["q"].shape[0]
    solver = WD.walk_solver(model, flat, n, dtype, observer=1)
    d = WD.buffers(torch, case, "stick", observer=True)
    st = WD.state(torch, case, "stick", observer=solver)
    st["base"] = torch.cat([st["q"][0:3], st["v"][0:3]]).contiguous()
    st["odo_anchor"] = torch.full((12, n), float("nan"), dtype=torch.float64, device="cuda")      # needs no initial value
    st["odo"] = torch.zeros(n, dtype=torch.int32, device="cuda")
    d["q_est"], d["v_est"] = torch.full_like(st["q"], JUNK), torch.full_like(st["v"], JUNK)
    return solver, d, st


def _tick(solver, d, st, k, first=False):
    T = d["tick"]
    a, b = str(k % 2), str((k + 1) % 2)
    tau, f = st["tau" + b], st["f" + b]
    if first:
        solver.base_estimate(st["q"], st["v"], st["contact"], st["mask"], st["base"], st["odo_anchor"], st["odo"], normals=d["normals"],
                             height=d["height"], q_est=d["q_est"], v_est=d["v_est"])
        solver.gait(d["q_est"], d["v_est"], d["cmd"], st["phase"], st["mask"], st["swing"], contact=None, events=d["events"])
    else:
        solver.gait_estimated_odom(st["q"], st["v"], d["cmd"], T["Jc"], st["r"], f, d["normals"], st["contact"], st["phase"], st["mask"], st["swing"],
                                   st["base"], st["odo_anchor"], st["odo"], height=d["height"], q_est=d["q_est"], v_est=d["v_est"],
                                   events=d["events"])
    solver.reference_swing(d["q_est"], d["v_est"], d["plan"], st["mask"], st["swing"], 0.0, out=d["ref"])
    solver.step(d["q_est"], d["v_est"], d["ref"]["w_des"], d["ref"]["vdot_des"], d["normals"], d["mu"], st["mask"], out=dict(T, tau=tau, f=f),
                want_mats=True, tau_prev=st["tau" + a], f_prev=st["f" + a], obs_integ=st["integ"], obs_r=st["r"])
    solver.integrate_ground_stick(st["q"], st["v"], T["M"], T["h"], T["Jc"], tau, d["normals"], d["height"], d["mu"], st["anchor"], st["stick"],
                                  f_gr=d["f_gr"], contact=d["plant_contact"])


@functools.lru_cache(maxsize=None)
def _walk_case(n):
    flat, oracle = _FLATS["walk"]
    return R.walk_case(flat, oracle, n)


FUSED_FROM, FUSED_TICKS = 96, 36      # the bumped feet touch down early in these ticks and the stance pair changes at 127: trust words, anchors and masks change here


@pytest.mark.parametrize("n", SIZES)
def test_gait_estimated_odom_equals_base_estimate_then_gait_estimated(torch_cuda, gpu_model, flat_model, oracle, n):
    """The one launch against the two it replaces, on the walking loop's mid-loop states (the fp64 device loop; the fp32 comparison runs on the same
    states rounded to float32), in both scalar types, with and without height: every output bit for bit.  The plant's base rows are overwritten with
    NaN in the copies both paths read."""
    torch = torch_cuda
    _FLATS["walk"] = (flat_model, oracle)
    case = _walk_case(n)
    solver, d, st = _walk(torch, gpu_model, flat_model, case)
    s32 = WD.walk_solver(gpu_model, flat_model, n, "f32", observer=1)
    swap = WD.terrain_swap(d)
    anchored = False
    for k in range(FUSED_FROM + FUSED_TICKS):
        swap(k)
        if k >= FUSED_FROM:
            for sv, td in ((solver, torch.float64), (s32, torch.float32)):
                cv = lambda t: t.to(td).contiguous() if t.dtype.is_floating_point else t.clone()
                q, v = cv(st["q"]).clone(), cv(st["v"]).clone()          # (cv returns the tensor itself where nothing converts)
                q[0:3] = float("nan")
                v[0:3] = float("nan")
                ins = [q, v, cv(d["cmd"]), cv(d["tick"]["Jc"]), cv(st["r"]), cv(st["f" + str((k + 1) % 2)]), cv(d["normals"])]
                for height in (cv(d["height"]), None):
                    one = dict(contact=st["contact"].clone(), phase=cv(st["phase"]), mask=st["mask"].clone(), swing=cv(st["swing"]),
                               events=torch.full_like(d["events"], -1), f_est=torch.full((12, n), JUNK, dtype=td, device="cuda"),
                               base=cv(st["base"]), anchor=cv(st["odo_anchor"]), odo=st["odo"].clone(),
                               q_est=torch.full((19, n), JUNK, dtype=td, device="cuda"), v_est=torch.full((18, n), JUNK, dtype=td, device="cuda"))
                    two = {key: x.clone() for key, x in one.items()}
                    sv.gait_estimated_odom(*ins, one["contact"], one["phase"], one["mask"], one["swing"], one["base"], one["anchor"], one["odo"],
                                           height=height, q_est=one["q_est"], v_est=one["v_est"], events=one["events"], f_est=one["f_est"])
                    sv.base_estimate(q, v, two["contact"], two["mask"], two["base"], two["anchor"], two["odo"],
                                     normals=None if height is None else ins[6], height=height, q_est=two["q_est"], v_est=two["v_est"])
                    sv.gait_estimated(two["q_est"], two["v_est"], *ins[2:], two["contact"], two["phase"], two["mask"], two["swing"],
                                      events=two["events"], f_est=two["f_est"])
                    torch.cuda.synchronize()
                    for key in one:
                        a, b = one[key].cpu().numpy(), two[key].cpu().numpy()
                        assert _same_bits(a, b), (key, k, str(td), height is None)
                    assert bool(torch.isfinite(one["base"]).all()) and bool(torch.isfinite(one["swing"]).all())
                    anchored = anchored or bool(((one["odo"] >> 4) != 0).any())
        _tick(solver, d, st, k, first=(k == 0))
    torch.cuda.synchronize()
    assert bool((d["tick"]["status"] == 0).all())
    assert anchored                                # the new stance pair takes its anchors in these ticks


def test_captured_walking_tick_replays_bit_for_bit(torch_cuda, gpu_model, flat_model, oracle):
    """gait_estimated_odom -> reference_swing -> step -> integrate_ground_stick at N = 17 as ONE graph: a single chain of launches.  The tau / f pairs
    alternate from tick to tick, so the graph holds the even tick followed by the odd one (eight launches); four replays from the state after two
    eager ticks = eight eager ticks, bit for bit.  A captured graph keeps the gains it was captured with."""
    torch = torch_cuda
    n = 17
    _FLATS["walk"] = (flat_model, oracle)
    case = _walk_case(n)
    solver, d, start = _walk(torch, gpu_model, flat_model, case)
    d["height"] += 1e-3
    _tick(solver, d, start, 0, first=True)
    _tick(solver, d, start, 1)
    torch.cuda.synchronize()
    Jc2 = d["tick"]["Jc"].clone()          # the matrices the second tick left: gait_estimated_odom of the next tick reads Jc
    st = {k: x.clone() for k, x in start.items()}
    for k in range(2, 10):
        _tick(solver, d, st, k)
    torch.cuda.synchronize()
    assert bool((st["odo"] & 15 != 0).any()) and bool((st["r"] != 0).any())
    eager = {k: x.clone() for k, x in st.items()}
    eager.update(f_gr=d["f_gr"].clone(), q_est=d["q_est"].clone(), v_est=d["v_est"].clone())

    def rewind():
        for k in st:
            st[k].copy_(start[k])
        d["tick"]["Jc"].copy_(Jc2)

    def two_ticks():
        _tick(solver, d, st, 2)
        _tick(solver, d, st, 3)

    WD.capture_replay(torch, two_ticks, rewind, 4, lambda: solver.set_odom_params(dict(a_v=1.0, a_p=1.0)))
    for k in st:
        assert _same_bits(st[k].cpu().numpy(), eager[k].cpu().numpy()), k
    assert torch.equal(d["f_gr"], eager["f_gr"]) and torch.equal(d["q_est"], eager["q_est"]) and torch.equal(d["v_est"], eager["v_est"])
    assert not torch.equal(st["q"], start["q"]) and not torch.equal(st["base"], start["base"])


def test_closed_loop_matches_the_cpu_loop(torch_cuda, gpu_model, flat_model, oracle):
    """odom_ref.closed_loop("estimate") on the device, 4 robots, fp64, 512 ticks, the terrain changing under the marked feet at tick 64: mask, events,
    the estimated contact word and the odo word of every tick equal the CPU loop's exactly, every status is 0, and q, v and base at the end agree
    within max(1e-6, 10 A 1e-9).  reference_swing and step are handed q_est and v_est; the plant alone advances the true state."""
    torch = torch_cuda
    n, ticks = R.WALK_N, GND.WALK_TICKS
    case, cpu = R.cpu_walk(flat_model, oracle)
    assert cpu["status_ok"]
    gq, gv = (max(1e-6, 10 * R.WALK_AMPLIFICATION[k] * 1e-9) for k in ("q", "v"))
    assert gq <= 1e-3 and gv <= 1e-3
    solver, d, st = _walk(torch, gpu_model, flat_model, case)
    rec = WD.run_loop(torch, d, ticks, lambda k: _tick(solver, d, st, k, first=(k == 0)), WD.terrain_swap(d),
                      dict(mask=st["mask"], events=d["events"], contact=st["contact"], odo=st["odo"], status=d["tick"]["status"], base=st["base"],
                           q=st["q"]))
    assert np.all(rec["status"] == 0)
    assert np.array_equal(rec["mask"], cpu["masks"]) and np.array_equal(rec["events"], cpu["events"])
    assert np.array_equal(rec["odo"], cpu["odos"])
    assert np.all(rec["contact"][0] == 0) and np.array_equal(rec["contact"][1:], cpu["contacts"][:-1])
    eq, ev = relerr(to_host(st["q"]), cpu["q"]), relerr(to_host(st["v"]), cpu["v"])
    eb = relerr(to_host(st["base"]), cpu["base"])
    print("odometry walking loop: q %.3g (gate %.3g) v %.3g (gate %.3g) base %.3g" % (eq, gq, ev, gv, eb))
    assert eq < gq and ev < gv and eb < gv
    # the estimate's error on the device is the CPU loop's: base after tick k against the state tick k started from
    q_start = np.concatenate([cpu["q0"][None], rec["q"][:-1].transpose(0, 2, 1)])[:, :, 0:3]
    perr = np.abs(rec["base"].transpose(0, 2, 1)[:, :, 0:3] - q_start).max((0, 1))
    print("worst |p^ - p| on the device %s, on the CPU %s" % (perr, np.abs(cpu["perr"]).max((0, 1))))
    assert np.all(perr <= np.asarray(R.PERR_BAND["estimate"]))
