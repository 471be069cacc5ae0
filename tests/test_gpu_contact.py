"""GPU: contact sensing from the disturbance observer (wbc_contact_estimate_batch, wbc_gait_estimated_batch, wbc_compute_contact_estimate) through the
C-ABI against the numpy restatement tests/contact_ref.py: parity in both scalar types on ragged sizes over every branch of the law, models whose joint
and foot order is not leg-major, the one-launch gait against the two launches it replaces, the in-place word, the parameters, argument checks, a
captured walking tick and the walking closed loop with the observer on and the ESTIMATED word fed to the gait scheduler.

Gates.  contact, singular: exact (the CPU side first asserts the case's decision margins: 1e-6 in float64, 1e-3 in float32 terms).  f_est, fn_est:
util.elementwise_excess at the project's standing tolerances -- fp64 1e-6 of every entry + 1e-9 of the largest; fp32 5e-4 of the largest entry
(DESIGN.md 6).  The adjugate solve needs no more: the worst cond(J_leg) of the cases is 3.7 (contact_ref.COND_MAX = 5), so cond x eps x 10 is 6e-6 in
fp32 and 1e-14 in fp64 (tests/test_contact_oracle.py).  Fused against unfused, graph replay against eager: bit for bit.  Closed loop: words equal at
every tick, q, v at the end within max(1e-6, 10 A 1e-9), A = contact_ref.WALK_AMPLIFICATION."""
import functools

import numpy as np
import pytest

from tests import contact_ref as R, gait_ref as GR, ground_ref as GND, limit_models, limit_ref, walk_dev as WD
from tests.util import elementwise_excess, relerr, to_dev, to_host, torch_dtype as _td
from wbc_quadruped_dob_amd import synth

pytestmark = pytest.mark.gpu
SIZES = R.PARITY_SIZES


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


_solver = functools.partial(WD.solver, observer=1)


_FLATS = {}


@functools.lru_cache(maxsize=None)
def _case(flat_id, n):
    """(case, reference in float64, reference in float32): computed once per size, read only"""
    flat = _FLATS[flat_id]
    legs = limit_ref.leg_joints(flat)
    c = R.branch_case(flat, n, rank=n)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    e64 = R.estimate(R.params(), c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
    e32 = R.estimate(R.params(), f(c["Jc"]), f(c["r"]), f(c["f_prev"]), f(c["normals"]), c["contact"], legs)
    return c, e64, e32


def _branch(flat, n):
    _FLATS["synthetic"] = flat
    return _case("synthetic", n)


def _dev_case(torch, c, dtype):
    td = _td(torch, dtype)
    d = {k: to_dev(c[k], torch, td) for k in ("Jc", "r", "f_prev", "normals")}
    d["contact"] = torch.from_numpy(np.ascontiguousarray(c["contact"], np.int32)).cuda()
    return d


def _outs(torch, n, dtype):
    """outputs prefilled with recognisable junk: a word the call does not write shows"""
    td = _td(torch, dtype)
    return dict(f_est=torch.full((12, n), 7.5, dtype=td, device="cuda"), fn_est=torch.full((4, n), 7.5, dtype=td, device="cuda"),
                singular=torch.full((n,), -1, dtype=torch.int32, device="cuda"))


def _estimate(torch, solver, d, o, contact=None):
    w = d["contact"].clone() if contact is None else contact
    solver.contact_estimate(d["Jc"], d["r"], d["f_prev"], d["normals"], w, f_est=o["f_est"], fn_est=o["fn_est"], singular=o["singular"])
    torch.cuda.synchronize()
    return dict(contact=w.cpu().numpy(), f_est=to_host(o["f_est"]), fn=to_host(o["fn_est"]), singular=o["singular"].cpu().numpy())


def _gate(got, ref, dtype, what, n):
    ex = elementwise_excess(got, ref) if dtype == "f64" else elementwise_excess(got, ref, rtol=0.0, atol_frac=R.F32_GATE)
    print("%s %s n=%d: excess %.3g (max |ref| %.3g, max |diff| %.3g)" % (what, dtype, n, ex, np.abs(ref).max(), np.abs(np.asarray(got, np.float64) - ref).max()))
    assert np.all(np.isfinite(got)), what
    assert ex <= 1.0, (what, ex)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_contact_estimate_parity_over_every_branch(torch_cuda, gpu_model, flat_model, dtype, n):
    torch = torch_cuda
    c, e64, e32 = _branch(flat_model, n)
    P = R.params()
    m64, m32 = R.margins(P, e64), R.margins(P, e32)
    assert m64["thr"] >= R.MARGIN64 and m64["det"] >= R.MARGIN64 and m32["thr"] >= R.MARGIN32 and m32["det"] >= R.MARGIN32
    assert np.array_equal(e32["contact"], e64["contact"]) and np.array_equal(e32["singular"], e64["singular"])
    if n >= 15:
        assert R.branches_taken(P, e64) == R.ALL_BRANCHES
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    got = _estimate(torch, solver, d, _outs(torch, n, dtype))
    assert np.array_equal(got["contact"], e64["contact"]) and np.array_equal(got["singular"], e64["singular"])
    assert np.all(got["contact"] & ~15 == 0x50)                       # bits outside 0-3 are kept
    _gate(got["f_est"], e64["f_est"], dtype, "f_est", n)
    _gate(got["fn"], e64["fn"], dtype, "fn_est", n)
    # a singular leg and a leg with r = 0 get f_est = f_prev exactly
    fp = to_host(d["f_prev"])
    for k in range(4):
        same = (c["kinds"][:, k] == 6) | (c["kinds"][:, k] == 7)
        assert np.array_equal(got["f_est"][same, 3 * k:3 * k + 3], fp[same, 3 * k:3 * k + 3])
    # f_est, fn_est and singular are optional: the word does not depend on them
    w = d["contact"].clone()
    solver.contact_estimate(d["Jc"], d["r"], d["f_prev"], d["normals"], w)
    torch.cuda.synchronize()
    assert np.array_equal(w.cpu().numpy(), got["contact"])
    out = solver.contact_estimate(d["Jc"], d["r"], d["f_prev"], d["normals"], d["contact"].clone(), want_f=True, want_fn=True, want_singular=True)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(out["f_est"]), got["f_est"]) and np.array_equal(to_host(out["fn_est"]), got["fn"])
    assert np.array_equal(out["singular"].cpu().numpy(), got["singular"])


def test_compute_contact_estimate_is_the_batch_call_for_one_robot(torch_cuda, gpu_model, flat_model):
    c, e64, _ = _branch(flat_model, 16)
    solver = _solver(gpu_model, "f64", max_batch=1)
    for i in (0, 5, 6, 15):
        word, fe, fn, sing = solver.compute_contact_estimate(c["Jc"][i], c["r"][i], c["f_prev"][i], c["normals"][i], contact=int(c["contact"][i]))
        assert word == int(e64["contact"][i]) and sing == int(e64["singular"][i])
        assert elementwise_excess(fe, e64["f_est"][i]) <= 1.0 and elementwise_excess(fn, e64["fn"][i]) <= 1.0


NAMED_FOOT = {"G": "fl_foot", "P": "back_left_foot"}      # feet whose leg joints are NOT the leg-major ones of their row (asserted below)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which", ["G", "P"])
def test_reordered_models_only_the_named_foot_responds(torch_cuda, hip_lib, tmp_path, which, dtype):
    """Joint and foot order not leg-major: a residual J_leg^T (50 N n) on the joints of ONE leg, named by its foot, planned forces zero.  Only that
    foot's rows of f_est, only its fn_est and only its contact bit respond, and they equal the reference's, which reads the leg's joint columns by
    the caller's indices."""
    torch = torch_cuda
    n = 17
    spec = limit_models.specs(tmp_path)[which]
    assert [j for js in spec.legs for j in js] != list(range(12))
    b = spec.feet.index(NAMED_FOOT[which])
    B = synth.make_batch(3, n, spec.total_mass, rank=140)
    Jc = spec.oracle.dynamics(B["q"], B["v"])["Jc"]
    Jl = R.leg_block(Jc, b, spec.legs)
    P = R.params()
    assert spec.legs[b] != [3 * b, 3 * b + 1, 3 * b + 2] and np.abs(np.linalg.det(Jl)).min() > 10 * P["det_min"]
    nb = B["normals"][:, 3 * b:3 * b + 3]
    r = np.zeros((n, 18))
    r[:, [6 + j for j in spec.legs[b]]] = np.einsum("nij,ni->nj", Jl, 50.0 * nb)
    c = dict(Jc=Jc, r=r, f_prev=np.zeros((n, 12)), normals=B["normals"], contact=np.zeros(n, np.int32))
    ref = R.estimate(P, c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], spec.legs)
    assert np.all(ref["contact"] == 1 << b) and np.abs(ref["fn"][:, b] - 50.0).max() < 1e-9
    # the own-leg columns matter: read leg-major, the same residual gives another answer
    wrong = R.estimate(P, c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(4)])
    assert np.abs(wrong["f_est"] - ref["f_est"]).max() > 1.0
    solver = _solver(spec.model, dtype, max_batch=n)
    got = _estimate(torch, solver, _dev_case(torch, c, dtype), _outs(torch, n, dtype))
    rows = [3 * b, 3 * b + 1, 3 * b + 2]
    assert np.all(got["contact"] == 1 << b) and np.all((got["singular"] >> b) & 1 == 0) and np.array_equal(got["singular"], ref["singular"])
    assert np.array_equal(np.delete(got["f_est"], rows, 1), np.zeros((n, 9))) and np.array_equal(np.delete(got["fn"], b, 1), np.zeros((n, 3)))
    _gate(got["f_est"], ref["f_est"], dtype, "f_est", n)
    _gate(got["fn"], ref["fn"], dtype, "fn_est", n)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_in_place_word_keeps_the_hysteresis(torch_cuda, gpu_model, flat_model, dtype):
    """Two consecutive calls on the same word: a foot between f_off and f_on keeps its bit either way, and the second call changes nothing."""
    torch = torch_cuda
    n = 16
    c, e64, _ = _branch(flat_model, n)
    legs = limit_ref.leg_joints(flat_model)
    e2 = R.estimate(R.params(), c["Jc"], c["r"], c["f_prev"], c["normals"], e64["contact"], legs)
    assert np.array_equal(e2["contact"], e64["contact"])
    mid = (c["kinds"] == 1) | (c["kinds"] == 4)
    bits = lambda w: ((w[:, None] >> np.arange(4)[None, :]) & 1) == 1
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    word = d["contact"].clone()
    one = _estimate(torch, solver, d, _outs(torch, n, dtype), contact=word)["contact"].copy()
    two = _estimate(torch, solver, d, _outs(torch, n, dtype), contact=word)["contact"]
    assert np.array_equal(one, e64["contact"]) and np.array_equal(two, e2["contact"])
    assert mid.any() and np.array_equal(bits(two)[mid], bits(c["contact"])[mid])
    assert bits(c["contact"])[mid].any() and not bits(c["contact"])[mid].all()        # both ways


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_set_contact_params_reaches_the_kernel(torch_cuda, gpu_model, flat_model, dtype):
    torch = torch_cuda
    n = 16
    c, e64, _ = _branch(flat_model, n)
    legs = limit_ref.leg_joints(flat_model)
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    base = _estimate(torch, solver, d, _outs(torch, n, dtype))
    assert np.array_equal(base["contact"], e64["contact"])
    for P in (R.params(f_on=100.0, f_off=99.0), R.params(f_on=4.0, f_off=4.0), R.params(det_min=1.0)):
        ref = R.estimate(P, c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
        assert not np.array_equal(ref["contact"], e64["contact"]) or not np.array_equal(ref["singular"], e64["singular"])     # a known bit flips
        solver.set_contact_params(P)
        got = _estimate(torch, solver, d, _outs(torch, n, dtype))
        assert np.array_equal(got["contact"], ref["contact"]) and np.array_equal(got["singular"], ref["singular"])
    assert np.all(got["singular"] == 15) and np.array_equal(got["contact"], c["contact"])      # det_min = 1: every leg keeps its bit


def test_argument_checks_through_the_binding(torch_cuda, gpu_model):
    import ctypes as C
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    solver = _solver(gpu_model, "f64", max_batch=16)
    L = W.lib()
    z = lambda r, n=16: torch.zeros((r, n), dtype=torch.float64, device="cuda")
    zi = lambda n=16: torch.zeros(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    q = z(19); q[6] = 1.0; q[2] = 0.4
    keep = dict(q=q, v=z(18), cmd=z(4), Jc=z(216), r=z(18), fp=z(12), nrm=z(12), w=zi(), phase=z(1), mask=zi(), swing=z(36))
    est = [p(keep[k]) for k in ("Jc", "r", "fp", "nrm", "w")] + [None, None, None]
    assert L.wbc_contact_estimate_batch(solver._h, 0, *([None] * 8), None) == 0
    assert L.wbc_contact_estimate_batch(solver._h, 16, *est, None) == 0
    for i in range(5):
        a = list(est); a[i] = None
        assert L.wbc_contact_estimate_batch(solver._h, 16, *a, None) == 1, i
    assert L.wbc_contact_estimate_batch(None, 16, *est, None) == 1
    fused = [p(keep[k]) for k in ("q", "v", "cmd", "Jc", "r", "fp", "nrm", "w", "phase", "mask", "swing")] + [None, None]
    assert L.wbc_gait_estimated_batch(solver._h, 0, *([None] * 13), None) == 0
    assert L.wbc_gait_estimated_batch(solver._h, 16, *fused, None) == 0
    for i in range(11):
        a = list(fused); a[i] = None
        assert L.wbc_gait_estimated_batch(solver._h, 16, *a, None) == 1, i
    assert L.wbc_gait_estimated_batch(None, 16, *fused, None) == 1
    torch.cuda.synchronize()
    for call in (lambda: solver.contact_estimate(z(216, 17), z(18, 17), z(12, 17), z(12, 17), zi(17)),
                 lambda: solver.gait_estimated(z(19, 17), z(18, 17), z(4, 17), z(216, 17), z(18, 17), z(12, 17), z(12, 17), zi(17), z(1, 17), zi(17),
                                               z(36, 17))):
        with pytest.raises(W.WbcError) as e:
            call()
        assert e.value.code == 7   # WBC_E_CAPACITY
    with pytest.raises(ValueError):
        solver.contact_estimate(z(216), z(18), z(12), z(12), None)
    for bad in (dict(f_on=-1.0), dict(f_off=float("nan")), dict(det_min=float("inf")), dict(f_on=5.0, f_off=6.0)):
        with pytest.raises(W.WbcError):
            solver.set_contact_params(bad)
    assert W.ContactParams.default().as_dict() == R.DEFAULT_PARAMS


# ---- the estimated walking tick: gait_estimated -> reference_swing -> step (observer on) -> integrate_ground (walk_dev.tick, which says which
# buffers belong together)
WALK = dict(plant="ground", sense="estimate")


def _walk(torch, model, flat, case):
    """solver, buffers and state of the estimated walking loop"""
    solver = WD.walk_solver(model, flat, case["q"].shape[0], observer=1)
    return solver, WD.buffers(torch, case, "ground", observer=True), WD.state(torch, case, "ground", observer=solver)


@functools.lru_cache(maxsize=None)
def _walk_case(n):
    flat, oracle = _FLATS["walk"]
    return GND.walk_case(flat, oracle, n)


FUSED_FROM, FUSED_TICKS = 96, 12      # the bumped feet touch down early in these ticks (CPU loop: 102, 103): the sensed word decides masks here


@pytest.mark.parametrize("n", SIZES)
def test_gait_estimated_equals_contact_estimate_then_gait(torch_cuda, gpu_model, flat_model, oracle, n):
    """The one launch against the two it replaces, on the walking loop's mid-loop states (the fp64 device loop; the fp32 comparison runs on the same
    states rounded to float32), in both scalar types: phase, mask, swing, events, contact and f_est bit for bit."""
    torch = torch_cuda
    _FLATS["walk"] = (flat_model, oracle)
    case = _walk_case(n)
    solver, d, st = _walk(torch, gpu_model, flat_model, case)
    s32 = WD.walk_solver(gpu_model, flat_model, n, "f32", observer=1)
    swap = WD.terrain_swap(d)
    sensed_mattered = False
    for k in range(FUSED_FROM + FUSED_TICKS):
        swap(k)
        if k >= FUSED_FROM:
            for sv, td in ((solver, torch.float64), (s32, torch.float32)):
                cv = lambda t: t.to(td).contiguous() if t.dtype.is_floating_point else t.clone()
                ins = [cv(x) for x in (st["q"], st["v"], d["cmd"], d["tick"]["Jc"], st["r"], st["f" + str((k + 1) % 2)], d["normals"])]
                one = dict(contact=st["contact"].clone(), phase=cv(st["phase"]), mask=st["mask"].clone(), swing=cv(st["swing"]),
                           events=torch.full_like(d["events"], -1), f_est=torch.full((12, n), 7.5, dtype=td, device="cuda"))
                two = {key: x.clone() for key, x in one.items()}
                blind = {key: x.clone() for key, x in one.items()}
                sv.gait_estimated(*ins, one["contact"], one["phase"], one["mask"], one["swing"], events=one["events"], f_est=one["f_est"])
                sv.contact_estimate(*ins[3:], two["contact"], f_est=two["f_est"])
                sv.gait(ins[0], ins[1], ins[2], two["phase"], two["mask"], two["swing"], contact=two["contact"], events=two["events"])
                sv.gait(ins[0], ins[1], ins[2], blind["phase"], blind["mask"], blind["swing"], contact=None, events=blind["events"])
                torch.cuda.synchronize()
                for key in one:
                    assert torch.equal(one[key], two[key]), (key, k, str(td))
                sensed_mattered = sensed_mattered or not torch.equal(one["mask"], blind["mask"])
        WD.tick(solver, d, st, k=k, first=(k == 0), **WALK)
    torch.cuda.synchronize()
    assert bool((d["tick"]["status"] == 0).all())
    assert sensed_mattered          # robot 0 stands over a bump: its early touchdown falls in these ticks


def test_captured_walking_tick_replays_bit_for_bit(torch_cuda, gpu_model, flat_model, oracle):
    """gait_estimated -> reference_swing -> step -> integrate_ground at N = 17 as ONE graph: a single chain of launches, no parallel branches.  The
    tau / f pairs alternate from tick to tick, so the graph holds the even tick followed by the odd one (eight launches); four replays from the
    state after two eager ticks = eight eager ticks, bit for bit.  The ground lies 1 mm above the feet's starting height, so the plant pushes, and
    the residual is not zero, from the first tick."""
    torch = torch_cuda
    n = 17
    _FLATS["walk"] = (flat_model, oracle)
    case = _walk_case(n)
    solver, d, start = _walk(torch, gpu_model, flat_model, case)
    d["height"] += 1e-3
    WD.tick(solver, d, start, k=0, first=True, **WALK)
    WD.tick(solver, d, start, k=1, **WALK)
    torch.cuda.synchronize()
    Jc2 = d["tick"]["Jc"].clone()          # the matrices the second tick left: gait_estimated of the next tick reads Jc
    st = {k: x.clone() for k, x in start.items()}
    for k in range(2, 10):
        WD.tick(solver, d, st, k=k, **WALK)
    torch.cuda.synchronize()
    assert bool((st["contact"] != 0).all()) and bool((st["r"] != 0).any())
    eager = {k: x.clone() for k, x in st.items()}
    eager["f_gr"] = d["f_gr"].clone()

    def rewind():
        for k in st:
            st[k].copy_(start[k])
        d["tick"]["Jc"].copy_(Jc2)

    def two_ticks():
        WD.tick(solver, d, st, k=2, **WALK)
        WD.tick(solver, d, st, k=3, **WALK)

    WD.capture_replay(torch, two_ticks, rewind, 4,
                      lambda: solver.set_contact_params(dict(f_on=1e5, f_off=1e5)))   # a captured graph keeps the thresholds it was captured with
    for k in st:
        assert torch.equal(st[k], eager[k]), k
    assert torch.equal(d["f_gr"], eager["f_gr"]) and bool((d["f_gr"] != 0).any())
    assert not torch.equal(st["q"], start["q"])


def test_closed_loop_matches_the_cpu_loop(torch_cuda, gpu_model, flat_model, oracle):
    """contact_ref.closed_loop("estimate") on the device, 4 robots, fp64, 512 ticks, the terrain changing under the marked feet at tick 64: mask and
    events of every tick and every estimated word equal the CPU loop's exactly (the word gait_estimated forms at tick k is the one the CPU loop formed
    after step k - 1), every status is 0, the bumped feet land early on the same ticks, and q, v at the end agree within max(1e-6, 10 A 1e-9)."""
    torch = torch_cuda
    n, ticks = R.WALK_N, GND.WALK_TICKS
    case, cpu = R.cpu_walk(flat_model, oracle, "estimate")
    assert cpu["status_ok"] and all(R.first_early(cpu["early"], s, 1) is not None for s in range(0, n, 2))
    gate = max(1e-6, 10 * R.WALK_AMPLIFICATION * 1e-9)
    assert gate <= 1e-3
    solver, d, st = _walk(torch, gpu_model, flat_model, case)
    rec = WD.run_loop(torch, d, ticks, lambda k: WD.tick(solver, d, st, k=k, first=(k == 0), **WALK), WD.terrain_swap(d),
                      dict(mask=st["mask"], events=d["events"], contact=st["contact"], status=d["tick"]["status"], phase=st["phase"]))
    # the word after the last step, as the next tick's gait_estimated would form it
    solver.contact_estimate(d["tick"]["Jc"], st["r"], st["f" + str((ticks - 1) % 2)], d["normals"], st["contact"])
    torch.cuda.synchronize()
    assert np.all(rec["status"] == 0)
    assert np.array_equal(rec["mask"], cpu["masks"]) and np.array_equal(rec["events"], cpu["events"])
    assert np.all(rec["contact"][0] == 0) and np.array_equal(rec["contact"][1:], cpu["contacts"][:-1])
    assert np.array_equal(st["contact"].cpu().numpy(), cpu["contacts"][-1])
    early = GND.early_touchdowns(GR.walk_params(flat_model), rec["phase"], rec["events"])
    assert early == cpu["early"]
    eq, ev = relerr(to_host(st["q"]), cpu["q"]), relerr(to_host(st["v"]), cpu["v"])
    print("estimated walking loop: q %.3g v %.3g (gate %.3g); %d early touchdowns" % (eq, ev, gate, len(early)))
    assert eq < gate and ev < gate
