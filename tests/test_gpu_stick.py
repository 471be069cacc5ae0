"""GPU: stiction on the ground plant (wbc_ground_stick_force_batch, wbc_integrate_ground_stick_batch) through the C-ABI against the numpy restatement
tests/stick_ref.py: parity in both scalar types on ragged sizes over every branch of the law, the one-launch plant against the two launches it
replaces and against the reference, the zero-stiffness limit against the stateless ground calls, models whose joint and foot order is not leg-major,
argument checks, the ragged tail, a captured four-call tick, the walking closed loop and the slope hold.

Gates.  stick, contact: exact.  f_gr, gap, anchor, q, v -- fp64: 1e-6 of every entry (util.elementwise_excess, the project's gate).  fp32:
tests/stick_ref.py evaluated in float32 against float64 on this file's parity cases (sizes 1, 15, 16, 17, 33), error relative to the largest entry of
the array: f_gr 1.1e-5, gap 1.3e-5, anchor 6.9e-8 (over the words the law wrote), q 6.5e-8, v 5.4e-7 (stick_ref.F32_ERR, measured on the CPU and
checked by tests/test_stick_oracle.py).  The device contracts products and has its own square root, so the gates are 8 x those, as in
tests/test_gpu_ground.py.  integrate_ground_stick against the reference: the integrator's existing gates, 1e-9 (fp64) and 1e-4 (fp32) of the largest
entry (tests/test_gpu_envelope.py).  Anchor words the law does not move are the input's bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ground_ref as R, limit_models, limit_ref, stick_ref as S, swing_ref as SR, walk_dev as WD
from tests.util import gate as parity_gate, relerr, to_dev, to_host, torch_dtype as _td
from wbc_quadruped_dob_amd import synth

pytestmark = pytest.mark.gpu
SIZES = S.PARITY_SIZES
F32_GATE = {k: 8 * e for k, e in S.F32_ERR.items()}
TIGHT64, F32_DYN = 1e-9, 1e-4     # the integrator's gates of tests/test_gpu_envelope.py
DT = 1e-3                         # synth.default_params' control period
INPUTS = ("q", "v", "normals", "height", "mu", "tau", "tau_ext", "anchor")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


_solver = WD.solver
_gate = functools.partial(parity_gate, f32_gate=F32_GATE)


_FLATS = {}


def _register(name, flat, total_mass):
    _FLATS[name] = (flat, total_mass)
    return name


@functools.lru_cache(maxsize=None)
def _case(flat_id, n):
    """(case, reference: q', v', stick_force's dict, in float64): computed once per (model, size), read only"""
    flat, tm = _FLATS[flat_id]
    c = S.branch_case(flat, tm, n, rank=n)
    ref = S.integrate_ground_stick(R.params(), S.DEFAULT_KT, DT, c["dyn"], c["tau"], c["normals"], c["height"], c["mu"], c["tau_ext"], c["q"], c["v"],
                                   c["anchor"], c["stick"], limit_ref.leg_joints(flat))
    return c, ref


def _dev_case(torch, c, dtype):
    td = _td(torch, dtype)
    d = {k: to_dev(c[k], torch, td) for k in INPUTS}
    d.update({k: to_dev(c["dyn"][k], torch, td) for k in ("M", "h", "Jc")})
    d["stick"] = torch.from_numpy(np.asarray(c["stick"], np.int32)).cuda()
    return d


def _outs(torch, n, dtype):
    """outputs prefilled with recognisable junk: a word the call does not write shows"""
    td = _td(torch, dtype)
    return dict(f_gr=torch.full((12, n), 7.5, dtype=td, device="cuda"), contact=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                gap=torch.full((4, n), 7.5, dtype=td, device="cuda"))


def _force(torch, solver, d, o):
    """the law alone on copies of d's anchor and stick"""
    anchor, stick = d["anchor"].clone(), d["stick"].clone()
    solver.ground_stick_force(d["q"], d["v"], d["Jc"], d["normals"], d["height"], d["mu"], anchor, stick, f_gr=o["f_gr"], contact=o["contact"],
                              gap=o["gap"])
    torch.cuda.synchronize()
    return dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]), anchor=to_host(anchor), stick=stick.cpu().numpy())


def _plant(torch, solver, d, o):
    """the one-launch plant on copies of d's q, v, anchor and stick"""
    q, v, anchor, stick = d["q"].clone(), d["v"].clone(), d["anchor"].clone(), d["stick"].clone()
    solver.integrate_ground_stick(q, v, d["M"], d["h"], d["Jc"], d["tau"], d["normals"], d["height"], d["mu"], anchor, stick, tau_ext=d["tau_ext"],
                                  f_gr=o["f_gr"], contact=o["contact"], gap=o["gap"])
    torch.cuda.synchronize()
    return dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]), anchor=to_host(anchor), stick=stick.cpu().numpy(),
                q=to_host(q), v=to_host(v))


def _gate_law(got, g, anchor_in, dtype, n):
    """stick and contact exact; f_gr, gap gated; the anchor words the law wrote gated, every other one the input's bit for bit"""
    assert np.array_equal(got["stick"], g["stick"]) and np.array_equal(got["contact"], g["contact"])
    _gate(got["f_gr"], g["f_gr"], dtype, "f_gr", n)
    _gate(got["gap"], g["gap"], dtype, "gap", n)
    w = np.repeat(g["loaded"] & (g["slid"] | ~g["had"]), 3, 1)
    assert np.array_equal(got["anchor"][~w], anchor_in[~w])       # unloaded feet and sticking anchored feet
    if w.any():
        _gate(got["anchor"][w], g["anchor"][w], dtype, "anchor", n)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_stick_force_parity_over_every_branch(torch_cuda, gpu_model, flat_model, dtype, n):
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, (_, _, g) = _case(fid, n)
    if n >= 15:
        assert S.branches_taken(g) == S.ALL_BRANCHES
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    got = _force(torch, solver, d, _outs(torch, n, dtype))
    _gate_law(got, g, to_host(d["anchor"]), dtype, n)
    rest = c["kinds"][:, 0] == -1
    if rest.any():      # v_t = 0 exactly with e != 0: the tangential force is the spring's (or its part inside the cone)
        assert np.all(got["f_gr"][rest][:, [0, 1, 3, 4, 6, 7, 9, 10]] != 0)
    # contact and gap are optional
    o = _outs(torch, n, dtype)
    a2, s2 = d["anchor"].clone(), d["stick"].clone()
    solver.ground_stick_force(d["q"], d["v"], d["Jc"], d["normals"], d["height"], d["mu"], a2, s2, f_gr=o["f_gr"], want_contact=False)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(o["f_gr"]), got["f_gr"]) and np.array_equal(to_host(a2), got["anchor"]) and np.array_equal(s2.cpu().numpy(), got["stick"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_integrate_ground_stick_equals_force_then_integrate_and_the_reference(torch_cuda, gpu_model, flat_model, dtype, n):
    """One launch against the two it replaces (ground_stick_force -> integrate(f = f_gr)) on the same inputs, bit for bit, and against stick_ref."""
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, (q_ref, v_ref, g) = _case(fid, n)
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    two = _force(torch, solver, d, _outs(torch, n, dtype))
    q2, v2 = d["q"].clone(), d["v"].clone()
    solver.integrate(q2, v2, d["M"], d["h"], d["Jc"], d["tau"], to_dev(two["f_gr"], torch, _td(torch, dtype)), d["tau_ext"])
    torch.cuda.synchronize()
    two.update(q=to_host(q2), v=to_host(v2))
    one = _plant(torch, solver, d, _outs(torch, n, dtype))
    for k in ("stick", "contact", "f_gr", "gap", "anchor", "q", "v"):
        assert np.array_equal(one[k], two[k]), k
    # against the reference
    _gate_law(one, g, to_host(d["anchor"]), dtype, n)
    eq, ev = relerr(one["q"], q_ref), relerr(one["v"], v_ref)
    print("integrate_ground_stick %s n=%d against stick_ref: q %.3g v %.3g" % (dtype, n, eq, ev))
    tol = TIGHT64 if dtype == "f64" else F32_DYN
    assert eq < tol and ev < tol
    assert not np.array_equal(one["q"], c["q"].astype(one["q"].dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_zero_stiffness_is_the_ground_plant(torch_cuda, gpu_model, flat_model, dtype, n):
    """k_t = 0: both new calls return f_gr, contact, gap and the new q, v of ground_force / integrate_ground on the same inputs, as numbers, for
    random anchors and random incoming stick words; bits 0-3 of the new word = f_n > 0"""
    torch = torch_cuda
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, (_, _, g) = _case(fid, n)
    solver = _solver(gpu_model, dtype, max_batch=n, k_t=0.0)
    d = _dev_case(torch, c, dtype)
    rng = np.random.default_rng(n)
    d["anchor"] = to_dev(rng.uniform(-10, 10, (n, 12)), torch, _td(torch, dtype))
    d["stick"] = torch.from_numpy(rng.integers(0, 1 << 16, n).astype(np.int32)).cuda()
    o = _outs(torch, n, dtype)
    solver.ground_force(d["q"], d["v"], d["Jc"], d["normals"], d["height"], d["mu"], f_gr=o["f_gr"], contact=o["contact"], gap=o["gap"])
    torch.cuda.synchronize()
    ref = dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]))
    got = _force(torch, solver, d, _outs(torch, n, dtype))
    for k in ("f_gr", "contact", "gap"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["stick"] & 0xf, g["stick"] & 0xf)      # (f_n does not depend on k_t)
    q, v, o = d["q"].clone(), d["v"].clone(), _outs(torch, n, dtype)
    solver.integrate_ground(q, v, d["M"], d["h"], d["Jc"], d["tau"], d["normals"], d["height"], d["mu"], tau_ext=d["tau_ext"], f_gr=o["f_gr"],
                            contact=o["contact"], gap=o["gap"])
    torch.cuda.synchronize()
    ref = dict(f_gr=to_host(o["f_gr"]), contact=o["contact"].cpu().numpy(), gap=to_host(o["gap"]), q=to_host(q), v=to_host(v))
    one = _plant(torch, solver, d, _outs(torch, n, dtype))
    for k in ("f_gr", "contact", "gap", "q", "v"):
        assert np.array_equal(one[k], ref[k]), k
    assert np.array_equal(one["stick"], got["stick"])


STRETCH_FOOT = {"G": "rl_foot", "P": "back_right_foot"}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("which", ["G", "P"])
def test_reordered_models_only_the_named_foot_feels_its_anchor(torch_cuda, hip_lib, tmp_path, which, n, dtype):
    """Joint and foot order not leg-major: every foot 5 mm in its ground and slow.  Run A: stick = 0 (every foot drops its anchor where it is).  Run B:
    ONE foot, named, comes with an anchor 1.5 mm away (a spring force of 30 N, inside its cone).  Only that foot's rows of f_gr differ between the
    runs -- the others are equal bit for bit --, its force equals the reference's, only its anchor words stay, and the one-launch plant applies the
    force to that leg (= ground_stick_force -> integrate bit for bit, = stick_ref)."""
    torch = torch_cuda
    spec = limit_models.specs(tmp_path)[which]
    assert [j for js in spec.legs for j in js] != list(range(12))
    b = spec.feet.index(STRETCH_FOOT[which])
    B = synth.make_batch(3, n, spec.total_mass, rank=130)
    q, v = B["q"], 0.05 * B["v"]
    dyn = spec.oracle.dynamics(q, v)
    P = R.params()
    height, anchor = np.zeros((n, 4)), np.full((n, 12), S.JUNK)
    rng = np.random.default_rng(130 + n)
    for k in range(4):
        pf = SR.foot_kin(spec.flat, k, q, v)["pf"]
        nk = B["normals"][:, 3 * k:3 * k + 3]
        assert np.abs(q[:, 0:3] + R.foot_words(dyn["Jc"], v, k, spec.legs)[0] - pf).max() < 1e-12      # row k of the buffers is foot k of the caller's list
        height[:, k] = (nk * pf).sum(1) + 5e-3
        if k == b:
            t = np.cross(nk, rng.normal(size=(n, 3)))
            anchor[:, 3 * k:3 * k + 3] = pf - 1.5e-3 * t / np.linalg.norm(t, axis=1, keepdims=True)
    c = dict(q=q, v=v, normals=B["normals"], height=height, mu=B["mu"], tau=B["tau_prev"], tau_ext=np.zeros((n, 18)), dyn=dyn, anchor=anchor,
             stick=np.full(n, 1 << b, np.int32))
    args = (DT, dyn, c["tau"], c["normals"], height, c["mu"], c["tau_ext"], q, v, anchor)
    qA, vA, gA = S.integrate_ground_stick(P, S.DEFAULT_KT, *args, np.zeros(n, np.int32), spec.legs)
    qB, vB, gB = S.integrate_ground_stick(P, S.DEFAULT_KT, *args, c["stick"], spec.legs)
    m = S.margins(P, gB)
    assert all(x >= 1.0 for x in m.values()) and all(x >= 1.0 for x in S.margins(P, gA).values()), m
    assert np.all(gB["stick"] == 0b1111) and np.all(gB["fn"] > 1.5 * P["f_touch"])       # all loaded, the named foot sticks
    rows = [3 * b, 3 * b + 1, 3 * b + 2]
    assert np.abs(gB["f_gr"][:, rows] - gA["f_gr"][:, rows]).max() > 10 * F32_GATE["f_gr"] * np.abs(gB["f_gr"]).max()
    solver = _solver(spec.model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    dA = dict(d, stick=torch.zeros_like(d["stick"]))
    gotA = _force(torch, solver, dA, _outs(torch, n, dtype))
    gotB = _force(torch, solver, d, _outs(torch, n, dtype))
    assert np.array_equal(np.delete(gotB["f_gr"], rows, 1), np.delete(gotA["f_gr"], rows, 1))
    assert np.abs(gotB["f_gr"][:, rows].astype(np.float64) - gotA["f_gr"][:, rows]).max() > 10 * F32_GATE["f_gr"] * np.abs(gB["f_gr"]).max()
    _gate_law(gotA, gA, to_host(d["anchor"]), dtype, n)
    _gate_law(gotB, gB, to_host(d["anchor"]), dtype, n)
    assert np.array_equal(gotB["anchor"][:, rows], to_host(d["anchor"])[:, rows])          # the named foot's anchor stays
    q2, v2 = d["q"].clone(), d["v"].clone()
    solver.integrate(q2, v2, d["M"], d["h"], d["Jc"], d["tau"], to_dev(gotB["f_gr"], torch, _td(torch, dtype)), d["tau_ext"])
    oneA = _plant(torch, solver, dA, _outs(torch, n, dtype))
    oneB = _plant(torch, solver, d, _outs(torch, n, dtype))
    for k in ("stick", "contact", "f_gr", "gap", "anchor"):
        assert np.array_equal(oneB[k], gotB[k]), k
    assert np.array_equal(oneB["q"], to_host(q2)) and np.array_equal(oneB["v"], to_host(v2))
    tol = TIGHT64 if dtype == "f64" else F32_DYN
    eq, ev = relerr(oneB["q"], qB), relerr(oneB["v"], vB)
    print("reordered %s %s n=%d against stick_ref: q %.3g v %.3g" % (which, dtype, n, eq, ev))
    assert eq < tol and ev < tol and relerr(oneA["v"], vA) < tol
    # ... and the spring reached the plant, at that leg: its joint velocities differ between the runs, in the reference and on the device alike
    cols = [6 + j for j in spec.legs[b]]
    assert relerr(vA, vB) > 100 * tol
    moved = np.abs(oneB["v"][:, cols].astype(np.float64) - oneA["v"][:, cols]).max()
    assert moved > 0.5 * np.abs(vB[:, cols] - vA[:, cols]).max() > 100 * tol


def test_argument_checks_and_parameters(torch_cuda, gpu_model):
    import wbc_quadruped_dob_amd as W
    torch = torch_cuda
    solver = _solver(gpu_model, "f64", max_batch=16)
    L = W.lib()
    z = lambda r, n=16: torch.zeros((r, n), dtype=torch.float64, device="cuda")
    zi = lambda n=16: torch.zeros(n, dtype=torch.int32, device="cuda")
    q = z(19); q[6] = 1.0; q[2] = 0.4
    nrm = z(12); nrm[2::3] = 1.0
    p = lambda t: C.c_void_p(t.data_ptr())
    d = solver.dynamics(q, z(18), want=("M", "h", "Jc"))
    # N = 0: WBC_OK without looking at the buffers
    assert L.wbc_ground_stick_force_batch(solver._h, 0, *([None] * 12)) == 0
    assert L.wbc_integrate_ground_stick_batch(solver._h, 0, *([None] * 16)) == 0
    # each required pointer in turn, anchor and stick among them; contact, gap (and tau_ext) may be NULL
    keep = dict(v=z(18), height=z(4), mu=z(4) + 0.5, f_gr=z(12), tau=z(12), q2=q.clone(), anchor=z(12), stick=zi())      # alive while in use
    full = [p(q), p(keep["v"]), p(d["Jc"]), p(nrm), p(keep["height"]), p(keep["mu"]), p(keep["anchor"]), p(keep["stick"]), p(keep["f_gr"]), None, None]
    assert L.wbc_ground_stick_force_batch(solver._h, 16, *full, None) == 0
    for i in range(9):
        a = list(full); a[i] = None
        assert L.wbc_ground_stick_force_batch(solver._h, 16, *a, None) == 1, i
    assert L.wbc_ground_stick_force_batch(None, 16, *full, None) == 1
    full = [p(keep["q2"]), p(keep["v"]), p(d["M"]), p(d["h"]), p(d["Jc"]), p(keep["tau"]), p(nrm), p(keep["height"]), p(keep["mu"]), None,
            p(keep["anchor"]), p(keep["stick"]), p(keep["f_gr"]), None, None]
    assert L.wbc_integrate_ground_stick_batch(solver._h, 16, *full, None) == 0
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12):
        a = list(full); a[i] = None
        assert L.wbc_integrate_ground_stick_batch(solver._h, 16, *a, None) == 1, i
    assert L.wbc_integrate_ground_stick_batch(None, 16, *full, None) == 1
    with pytest.raises(ValueError):
        solver.ground_stick_force(q, z(18), d["Jc"], nrm, z(4), z(4), None, zi())
    # N > max_batch
    for call in (lambda: solver.ground_stick_force(z(19, 17), z(18, 17), z(216, 17), z(12, 17), z(4, 17), z(4, 17), z(12, 17), zi(17)),
                 lambda: solver.integrate_ground_stick(z(19, 17), z(18, 17), z(171, 17), z(18, 17), z(216, 17), z(12, 17), z(12, 17), z(4, 17), z(4, 17),
                                                       z(12, 17), zi(17))):
        with pytest.raises(W.WbcError) as e:
            call()
        assert e.value.code == 7   # WBC_E_CAPACITY
    # invalid and non-finite parameters; a struct of a smaller build; a valid set is taken
    for bad in (dict(k_t=-1.0), dict(k_t=-1e-9), dict(k_t=float("nan")), dict(k_t=float("inf"))):
        with pytest.raises(W.WbcError):
            solver.set_stiction_params(bad)
    small = W.StictionParams.default(); small.struct_size = 8
    assert L.wbc_solver_set_stiction_params(solver._h, C.byref(small)) == 1
    assert L.wbc_solver_set_stiction_params(solver._h, None) == 1
    assert W.StictionParams.default().as_dict() == dict(k_t=S.DEFAULT_KT)
    assert L.wbc_abi_version() == 10
    solver.set_stiction_params(dict(k_t=0.0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_parameters_reach_the_kernels(torch_cuda, gpu_model, flat_model, dtype):
    """On the branch case of 17 states: a doubled k_t changes f_gr of both calls by more than 10 x the gate and as the reference says; so does a doubled
    k_n through set_ground_params (the new kernels read the ground parameters of the same solver)."""
    torch = torch_cuda
    n = 17
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, (_, _, g) = _case(fid, n)
    legs = limit_ref.leg_joints(flat_model)
    gate = 1e-6 if dtype == "f64" else F32_GATE["f_gr"]
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    base = _force(torch, solver, d, _outs(torch, n, dtype))
    for kt, ground in ((2 * S.DEFAULT_KT, {}), (S.DEFAULT_KT, dict(k_n=2 * R.DEFAULT_PARAMS["k_n"]))):
        solver.set_stiction_params(dict(k_t=kt))
        solver.set_ground_params(ground)
        ref = S.stick_force(R.params(**ground), kt, c["q"], c["v"], c["dyn"]["Jc"], c["normals"], c["height"], c["mu"], c["anchor"], c["stick"], legs)
        assert np.abs(ref["f_gr"] - g["f_gr"]).max() > 10 * gate * np.abs(g["f_gr"]).max()
        for got in (_force(torch, solver, d, _outs(torch, n, dtype)), _plant(torch, solver, d, _outs(torch, n, dtype))):
            assert np.abs(got["f_gr"].astype(np.float64) - base["f_gr"]).max() > 10 * gate * np.abs(g["f_gr"]).max()
            _gate(got["f_gr"], ref["f_gr"], dtype, "f_gr", n)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ragged_tail_writes_nothing_beyond_the_batch(torch_cuda, gpu_model, flat_model, dtype):
    """N = 17: the second workgroup has 15 lanes per leg beyond the batch.  Every buffer the calls write lies in an allocation with 16 more words
    behind it (where the row of a state >= 17 of the LAST row would fall; in any other row it would hit the next row, which the parity asserts).
    Those words and the results' equality with the unpadded call show that the dead lanes store nothing."""
    torch = torch_cuda
    import wbc_quadruped_dob_amd as W
    n, pad = 17, 16
    fid = _register("synthetic", flat_model, gpu_model.total_mass)
    c, _ = _case(fid, n)
    solver = _solver(gpu_model, dtype, max_batch=n)
    d = _dev_case(torch, c, dtype)
    want = _plant(torch, solver, d, _outs(torch, n, dtype))
    want_f = _force(torch, solver, d, _outs(torch, n, dtype))
    td = _td(torch, dtype)

    def padded(t, fill):
        big = torch.full((t.numel() + pad,), fill, dtype=t.dtype, device="cuda")
        big[:t.numel()] = t.reshape(-1)
        return big

    o = _outs(torch, n, dtype)
    for fused in (False, True):
        buf = dict(q=padded(d["q"], 9.5), v=padded(d["v"], 9.5), anchor=padded(d["anchor"], 9.5), stick=padded(d["stick"], -7),
                   f_gr=padded(o["f_gr"], 9.5), contact=padded(o["contact"], -7), gap=padded(o["gap"], 9.5))
        p = lambda t: C.c_void_p(t.data_ptr())
        if fused:
            rc = W.lib().wbc_integrate_ground_stick_batch(solver._h, n, p(buf["q"]), p(buf["v"]), p(d["M"]), p(d["h"]), p(d["Jc"]), p(d["tau"]),
                                                          p(d["normals"]), p(d["height"]), p(d["mu"]), p(d["tau_ext"]), p(buf["anchor"]),
                                                          p(buf["stick"]), p(buf["f_gr"]), p(buf["contact"]), p(buf["gap"]), None)
        else:
            rc = W.lib().wbc_ground_stick_force_batch(solver._h, n, p(buf["q"]), p(buf["v"]), p(d["Jc"]), p(d["normals"]), p(d["height"]), p(d["mu"]),
                                                      p(buf["anchor"]), p(buf["stick"]), p(buf["f_gr"]), p(buf["contact"]), p(buf["gap"]), None)
        torch.cuda.synchronize()
        assert rc == 0
        exp = want if fused else want_f
        for k, t in buf.items():
            tail = t[-pad:].cpu().numpy()
            assert np.all(tail == (-7 if t.dtype == torch.int32 else 9.5)), (k, fused)
            body = t[:-pad].cpu().numpy()
            if k in exp:
                rows = 1 if body.size == n else body.size // n
                assert np.array_equal(body.reshape(rows, n).T.squeeze(), exp[k].squeeze()), (k, fused)
        if not fused:
            assert torch.equal(buf["q"][:-pad].reshape(19, n), d["q"]) and torch.equal(buf["v"][:-pad].reshape(18, n), d["v"])
    assert td == d["q"].dtype


# ---- the four-call tick: gait(contact = last tick's) -> reference_swing -> step -> integrate_ground_stick (walk_dev.tick)
WALK = dict(plant="stick", sense="plant")


def test_captured_four_call_tick_replays_bit_for_bit(torch_cuda, gpu_model, flat_model, oracle):
    """gait -> reference_swing -> step -> integrate_ground_stick at N = 17, captured once: three replays from the same start = three eager ticks, bit
    for bit, anchor and stick included -- the pattern of tests/test_gpu_ground.py."""
    torch = torch_cuda
    n = 17
    case = S.walk_case(flat_model, oracle, n)
    solver = WD.walk_solver(gpu_model, flat_model, n)
    d = WD.buffers(torch, case, "stick")
    start = WD.state(torch, case, "stick")
    st = {k: x.clone() for k, x in start.items()}
    for _ in range(3):
        WD.tick(solver, d, st, **WALK)
    torch.cuda.synchronize()
    assert bool((st["contact"] != 0).all()) and bool(((st["stick"] & 0xf) != 0).all()) and bool((st["anchor"] != 0).any())
    eager = {k: x.clone() for k, x in st.items()}
    eager["f_gr"] = d["f_gr"].clone()
    WD.capture_replay(torch, lambda: WD.tick(solver, d, st, **WALK), WD.rewinder(st, start), 3,
                      lambda: solver.set_stiction_params(dict(k_t=1.0)))   # a captured graph keeps the law it was captured with
    for k in st:
        assert torch.equal(st[k], eager[k]), k
    assert torch.equal(d["f_gr"], eager["f_gr"]) and bool((d["f_gr"] != 0).any())
    assert not torch.equal(st["q"], start["q"])


def test_closed_loop_matches_the_cpu_loop(torch_cuda, gpu_model, flat_model, oracle):
    """The walking loop of tests/test_stick_oracle.py on the device, 16 robots, fp64, 512 ticks: mask, events, contact and stick of every tick equal
    the CPU loop's exactly, every status is 0, and end-of-loop q, v agree within max(1e-6, 10 A 1e-9) of the largest entry = 1e-6 (A = 2.9,
    stick_ref.WALK_AMPLIFICATION = 3 its bound)."""
    torch = torch_cuda
    n, ticks = 16, S.WALK_TICKS
    case, cpu = S.cpu_walk(flat_model, oracle, n)
    assert cpu["status_ok"] and len(cpu["early"]) >= 1
    gate = max(1e-6, 10 * S.WALK_AMPLIFICATION * 1e-9)
    assert gate <= 1e-3
    solver = WD.walk_solver(gpu_model, flat_model, n)
    d = WD.buffers(torch, case, "stick")
    st = WD.state(torch, case, "stick")
    rec = WD.run_loop(torch, d, ticks, lambda k: WD.tick(solver, d, st, **WALK), WD.terrain_swap(d),
                      dict(mask=st["mask"], events=d["events"], contact=st["contact"], stick=st["stick"], status=d["tick"]["status"]))
    assert np.all(rec["status"] == 0)
    assert np.array_equal(rec["mask"], cpu["masks"]) and np.array_equal(rec["events"], cpu["events"])
    assert np.array_equal(rec["contact"], cpu["contacts"]) and np.array_equal(rec["stick"], cpu["sticks"])
    eq, ev = relerr(to_host(st["q"]), cpu["q"]), relerr(to_host(st["v"]), cpu["v"])
    print("walking loop with stiction: q %.3g v %.3g (gate %.3g)" % (eq, ev, gate))
    assert eq < gate and ev < gate


def test_slope_hold(torch_cuda, gpu_model, flat_model, oracle):
    """stick_ref's slope case on the device: one robot, padded to 16 states, 1500 ticks of reference -> step -> integrate_ground_stick at dt = 1e-3.
    The mean foot position (the tick's pf output) moves at most 1e-2 x the CPU-measured viscous drift between ticks 500 and 1499, and no slide bit
    is set from tick 500 on."""
    torch = torch_cuda
    n, ticks = 16, S.SLOPE_TICKS
    case, vis = S.cpu_slope(flat_model, oracle, 0.0)
    viscous = float(np.linalg.norm(S.drift(vis)[0]))
    padded = {k: np.repeat(case[k], n, 0) for k in ("q", "v", "plan", "normals", "height", "mu", "mask", "swing")}
    solver = _solver(gpu_model, "f64", max_batch=n, ref_params=SR.loop_ref_params())
    d = WD.buffers(torch, padded, "stick")
    st = WD.state(torch, padded, "stick")
    ref, tick, q, v = d["ref"], d["tick"], st["q"], st["v"]
    assert bool((st["mask"] == 0b1111).all())
    sticks = torch.zeros((ticks, n), dtype=torch.int32, device="cuda")
    status = torch.zeros((ticks, n), dtype=torch.int32, device="cuda")
    pf_from = None
    for k in range(ticks):
        solver.reference(q, v, d["plan"], 0.0, out=ref)
        solver.step(q, v, ref["w_des"], ref["vdot_des"], d["normals"], d["mu"], st["mask"], out=tick, want_mats=True)
        if k == S.SLOPE_FROM:
            pf_from = tick["pf"].clone()
        solver.integrate_ground_stick(q, v, tick["M"], tick["h"], tick["Jc"], tick["tau"], d["normals"], d["height"], d["mu"], st["anchor"], st["stick"],
                                      f_gr=d["f_gr"], want_contact=False)
        sticks[k].copy_(st["stick"]); status[k].copy_(tick["status"])
    torch.cuda.synchronize()
    mean = lambda t: to_host(t).reshape(n, 4, 3).mean(1)
    moved = np.linalg.norm(mean(tick["pf"]) - mean(pf_from), axis=1)
    sticks = sticks.cpu().numpy()
    _, cpu = S.cpu_slope(flat_model, oracle, S.DEFAULT_KT)
    off = np.abs(mean(pf_from) - cpu["pf"][S.SLOPE_FROM].mean(1)).max()
    print("slope hold on the device: foot drift %.3g m (viscous on the CPU %.3g); mean foot position at tick %d against the CPU loop's %.3g"
          % (moved.max(), viscous, S.SLOPE_FROM, off))
    assert off < 1e-6                                     # (the pf output is this tick's foot positions, and the device loop is the CPU's)
    assert np.all(status.cpu().numpy() == 0)
    assert moved.max() <= 1e-2 * viscous
    assert np.all(sticks[S.SLOPE_FROM:] == 0b1111)
    assert np.all(sticks == sticks[:, :1])                # the 16 copies take the same branches
