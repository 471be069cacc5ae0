"""CPU: the referee of tests/test_gpu_envelope.py on exactly that file's inputs (tests/envelope.py) -- robot states outside the narrow kinematic box of
synth.make_batch.  The inputs are what they claim to be (every quadrant of the device's sincos, both hemispheres of the quaternion sphere, base
positions far from the origin, step angles on both sides of the fp32 quaternion step's switch); the oracle solves every one of them (status 0) and agrees
with the numpy second implementation; and what float32 costs on them is measured HERE, on the CPU, and asserted below the project's fp32 gates, so that
the GPU gates are not taken from the code under test."""
import numpy as np
import pytest

from oracle import crosscheck_np as X
from tests import envelope as E, gait_ref as GR, limit_ref, swing_ref as SR
from tests.util import _obs_state, relerr, unpack_M
from wbc_quadruped_dob_amd import synth

F32_TOL, F32_DYN = 5e-4, 1e-4       # the project's fp32 gates: tau and f against the fp32 oracle; the dynamics outputs


@pytest.fixture(scope="module")
def total_mass(flat_model):
    return float(np.sum(flat_model["mass"]))


def _quadrants(x):
    """reduction count n = rint(x 2 / pi) of the device's sincos and its quadrant n & 3"""
    n = np.rint(np.asarray(x, np.float64) * 0.6366197723675814).astype(np.int64)
    return n, n & 3


def test_wide_batch_is_what_it_claims(total_mass):
    n = 258
    narrow = synth.make_batch(3, n, total_mass, rank=n)
    wide = E.wide_batch(3, n, total_mass, rank=n)
    # what make_batch reaches: reduction counts -1, 0, 1 only, w > 0, x = y = 0
    assert set(np.unique(_quadrants(narrow["q"][:, 7:])[0])) == {-1, 0, 1}
    assert np.all(narrow["q"][:, 6] > 0) and np.all(narrow["q"][:, 0:2] == 0)
    # joints: every reduction count from -14 to 14, so every residue mod 4 with both signs; exact multiples of pi/4 among them, odd ones (ties of rint,
    # |r| = pi/4) and multiples of four (quadrant boundaries)
    cnt, quad = _quadrants(wide["q"][:, 7:])
    assert set(np.unique(cnt)) == set(range(-14, 15))
    assert {(int(s), int(r)) for s, r in zip(np.sign(cnt).ravel(), quad.ravel()) if s} == {(s, r) for s in (-1, 1) for r in range(4)}
    k = wide["q"][:, 7:] / (np.pi / 4)
    snapped = k == np.rint(k)
    assert 0.10 < snapped.mean() < 0.20
    ks = np.rint(k[snapped]).astype(int)
    assert (ks % 2 == 1).sum() > 50 and (ks % 4 == 0).sum() > 20 and ks.min() <= -26 and ks.max() >= 26
    # attitude: unit, both hemispheres, the edge rows
    assert np.allclose(np.linalg.norm(wide["q"][:, 3:7], axis=1), 1.0, atol=1e-15)
    assert 0.35 < (wide["q"][:, 6] < 0).mean() < 0.65
    assert np.array_equal(wide["q"][:5, 3:7], E.EDGE_QUATS) and np.all(wide["q"][:3, 6] == 0)
    R = SR._quat_R(wide["q"][:, 3:7])
    assert np.abs(np.arctan2(R[:, 1, 0], R[:, 0, 0])).max() > 3.0            # yaw over the whole circle
    # position
    assert np.abs(wide["q"][:, 0:2]).max() > 45 and np.abs(wide["q"][:, 0:2]).min() > 1e-3
    # everything else is make_batch's, and a single layer touches only its words
    for key in narrow:
        if key != "q":
            assert np.array_equal(wide[key], narrow[key]), key
    assert np.array_equal(wide["q"][:, 2], narrow["q"][:, 2])
    for layer, cols in (("joints", slice(7, 19)), ("attitude", slice(3, 7)), ("position", slice(0, 2))):
        one = E.wide_batch(3, n, total_mass, rank=n, layers=(layer,))
        rest = np.ones(19, bool); rest[cols] = False
        assert np.array_equal(one["q"][:, cols], wide["q"][:, cols]) and np.array_equal(one["q"][:, rest], narrow["q"][:, rest]), layer


def _sincos_restated(x, sin_flip=lambda q: (q & 2) != 0, cos_flip=lambda q: ((q + 1) & 2) != 0):
    """sincos_t(double) of csrc/dyn_sweep.hip.hpp restated: Cody-Waite reduction (the two fused multiply-adds emulated in extended precision), the
    fdlibm kernels on |r| <= pi/4, the quadrant fix-up on (int)n & 3 -- with the two sign selects as parameters"""
    x = np.asarray(x, np.float64)
    n = np.rint(x * 0.6366197723675814)
    L = np.longdouble
    r = (L(x) - L(n) * L(1.5707963267948966)).astype(np.float64)
    r = (L(r) - L(n) * L(6.123233995736766e-17)).astype(np.float64)
    z = r * r
    ps = np.polyval([1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
                     8.33333333332248946124e-03, -1.66666666666666324348e-01], z)
    sr = r * z * ps + r
    pc = np.polyval([-1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05,
                     -1.38888888888741095749e-03, 4.16666666666666019037e-02], z)
    cr = z * z * pc + (1.0 - 0.5 * z)
    q = n.astype(np.int64) & 3
    s1, c1 = np.where(q & 1, cr, sr), np.where(q & 1, sr, cr)
    return np.where(sin_flip(q), -s1, s1), np.where(cos_flip(q), -c1, c1)


def test_the_wide_joints_tell_a_wrong_quadrant_select_from_the_right_one(total_mass):
    """The arithmetic of the device's fp64 sincos as written, restated on the host: right on the narrow and on the wide joints.  A sign select that is
    wrong in quadrant 2 only (q == 3 for q & 2, or q == 1 for (q + 1) & 2: -1, 0 and 1 reduce to 3, 0, 1) is invisible on synth.make_batch's joints
    and off by 2 on the wide ones.  (q & 1 for q & 2 is already wrong in quadrant 1, which the narrow box reaches: the older parity tests see that one.)"""
    n = 258
    narrow = synth.make_batch(3, n, total_mass, rank=n)["q"][:, 7:]
    wide = E.wide_batch(3, n, total_mass, rank=n)["q"][:, 7:]
    err = lambda x, **kw: max(np.abs(_sincos_restated(x, **kw)[0] - np.sin(x)).max(), np.abs(_sincos_restated(x, **kw)[1] - np.cos(x)).max())
    assert err(narrow) < 2.3e-16 and err(wide) < 2.3e-16
    for kw in (dict(sin_flip=lambda q: q == 3), dict(cos_flip=lambda q: q == 1)):
        assert err(narrow, **kw) < 2.3e-16 and err(wide, **kw) > 1.0
    assert err(narrow, sin_flip=lambda q: (q & 1) != 0) > 1.0


def test_far_joints_are_rounded_to_the_scalar_type():
    for nd, span in ((np.float64, 1e5), (np.float32, 1e4)):
        j = E.far_joints(130, nd, rank=130)
        assert j.dtype == nd and np.abs(j).max() <= span and np.abs(j).max() > 0.98 * span and (j < 0).any()
        assert set(np.unique(_quadrants(j)[1])) == {0, 1, 2, 3}


def test_spin_batch_is_what_it_claims(total_mass):
    for n in (17, 65, 130):
        B = E.spin_batch(4, n, total_mass, rank=n)
        th = np.linalg.norm(B["v"][:, 3:6], axis=1) * B["dt"]
        assert np.allclose(th, B["theta"], atol=1e-12)
        for g in range(0, n - 15, 16):
            t = th[g:g + 16]
            assert t.min() < 0.1 and t.max() > 1.4 and (t < E.SPIN_SWITCH).sum() >= 4 and (t > E.SPIN_SWITCH).sum() >= 4
        assert np.all(B["v"][1:3, 3:6] == 0) and np.all(np.sum(B["q"][1:3, 3:7] ** 2, axis=1) == 1.0)
        assert 0 < E.SPIN_SWITCH - th[3] < 1e-3 and 0 < th[4] - E.SPIN_SWITCH < 1e-3
        assert list(B["quiet"]) == [1, 2, 3, 4]
        # ... also after rounding to float32
        th32 = np.linalg.norm(B["v"][:, 3:6].astype(np.float32).astype(np.float64), axis=1) * float(np.float32(B["dt"]))
        assert th32[3] < E.SPIN_SWITCH < th32[4]


def _sub(n):
    """the states the (slow) numpy model is evaluated on: the first 24 (edge attitudes among them) and every fifth"""
    return sorted(set(range(min(n, 24))) | set(range(0, n, 5)))


@pytest.mark.parametrize("cfg", [2, 3, 4])
def test_oracle_dynamics_agree_with_the_numpy_model_on_wide_states(oracle, flat_model, total_mass, cfg):
    """tests/test_oracle_identities.py::test_property_random_states' tolerances (M 1e-12, h 1e-10, absolute), on the GPU file's states: the exact
    multiples of pi/4 and the half-turn attitudes included."""
    npm = X.NPModel(flat_model)
    for n in E.SIZES:
        B = E.wide_batch(cfg, n, total_mass, rank=n)
        d = oracle.dynamics(B["q"], B["v"])
        M = unpack_M(d["M"])
        for s in _sub(n):
            np.testing.assert_allclose(M[s], npm.mass_matrix(B["q"][s]), atol=1e-12)
            np.testing.assert_allclose(d["h"][s], npm.bias(B["q"][s], B["v"][s]), atol=1e-10)
            Jc, pf = npm.contact_jacobians(B["q"][s])
            np.testing.assert_allclose(d["Jc"][s].reshape(4, 3, 18), Jc, atol=1e-12)
            np.testing.assert_allclose(d["pf"][s].reshape(4, 3), pf, atol=1e-12)


def test_oracle_dynamics_agree_with_the_numpy_model_on_far_joints(oracle, flat_model, total_mass):
    npm = X.NPModel(flat_model)
    B = E.far_batch(4, 130, total_mass, np.float64, rank=130)
    d = oracle.dynamics(B["q"], B["v"])
    M = unpack_M(d["M"])
    for s in _sub(130):
        np.testing.assert_allclose(M[s], npm.mass_matrix(B["q"][s]), atol=1e-12)
        np.testing.assert_allclose(d["h"][s], npm.bias(B["q"][s], B["v"][s]), atol=1e-10)
    P = synth.default_params()
    ref = oracle.step(P, B["q"], B["v"], B["w_des"], B["vdot_des"], B["normals"], B["mu"], B["mask"], B["tau_prev"], B["f_prev"])
    assert np.all(ref["status"] == 0)


def _f32_against_f64(oracle, B, obs, what):
    """the fp32 oracle against the fp64 oracle on one batch: printed, and asserted below the project's fp32 gates"""
    n = B["q"].shape[0]
    f = lambda a: np.ascontiguousarray(a, np.float32)
    d = lambda a: np.ascontiguousarray(a, np.float64)
    res = {}
    for name, c in (("f64", d), ("f32", f)):
        P = synth.default_params(observer_order=obs, dtype=name)
        integ, r = _obs_state(oracle, dict(q=d(B["q"]), v=d(B["v"])), name, obs)
        res[name] = oracle.step(P, c(B["q"]), c(B["v"]), c(B["w_des"]), c(B["vdot_des"]), c(B["normals"]), c(B["mu"]), B["mask"], c(B["tau_prev"]),
                                c(B["f_prev"]), integ, r)
        res[name + "_dyn"] = oracle.dynamics(c(B["q"]), c(B["v"]))
    a, b = res["f32"], res["f64"]
    assert np.all(b["status"] == 0), what          # a condition of the INPUTS: a seed that breaks it is changed, not this line
    flips = int((a["status"] != b["status"]).sum())
    et, ef = relerr(a["tau"], b["tau"]), relerr(a["f"], b["f"])
    ed = {k: relerr(res["f32_dyn"][k], res["f64_dyn"][k]) for k in ("M", "h", "Jc", "pf")}
    print("%-18s n=%-3d fp32 oracle against fp64 oracle: tau %.2g f %.2g flips %d  " % (what, n, et, ef, flips) + "  ".join("%s %.2g" % kv for kv in ed.items()))
    assert flips == 0 and et < F32_TOL and ef < F32_TOL, (what, et, ef, flips)
    assert all(e < F32_DYN for e in ed.values()), (what, ed)
    return et, ef


def test_the_oracle_referees_every_tick_case_and_fp32_stays_below_the_gates(oracle, total_mass):
    """Every tick case of the GPU file (envelope.TICK_CASES): oracle status 0 for every state with at most 20 iterations, and the fp32 oracle within the
    existing fp32 gates of the fp64 oracle (measured on 2 048 wide config-4 states: tau 1.2e-4, f 1.8e-4, Jc 7.0e-6; the narrow envelope gives
    1.4e-4 / 1.7e-4) -- so those gates carry over to the wide states unchanged."""
    worst = [0.0, 0.0]
    for cid, dtype, obs, cfg, n, opt, mats, plan in E.TICK_CASES:
        B = E.wide_batch(cfg, n, total_mass, rank=n)
        P = synth.default_params(observer_order=obs)
        integ, r = _obs_state(oracle, B, "f64", obs)
        ref = oracle.step(P, B["q"], B["v"], B["w_des"], B["vdot_des"], B["normals"], B["mu"], B["mask"], B["tau_prev"], B["f_prev"], integ, r)
        assert np.all(ref["status"] == 0) and ref["iters"].max() <= 20, (cid, ref["iters"].max())
        et, ef = _f32_against_f64(oracle, B, obs, cid)
        worst = [max(worst[0], et), max(worst[1], ef)]
    print("worst over the tick cases: tau %.2g f %.2g (gate %.0e)" % (worst[0], worst[1], F32_TOL))


@pytest.mark.parametrize("cfg", [2, 3, 4])
def test_oracle_status_zero_on_every_size(oracle, total_mass, cfg):
    for n in E.SIZES:
        for layers in (E.LAYERS, ("joints",), ("attitude",), ("position",)):
            B = E.wide_batch(cfg, n, total_mass, rank=n, layers=layers)
            ref = oracle.step(synth.default_params(), B["q"], B["v"], B["w_des"], B["vdot_des"], B["normals"], B["mu"], B["mask"], B["tau_prev"], B["f_prev"])
            assert np.all(ref["status"] == 0), (cfg, n, layers)


def test_fp32_on_far_joints_stays_below_the_gates(oracle, total_mass):
    """float32 inputs rounded first: both oracles see the same numbers, so this is what the fp32 ARITHMETIC costs at +- 1e4 rad"""
    for n in (65, 130):
        _f32_against_f64(oracle, E.far_batch(4, n, total_mass, np.float32, rank=n), 1, "far joints")


def test_f32_swing_constants_are_what_the_restatement_measures(flat_model, total_mass):
    """envelope.F32_SWING (the base of the fp32 swing gates of the GPU file): tests/swing_ref.py in float32 against float64 on the wide cases.  The
    constants are the measured errors rounded up: never below them, never more than twice them.  vdot is three orders above the narrow envelope's
    7.4e-6: random postures put legs next to singular configurations, where the damped inverse amplifies the float32 rounding of J J^T."""
    worst = E.f32_swing_errors(flat_model, total_mass)
    print("swing, float32 against float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= E.F32_SWING[k] <= 2 * v, (k, v)
    for n in E.SIZES:
        c = E.wide_swing_case(flat_model, total_mass, n, rank=n)
        vd, foot = SR.swing_reference(flat_model, c["q"], c["v"], c["mask"], c["swing"], c["t"], c["vdot_des"])
        assert np.all(np.isfinite(vd)) and np.all(np.isfinite(foot))
        for k in range(4):      # the plans still lie around the feet
            assert np.abs(c["swing"][:, 9 * k:9 * k + 3] - foot[:, 6 * k:6 * k + 3]).max() < 0.021


def test_f32_gait_constants_are_what_the_restatement_measures(flat_model, total_mass):
    """envelope.F32_GAIT, as gait_ref.F32_ERR; the wide cases still take every branch of the mask rule for every foot, and at most 2 % of a case has a
    heading too close to undefined to be compared."""
    worst = E.f32_gait_errors(flat_model, total_mass)
    print("gait, float32 against float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= E.F32_GAIT[k] <= 2 * v, (k, v)
    P = GR.params(flat_model)
    for n in E.SIZES + (257,):
        c = E.wide_branch_case(flat_model, total_mass, n, rank=n, P=P)
        assert c["keep"].mean() >= 1 - E.HEADING_SKIP_CAP
        print("gait n=%d: smallest heading norm^2 %.3g, %d skipped" % (n, E.heading_norm2(c["q"]).min(), int((~c["keep"]).sum())))
        if n >= 17:
            assert GR.branches_taken(P, 1e-3, [c]) == GR.ALL_BRANCHES
        r = GR.gait_tick(flat_model, P, 1e-3, c["q"], c["v"], c["cmd"], c["contact"], c["phase"], c["mask"], c["swing"])
        assert np.all(np.isfinite(r[2][c["keep"]]))


def test_f32_reference_constants_and_the_numpy_second_opinion(oracle, flat_model, total_mass):
    """envelope.F32_REFERENCE: the fp32 oracle's reference generator against the fp64 one on the GPU file's cases (states 50 m out, desired attitudes over
    the whole sphere); and the fp64 one against crosscheck_np.reference at 1e-12, the gate of tests/test_reference_oracle.py's comparisons."""
    G = synth.default_ref_params()
    worst = E.f32_reference_errors(oracle, G, total_mass)
    print("reference generator, fp32 oracle against fp64 oracle:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= E.F32_REFERENCE[k] <= 2 * v, (k, v)
    npm = X.NPModel(flat_model)
    for n in E.REFERENCE_SIZES:
        B, plan = E.reference_case(n, total_mass)
        r = oracle.reference(G, B["q"], B["v"], plan, E.REFERENCE_T)
        second = [X.reference(npm, G, B["q"][s], B["v"][s], plan[s], E.REFERENCE_T) for s in range(n)]
        for i, k in enumerate(("w_des", "vdot_des", "com")):
            assert relerr(np.array([x[i] for x in second]), r[k]) < 1e-12, (n, k)


def test_tracking_rollout_case_is_solvable(oracle, total_mass):
    """the tracking rollout of the GPU file: status 0 in every state after 3 ticks, finite"""
    B, plan = E.reference_case(65, total_mass)
    o = E.oracle_rollout(oracle, B, 3, 1, np.float64, plan=plan, G=synth.default_ref_params())
    assert np.all(o["status"] == 0) and np.all(np.isfinite(o["q"])) and np.all(np.isfinite(o["v"]))


def test_limit_reference_sees_both_classes_on_wide_states(oracle, total_mass):
    """the torque-limit case of the GPU file: states within the limits and re-solved states both occur, none within the band of the limit"""
    for dtype, obs in (("f64", 0), ("f64", 1), ("f32", 1)):
        B = E.wide_batch(4, 65, total_mass, rank=65)
        P = synth.default_params(observer_order=obs, dtype=dtype)
        integ, r = _obs_state(oracle, B, dtype, obs)
        ref = limit_ref.step_limited(oracle, P, B, 45.0, np.float64 if dtype == "f64" else np.float32, integ, r)
        assert (ref["limited"] == 0).sum() >= 10 and (ref["limited"] == 1).sum() >= 5, np.bincount(ref["limited"], minlength=3)
        assert ref["margin"].min() > 0.045


def test_numpy_quaternion_step_is_continuous_and_unit_on_spin_batch(total_mass):
    """crosscheck_np.integrate_q, the referee of the device's quaternion step: no seam at theta = 0.5 (where the fp32 kernel switches forms), |q| = 1 to
    1e-15, and omega = 0 returns the attitude bit for bit"""
    B = E.spin_batch(4, 130, total_mass, rank=130)
    dt = B["dt"]
    for s in range(130):
        qn = X.integrate_q(B["q"][s], B["v"][s], dt)
        assert abs(np.linalg.norm(qn[3:7]) - 1.0) < 1e-15
    for s in (1, 2):
        assert np.array_equal(X.integrate_q(B["q"][s], B["v"][s], dt)[3:7], B["q"][s, 3:7])
    q, v = B["q"][7].copy(), B["v"][7].copy()
    ax = v[3:6] / np.linalg.norm(v[3:6])
    lo, hi = (X.integrate_q(q, np.concatenate([v[:3], ax * th / dt, v[6:]]), dt)[3:7] for th in (0.5 - 1e-9, 0.5 + 1e-9))
    assert 0 < np.abs(hi - lo).max() < 2e-9
    # across the switch the step is the same rotation about the same axis: dq (x) q with dq = [sin(th/2) ax, cos(th/2)]
    for th in (0.5 - 5e-4, 0.5, 0.5 + 5e-4):
        got = X.integrate_q(q, np.concatenate([v[:3], ax * th / dt, v[6:]]), dt)[3:7]
        want = X.quat_mul(np.concatenate([np.sin(th / 2) * ax, [np.cos(th / 2)]]), q[3:7])
        assert np.abs(got - want).max() < 1e-15


def test_f32_rollout_errors_on_spin_and_wide_states(oracle, total_mass):
    """The rollouts of the GPU file on the CPU: the fp64 oracle stays finite with status 0 over horizon 2 from spin_batch (dt = 0.02: a closed loop over
    these states is unstable, |v| reaches ~2e3 after two ticks) and horizon 3 from wide states, and the fp32 oracle's end states stay within the fp32
    dynamics gate of it (printed)."""
    for src, H in (("spin", 2), ("wide", 3)):
        for n in (65, 130):
            B = E.spin_batch(4, n, total_mass, rank=n) if src == "spin" else E.wide_batch(4, n, total_mass, rank=n)
            res = E.oracle_rollout(oracle, B, H, 1, np.float64), E.oracle_rollout(oracle, B, H, 1, np.float32)
            assert np.all(res[0]["status"] == 0) and np.all(np.isfinite(res[0]["q"])) and np.all(np.isfinite(res[0]["v"]))
            assert np.array_equal(res[0]["status"], res[1]["status"])
            e = {k: relerr(res[1][k], res[0][k]) for k in ("q", "v", "tau_traj")}
            print("%s rollout n=%d H=%d: fp32 oracle against fp64 oracle %s, max |v| %.3g" % (src, n, H, {k: "%.2g" % x for k, x in e.items()}, np.abs(res[0]["v"]).max()))
            assert e["q"] < F32_DYN and e["v"] < F32_DYN and e["tau_traj"] < F32_TOL
