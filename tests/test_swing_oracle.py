"""Swing-foot references without a GPU: the time law, tests/swing_ref.py's kinematics against the CPU oracle, the analytic Jdot v against a
central difference of the oracle's Jacobian, the point of the feature (the commanded foot acceleration is what the written rows produce), a
closed loop of swing_ref + oracle tick + the oracle's integrator restated, and the defaults of wbc_swing_params."""
import ctypes as C

import numpy as np
import pytest

from tests import swing_ref as SR
from tests.payload_ref import integrate_state
from wbc_quadruped_dob_amd import synth


def _sw(p0, p1, hgt, T, t0):
    return np.array([[*p0, *p1, hgt, T, t0]], np.float64)


def test_time_law_ends_apex_and_clamp():
    p0, p1, hgt, T = np.array([0.1, -0.2, 0.0]), np.array([0.25, -0.15, 0.02]), 0.07, 0.3
    sw = _sw(p0, p1, hgt, T, 0.0)
    for t, want in ((0.0, p0), (T, p1), (-0.1, p0), (2 * T, p1)):       # the ends, and the clamp outside [0, 1]
        p, pd, pdd, u = SR.time_law(sw, t)
        assert np.allclose(p[0], want, atol=1e-15) and np.all(pd == 0) and np.all(pdd == 0), t
        assert u[0] == (0.0 if t <= 0 else 1.0)
    p, pd, pdd, u = SR.time_law(sw, T / 2)
    assert abs(u[0] - 0.5) < 1e-15
    assert np.allclose(p[0], 0.5 * (p0 + p1) + [0, 0, hgt], atol=1e-15)   # apex = hgt above the chord's midpoint
    assert abs(pd[0, 2] - 1.875 * (p1 - p0)[2] / T) < 1e-12               # b'(1/2) = 0: only the quintic's s1(1/2) = 15/8 moves z there
    # elapsed time t0 shifts the law; T <= 0 holds the touchdown point
    assert np.allclose(SR.time_law(_sw(p0, p1, hgt, T, 0.1), 0.05)[0], SR.time_law(sw, 0.15)[0], atol=1e-15)
    for Tz in (0.0, -1.0):
        p, pd, pdd, u = SR.time_law(_sw(p0, p1, hgt, Tz, 0.0), 0.01)
        assert np.array_equal(p[0], p1) and np.all(pd == 0) and np.all(pdd == 0) and u[0] == 1.0
    # the derivatives are the derivatives: central differences of p_ref and pd_ref in t
    h = 1e-6
    for t in (0.03, 0.11, 0.2, 0.29):
        p, pd, pdd, _ = SR.time_law(sw, t)
        fd1 = (SR.time_law(sw, t + h)[0] - SR.time_law(sw, t - h)[0]) / (2 * h)
        fd2 = (SR.time_law(sw, t + h)[1] - SR.time_law(sw, t - h)[1]) / (2 * h)
        assert np.abs(fd1 - pd).max() < 1e-8 and np.abs(fd2 - pdd).max() < 1e-6


@pytest.fixture(scope="module")
def batch(flat_model):
    return synth.make_batch(3, 33, float(np.sum(flat_model["mass"])), rank=1)


def test_foot_position_and_velocity_match_the_oracle(flat_model, oracle, batch):
    q, v = batch["q"], batch["v"]
    d = oracle.dynamics(q, v)
    Jc = d["Jc"].reshape(-1, 12, 18)
    for k in range(4):
        K = SR.foot_kin(flat_model, k, q, v)
        assert np.abs(K["pf"] - d["pf"][:, 3 * k:3 * k + 3]).max() < 1e-14
        assert np.abs(K["Jv"] - np.einsum("nij,nj->ni", Jc[:, 3 * k:3 * k + 3], v)).max() < 1e-14
        assert np.abs(K["Jl"] - Jc[:, 3 * k:3 * k + 3][:, :, [6 + j for j in K["joints"]]]).max() < 1e-14


def _plus(q, v, e):
    """q (+) e v, the integrator's configuration update"""
    return np.stack([integrate_state(q[s], v[s], np.zeros(v.shape[1]), e)[0] for s in range(q.shape[0])])


def test_jdot_v_matches_a_central_difference_of_the_oracle_jacobian(flat_model, oracle, batch):
    """Jdot_k v = d/de [J_k(q (+) e v)] v.  Step scan on this batch (33 states, |Jdot v| up to 4.3): worst error 1.2e-5 at e = 1e-3 (truncation, ~e^2),
    1.2e-9 at 1e-5, 1.7e-10 at 3e-6 (the best), 3.1e-10 at 1e-6, 3.1e-9 at 1e-7 (rounding, ~1/e).  Gate: 10 x the best = 1.7e-9; the margin covers the
    seeds not scanned."""
    q, v = batch["q"], batch["v"]
    an = np.concatenate([SR.foot_kin(flat_model, k, q, v)["Jdv"] for k in range(4)], 1)
    best = np.inf
    for e in (1e-5, 3e-6, 1e-6):
        Jp = oracle.dynamics(_plus(q, v, e), v)["Jc"].reshape(-1, 12, 18)
        Jm = oracle.dynamics(_plus(q, v, -e), v)["Jc"].reshape(-1, 12, 18)
        err = np.abs(np.einsum("nij,nj->ni", (Jp - Jm) / (2 * e), v) - an).max()
        print("e %g: %.3g" % (e, err))
        best = min(best, err)
    assert best < 1.7e-9, best


def test_written_rows_realise_the_commanded_foot_acceleration(flat_model, oracle):
    """damping = 0 on well-conditioned legs: J_k vdot + Jdot_k v = a_cmd with vdot = the base rows as given and the rows the call wrote."""
    tm = float(np.sum(flat_model["mass"]))
    c = SR.swing_case(flat_model, tm, 33, rank=5)
    vd, foot, a_cmd = SR.swing_reference(flat_model, c["q"], c["v"], c["mask"], c["swing"], c["t"], c["vdot_des"], dict(damping=0.0), want_acmd=True)
    Jc = oracle.dynamics(c["q"], c["v"])["Jc"].reshape(-1, 12, 18)
    checked = 0
    for k in range(4):
        K = SR.foot_kin(flat_model, k, c["q"], c["v"])
        use = (((c["mask"] >> k) & 1) == 0) & (np.abs(np.linalg.det(K["Jl"])) > 1e-2)
        acc = np.einsum("nij,nj->ni", Jc[:, 3 * k:3 * k + 3], vd) + K["Jdv"]
        assert np.abs(acc[use] - a_cmd[use, k]).max() < 1e-9 * max(1.0, np.abs(a_cmd[use, k]).max())
        checked += int(use.sum())
        # and the stance legs keep what they had
        st = ((c["mask"] >> k) & 1) == 1
        cols = [6 + j for j in K["joints"]]
        assert np.array_equal(vd[st][:, cols], c["vdot_des"][st][:, cols])
    assert checked >= 20
    assert np.array_equal(vd[:, :6], c["vdot_des"][:, :6])


def test_closed_loop_swing_feet_land(flat_model, oracle):
    """4 robots, a diagonal pair in stance, the two lifted feet stepping 6 cm forward in 0.16 s with 5 cm clearance, default gains, dt = 1 ms,
    180 ticks.  Condition: every swing foot ends within 0.1 |p1 - p0| of its touchdown point.  The reference loop meets it with the worst foot at
    0.036 (2.2 mm of 60 mm); at tick 160, right behind touchdown, the worst is 0.026, and it drifts to 0.049 by tick 200 as the trunk, held by two
    point feet, starts to roll."""
    case = SR.loop_case(flat_model, oracle, 4)
    r = SR.closed_loop(flat_model, oracle, case)
    assert r["status_ok"]
    err = SR.landing_errors(case, r["foot"])
    lifted = ((case["mask"][:, None] >> np.arange(4)[None]) & 1) == 0
    assert lifted.sum() == 8
    print("landing errors / step:", np.round(err[lifted], 4))
    assert np.all(err[lifted] < 0.1), err
    assert np.all(err[~lifted] > 0.5)   # the stance feet stayed where they were: the case is not trivially met


def test_swing_params_default(hip_lib):
    import wbc_quadruped_dob_amd as W
    p = W.SwingParams.default()
    assert p.struct_size == C.sizeof(W.SwingParams) == 64
    assert list(p.kp) == [400.0] * 3 and list(p.kd) == [40.0] * 3 and p.damping == 1e-4
    assert all(abs(kd - 2 * np.sqrt(kp)) < 1e-12 for kp, kd in zip(p.kp, p.kd))   # critically damped
    assert SR.DEFAULT_PARAMS == dict(kp=tuple(p.kp), kd=tuple(p.kd), damping=p.damping)
    p = W.SwingParams.from_dict(dict(kp=[1, 2, 3], damping=0.0))
    assert list(p.kp) == [1, 2, 3] and list(p.kd) == [40.0] * 3 and p.damping == 0.0
    with pytest.raises(KeyError):
        W.SwingParams.from_dict(dict(nope=1))
    assert (W.SWING_WORDS, W.FOOT_WORDS) == (SR.SWING_WORDS, SR.FOOT_WORDS) == (36, 24)
