"""Gait scheduler without a GPU: tests/gait_ref.py's schedule with dyadic numbers (exact), duty = 1, latching of the plan words, the foothold against an
independent evaluation with complex numbers, every branch of the late / contact rule, and the closed loop
gait -> oracle.reference -> swing_reference -> oracle.step -> integrator."""
import numpy as np
import pytest

from tests import gait_ref as GR, swing_ref as SR

TROT = (0b1001, 0b0110)


def _standing(flat, n, seed=3):
    G = SR.loop_ref_params()
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 19)); q[:, 2] = 0.40; q[:, 6] = 1.0
    q[:, 7:] = G["q_nom"] + rng.uniform(-0.03, 0.03, (n, 12))
    return q, np.zeros((n, 18))


def _quat_zyx(yaw, pitch, roll):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll)"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def test_exact_schedule_with_dyadic_numbers(flat_model):
    """dt = 2^-10, period = 2^-2, duty = 0.5, offsets {0, .5, .5, 0}, two periods: every mask a diagonal pair, one lift-off and one touchdown per foot
    and period, and the phase back at its start value exactly -- in float64 and in float32."""
    for dtype in (np.float64, np.float32):
        r = GR.exact_schedule(flat_model, dtype, 3)
        assert r["masks"].shape == (512, 3)
        assert np.all(np.isin(r["masks"], TROT))
        # Tick 0 is the start-up: phi' = 2^-8, so feet 1 and 2 find themselves 1/128 into their swing window and lift (a late lift-off, u < late).
        # From tick 1 on a period is 256 ticks, and each foot lifts once and lands once in it.
        assert np.all(r["events"][0] == 0b0110)
        for lo, hi in ((1, 257), (257, 512)):
            ev = r["events"][lo:hi]
            for k in range(4):
                assert np.all(((ev >> k) & 1).sum(0) == 1) and np.all(((ev >> (4 + k)) & 1).sum(0) == 1), (lo, k)
        assert np.array_equal(r["phase"], r["phase0"]) and r["phase"].dtype == dtype
        # the pairs alternate: feet {1, 2} swing through the first half period
        assert np.all(r["masks"][:127] == 0b1001) and np.all(r["masks"][127:255] == 0b0110) and np.all(r["masks"][255:383] == 0b1001)
    a, b = GR.exact_schedule(flat_model, np.float64, 3), GR.exact_schedule(flat_model, np.float32, 3)
    assert np.array_equal(a["masks"], b["masks"]) and np.array_equal(a["events"], b["events"])


def test_duty_one_never_lifts_and_never_touches_swing(flat_model):
    q, v = _standing(flat_model, 4)
    P = GR.params(flat_model, duty=(1.0, 0.5, 1.0, 0.5), **{k: GR.DYADIC[k] for k in ("period", "offset")})
    rng = np.random.default_rng(0)
    swing0 = rng.uniform(-1, 1, (4, 36))
    phase, mask, swing = np.zeros(4), np.full(4, 0b1111, np.int32), swing0.copy()
    cmd = np.tile([0.2, 0.0, 0.0, -0.05], (4, 1))
    lifted = np.zeros(4, int)
    for _ in range(512):
        phase, mask, swing, ev = GR.gait_tick(flat_model, P, GR.DYADIC_DT, q, v, cmd, None, phase, mask, swing)
        assert np.all(mask & 0b0101 == 0b0101) and np.all(ev & 0b01010101 == 0)
        lifted |= ev
    assert np.all(lifted & 0b1010 == 0b1010)       # the other two feet did walk
    for k in (0, 2):
        assert np.array_equal(swing[:, 9 * k:9 * k + 9], swing0[:, 9 * k:9 * k + 9])
    for k in (1, 3):
        assert not np.array_equal(swing[:, 9 * k:9 * k + 9], swing0[:, 9 * k:9 * k + 9])


@pytest.mark.parametrize("retarget", [1, 0])
def test_latching_of_the_plan_words(flat_model, retarget):
    """p0 = foot_kin's p_f at the lift-off tick; p0, hgt, T bit-identical for the rest of the swing (the trunk moves on meanwhile); with
    retarget = 0 so is p1, with retarget = 1 it follows the trunk; t0 = u T_sw grows by dt per tick."""
    n = 3
    q, v = _standing(flat_model, n)
    v[:, 0], v[:, 1] = 0.3, -0.1
    P = GR.params(flat_model, retarget=retarget, **GR.DYADIC)
    phase, mask, swing = np.zeros(n), np.full(n, 0b1111, np.int32), np.zeros((n, 36))
    cmd = np.tile([0.3, -0.1, 0.2, -0.05], (n, 1))
    lift, last, seen = {}, {}, set()      # per foot: (tick, words) at lift-off; the words of the latest tick in the air
    for tick in range(300):
        q[:, 0:2] += 2 * GR.DYADIC_DT * v[:, 0:2]      # the trunk travels, and not at v (then v T_rem would keep p1 where it is): p_f and p1 change every tick
        phase, mask, swing, ev = GR.gait_tick(flat_model, P, GR.DYADIC_DT, q, v, cmd, None, phase, mask, swing)
        for k in range(4):
            sw = swing[:, 9 * k:9 * k + 9].copy()
            bit = (mask >> k) & 1
            assert np.all(bit == bit[0])               # the robots share the clock
            if np.all((ev >> k) & 1):
                assert np.array_equal(sw[:, 0:3], SR.foot_kin(flat_model, k, q, v)["pf"])
                assert np.all(sw[:, 6] == P["clearance"]) and np.all(sw[:, 7] == 0.125) and np.all(sw[:, 5] == -0.05)
                lift[k] = (tick, sw)
                seen.add(k)
            elif bit[0] == 0:
                t_lift, w = lift[k]
                assert np.array_equal(sw[:, [0, 1, 2, 6, 7]], w[:, [0, 1, 2, 6, 7]])
                assert np.array_equal(sw[:, 3:6], w[:, 3:6]) == (retarget == 0)
                assert np.array_equal(sw[:, 8], w[:, 8] + (tick - t_lift) * GR.DYADIC_DT)     # dyadic: exact
            elif k in last:
                assert np.array_equal(sw, last[k])     # a landed foot keeps the words of its last tick in the air
            if bit[0] == 0:
                last[k] = sw
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("yaw,pitch,roll", [(0.0, 0.0, 0.0), (np.pi / 2, 0.0, 0.0), (-2.1, 0.3, -0.25)])
def test_foothold_against_an_independent_evaluation(flat_model, yaw, pitch, roll):
    """The Raibert rule written once more with complex numbers and the yaw angle of Rz(yaw) Ry(pitch) Rx(roll) (whose heading (R00, R10) / |.| is
    (cos yaw, sin yaw) for |pitch| < pi / 2), at a lift-off (u = 1 / 32) and deep in a swing."""
    P = GR.params(flat_model, period=0.5, duty=(0.75, 0.5, 0.5, 0.75), k_v=0.05)
    dt_ctl = 2.0 ** -9
    n = 2
    q, v = _standing(flat_model, n)
    q[:, 0:3] = [[1.5, -0.7, 0.41], [-0.3, 2.2, 0.39]]
    q[:, 3:7] = _quat_zyx(yaw, pitch, roll)
    v[:, 0:3] = [[0.4, -0.2, 0.05], [-0.1, 0.3, 0.0]]
    cmd = np.array([[0.5, 0.1, 0.7, -0.03], [-0.2, 0.25, -0.4, 0.02]])
    for phase0, prev in ((0.75 - 2.0 ** -8, 0b1111), (0.9, 0b0000)):
        phase, mask, swing, ev = GR.gait_tick(flat_model, P, dt_ctl, q, v, cmd, None, np.full(n, phase0), np.full(n, prev, np.int32), np.zeros((n, 36)))
        checked = 0
        for k in range(4):
            duty, off = P["duty"][k], P["offset"][k]
            pk = (phase0 + dt_ctl / 0.5 + off) % 1.0
            if pk < duty:
                continue
            u = (pk - duty) / (1.0 - duty)
            if prev and u >= P["late"]:
                continue
            T_rem, T_st = (1.0 - u) * (1.0 - duty) * 0.5, duty * 0.5
            rot = np.exp(1j * yaw)
            B = rot * complex(*P["base_xy"][k])
            for s in range(n):
                vc = rot * complex(cmd[s, 0], cmd[s, 1])
                vv = complex(v[s, 0], v[s, 1])
                want = complex(q[s, 0], q[s, 1]) + B + vv * T_rem + 0.5 * T_st * vc + P["k_v"] * (vv - vc) + 0.5 * T_st * cmd[s, 2] * 1j * B
                got = swing[s, 9 * k + 3:9 * k + 6]
                assert abs(complex(got[0], got[1]) - want) < 1e-14 and got[2] == cmd[s, 3], (k, s)
                assert abs(swing[s, 9 * k + 8] - u * (1.0 - duty) * 0.5) < 1e-15
                checked += 1
        assert checked >= 4


def test_late_and_contact_rules_take_every_branch(flat_model):
    q, v = _standing(flat_model, 1)
    P = GR.params(flat_model)              # duty 0.6, late 0.5: foot 0 swings for phi in [0.6, 1), late from 0.8
    cmd = np.array([[0.2, 0.0, 0.0, -0.05]])
    junk = np.arange(36.0)[None] + 0.5

    def tick(phase, prev, contact):
        ph, m, sw, ev = GR.gait_tick(flat_model, P, 1e-3, q, v, cmd, np.array([contact], np.int32), np.array([phase]), np.array([prev], np.int32), junk)
        return int(m[0]) & 1, int(ev[0]) & 0b10001, sw[0, 0:9]

    untouched = lambda w: np.array_equal(w, junk[0, 0:9])
    b, ev, w = tick(0.3, 1, 0); assert (b, ev) == (1, 0) and untouched(w)                  # scheduled stance
    b, ev, w = tick(0.3, 0, 0); assert (b, ev) == (1, 0b10000) and untouched(w)            # scheduled touchdown
    b, ev, w = tick(0.65, 1, 1); assert (b, ev) == (0, 0b00001) and not untouched(w)       # lift-off (contact does not hold a stance foot down)
    assert w[6] == P["clearance"] and abs(w[7] - 0.16) < 1e-15
    b, ev, w = tick(0.85, 1, 0); assert (b, ev) == (1, 0) and untouched(w)                 # a start-up foot scheduled late in swing stays down
    b, ev, w = tick(0.7, 0, 1); assert (b, ev) == (0, 0)                                  # contact before `late` ignored
    assert np.array_equal(w[[0, 1, 2, 6, 7]], junk[0, [0, 1, 2, 6, 7]]) and not np.array_equal(w[3:6], junk[0, 3:6]) and w[8] != junk[0, 8]
    b, ev, w = tick(0.85, 0, 1); assert (b, ev) == (1, 0b10000) and untouched(w)           # early touchdown
    b, ev, w = tick(0.85, 0, 0); assert (b, ev) == (0, 0)                                  # no contact: the swing goes on
    b, ev, w = tick(0.7, 0, 0); assert (b, ev) == (0, 0)
    # NULL contact = no bit set
    a = GR.gait_tick(flat_model, P, 1e-3, q, v, cmd, None, np.array([0.85]), np.array([0], np.int32), junk)
    c = GR.gait_tick(flat_model, P, 1e-3, q, v, cmd, np.array([0], np.int32), np.array([0.85]), np.array([0], np.int32), junk)
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    # and the branch case the GPU tests use covers all of this for every foot
    tm = float(np.sum(flat_model["mass"]))
    assert GR.branches_taken(P, 1e-3, [GR.branch_case(flat_model, tm, 15, rank=15)]) == GR.ALL_BRANCHES


def test_f32_error_constants_are_what_the_restatement_measures(flat_model):
    """gait_ref.F32_ERR (the base of the fp32 gates of tests/test_gpu_gait.py): float32 against float64 on the parity cases, where float32 takes the
    same branches on every state.  The constants are the measured errors rounded up: never below them, never more than twice them."""
    worst = GR.f32_errors(flat_model, float(np.sum(flat_model["mass"])))
    print("float32 against float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= GR.F32_ERR[k] <= 2 * v, (k, v)


def test_closed_loop_walks_and_lands(flat_model, oracle):
    """16 robots, dyadic trot, two periods (gait_ref.walk_case; what the case took: see WALK_SWING_PARAMS).  Every QP status 0; at every touchdown
    whose step is at least 2 cm the foot is within 0.1 |p1 - p0| of p1.  Nothing is asserted about the stance feet: the plant has no ground."""
    case, r = GR.cpu_walk(flat_model, oracle, 16)
    assert r["status_ok"]
    assert np.all(np.isin(r["masks"], TROT))
    assert len(r["landings"]) == 16 * 8                  # four feet, two periods
    ratios = GR.landing_ratios(r["landings"])
    print("touchdowns %d, of them with a step >= 2 cm: %d, worst |pf - p1| / |p1 - p0| %.4f" % (len(r["landings"]), len(ratios), ratios.max()))
    assert len(ratios) >= 64                             # the assertion below is not met by leaving steps out
    assert np.all(ratios < 0.1), ratios.max()
    assert r["q"][:, 0].min() > case["q"][:, 0].min() + 0.03      # and the robots did travel forward
