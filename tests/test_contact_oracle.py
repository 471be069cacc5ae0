"""Contact sensing from the disturbance observer on the CPU: the numpy restatement tests/contact_ref.py against a brute-force solve, its branch case, how
det_min and the thresholds were fixed, and the walking loop of the ground plant with the observer ON and the estimate fed back to the gait scheduler.

Measured (synthetic model, observer_order 1, K1 = 50, dt = 2^-10, default ground and contact parameters; the asserts below hold these):
  branch_case(n, rank=n), n in 1, 15, 16, 17, 33, 64: every branch from n = 15 on; smallest threshold margin 2.3e-2 of the largest |fn| (float32: the
  same to 1e-8); worst cond(J_leg) of a regular leg 3.7; float32 against float64: f_est 2.1e-7, fn 2.4e-7 of the largest entry, all words equal.
  |det J_leg|: changes sign inside the URDF's joint limits (-4.3e-2 .. 4.3e-2: it reaches 0); 1.9e-2 .. 4.4e-2 within 0.5 rad of the standing posture on every joint.
  closed_loop, 4 robots, 512 ticks, +15 mm under foot 1 of robots 0 and 2 from tick 64 on:
    "estimate"  every status 0; early touchdowns of the bumped feet at ticks 102, 103 (u = 0.80, 0.81); base z at the end 0.4022 .. 0.4031
    "truth"     the same feet at ticks 99, 100; base z 0.4022 .. 0.4030; largest |base z difference| to "estimate" 1.01e-4 m
    "none"      no early touchdown at all; base z 0.4022 .. 0.4056
    every early touchdown the two sensed loops share on the same foot and swing: the estimate is 2 .. 5 ticks behind
    smallest threshold margin of the estimated loop 2.2e-5 of the largest |fn_est| (227 N); no leg ever singular (|det| 4.0e-2 .. 4.2e-2)
    amplification of a 1e-12 relative perturbation of q0 over the estimated loop: A = 1.5
  f_on = f_off = 5 N in the 16-robot loop: one bit flips 0 -> 1 -> 0 on consecutive ticks; with the defaults none does."""
import numpy as np
import pytest

from tests import contact_ref as R, ground_ref as GND, limit_ref


@pytest.fixture(scope="module")
def legs(flat_model):
    return limit_ref.leg_joints(flat_model)


def _f32(c):
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(c["Jc"]), f(c["r"]), f(c["f_prev"]), f(c["normals"]), c["contact"]


@pytest.mark.parametrize("n", R.PARITY_SIZES)
def test_law_against_a_brute_force_solve_and_every_branch(flat_model, legs, n):
    P = R.params()
    c = R.branch_case(flat_model, n, rank=n)
    e = R.estimate(P, c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
    b = R.estimate_brute(P, c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
    assert np.array_equal(e["contact"], b["contact"]) and np.array_equal(e["singular"], b["singular"])
    assert np.abs(e["f_est"] - b["f_est"]).max() < 1e-11 and np.abs(e["fn"] - b["fn"]).max() < 1e-11
    assert np.all(e["contact"] & ~15 == 0x50)                         # bits outside 0-3 are kept
    if n >= 15:
        assert R.branches_taken(P, e) == R.ALL_BRANCHES
    # the two special kinds: a singular leg keeps its bit and gets df = 0; r = 0 gives f_est = f_prev exactly
    for k in range(4):
        s6, s7 = c["kinds"][:, k] == 6, c["kinds"][:, k] == 7
        assert np.all(((e["singular"] >> k) & 1)[s6] == 1) and np.all(((e["singular"] >> k) & 1)[~s6] == 0)
        assert np.array_equal(((e["contact"] >> k) & 1)[s6], ((c["contact"] >> k) & 1)[s6])
        assert np.array_equal(e["f_est"][s6 | s7, 3 * k:3 * k + 3], c["f_prev"][s6 | s7, 3 * k:3 * k + 3])
    # margins, in float64 and in float32 terms, and the same words in float32
    m64 = R.margins(P, e)
    e32 = R.estimate(P, *_f32(c), legs)
    m32 = R.margins(P, e32)
    print("n=%d margins f64 %s f32 %s cond %.2f" % (n, m64, m32, R.worst_cond(c, legs)))
    assert m64["thr"] >= R.MARGIN64 and m64["det"] >= R.MARGIN64 and m32["thr"] >= R.MARGIN32 and m32["det"] >= R.MARGIN32
    assert np.array_equal(e32["contact"], e["contact"]) and np.array_equal(e32["singular"], e["singular"])
    assert R.worst_cond(c, legs) <= R.COND_MAX
    eps32 = float(np.finfo(np.float32).eps)
    assert R.COND_MAX * eps32 * 10 <= R.F32_GATE and R.COND_MAX * float(np.finfo(np.float64).eps) * 10 <= R.F64_GATE
    for what in ("f_est", "fn"):
        assert np.abs(e32[what] - e[what]).max() <= R.COND_MAX * eps32 * 10 * np.abs(e[what]).max(), what


def test_hysteresis_and_parameters_of_the_law(flat_model, legs):
    """A foot between the thresholds keeps its bit either way over two consecutive calls; new thresholds flip it."""
    P = R.params()
    c = R.branch_case(flat_model, 16, rank=16)
    mid = (c["kinds"] == 1) | (c["kinds"] == 4)
    e1 = R.estimate(P, c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
    e2 = R.estimate(P, c["Jc"], c["r"], c["f_prev"], c["normals"], e1["contact"], legs)
    bits = lambda w: ((w[:, None] >> np.arange(4)[None, :]) & 1) == 1
    assert mid.any() and np.array_equal(bits(e1["contact"])[mid], bits(c["contact"])[mid]) and np.array_equal(e2["contact"], e1["contact"])
    hi = R.estimate(R.params(f_on=100.0, f_off=99.0), c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
    reg = c["kinds"] != 6
    assert not bits(hi["contact"])[reg].any()
    lo = R.estimate(R.params(f_on=4.0, f_off=4.0), c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
    assert bits(lo["contact"])[mid].all()
    assert bits(R.estimate(R.params(det_min=1.0), c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)["singular"]).all()


def test_det_min_lies_a_factor_of_ten_below_what_a_walking_robot_reaches(flat_model):
    lim = R.leg_det_range(flat_model, [[0.0] * 3] * 4, (1.0, 2.5, 2.6))
    std = R.leg_det_range(flat_model, R.standing_centre(flat_model), (0.5, 0.5, 0.5))
    print("|det J_leg|: joint limits %.3g .. %.3g; standing +- 0.5 rad %.3g .. %.3g" % (lim + std))
    sgn = R.leg_det_range(flat_model, [[0.0] * 3] * 4, (1.0, 2.5, 2.6), signed=True)
    assert sgn[0] < -1e-2 and sgn[1] > 1e-2 and lim[0] < R.DEFAULT_PARAMS["det_min"]     # det changes sign inside the limits: it reaches 0 there
    assert R.DET_MEASURED["standing"] <= std[0] <= 1.1 * R.DET_MEASURED["standing"]
    assert R.DEFAULT_PARAMS["det_min"] <= std[0] / 10 and R.DEFAULT_PARAMS["det_min"] >= std[0] / 20


def _bumped(n):
    return [(s, 1) for s in range(0, n, 2)]


def test_estimated_walking_loop_lands_early_on_the_bump(flat_model, oracle):
    n = R.WALK_N
    _, est = R.cpu_walk(flat_model, oracle, "estimate")
    _, tru = R.cpu_walk(flat_model, oracle, "truth")
    _, non = R.cpu_walk(flat_model, oracle, "none")
    assert est["status_ok"] and tru["status_ok"] and non["status_ok"]
    assert not est["singular_any"]
    assert non["early"] == []
    GP_T = 128                                               # ticks of one swing of the dyadic trot
    for s, f in _bumped(n):
        te, tt = R.first_early(est["early"], s, f), R.first_early(tru["early"], s, f)
        print("robot %d foot %d: early touchdown at tick %s (truth %s)" % (s, f, te, tt))
        assert te is not None and tt is not None and te < GP_T and tt < GP_T        # in the swing that was under way at BUMP_TICK
        assert tt <= te <= tt + R.LAG_TICKS
    # every early touchdown the two loops share (same robot, foot and swing window): the measured lag
    lags = []
    for t, s, f, _ in est["early"]:
        same = [x[0] for x in tru["early"] if x[1] == s and x[2] == f and x[0] // GP_T == t // GP_T]
        if same:
            lags.append(t - same[0])
    print("lags of the shared early touchdowns:", lags)
    assert lags and min(lags) >= 0 and max(lags) + 2 <= R.LAG_TICKS
    dz = float(np.abs(est["q"][:, 2] - tru["q"][:, 2]).max())
    print("base z: estimate %s truth %s none %s; |estimate - truth| %.3g; threshold margin %.3g of %.1f N" %
          (est["q"][:, 2], tru["q"][:, 2], non["q"][:, 2], dz, est["thr_margin"], est["fn_max"]))
    assert dz <= R.BASE_Z_BAND and 2 * dz >= 0.5 * R.BASE_Z_BAND        # the band is the measured difference x 2, not a loose number
    assert np.all(est["q"][:, 2] > 0.39)
    assert est["thr_margin"] >= 1e-6
    assert len(np.unique(est["contacts"])) >= 4


def test_estimated_walking_loop_sensitivity(flat_model, oracle):
    """A = |delta end| / |delta start| for q0 perturbed by 1e-12 relative: tests/test_gpu_contact.py derives its closed-loop gate from it"""
    case, cpu = R.cpu_walk(flat_model, oracle, "estimate")
    q0 = case["q"] * (1 + 1e-12 * np.random.default_rng(1).uniform(-1, 1, case["q"].shape))
    p = R.closed_loop(flat_model, oracle, case, "estimate", q0=q0)
    d0 = np.abs(q0 - case["q"]).max()
    d1 = max(np.abs(p["q"] - cpu["q"]).max(), np.abs(p["v"] - cpu["v"]).max())
    A = d1 / d0
    print("A = %.3g (start %.3g, end %.3g)" % (A, d0, d1))
    assert np.array_equal(p["masks"], cpu["masks"]) and np.array_equal(p["contacts"], cpu["contacts"])
    assert A <= R.WALK_AMPLIFICATION


def test_no_hysteresis_chatters_and_the_defaults_do_not(flat_model, oracle):
    """What was tried and failed: f_on = f_off = 5 N in the 16-robot loop."""
    case = GND.walk_case(flat_model, oracle, 16)
    flat5 = R.closed_loop(flat_model, oracle, case, "estimate", P=R.params(**R.NO_HYSTERESIS))
    dflt = R.closed_loop(flat_model, oracle, case, "estimate")
    print("bits flipping on two consecutive ticks: 5/5 N %d, defaults %d" % (R.toggles(flat5["contacts"]), R.toggles(dflt["contacts"])))
    assert flat5["status_ok"] and dflt["status_ok"]
    assert R.toggles(flat5["contacts"]) >= 1 and R.toggles(dflt["contacts"]) == 0
