"""CPU: the numpy restatement of the ground-contact plant (tests/ground_ref.py) -- the branch case's coverage and decision margins, what float32 costs,
how the default parameters were fixed, and the walking loop on the ground plant that tests/test_gpu_ground.py repeats on the device.

How the defaults were fixed (ground_ref.settle: the standing loop reference -> step -> integrate_ground at dt = 1e-3, one robot of 25.38 kg released with
its feet 5 mm above flat ground, 1500 ticks).  Measured with k_n 2e4, c_n 150, c_t 200, f_touch 5:
  settling time      126 ticks (0.126 s): from there sum_k n . f_gr,k stays within 1e-3 of m g = 248.9778 N; all four feet touch from tick 15 on and no
                     contact bit changes after that
  residuals at the end    |sum_k n . f_gr,k - m g| / (m g) = 5.0e-7;   |mean penetration - m g / (4 k_n)| / (3.112 mm) = 5.1e-7
  explicit-stability ratios per foot   c_n dt / m_eff = 0.443, 0.434, 0.455, 0.457;   k_n dt^2 / m_eff = 0.0591, 0.0579, 0.0607, 0.0609
  coupled over the four feet           largest eigenvalue of dt (Jc M^-1 Jc^T) diag(c_t, c_t, c_n) = 0.97 (limit 2)
The starting point k_n 2e4, c_n 200, c_t 500 fails: per-foot ratios 0.60 and 0.060, but the coupled eigenvalue is 2.03 and the total normal force
alternates between 222 and 273 N from tick to tick without end.

The walking loop (ground_ref.closed_loop: 16 robots, 512 ticks of 2^-10 s, bump +1.5 cm under foot 1 of the even robots and hole -1.5 cm under foot 2 of
robots 1, 5, 9, 13 from tick 64 on).  Measured: 64 early touchdowns caused by sensed contact (u = 0.75 ... 0.97), none without it; smallest
|f_n - f_touch| / max f_n = 4.7e-5 (max f_n 799 N); amplification of a 1e-12 relative perturbation of q0 over the loop A = 2.3."""
import numpy as np
import pytest

from tests import envelope, ground_ref as R, limit_ref
from tests.util import unpack_M


@pytest.fixture(scope="module")
def total_mass(flat_model):
    return float(np.sum(flat_model["mass"]))


@pytest.mark.parametrize("n", R.PARITY_SIZES)
def test_branch_case_margins_and_coverage(flat_model, total_mass, n):
    P = R.params()
    legs = limit_ref.leg_joints(flat_model)
    c = R.branch_case(flat_model, total_mass, n, rank=n, P=P)
    g = R.ground_force(P, c["q"], c["v"], c["dyn"]["Jc"], c["normals"], c["height"], c["mu"], legs)
    m = R.margins(P, g)
    print(n, m)
    assert all(x >= 1.0 for x in m.values()), m          # every state of the case: nothing is excluded
    assert np.all(np.isfinite(g["f_gr"]))
    if n >= 15:
        assert R.branches_taken(P, g) == R.ALL_BRANCHES
        rest = c["kinds"][:, 0] == -1
        assert rest.any() and np.all(g["vt"][rest] == 0) and np.all(g["fn"][rest] > 0)
        assert np.array_equal(g["f_gr"][rest][:, [0, 1, 3, 4, 6, 7, 9, 10]], np.zeros((rest.sum(), 8)))     # f_t = 0 exactly, no 0/0
    # the law is the controller-independent one: v_f of the restatement is Jc_k v
    J = c["dyn"]["Jc"].reshape(n, 12, 18)
    vf = np.einsum("nij,nj->ni", J, c["v"])
    for k in range(4):
        lever, Jl, qd = R.foot_words(c["dyn"]["Jc"], c["v"], k, legs)
        mine = c["v"][:, 0:3] + np.cross(c["v"][:, 3:6], lever) + np.einsum("nij,nj->ni", Jl, qd)
        assert np.abs(mine - vf[:, 3 * k:3 * k + 3]).max() < 1e-12


def test_plant_step_is_integrate_ref_in_float64(flat_model, total_mass):
    c = R.branch_case(flat_model, total_mass, 17, rank=17)
    f = np.random.default_rng(5).uniform(-50, 50, (17, 12))
    M = unpack_M(c["dyn"]["M"])
    a = envelope.integrate_ref(1e-3, M, c["dyn"]["h"], c["dyn"]["Jc"], c["tau"], f, c["tau_ext"], c["q"], c["v"])
    b = R.plant_step(1e-3, M, c["dyn"]["h"], c["dyn"]["Jc"], c["tau"], f, c["tau_ext"], c["q"], c["v"])
    assert np.abs(a[0] - b[0]).max() < 1e-13 and np.abs(a[1] - b[1]).max() < 1e-11


def test_f32_errors_reproduced(flat_model, total_mass):
    got = R.f32_errors(flat_model, total_mass)
    print(got)
    for k, e in R.F32_ERR.items():
        assert 0.5 * e <= got[k] <= e, (k, got[k], e)


def test_defaults_settle_a_standing_robot(flat_model, oracle):
    P = R.params()
    assert P == dict(k_n=2e4, c_n=150.0, c_t=200.0, f_touch=5.0)
    s = R.settle(flat_model, oracle, P)
    m_g = s["m_g"]
    st = R.settle_tick(s["weight"], m_g)
    pen_ref = m_g / (4 * P["k_n"])
    rw, rp = abs(s["weight"][-1, 0] - m_g) / m_g, abs(s["pen"][-1, 0] - pen_ref) / pen_ref
    print("settle tick %s; residuals weight %.3g penetration %.3g; ratios c_n dt / m_eff %s, k_n dt^2 / m_eff %s; coupled %.3f"
          % (st, rw, rp, np.round(s["ratios"][0][0], 4), np.round(s["ratios"][1][0], 5), s["coupled"][0]))
    assert s["status_ok"]
    assert st is not None and st <= 300                       # (a) it settles ...
    assert rw < 1e-5 and rp < 1e-5                            # ... to the two identities
    first = int(np.nonzero(s["contact"][:, 0] == 15)[0][0])
    assert np.all(s["contact"][first:] == 15)                 # (b) no bit toggles once all four feet touch, let alone after settling
    assert s["coupled"][0] < 2.0 and s["ratios"][0].max() < 2.0 and s["ratios"][1].max() < 4.0


def test_starting_point_does_not_settle(flat_model, oracle):
    s = R.settle(flat_model, oracle, R.params(c_n=200.0, c_t=500.0), ticks=600)
    assert R.settle_tick(s["weight"], s["m_g"]) is None and s["coupled"][0] > 2.0


def test_walking_loop_lands_early_on_sensed_contact(flat_model, oracle):
    n = 16
    case, cpu = R.cpu_walk(flat_model, oracle, n)
    blind = R.closed_loop(flat_model, oracle, case, sensed=False)
    print("early touchdowns %d (blind %d), u %.3f ... %.3f; touch margin %.3g, max f_n %.1f" %
          (len(cpu["early"]), len(blind["early"]), min(e[3] for e in cpu["early"]), max(e[3] for e in cpu["early"]), cpu["touch_margin"], cpu["fn_max"]))
    assert cpu["status_ok"] and blind["status_ok"]
    sensed = {e[:3] for e in cpu["early"]} - {e[:3] for e in blind["early"]}
    assert len(sensed) >= 1 and all(e[3] < 1.0 for e in cpu["early"])
    assert {(s, f) for _, s, f in sensed} >= {(s, 1) for s in range(0, n, 2)}      # every bump is found by the foot above it
    assert cpu["touch_margin"] >= 1e-6
    assert len(np.unique(cpu["contacts"])) >= 4


def test_walking_loop_sensitivity(flat_model, oracle):
    """A = |delta end| / |delta start| for q0 perturbed by 1e-12 relative: tests/test_gpu_ground.py derives its closed-loop gate from it"""
    n = 16
    case, cpu = R.cpu_walk(flat_model, oracle, n)
    q0 = case["q"] * (1 + 1e-12 * np.random.default_rng(1).uniform(-1, 1, case["q"].shape))
    p = R.closed_loop(flat_model, oracle, case, q0=q0)
    d0 = np.abs(q0 - case["q"]).max()
    d1 = max(np.abs(p["q"] - cpu["q"]).max(), np.abs(p["v"] - cpu["v"]).max())
    A = d1 / d0
    print("A = %.3g (start %.3g, end %.3g)" % (A, d0, d1))
    assert np.array_equal(p["masks"], cpu["masks"]) and np.array_equal(p["contacts"], cpu["contacts"])
    assert A <= R.WALK_AMPLIFICATION
