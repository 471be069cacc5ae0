"""CPU: the numpy restatement of stiction on the ground plant (tests/stick_ref.py) -- the branch case's coverage and decision margins, the
zero-stiffness limit, what float32 costs, how the default k_t was fixed (slope hold, slide, flat settle) and the walking loop that
tests/test_gpu_stick.py repeats on the device.

How the default was fixed.  Synthetic model (25.38 kg, m g = 248.9778 N), default ground parameters, k_t = k_n = 2e4, the standing loop
reference -> step -> integrate_ground_stick at dt = 1e-3, one robot, every foot on its own plane tilted by 0.2 rad about y, 5 mm under the foot,
mu = 0.6, 1500 ticks.  Measured:
  viscous law (k_t = 0)    the mean foot position moves 61.70 mm between ticks 500 and 1499, 60.47 mm of it along x, against the predicted
                           m g sin 0.2 / (4 c_t) x 1 s = 61.83 mm; |v| = 0.144 at the end: the slide goes on
  k_t = 2e4                7.5e-7 m over the same ticks, |v| = 2.5e-7 at the end, no slide bit after tick 500 (none after the landing at all);
                           sum_k f_gr,k along the slope = -49.464245 N against -m g sin 0.2 = -49.464253 (1.6e-7), along the normal 244.014821 against
                           m g cos 0.2 = 244.014820; per foot k_t |e| = |f_t| = 10.19, 11.51, 14.25, 13.54 N to 3e-8
  stability                a = largest eigenvalue of dt (Jc M^-1 Jc^T) diag(c_t, c_t, c_n) = 0.967;  b = that of dt^2 (Jc M^-1 Jc^T) diag(k_t, k_t, k_n)
                           = 0.108;  one mode of the semi-implicit step needs b < 4 - 2 a = 2.07
  slide (plant mu 0.1, controller's 0.6, ticks 0 ... 150)   143 ticks with all eight stick bits set, | |f_t| - mu f_n | <= 4e-17 f_n on every sliding
                           foot-tick, every QP status 0
  flat ground              settles at tick 119 (viscous: 126), weight residual 2.3e-9, penetration residual 2.5e-9, foot drift over ticks 500 ... 1499
                           9.7e-7 m, no slide bit after tick 500
The starting point 2e4 passed all of it, so nothing was lowered.

The walking loop (stick_ref.closed_loop: ground_ref's, 16 robots, 512 ticks of 2^-10 s, both height arrays raised by m g / (4 k_n) = 3.112 mm).
Measured: every status 0 with either law, the trunk ends at x = 0.0474 m with both; 84 early touchdowns, every bump among them; the tangential
path of feet carrying more than 50 N is 0.0293 m per robot against the viscous law's 0.0622 (ratio 0.47); amplification of a 1e-12 relative
perturbation of q0 A = 2.9, stick, contact and mask words equal between the two runs."""
import numpy as np
import pytest

from tests import ground_ref as R, limit_ref, stick_ref as S


@pytest.fixture(scope="module")
def total_mass(flat_model):
    return float(np.sum(flat_model["mass"]))


def _law(flat, c, k_t=S.DEFAULT_KT, anchor=None, stick=None, P=None):
    return S.stick_force(P or R.params(), k_t, c["q"], c["v"], c["dyn"]["Jc"], c["normals"], c["height"], c["mu"],
                         c["anchor"] if anchor is None else anchor, c["stick"] if stick is None else stick, limit_ref.leg_joints(flat))


@pytest.mark.parametrize("n", S.PARITY_SIZES)
def test_branch_case_margins_and_coverage(flat_model, total_mass, n):
    P = R.params()
    c = S.branch_case(flat_model, total_mass, n, rank=n, P=P)
    g = _law(flat_model, c)
    m = S.margins(P, g)
    print(n, m)
    assert all(x >= 1.0 for x in m.values()), m          # every state of the case: nothing is excluded
    assert np.all(np.isfinite(g["f_gr"]))
    w = S.written_anchor(g, c["anchor"])                 # (asserts that every other anchor word is the input's, bit for bit)
    un = np.repeat(~g["loaded"], 3, 1)
    assert np.array_equal(g["anchor"][un], c["anchor"][un])
    assert np.all((g["stick"] & 0xf) == sum(g["loaded"][:, k].astype(int) << k for k in range(4))) and np.all(g["stick"] >> 8 == 0)
    first = np.repeat(g["loaded"] & ~g["had"], 3, 1)
    assert np.array_equal(g["anchor"][first], g["pf"].reshape(n, 12)[first]) and np.all(g["e"][g["loaded"] & ~g["had"]] == 0)
    if n >= 15:
        assert S.branches_taken(g) == S.ALL_BRANCHES
        moved = g["slid"] & g["had"]
        assert moved.any() and not np.any(g["anchor"][np.repeat(moved, 3, 1)] == c["anchor"][np.repeat(moved, 3, 1)])
        assert w.any() and not w.all()
        # on a sliding foot the force lies on the cone and the stretch has shrunk by the factor the force has
        ftn = np.linalg.norm(g["ft"], axis=2)
        assert np.abs(ftn - g["cone"])[g["slid"]].max() < 1e-12 * g["cone"].max()
        for k in range(4):
            sl = g["slid"][:, k] & g["had"][:, k]
            nk = c["normals"][sl, 3 * k:3 * k + 3]
            da = g["pf"][sl, k] - g["anchor"][sl, 3 * k:3 * k + 3]
            e1 = da - (nk * da).sum(1)[:, None] * nk
            s = (g["cone"] / g["gnorm"])[sl, k]
            assert np.abs(e1 - s[:, None] * g["e"][sl, k]).max() < 1e-15


@pytest.mark.parametrize("n", (17, 33))
def test_zero_stiffness_is_the_stateless_law(flat_model, total_mass, n):
    """k_t = 0: f_gr, contact, gap equal ground_ref.ground_force's for random anchors and random incoming stick words; bits 0-3 out = f_n > 0"""
    P = R.params()
    legs = limit_ref.leg_joints(flat_model)
    c = R.branch_case(flat_model, total_mass, n, rank=n, P=P)
    ref = R.ground_force(P, c["q"], c["v"], c["dyn"]["Jc"], c["normals"], c["height"], c["mu"], legs)
    rng = np.random.default_rng(n)
    for _ in range(4):
        anchor, stick = rng.uniform(-10, 10, (n, 12)), rng.integers(0, 1 << 16, n).astype(np.int32)
        g = S.stick_force(P, 0.0, c["q"], c["v"], c["dyn"]["Jc"], c["normals"], c["height"], c["mu"], anchor, stick, legs)
        for k in ("f_gr", "contact", "gap"):
            assert np.array_equal(g[k], ref[k]), k
        assert np.array_equal(g["stick"] & 0xf, sum((ref["fn"][:, k] > 0).astype(np.int32) << k for k in range(4)))


def test_f32_errors_reproduced(flat_model, total_mass):
    got = S.f32_errors(flat_model, total_mass)
    print(got)
    for k, e in S.F32_ERR.items():
        assert 0.5 * e <= got[k] <= e, (k, got[k], e)


def test_slope_hold(flat_model, oracle):
    P = R.params()
    case, vis = S.cpu_slope(flat_model, oracle, 0.0)
    _, rec = S.cpu_slope(flat_model, oracle, S.DEFAULT_KT)
    m_g = rec["m_g"]
    pred = m_g * np.sin(S.SLOPE) / (4 * P["c_t"]) * 1.0
    dv, ds = float(np.linalg.norm(S.drift(vis)[0])), float(np.linalg.norm(S.drift(rec)[0]))
    F = rec["f_gr"][-1, 0].reshape(4, 3).sum(0)
    along, normal = float(F @ case["downhill"]), float(F @ case["normals"][0, :3])
    spring, ft = S.DEFAULT_KT * np.linalg.norm(rec["e"][-1, 0], axis=1), np.linalg.norm(rec["ft"][-1, 0], axis=1)
    a, b = float(R.stability_coupled(P, rec["dt"], rec["dyn"])[0]), float(S.stability_spring(P, S.DEFAULT_KT, rec["dt"], rec["dyn"])[0])
    print("viscous drift %.5g m (predicted %.5g), |v| %.3g; with k_t %.3g m, |v| %.3g; along %.9g (-m g sin %.9g) normal %.9g (m g cos %.9g); "
          "k_t |e| %s |f_t| %s; a %.3f b %.3f" % (dv, pred, np.abs(vis["v"]).max(), ds, np.abs(rec["v"]).max(), along, -m_g * np.sin(S.SLOPE), normal,
                                                 m_g * np.cos(S.SLOPE), spring, ft, a, b))
    assert all(vis["status_ok"]) and all(rec["status_ok"])
    assert abs(dv - pred) <= 0.1 * pred
    assert ds <= 1e-2 * dv
    assert not np.any(rec["stick"][S.SLOPE_FROM:] >> 4)
    assert np.all(rec["stick"][S.SLOPE_FROM:] == 0b1111)
    # the weight: sum_k f_gr,k = -m g, along the slope, along the normal and (so) vertically
    assert abs(along + m_g * np.sin(S.SLOPE)) <= 1e-5 * m_g * np.sin(S.SLOPE)
    assert abs(normal - m_g * np.cos(S.SLOPE)) <= 1e-5 * m_g and abs(F[2] - m_g) <= 1e-5 * m_g
    assert np.abs(spring - ft).max() <= 1e-5 * ft.max()
    assert a < 2.0 and b < 4.0 - 2.0 * a


def test_slide_stays_on_the_cone(flat_model, oracle):
    case = S.slope_case(flat_model, oracle, 1)
    rec = S.stand_loop(flat_model, oracle, case, S.DEFAULT_KT, ticks=S.SLIDE_TICKS + 1, mu_plant=S.SLIDE_MU)
    all8 = int(((rec["stick"][:, 0] & 0xff) == 0xff).sum())
    slid = ((rec["stick"][:, :, None] >> (4 + np.arange(4))) & 1) == 1
    err = np.abs(np.linalg.norm(rec["ft"], axis=3) - S.SLIDE_MU * rec["fn"])
    print("ticks with all eight bits %d; worst | |f_t| - mu f_n | / f_n on a sliding foot %.3g" % (all8, (err[slid] / rec["fn"][slid]).max()))
    assert all8 >= 100
    assert np.all(rec["fn"][slid] > 0) and np.all(err[slid] <= 1e-12 * rec["fn"][slid])
    assert all(rec["status_ok"])


def test_default_settles_a_standing_robot_on_flat_ground(flat_model, oracle):
    """the assertions of test_ground_oracle.py::test_defaults_settle_a_standing_robot, with the default k_t"""
    P = R.params()
    rec = S.stand_loop(flat_model, oracle, R.stand_case(flat_model, oracle, 1), S.DEFAULT_KT, ticks=R.SETTLE_TICKS)
    m_g = rec["m_g"]
    weight, pen = rec["fn"].sum(2), -rec["gap"].mean(2)
    st = R.settle_tick(weight, m_g)
    pen_ref = m_g / (4 * P["k_n"])
    rw, rp = abs(weight[-1, 0] - m_g) / m_g, abs(pen[-1, 0] - pen_ref) / pen_ref
    ratios, coupled = R.stability_ratios(P, rec["dt"], rec["dyn"], np.tile([0.0, 0.0, 1.0], (1, 4))), R.stability_coupled(P, rec["dt"], rec["dyn"])
    print("settle tick %s; residuals weight %.3g penetration %.3g; foot drift %.3g" % (st, rw, rp, np.linalg.norm(S.drift(rec)[0])))
    assert all(rec["status_ok"])
    assert st is not None and st <= 300
    assert rw < 1e-5 and rp < 1e-5
    first = int(np.nonzero(rec["contact"][:, 0] == 15)[0][0])
    assert np.all(rec["contact"][first:] == 15)
    assert coupled[0] < 2.0 and ratios[0].max() < 2.0 and ratios[1].max() < 4.0
    assert not np.any(rec["stick"][S.SLOPE_FROM:] >> 4)


def test_walking_loop_slips_less_and_still_lands_early(flat_model, oracle):
    n = 16
    case, cpu = S.cpu_walk(flat_model, oracle, n)
    _, vis = S.cpu_walk(flat_model, oracle, n, 0.0)
    print("slip path %.4g m per robot (viscous %.4g, ratio %.3g); trunk x %.4g (viscous %.4g); %d early touchdowns; touch margin %.3g, max f_n %.1f"
          % (cpu["slip"], vis["slip"], cpu["slip"] / vis["slip"], cpu["q"][:, 0].mean(), vis["q"][:, 0].mean(), len(cpu["early"]),
             cpu["touch_margin"], cpu["fn_max"]))
    assert cpu["status_ok"] and vis["status_ok"]
    assert all(e[3] < 1.0 for e in cpu["early"])
    assert {(s, f) for _, s, f, _ in cpu["early"]} >= {(s, 1) for s in range(0, n, 2)}      # every bump is found by the foot above it
    assert cpu["slip"] < 0.6 * vis["slip"]
    assert cpu["touch_margin"] >= 1e-6
    assert np.any(cpu["sticks"] >> 4) and len(np.unique(cpu["sticks"] & 0xf)) >= 4


def test_walking_loop_sensitivity(flat_model, oracle):
    """A = |delta end| / |delta start| for q0 perturbed by 1e-12 relative: tests/test_gpu_stick.py derives its closed-loop gate from it.  A value like
    1e8 would mean that the case has a decision on an edge (the zero-gap start of ground_ref.walk_case has, with an anchor)"""
    n = 16
    case, cpu = S.cpu_walk(flat_model, oracle, n)
    q0 = case["q"] * (1 + 1e-12 * np.random.default_rng(1).uniform(-1, 1, case["q"].shape))
    p = S.closed_loop(flat_model, oracle, case, q0=q0)
    d0 = np.abs(q0 - case["q"]).max()
    d1 = max(np.abs(p["q"] - cpu["q"]).max(), np.abs(p["v"] - cpu["v"]).max())
    A = d1 / d0
    print("A = %.3g (start %.3g, end %.3g)" % (A, d0, d1))
    for k in ("masks", "contacts", "sticks"):
        assert np.array_equal(p[k], cpu[k]), k
    assert A <= S.WALK_AMPLIFICATION <= 50
